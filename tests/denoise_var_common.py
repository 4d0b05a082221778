"""What tests/test_denoise_var_host.py (CPU) and tests/test_gpu_accum_denoise.py (GPU) share: the variance-guided denoiser.

The frames and cases are denoise_common's (1 x 1 up to 130 x 19, both flags, bad guides, every sigma at +infinity; here sigma_color keeps
the filter's own default unless a case sets it).  Each case gets a VARIANCE MAP of the colour's scale - the frames' noise has a standard
deviation of 0.8, so variances are 0.64 times a factor in 0.2 .. 2 - with 0, 1e-12, 1e31, +Inf, NaN and -1 sprinkled into it."""
import numpy as np

import denoise_common as DC
import denoise_var_ref

F32 = np.float32
INF = float("inf")
SPECIALS = (0.0, 1e-12, 1e31, INF, np.nan, -1.0)
IDS = DC.IDS


def var_map(W, H, seed):
    rng = np.random.default_rng(seed + 90001)
    var = (0.64 * rng.uniform(0.2, 2.0, (H, W, 3))).astype(F32)
    flat = var.reshape(-1)
    n = flat.size
    idx = rng.permutation(n)[:max(len(SPECIALS), n // 10)] if n >= len(SPECIALS) else np.arange(n)
    for j, i in enumerate(idx):
        flat[i] = SPECIALS[j % len(SPECIALS)]
    var.setflags(write=False)
    return var


def inputs(cid):
    """(rgb, var, aov) of a case, read-only"""
    _, W, H, _, seed, _ = DC.case(cid)
    rgb, aov = DC.inputs(cid)
    return rgb, var_map(W, H, seed), aov


def params(B, cid):
    return B.denoise_var_default_params(**DC.case(cid)[3])


_ref = {}


def reference(cid):
    """denoise_var_ref's (out, rgba8, v_L) of a case, computed once per session and handed out read-only."""
    if cid not in _ref:
        rgb, var, aov = inputs(cid)
        r = denoise_var_ref.denoise_var(rgb, var, aov, **DC.case(cid)[3])
        for a in r:
            a.setflags(write=False)
        _ref[cid] = r
    return _ref[cid]
