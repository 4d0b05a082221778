"""Frames and cases shared by tests/test_upsample_host.py (CPU) and tests/test_gpu_upsample.py (GPU): the upsampling (pt_upsample).

A CASE is (id, w, h, W, H, params, seed, bad_guides): params are fields of pt_upsample_params that differ from the defaults.
  * high guides: denoise_common.guides - a few "surfaces" cut by random lines, so normals, depths and albedos repeat across the frame;
  * low guides: the high ones sampled at the pixel nearest to each low pixel's centre, plus noise of 0.02 on normals and on the non-zero
    albedo channels and of 0.02 relative on depths: taps of every weight from 0 to 1 occur, and so does the fallback branch (a high
    pixel none of whose low neighbours lies on its surface);
  * colour (low size): NaN, +Inf, -Inf, negatives and exact zeros among values of a few units;  albedo: exact zeros;
  * bad_guides: +Inf depths and NaN normals in a few pixels of BOTH guide sets."""
import numpy as np

import denoise_common as DC
import upsample_ref

F32 = np.float32
INF = float("inf")
SIZES = ((1, 1, 1, 1), (1, 1, 5, 3), (3, 2, 7, 5), (9, 1, 37, 1), (1, 9, 1, 37),
         (20, 15, 50, 37),    # a non-integer ratio
         (35, 23, 70, 45),
         (65, 10, 130, 19),   # rows cross 64 and 128
         (37, 23, 37, 23))    # equal sizes


def _cases():
    out = []
    for w, h, W, H in SIZES:
        for taps in (2, 4):
            for flag in (0, 1):
                out.append(("%dx%d_to_%dx%d_t%d_f%d" % (w, h, W, H, taps, flag), w, h, W, H, dict(taps=taps, flags=flag), 3000 + 7 * W + H + 13 * w + taps, False))
    for k, name in enumerate(("sigma_normal", "sigma_depth", "sigma_albedo")):
        out.append(("29x17_to_58x34_t%d_f%d_%s_inf" % (4 - 2 * (k & 1), k & 1, name), 29, 17, 58, 34, {"taps": 4 - 2 * (k & 1), "flags": k & 1, name: INF}, 700 + k, False))
    out.append(("29x17_to_58x34_t4_f1_badguides", 29, 17, 58, 34, dict(taps=4, flags=1), 77, True))
    out.append(("29x17_to_58x34_t2_f0_badguides", 29, 17, 58, 34, dict(taps=2, flags=0), 78, True))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]
bits = DC.bits
assert_same = DC.assert_same


def low_guides(rng, g_hi, w, h, bad=False):
    """(h, w, 8): g_hi at the pixel nearest to each low pixel's centre, plus noise."""
    H, W = g_hi.shape[:2]
    cx = np.clip(np.floor((np.arange(w) + 0.5) * W / w).astype(np.int64), 0, W - 1)
    cy = np.clip(np.floor((np.arange(h) + 0.5) * H / h).astype(np.int64), 0, H - 1)
    g = np.array(g_hi[cy][:, cx], F32)
    g[..., 0:3] += (rng.uniform(0.0, 0.02, (h, w, 3)) * (g[..., 0:3] > 0)).astype(F32)
    g[..., 4:7] += (rng.standard_normal((h, w, 3)) * 0.02).astype(F32)
    g[..., 7] *= (1.0 + rng.uniform(-0.02, 0.02, (h, w))).astype(F32)
    if bad:
        for k in range(4):
            g[rng.integers(h), rng.integers(w), 7] = INF
            g[rng.integers(h), rng.integers(w), 4 + k % 3] = np.nan
    return g


def frame(w, h, W, H, seed, bad=False):
    """(rgb_lo (h, w, 3), aov_lo (h, w, 8), aov_hi (H, W, 8)) float32, read-only."""
    rng = np.random.default_rng(seed)
    g_hi = np.array(DC.guides(rng, W, H, bad), F32)
    g_lo = low_guides(rng, g_hi, w, h, bad)
    rgb = (np.nan_to_num(g_lo[..., 0:3], nan=0.5, posinf=1.0) * rng.uniform(0.5, 3.0) + rng.standard_normal((h, w, 3)) * 0.8).astype(F32)  # noise of the signal's size: negatives
    n = w * h * 3
    flat = rgb.reshape(-1)
    specials = [np.nan, INF, -INF, 0.0, -0.0, -2.5]
    idx = rng.permutation(n)[:max(len(specials), n // 12)] if n >= len(specials) else np.arange(n)
    for j, i in enumerate(idx):
        flat[i] = specials[j % len(specials)]
    for a in (rgb, g_lo, g_hi):
        a.setflags(write=False)
    return rgb, g_lo, g_hi


_ref = {}
BRANCHES = {}  # id -> {"guided": pixels, "fallback": pixels} of step 5, filled by reference()


def case(cid):
    return CASES[IDS.index(cid)]


def inputs(cid):
    _, w, h, W, H, _, seed, bad = case(cid)
    return frame(w, h, W, H, seed, bad)


def reference(cid):
    """upsample_ref's (out, rgba8) of a case, computed once per session and handed out read-only."""
    if cid not in _ref:
        rgb, g_lo, g_hi = inputs(cid)
        BRANCHES[cid] = {}
        out, rgba = upsample_ref.upsample(rgb, g_lo, g_hi, branches=BRANCHES[cid], **case(cid)[5])
        out.setflags(write=False)
        rgba.setflags(write=False)
        _ref[cid] = (out, rgba)
    return _ref[cid]


def params(B, cid):
    return B.upsample_default_params(**case(cid)[5])
