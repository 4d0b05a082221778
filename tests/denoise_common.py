"""Frames and cases shared by tests/test_denoise_host.py (CPU) and tests/test_gpu_denoise.py (GPU): the denoiser (pt_denoise).

A CASE is (id, W, H, params, seed, bad_guides): params are fields of pt_denoise_params that differ from the defaults.  Every frame is
seeded noise over piecewise-constant guides (a few "surfaces" cut by random lines: normals, depths and albedos repeat across the frame,
so taps of every weight from 0 to 1 occur), in framebuffer order as the library's own frames are:
  * colour: NaN, +Inf, -Inf, negatives and exact zeros among values of a few units;
  * albedo: exact zeros (the demodulation's clamp) among values in 0..1;
  * bad_guides: a +Inf depth and a NaN normal in a few pixels."""
import numpy as np

import denoise_ref

F32 = np.float32
INF = float("inf")


def _cases():
    out = []
    for W, H, Ls in ((1, 1, (3,)), (3, 2, (3,)), (9, 1, (4,)), (1, 9, (4,)),  # smaller than the kernel
                     (37, 23, (1, 5, 8)),                                      # taps reach past the frame at the large steps
                     (70, 45, (3,)), (130, 19, (2,))):                         # no plausible tile divides them; rows cross 64 and 128
        for L in Ls:
            for flag in (0, 1):
                out.append(("%dx%d_L%d_f%d" % (W, H, L, flag), W, H, dict(iterations=L, flags=flag), 1000 + 7 * W + H + L, False))
    out.append(("37x23_L5_f1_badguides", 37, 23, dict(iterations=5, flags=1), 77, True))
    for k, name in enumerate(("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo")):
        out.append(("29x17_L3_f%d_%s_inf" % (k & 1, name), 29, 17, {"iterations": 3, "flags": k & 1, name: INF}, 500 + k, False))
    return out


CASES = _cases()
IDS = [c[0] for c in CASES]


def guides(rng, W, H, bad=False):
    """(H, W, 8) guide buffers: 5 surfaces (albedo, unit normal, depth plane) behind random lines."""
    ys, xs = np.mgrid[0:H, 0:W]
    label = np.zeros((H, W), np.int64)
    for k in range(4):
        ax, ay, b = rng.standard_normal(3)
        label += (ax * (xs - W / 2.0) + ay * (ys - H / 2.0) + b * 3.0 > 0).astype(np.int64) << k
    label %= 5
    nrm = rng.standard_normal((5, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    alb = rng.uniform(0.05, 1.0, (5, 3))
    alb[1, 1] = 0.0  # a surface with an albedo channel of exactly 0
    alb[3] = 0.0     # and a black one
    z0, zx, zy = rng.uniform(1.0, 6.0, 5), rng.uniform(-0.02, 0.02, 5), rng.uniform(-0.02, 0.02, 5)
    g = np.zeros((H, W, 8), F32)
    g[..., 0:3] = alb[label] + rng.uniform(0.0, 0.02, (H, W, 3)) * (alb[label] > 0)
    g[..., 3] = 1.0
    g[..., 4:7] = nrm[label] + rng.standard_normal((H, W, 3)) * 0.02
    g[..., 7] = z0[label] + zx[label] * xs + zy[label] * ys
    if bad:
        for k in range(6):
            g[rng.integers(H), rng.integers(W), 7] = INF
            g[rng.integers(H), rng.integers(W), 4 + k % 3] = np.nan
    return g


def frame(W, H, seed, bad=False):
    """(rgb (H, W, 3), aov (H, W, 8)) float32, read-only."""
    rng = np.random.default_rng(seed)
    g = guides(rng, W, H, bad)
    rgb = (g[..., 0:3] * rng.uniform(0.5, 3.0) + rng.standard_normal((H, W, 3)) * 0.8).astype(F32)  # noise of the signal's size: negatives
    n = W * H * 3
    flat = rgb.reshape(-1)
    specials = [np.nan, INF, -INF, 0.0, -0.0, -2.5]
    idx = rng.permutation(n)[:max(len(specials), n // 12)] if n >= len(specials) else np.arange(n)
    for j, i in enumerate(idx):
        flat[i] = specials[j % len(specials)]
    rgb.setflags(write=False)
    g.setflags(write=False)
    return rgb, g


_ref = {}


def case(cid):
    return CASES[IDS.index(cid)]


def inputs(cid):
    _, W, H, _, seed, bad = case(cid)
    return frame(W, H, seed, bad)


def reference(cid):
    """denoise_ref's (out, rgba8) of a case, computed once per session and handed out read-only."""
    if cid not in _ref:
        rgb, aov = inputs(cid)
        out, rgba = denoise_ref.denoise(rgb, aov, **case(cid)[3])
        out.setflags(write=False)
        rgba.setflags(write=False)
        _ref[cid] = (out, rgba)
    return _ref[cid]


def params(B, cid):
    return B.denoise_default_params(**case(cid)[3])


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d floats differ in bits; first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, i, np.asarray(got)[i], np.asarray(want)[i]))
