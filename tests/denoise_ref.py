"""The denoiser (pt_denoise, include/mi355pt.h "denoiser") restated in numpy float32: one IEEE operation per numpy operation, nothing
contracted, aov_ref.fma32 for every fma and the oracle's dm("exp") for exp_.  Nothing here imports the library under test.

The frame is filtered whole: every tap (dx, dy) of an iteration is one shifted view of the records, and a pixel whose tap is skipped
(outside the frame, or !(w > 0)) keeps its sums untouched, which is what "skipped" means in the definition."""
import numpy as np

import oracle as orc
from aov_ref import fma32

F32 = np.float32
K = (F32(0.375), F32(0.25), F32(0.0625))
DEFAULTS = dict(iterations=5, flags=0, sigma_color=4.0, sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=0.2)


def max_(a, b):
    """pt_device.h max_: (b != b || a > b) ? a : b"""
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    return np.where((b != b) | (a > b), a, b).astype(F32)


def dot3(a, b):
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def exp_(x):
    x = np.ascontiguousarray(x, F32)
    return orc.dm("exp", x.reshape(-1)).reshape(x.shape)


def host_constants(p):
    one = F32(1.0)
    sn, sa, sc0 = F32(p["sigma_normal"]), F32(p["sigma_albedo"]), F32(p["sigma_color"])
    kn = one / (sn * sn)
    ka = one / (sa * sa)
    kc = []
    for i in range(int(p["iterations"])):
        sc = sc0 * F32(2.0 ** -i)
        kc.append(one / (sc * sc))
    return F32(kn), F32(ka), [F32(k) for k in kc]


def make_rgba(c):
    """pt_device.h make_rgba: min(255, max(0, int(f * 256))) per channel (NaN -> 0), alpha 255"""
    s = (np.asarray(c, F32) * F32(256.0)).astype(F32)
    s = np.where(s != s, F32(0.0), s)
    q = np.clip(np.trunc(np.clip(s.astype(np.float64), -2147483647.0, 2147483647.0)), 0, 255).astype(np.uint32)
    return (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(0xFF000000)).astype(np.uint32)


def denoise(rgb, aov, **params):
    """rgb (H, W, 3), aov (H, W, 8) float32 in framebuffer order -> (out (H, W, 3) float32, rgba8 (H, W) uint32)."""
    p = dict(DEFAULTS, **params)
    rgb = np.asarray(rgb, F32)
    aov = np.asarray(aov, F32)
    H, W = rgb.shape[:2]
    dm = bool(int(p["flags"]) & 1)
    with np.errstate(all="ignore"):
        a, n, z = aov[..., 0:3], aov[..., 4:7], aov[..., 7]
        c = np.where(np.isfinite(rgb), rgb, F32(0.0)).astype(F32)
        d = max_(a, F32(1e-3)) if dm else np.ones_like(a)
        if dm:
            c = (c / d).astype(F32)
        sd = F32(p["sigma_depth"]) * max_(z, F32(1e-6))
        kz = (F32(1.0) / (sd * sd)).astype(F32)
        kn, ka, kc = host_constants(p)
        ys, xs = np.mgrid[0:H, 0:W]
        for i in range(int(p["iterations"])):
            s = 1 << i
            acc = np.zeros((H, W, 3), F32)
            wsum = np.zeros((H, W), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    h = K[abs(dx)] * K[abs(dy)]
                    cq = c[qy, qx]
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), h, F32)
                        take = inside
                    else:
                        dc, dn, da = cq - c, n[qy, qx] - n, a[qy, qx] - a
                        ec, en, ea = dot3(dc, dc), dot3(dn, dn), dot3(da, da)
                        dz = z[qy, qx] - z
                        ez = dz * dz
                        e = fma32(ea, ka, fma32(ez, kz, fma32(en, kn, ec * kc[i])))
                        w = (h * exp_(-e)).astype(F32)
                        take = inside & (w > 0)
                    acc = np.where(take[..., None], fma32(w[..., None], cq, acc), acc).astype(F32)
                    wsum = np.where(take, wsum + w, wsum).astype(F32)
            c = (acc / wsum[..., None]).astype(F32)
        out = (c * d).astype(F32) if dm else c
    return np.ascontiguousarray(out, F32), make_rgba(out)
