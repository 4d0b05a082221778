"""The variance-guided denoiser (pt_denoise_var, pt_accum_variance; include/mi355pt.h "variance-guided denoise") restated in numpy
float32, in the style of denoise_ref.py: one IEEE operation per numpy operation, nothing contracted, aov_ref.fma32 for every fma and the
oracle's dm("exp") for exp_.  Nothing here imports the library under test.

accum_variance is section 1 of the definition (flat arrays), denoise_var section 2 (a whole frame: every tap is one shifted view, a
skipped tap leaves a pixel's sums untouched)."""
import numpy as np

from aov_ref import fma32
from denoise_ref import K, dot3, exp_, host_constants, make_rgba, max_

F32 = np.float32
VMAX = F32(1e30)
M = (F32(0.5), F32(0.25))
DEFAULTS = dict(iterations=5, flags=0, sigma_color=3.0, sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=0.2)


def min_(a, b):
    """pt_device.h min_: (b != b || a < b) ? a : b"""
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    return np.where((b != b) | (a < b), a, b).astype(F32)


def accum_variance(sum_, half, n, n_half, owned):
    """sum, half (N, 3) float32; n, n_half (N,) uint32; owned (N,) flags -> (rgb (N, 3), var (N, 3)) float32."""
    s, h = np.asarray(sum_, F32).reshape(-1, 3), np.asarray(half, F32).reshape(-1, 3)
    n, nh, own = np.asarray(n, np.uint32).ravel(), np.asarray(n_half, np.uint32).ravel(), np.asarray(owned).ravel() != 0
    one = F32(1.0)
    with np.errstate(all="ignore"):
        nf, nhf, restf = n.astype(F32), nh.astype(F32), (n - nh).astype(F32)  # (uint32 arithmetic wraps as the C expression does)
        rgb = np.where((n >= 1)[:, None], s * (one / nf)[:, None], F32(0.0)).astype(F32)
        ia, ib = (one / nhf).astype(F32), (one / restf).astype(F32)
        fh = (nhf / nf).astype(F32)
        r = (fh * (one - fh)).astype(F32)
        a, b = (h * ia[:, None]).astype(F32), ((s - h) * ib[:, None]).astype(F32)
        e = (a - b).astype(F32)
        var = (r[:, None] * (e * e)).astype(F32)
        var = np.where(var <= VMAX, var, VMAX).astype(F32)
        var = np.where((nh == 0)[:, None], VMAX, var).astype(F32)
    zero = np.zeros_like(rgb)
    return np.where(own[:, None], rgb, zero).astype(F32), np.where(own[:, None], var, zero).astype(F32)


def denoise_var(rgb, var, aov, **params):
    """rgb, var (H, W, 3), aov (H, W, 8) float32 in framebuffer order -> (out (H, W, 3) float32, rgba8 (H, W) uint32, v_L (H, W) float32)."""
    p = dict(DEFAULTS, **params)
    rgb, var, aov = np.asarray(rgb, F32), np.asarray(var, F32), np.asarray(aov, F32)
    H, W = rgb.shape[:2]
    dm = bool(int(p["flags"]) & 1)
    with np.errstate(all="ignore"):
        a, n, z = aov[..., 0:3], aov[..., 4:7], aov[..., 7]
        c = np.where(np.isfinite(rgb), rgb, F32(0.0)).astype(F32)
        d = max_(a, F32(1e-3)) if dm else np.ones_like(a)
        vk = var
        if dm:
            c = (c / d).astype(F32)
            vk = (var / (d * d).astype(F32)).astype(F32)
        v = ((vk[..., 0] + vk[..., 1]) + vk[..., 2]).astype(F32)
        v = np.where((v >= 0) & (v <= VMAX), v, VMAX).astype(F32)
        sd = F32(p["sigma_depth"]) * max_(z, F32(1e-6))
        kz = (F32(1.0) / (sd * sd)).astype(F32)
        kn, ka, _ = host_constants(p)
        s2 = F32(F32(p["sigma_color"]) * F32(p["sigma_color"]))
        ys, xs = np.mgrid[0:H, 0:W]
        for i in range(int(p["iterations"])):
            s = 1 << i
            gs = np.zeros((H, W), F32)
            gw = np.zeros((H, W), F32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    qy, qx = ys + dy, xs + dx
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    g = M[abs(dx)] * M[abs(dy)]
                    gs = np.where(inside, fma32(np.full((H, W), g, F32), v[qy, qx], gs), gs).astype(F32)
                    gw = np.where(inside, gw + g, gw).astype(F32)
            vb = (gs / gw).astype(F32)
            kc = np.zeros((H, W), F32) if np.isposinf(s2) else (F32(1.0) / fma32(np.full((H, W), s2, F32), vb, np.full((H, W), 1e-10, F32))).astype(F32)
            acc = np.zeros((H, W, 3), F32)
            wsum = np.zeros((H, W), F32)
            vs = np.zeros((H, W), F32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = ys + dy * s, xs + dx * s
                    inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                    qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
                    h = K[abs(dx)] * K[abs(dy)]
                    cq, vq = c[qy, qx], v[qy, qx]
                    if dx == 0 and dy == 0:
                        w = np.full((H, W), h, F32)
                        take = inside
                    else:
                        dc, dn, da = cq - c, n[qy, qx] - n, a[qy, qx] - a
                        ec, en, ea = dot3(dc, dc), dot3(dn, dn), dot3(da, da)
                        dz = z[qy, qx] - z
                        ez = dz * dz
                        e = fma32(ea, ka, fma32(ez, kz, fma32(en, kn, ec * kc)))
                        w = (h * exp_(-e)).astype(F32)
                        take = inside & (w > 0)
                    acc = np.where(take[..., None], fma32(w[..., None], cq, acc), acc).astype(F32)
                    vs = np.where(take, fma32((w * w).astype(F32), vq, vs), vs).astype(F32)
                    wsum = np.where(take, wsum + w, wsum).astype(F32)
            c = (acc / wsum[..., None]).astype(F32)
            v = min_((vs / (wsum * wsum).astype(F32)).astype(F32), VMAX)
        out = (c * d).astype(F32) if dm else c
    return np.ascontiguousarray(out, F32), make_rgba(out), np.ascontiguousarray(v, F32)
