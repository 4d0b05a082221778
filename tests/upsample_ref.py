"""The upsampling (pt_upsample, include/mi355pt.h "upsampling") restated in numpy float32: one IEEE operation per numpy operation,
nothing contracted, aov_ref.fma32 for every fma and the oracle's dm("exp") for exp_.  Nothing here imports the library under test.

The high frame is computed whole: every tap (i, j) of the window is one gather of the low records, and a pixel whose tap is skipped keeps
its sums untouched, which is what "skipped" means in the definition.  `branches` reports how many pixels took each side of step 5."""
import numpy as np

from aov_ref import fma32
from denoise_ref import F32, dot3, exp_, make_rgba, max_

DEFAULTS = dict(taps=4, flags=1, sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=0.2, reserved=0)


def host_constants(p, w, h, W, H):
    one = F32(1.0)
    rx = F32(w) / F32(W)
    ry = F32(h) / F32(H)
    sn, sa = F32(p["sigma_normal"]), F32(p["sigma_albedo"])
    kn = one / (sn * sn)
    ka = one / (sa * sa)
    R = int(p["taps"]) // 2
    ir = one / F32(R)
    return F32(rx), F32(ry), F32(kn), F32(ka), R, F32(ir)


def upsample(rgb_lo, aov_lo, aov_hi, branches=None, **params):
    """rgb_lo (h, w, 3), aov_lo (h, w, 8), aov_hi (H, W, 8) float32 in framebuffer order -> (out (H, W, 3) float32, rgba8 (H, W) uint32)."""
    p = dict(DEFAULTS, **params)
    rgb_lo = np.asarray(rgb_lo, F32)
    aov_lo = np.asarray(aov_lo, F32)
    aov_hi = np.asarray(aov_hi, F32)
    h, w = rgb_lo.shape[:2]
    H, W = aov_hi.shape[:2]
    dm = bool(int(p["flags"]) & 1)
    with np.errstate(all="ignore"):
        rx, ry, kn, ka, R, ir = host_constants(p, w, h, W, H)
        # prepare
        a, n, z = aov_lo[..., 0:3], aov_lo[..., 4:7], aov_lo[..., 7]
        c = np.where(np.isfinite(rgb_lo), rgb_lo, F32(0.0)).astype(F32)
        if dm:
            c = (c / max_(a, F32(1e-3))).astype(F32)
        # per high pixel
        a_p, n_p, z_p = aov_hi[..., 0:3], aov_hi[..., 4:7], aov_hi[..., 7]
        sd = F32(p["sigma_depth"]) * max_(z_p, F32(1e-6))
        kz = (F32(1.0) / (sd * sd)).astype(F32)
        rows, xs = np.mgrid[0:H, 0:W]
        fx = ((xs.astype(F32) + F32(0.5)) * rx - F32(0.5)).astype(F32)
        fy = ((rows.astype(F32) + F32(0.5)) * ry - F32(0.5)).astype(F32)
        x0f, y0f = np.floor(fx).astype(F32), np.floor(fy).astype(F32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tx, ty = (fx - x0f).astype(F32), (fy - y0f).astype(F32)
        acc = np.zeros((H, W, 3), F32)
        pacc = np.zeros((H, W, 3), F32)
        wsum = np.zeros((H, W), F32)
        pw = np.zeros((H, W), F32)
        for j in range(1 - R, R + 1):
            for i in range(1 - R, R + 1):
                qx, qy = x0 + i, y0 + j
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                bx = (F32(1.0) - np.abs(F32(i) - tx) * ir).astype(F32)
                by = (F32(1.0) - np.abs(F32(j) - ty) * ir).astype(F32)
                take = inside & (bx > 0) & (by > 0)
                b = (bx * by).astype(F32)
                cq = c[qy, qx]
                pacc = np.where(take[..., None], fma32(b[..., None], cq, pacc), pacc).astype(F32)
                pw = np.where(take, pw + b, pw).astype(F32)
                dn, da = n[qy, qx] - n_p, a[qy, qx] - a_p
                en, ea = dot3(dn, dn), dot3(da, da)
                dz = z[qy, qx] - z_p
                ez = dz * dz
                e = fma32(ea, ka, fma32(ez, kz, en * kn))
                wt = (b * exp_(-e)).astype(F32)
                take = take & (wt > 0)
                acc = np.where(take[..., None], fma32(wt[..., None], cq, acc), acc).astype(F32)
                wsum = np.where(take, wsum + wt, wsum).astype(F32)
        guided = wsum >= F32(1e-4) * pw
        v = np.where(guided[..., None], acc / wsum[..., None], pacc / pw[..., None]).astype(F32)
        out = (v * max_(a_p, F32(1e-3))).astype(F32) if dm else v
    if branches is not None:
        branches["guided"] = branches.get("guided", 0) + int(guided.sum())
        branches["fallback"] = branches.get("fallback", 0) + int((~guided).sum())
    return np.ascontiguousarray(out, F32), make_rgba(out)
