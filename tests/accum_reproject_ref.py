"""numpy restatement of pt_accum_reproject (include/mi355pt.h, "reprojection"), written from the header text alone: float32 throughout, one
rounding per written operation (numpy's float32 +, -, *, / and sqrt are correctly rounded), dot / cross / normalize as csrc/pt_device.h
defines them - through fma32, dot3 and normalize3 of tests/aov_ref.py - and step 7 through resolve of tests/accum_ref.py.  Everything is in
framebuffer order, rows top to bottom: the pixel (px, py) of the definition is row H - 1 - py, column px.  Nothing here imports the library
under test."""
import numpy as np

import accum_ref as AR
from aov_ref import dot3, fma32, normalize3

F32, U32 = np.float32, np.uint32
DEFAULTS = dict(max_history=0, reserved=0, depth_tol=0.05, normal_min=0.9, albedo_tol=0.1)


def cross3(a, b):
    """pt_device.h cross: fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x))"""
    a, b = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32))
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1).astype(F32)


def is_surface(g):
    with np.errstate(invalid="ignore"):
        return (g[..., 3] >= F32(0.5)) & (g[..., 7] > F32(0.0)) & ~np.isinf(g[..., 7])


def sources(old_cam, new_cam, aov_prev, aov_cur, owned=None, depth_tol=0.05, normal_min=0.9, albedo_tol=0.1, **_):
    """Steps 1 to 5 -> (has (H, W) bool, row (H, W), col (H, W)): whether the pixel keeps history, and the framebuffer row and column
    of its source (valid where has)."""
    prev, cur = np.asarray(aov_prev, F32), np.asarray(aov_cur, F32)
    H, W = cur.shape[:2]
    own = np.ones((H, W), bool) if owned is None else np.asarray(owned).reshape(H, W) != 0
    o, llc, hor, ver = np.asarray(new_cam, F32).reshape(4, 3)
    oo, llco, ho, vo = np.asarray(old_cam, F32).reshape(4, 3)
    with np.errstate(all="ignore"):
        # host constants
        a = (llco - oo).astype(F32)
        N = cross3(ho, vo)
        inn = F32(1.0) / dot3(N, N)
        na = dot3(N, a)
        # 1. the ray through the pixel centre
        rows, px = np.mgrid[0:H, 0:W]
        py = H - 1 - rows
        su = ((px.astype(F32) + F32(0.5)) / F32(W)).astype(F32)
        sv = ((py.astype(F32) + F32(0.5)) / F32(H)).astype(F32)
        dc = normalize3((((llc + hor * su[..., None]).astype(F32) + (ver * sv[..., None]).astype(F32)).astype(F32) - o).astype(F32)).astype(F32)
        # 2. surface or sky
        surf = is_surface(cur)
        P = (o + (dc * cur[..., 7:8]).astype(F32)).astype(F32)
        rs = (P - oo).astype(F32)
        ze = np.sqrt(dot3(rs, rs)).astype(F32)
        r = np.where(surf[..., None], rs, dc).astype(F32)
        # 3. projection into the old camera
        dn = dot3(np.broadcast_to(N, r.shape), r)
        lam = (na / dn).astype(F32)
        ok = (lam > 0) & ~np.isinf(lam)
        w = ((r * lam[..., None]).astype(F32) - a).astype(F32)
        Nb = np.broadcast_to(N, w.shape)
        su_o = (dot3(cross3(w, vo), Nb) * inn).astype(F32)
        sv_o = (dot3(cross3(np.broadcast_to(ho, w.shape), w), Nb) * inn).astype(F32)
        fx, fy = (su_o * F32(W)).astype(F32), (sv_o * F32(H)).astype(F32)
        ok &= (fx >= 0) & (fx < F32(W)) & (fy >= 0) & (fy < F32(H))
        qx = np.where(ok, fx, 0).astype(np.int64)
        qy = np.where(ok, fy, 0).astype(np.int64)
        qrow = H - 1 - qy
        # 4. the source is owned (and so is the pixel)
        ok &= own & own[qrow, qx]
        # 5. consistency
        s = prev[qrow, qx]
        ssurf = is_surface(s)
        ok &= ssurf == surf
        depth_ok = np.abs((s[..., 7] - ze).astype(F32)) <= (F32(depth_tol) * ze).astype(F32)
        normal_ok = dot3(cur[..., 4:7], s[..., 4:7]) >= F32(normal_min)
        ok &= ~surf | (depth_ok & normal_ok)
        da = (s[..., 0:3] - cur[..., 0:3]).astype(F32)
        ok &= dot3(da, da) <= (F32(albedo_tol) * F32(albedo_tol)).astype(F32)
    return ok, qrow, qx


def reproject(old_cam, new_cam, aov_prev, aov_cur, state, owned=None, **params):
    """state: dict(sum, half (H, W, 3), n, n_half, passes (H, W)) -> dict(sum, half, n, n_half, passes, rgb, rgba8, noise, has)."""
    prm = dict(DEFAULTS, **params)
    has, qrow, qx = sources(old_cam, new_cam, aov_prev, aov_cur, owned, **prm)
    H, W = has.shape
    own = np.ones((H, W), bool) if owned is None else np.asarray(owned).reshape(H, W) != 0
    take3 = lambda v: np.where(has[..., None], np.asarray(v, F32)[qrow, qx], F32(0.0)).astype(F32)
    take = lambda v: np.where(has, np.asarray(v, U32)[qrow, qx], U32(0)).astype(U32)
    sum_, half, n, n_half, passes = take3(state["sum"]), take3(state["half"]), take(state["n"]), take(state["n_half"]), take(state["passes"])
    mh = int(prm["max_history"])
    if mh:
        cap = n > U32(mh)
        with np.errstate(all="ignore"):
            f = (F32(mh) / n.astype(F32)).astype(F32)
            sum_ = np.where(cap[..., None], (sum_ * f[..., None]).astype(F32), sum_)
            nh = (n_half.astype(np.uint64) * np.uint64(mh) // np.maximum(n, 1).astype(np.uint64)).astype(U32)
            fh = (nh.astype(F32) / n_half.astype(F32)).astype(F32)
            half_c = np.where((nh != 0)[..., None], (half * fh[..., None]).astype(F32), F32(0.0))
        half = np.where(cap[..., None], half_c, half).astype(F32)
        n_half = np.where(cap, nh, n_half).astype(U32)
        n = np.where(cap, U32(mh), n).astype(U32)
    r = AR.resolve(sum_, sum_, half, n, n_half, passes, np.zeros((H, W), np.uint8), own, 1)
    return dict(sum=sum_, half=half, n=n, n_half=n_half, passes=passes, rgb=r["rgb"], rgba8=r["rgba8"], noise=r["noise"], has=has)
