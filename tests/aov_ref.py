"""The guide pass (pt_render_aov, include/mi355pt.h "guide pass") restated in numpy from the oracle's exposed building blocks only:
rng_init / rng_next, dm("sqrt") / dm("div"), Scene.intersect_n(..., use_bvh=False) with the scene's watertight switch, tex_nearest and
uv_on_sphere.  Everything else is float32 numpy arithmetic (one IEEE operation per numpy operation, nothing contracted) and fma32 below.
Nothing here imports the library under test.

Python 3.10 has no math.fma: fma32(a, b, c) forms the product in float64 (exact: 24 + 24 bits), adds in float64 and rounds to float32;
the double rounding can only go wrong where the float64 sum sits exactly on a float32 rounding tie, and there the exact value decides
(fractions.Fraction).  tests/test_aov_host.py checks fma32 against pure Fraction arithmetic and ties this restatement to the oracle's own
per-bounce log (Scene.trace_sample)."""
from fractions import Fraction

import numpy as np

import oracle as orc

F32 = np.float32
MAT_DEFAULT = orc.MAT_DEFAULT


def round_fraction_to_f32(q):
    """Round-to-nearest-even of an exact rational to float32, by exact comparison with the neighbouring float32 values (the referee of
    fma32; slow).  Finite, non-overflowing q only."""
    q = Fraction(q)
    r = F32(float(q))  # Fraction -> float is correctly rounded to float64; the cast may then be one float32 off: look at the neighbours
    cands = {float(r), float(np.nextafter(r, F32(np.inf))), float(np.nextafter(r, F32(-np.inf)))}
    best = sorted(cands, key=lambda x: (abs(Fraction(x) - q), int(np.array([x], F32).view(np.uint32)[0]) & 1))
    return F32(best[0])


def fma32(a, b, c):
    """round32(a * b + c) with ONE rounding, elementwise on float32 arrays (finite operands, results in the normal range)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    s = p + c.astype(np.float64)                     # one float64 rounding
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(F32)                            # a second rounding: wrong only if s is a float32 tie that the exact sum is not
        d = s - r.astype(np.float64)                 # exact
        toward = np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32)
        nb = np.nextafter(r, toward)
        tie = (d != 0) & np.isfinite(s) & (2.0 * d == (nb.astype(np.float64) - r.astype(np.float64)))
        if tie.any():
            # s is then the midpoint of r and nb, so the exact sum lies on the side of s that the float64 addition's own error points
            # to: e of Knuth's TwoSum, p + c = s + e exactly (p, c, s finite).  e == 0 is a true tie: numpy's ties-to-even of s stands.
            t = s - p
            e = (p - (s - t)) + (c.astype(np.float64) - t)
            lo, hi = np.minimum(r, nb), np.maximum(r, nb)
            r = np.where(tie & (e < 0), lo, np.where(tie & (e > 0), hi, r)).astype(F32)
    return r


def dot3(a, b):
    """pt_device.h dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))"""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def normalize3(a):
    """a * (1 / sqrt(dot(a, a)))"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = orc.dm("div", np.ones(a.shape[:-1], F32), orc.dm("sqrt", dot3(a, a))).reshape(a.shape[:-1])
        return a * inv[..., None]


def interp3(bw, bx, by, a, b, c):
    """(1-u-v) a + u b + v c as the fma chain of the hit shader: fma(by, c, fma(bx, b, bw * a)), per component"""
    return fma32(by[..., None], c, fma32(bx[..., None], b, bw[..., None] * a))


def camera_rays(cam, W, H, n_samples, pixel_ids):
    """Rays of the guide pass: (n_pixels, n_samples, 6) float32 = origin, direction.  cam: 12 floats (origin, llc, horizontal, vertical)."""
    cam = np.asarray(cam, F32).reshape(4, 3)
    origin, llc, hor, ver = cam
    ids = np.asarray(pixel_ids, np.int64)
    px, py = ids % W, ids // W
    rx = np.zeros((ids.size, n_samples), F32)
    ry = np.zeros((ids.size, n_samples), F32)
    for i in range(ids.size):
        st = orc.rng_init(int(px[i]), int(py[i]))
        for k in range(n_samples):
            rx[i, k], st = orc.rng_next(st)
            ry[i, k], st = orc.rng_next(st)
    su = orc.dm("div", px.astype(F32)[:, None] + rx, F32(W)).reshape(rx.shape)
    sv = orc.dm("div", py.astype(F32)[:, None] + ry, F32(H)).reshape(ry.shape)
    d = ((llc + hor * su[..., None]) + ver * sv[..., None]) - origin
    d = normalize3(d.astype(F32))
    rays = np.empty((ids.size, n_samples, 6), F32)
    rays[..., :3] = origin
    rays[..., 3:] = d
    return rays


def miss_albedo(env, d):
    """The miss shader: env = dict(use_map, use_auto, color, intensity, env_map) as B.make_env / orc.make_env take it; d: (n, 3)."""
    n = d.shape[0]
    rad = np.zeros((n, 3), F32)
    env_map = env.get("env_map")
    if env.get("use_map") and env_map is not None and env_map.shape[1] > 0:
        for i in range(n):
            u, v = orc.uv_on_sphere(d[i])
            rad[i] = rad[i] + orc.tex_nearest(env_map, float(u), float(v))
    elif env.get("use_auto"):
        t = F32(0.5) * (d[:, 1] + F32(1.0))
        a, b = np.ones(3, F32), np.array([0.5, 0.7, 1.0], F32)
        rad = rad + fma32((b - a)[None, :], t[:, None], a[None, :])  # lerpf(a, b, t) = fma(b - a, t, a)
    else:
        rad = rad + np.asarray(env.get("color", (0, 0, 0)), F32)[None, :]
    return rad * F32(env.get("intensity", 0.0))


def samples(S, flat, env, cam, W, H, n_samples, pixel_ids, materials=None):
    """Every sample's contribution and hit: dict(contrib (n_pixels, n_samples, 8), rays, hit, t, u, v, prim).  S: orc.Scene(flat) with its
    watertight switch set as wanted; materials: the current table if not flat's."""
    rays = camera_rays(cam, W, H, n_samples, pixel_ids)
    flat_rays = rays.reshape(-1, 6)
    hit, t, u, v, prim = S.intersect_n(flat_rays, use_bvh=False)
    n = flat_rays.shape[0]
    out = np.zeros((n, 8), F32)
    miss = ~hit
    if miss.any():
        out[miss, :3] = miss_albedo(env, flat_rays[miss, 3:])
    if hit.any():
        p = prim[hit]
        bx, by = u[hit], v[hit]
        bw = F32(1.0) - bx - by
        nrm = np.asarray(flat["normals"], F32).reshape(-1, 3, 3)[p]
        with np.errstate(invalid="ignore", divide="ignore"):
            vn = normalize3(interp3(bw, bx, by, nrm[:, 0], nrm[:, 1], nrm[:, 2]))
        vn = np.where(np.isfinite(vn).all(-1, keepdims=True), vn, F32(0.0)).astype(F32)
        mats = np.asarray(flat["materials"] if materials is None else materials, F32).reshape(-1, orc.MAT_FLOATS)
        mi = np.asarray(flat["material_index"], np.int32)[p]
        m = np.where((mi >= 0)[:, None], mats[np.maximum(mi, 0)], MAT_DEFAULT[None, :]).astype(F32)
        alb = m[:, :3].copy()
        ti = np.where(mi >= 0, np.asarray(flat["texture_index"], np.int32)[p], -1)
        if (ti >= 0).any():
            tc = np.asarray(flat["texcoords"], F32).reshape(-1, 3, 2)[p]
            tu = fma32(by, tc[:, 2, 0], fma32(bx, tc[:, 1, 0], bw * tc[:, 0, 0]))
            tv = fma32(by, tc[:, 2, 1], fma32(bx, tc[:, 1, 1], bw * tc[:, 0, 1]))
            for i in np.nonzero(ti >= 0)[0]:
                alb[i] = orc.tex_nearest(flat["textures"][int(ti[i])], float(tu[i]), float(tv[i]))
        emit = m[:, 16] > 0
        alb[emit] = m[emit, 16:17]
        h = np.zeros((p.size, 8), F32)
        h[:, :3], h[:, 3], h[:, 4:7], h[:, 7] = alb, F32(1.0), vn, t[hit]
        out[hit] = h
    shape = rays.shape[:2]
    return dict(contrib=out.reshape(shape + (8,)), rays=rays, hit=hit.reshape(shape), t=t.reshape(shape), u=u.reshape(shape), v=v.reshape(shape),
                prim=prim.reshape(shape))


def aov(S, flat, env, cam, W, H, n_samples, pixel_ids=None, materials=None):
    """The guide buffers: (n_pixels, 8) float32 in list order, or with pixel_ids None the whole frame as (H, W, 8) in framebuffer order
    (row 0 = y = H-1), as Context.render_aov returns it."""
    whole = pixel_ids is None
    ids = np.arange(W * H) if whole else np.asarray(pixel_ids)
    c = samples(S, flat, env, cam, W, H, n_samples, ids, materials)["contrib"]
    acc = np.zeros((ids.size, 8), F32)
    for k in range(n_samples):  # float32, in sample order from 0
        acc = acc + c[:, k]
    out = acc * orc.dm("div", F32(1.0), F32(n_samples))[0]
    return out.reshape(H, W, 8)[::-1].copy() if whole else out
