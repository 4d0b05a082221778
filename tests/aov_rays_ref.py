"""The guide pass over a ray image (pt_render_aov_rays, include/mi355pt.h "ray images") restated in numpy, in the style of
tests/aov_follow_ref.py and from its helpers and those of tests/aov_ref.py: the oracle's exposed building blocks only - rng_init /
rng_next, dm("sqrt") / dm("div"), Scene.intersect_n(..., use_bvh=False) with the scene's watertight switch, tex_nearest and uv_on_sphere
(through aov_ref.miss_albedo) - float32 numpy arithmetic, one IEEE operation per numpy operation, and aov_ref.fma32 for every fma.  Nothing
here imports the library under test.

The definition is pt_render_aov_follow's with one substitution, and so is this file: table_rays is the ray generator of the ray image (the
stream and the two draws of aov_ref.camera_rays, then the record's ray), and the rounds behind it are aov_follow_ref.samples' rounds, all
samples advancing together, one surface per round."""
import numpy as np

import aov_ref
import oracle as orc
from aov_follow_ref import EMISSION, GLASS, IOR, NONE, classify, reflect, refract
from aov_ref import F32, dot3, fma32, interp3, normalize3


def table_rays(table, W, H, n_samples, pixel_ids):
    """Rays of the guide pass over the ray image `table` (W * H records with fields org, dir, du, dv; the record of pixel (x, y) at
    x + W * y): (n_pixels, n_samples, 6) float32 = origin, direction.  Per sample rx = rng_next, then ry = rng_next of the stream
    rng_init(x, y) - drawn whatever du and dv are - and the direction normalize((dir + du * rx) + dv * ry)."""
    table = np.asarray(table).reshape(-1)
    assert table.shape[0] == W * H
    ids = np.asarray(pixel_ids, np.int64)
    px, py = ids % W, ids // W
    rx = np.zeros((ids.size, n_samples), F32)
    ry = np.zeros((ids.size, n_samples), F32)
    for i in range(ids.size):
        st = orc.rng_init(int(px[i]), int(py[i]))
        for k in range(n_samples):
            rx[i, k], st = orc.rng_next(st)
            ry[i, k], st = orc.rng_next(st)
    rec = table[px + W * py]
    org, d0, du, dv = (np.ascontiguousarray(rec[f], F32)[:, None, :] for f in ("org", "dir", "du", "dv"))
    d = (d0 + du * rx[..., None]) + dv * ry[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = normalize3(d.astype(F32))
    rays = np.empty((ids.size, n_samples, 6), F32)
    rays[..., :3] = org
    rays[..., 3:] = d
    return rays


def samples(S, flat, env, table, W, H, n_samples, max_follow, roughness_max, pixel_ids, materials=None):
    """dict(contrib (n_pixels, n_samples, 8), rays0 (n_pixels, n_samples, 6): the camera rays, hit0 / t0 / prim0 (n_pixels, n_samples):
    what they hit)."""
    rays0 = table_rays(table, W, H, n_samples, pixel_ids)
    shape = rays0.shape[:2]
    n = shape[0] * shape[1]
    o, d = rays0.reshape(-1, 6)[:, :3].copy(), rays0.reshape(-1, 6)[:, 3:].copy()
    tint = np.ones((n, 3), F32)
    dist = np.zeros(n, F32)
    out = np.zeros((n, 8), F32)
    active = np.arange(n)
    pos = np.asarray(flat["positions"], F32).reshape(-1, 3, 3)
    nrms = np.asarray(flat["normals"], F32).reshape(-1, 3, 3)
    mats = np.asarray(flat["materials"] if materials is None else materials, F32).reshape(-1, orc.MAT_FLOATS)
    first = None
    step = 0
    while active.size:
        rays = np.concatenate([o[active], d[active]], 1).astype(F32)
        hit, t, u, v, prim = S.intersect_n(rays, use_bvh=False)
        if step == 0:
            first = (hit.copy(), t.copy(), prim.copy())
            out[active, 3] = np.where(hit, F32(1.0), F32(0.0))  # coverage stays first-hit
        mi_ = active[~hit]
        if mi_.size:
            out[mi_, :3] = tint[mi_] * aov_ref.miss_albedo(env, d[mi_])
            out[mi_, 4:7] = F32(0.0)
            out[mi_, 7] = dist[mi_]
        a = active[hit]
        if a.size == 0:
            break
        p, bx, by = prim[hit], u[hit], v[hit]
        dist[a] = dist[a] + t[hit]  # float32, in step order
        bw = F32(1.0) - bx - by
        with np.errstate(invalid="ignore", divide="ignore"):
            vn = normalize3(interp3(bw, bx, by, nrms[p, 0], nrms[p, 1], nrms[p, 2]))
        n_ok = np.isfinite(vn).all(-1)
        mi = np.asarray(flat["material_index"], np.int32)[p]
        m = np.where((mi >= 0)[:, None], mats[np.maximum(mi, 0)], aov_ref.MAT_DEFAULT[None, :]).astype(F32)
        with np.errstate(invalid="ignore"):
            emits = m[:, EMISSION] > 0
        base = m[:, :3].copy()
        ti = np.where(mi >= 0, np.asarray(flat["texture_index"], np.int32)[p], -1)
        look = (ti >= 0) & ~emits
        if look.any():
            tc = np.asarray(flat["texcoords"], F32).reshape(-1, 3, 2)[p]
            tu = fma32(by, tc[:, 2, 0], fma32(bx, tc[:, 1, 0], bw * tc[:, 0, 0]))
            tv = fma32(by, tc[:, 2, 1], fma32(bx, tc[:, 1, 1], bw * tc[:, 0, 1]))
            for i in np.nonzero(look)[0]:
                base[i] = orc.tex_nearest(flat["textures"][int(ti[i])], float(tu[i]), float(tv[i]))
        kind = np.where(emits | (step == max_follow) | ~n_ok, NONE, classify(m, roughness_max))
        wo = -d[a]
        wi = np.zeros((a.size, 3), F32)
        t2 = tint[a] * base
        through = np.zeros(a.size, bool)
        g = kind == GLASS
        if g.any():
            with np.errstate(invalid="ignore", divide="ignore"):
                ct = dot3(wo[g], vn[g])
                front = ct > 0
                ior = m[g, IOR]
                eta = np.where(front, orc.dm("div", np.ones(ior.size, F32), ior).reshape(ior.shape), ior).astype(F32)
                ok, w_t = refract(wo[g], np.where(front[:, None], vn[g], -vn[g]).astype(F32), eta)
            through[g] = ok
            wi[np.nonzero(g)[0][ok]] = w_t[ok]
        if through.any():
            with np.errstate(invalid="ignore"):
                t2[through] = tint[a][through] * orc.dm("sqrt", base[through].reshape(-1)).reshape(-1, 3)
        refl = (kind != NONE) & ~through
        if refl.any():
            wi[refl] = reflect(wo[refl], vn[refl])  # a mirror, or total internal reflection
        with np.errstate(invalid="ignore", divide="ignore"):
            dn = normalize3(wi)
        go = (kind != NONE) & np.isfinite(dn).all(-1)
        stop = ~go
        if stop.any():
            s_ = a[stop]
            out[s_, :3] = tint[s_] * np.where(emits[stop, None], m[stop, EMISSION:EMISSION + 1], base[stop])
            out[s_, 4:7] = np.where(n_ok[stop, None], vn[stop], F32(0.0))
            out[s_, 7] = dist[s_]
        if go.any():
            g_ = a[go]
            pg = p[go]
            o[g_] = interp3(bw[go], bx[go], by[go], pos[pg, 0], pos[pg, 1], pos[pg, 2])  # the hit shader's hit point, no normal offset
            d[g_] = dn[go]
            tint[g_] = t2[go]
        active = a[go]
        step += 1
    return dict(contrib=out.reshape(shape + (8,)), rays0=rays0, hit0=first[0].reshape(shape), t0=first[1].reshape(shape), prim0=first[2].reshape(shape))


def aov(S, flat, env, table, W, H, n_samples, max_follow, roughness_max, pixel_ids=None, materials=None, want_samples=False):
    """The guide buffers of the ray image: (n_pixels, 8) float32 in list order, or with pixel_ids None the whole frame as (H, W, 8) in
    framebuffer order (row 0 = y = H-1), as Context.render_aov_rays returns it."""
    whole = pixel_ids is None
    ids = np.arange(W * H) if whole else np.asarray(pixel_ids)
    r = samples(S, flat, env, table, W, H, n_samples, max_follow, roughness_max, ids, materials)
    c = r["contrib"]
    acc = np.zeros((ids.size, 8), F32)
    for k in range(n_samples):  # float32, in sample order from 0
        acc = acc + c[:, k]
    out = acc * orc.dm("div", F32(1.0), F32(n_samples))[0]
    out = out.reshape(H, W, 8)[::-1].copy() if whole else out
    return (out, r) if want_samples else out
