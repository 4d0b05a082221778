"""The follow mode of the guide pass (pt_render_aov_follow, include/mi355pt.h "guide pass, follow mode") restated in numpy, in the style of
tests/aov_ref.py and from its helpers: the oracle's exposed building blocks only - rng_init / rng_next (through aov_ref.camera_rays),
dm("sqrt") / dm("div"), Scene.intersect_n(..., use_bvh=False) with the scene's watertight switch, tex_nearest and uv_on_sphere (through
aov_ref.miss_albedo) - float32 numpy arithmetic, one IEEE operation per numpy operation, and aov_ref.fma32 for every fma.  Nothing here
imports the library under test.

All samples of a frame advance together, one surface per round; a sample that has stopped keeps its contribution.  samples() also returns
the log the tests read: every ray walked, the triangle it hit, the kind the surface classified as, the segment lengths, and why a sample
stopped where it stopped."""
import numpy as np

import aov_ref
import oracle as orc
from aov_ref import F32, dot3, fma32, interp3, normalize3

NONE, MIRROR, GLASS = 0, 1, 2
# log field "stop", per hit: why the sample ended on this surface (the first reason of the definition's order that applies); WENT_ON: it did not
WENT_ON, STOP_EMITTER, STOP_CAP, STOP_BAD_NORMAL, STOP_CLASSIFIED_NONE, STOP_NON_FINITE_DIRECTION = 0, 1, 2, 3, 4, 5
# material row (orc.MAT_FLOATS floats): base colour 0..2, metallic 4, roughness 7, clearcoat 11, ior 13, specular_transmission 14,
# specular_transmission_roughness 15, emission 16
METALLIC, ROUGHNESS, CLEARCOAT, IOR, SPEC_TRANS, SPEC_TRANS_ROUGHNESS, EMISSION = 4, 7, 11, 13, 14, 15, 16


def classify(m, roughness_max):
    """kind per material row: the lobe weights are the BSDF sampler's expressions; NaN fields fail every comparison"""
    one, rmax = F32(1.0), F32(roughness_max)
    with np.errstate(invalid="ignore"):
        mw = m[:, METALLIC]
        gw = (one - m[:, METALLIC]) * m[:, SPEC_TRANS]
        dw = (one - m[:, SPEC_TRANS]) * (one - m[:, METALLIC])
        cw = F32(0.25) * m[:, CLEARCOAT]
        mirror = (mw > gw) & (mw > dw) & (mw > cw) & (m[:, ROUGHNESS] <= rmax)
        glass = (gw > mw) & (gw > dw) & (gw > cw) & (m[:, SPEC_TRANS_ROUGHNESS] <= rmax)
    return np.where(mirror, MIRROR, np.where(glass, GLASS, NONE))


def reflect(w, n):
    """pt_device.h: (n * dot(w, n)) * 2 - w"""
    return (n * dot3(w, n)[:, None]) * F32(2.0) - w


def refract(w, n, eta):
    """pt_device.h refract: (ok, wi); eta per row"""
    ci = dot3(w, n)
    s = F32(1.0) - ci * ci
    s2i = np.where((s != s) | (F32(0.0) > s), F32(0.0), s).astype(F32)  # max_(0.0f, s)
    s2t = (eta * eta) * s2i
    with np.errstate(invalid="ignore"):
        ok = ~(s2t > F32(1.0))
        ct = orc.dm("sqrt", np.where(ok, F32(1.0) - s2t, F32(0.0)).astype(F32)).reshape(ci.shape)
    wi = (-w) * eta[:, None] + n * (eta * ci - ct)[:, None]
    same = eta == F32(1.0)
    wi = np.where(same[:, None], -w, wi).astype(F32)
    return ok | same, wi


def samples(S, flat, env, cam, W, H, n_samples, max_follow, roughness_max, pixel_ids, materials=None):
    """dict(contrib (n_pixels, n_samples, 8), log): log[step] = dict(idx: flat sample indices walked in this round, rays (k, 6), hit, t, prim,
    kind (of the hit surfaces; -1 on a miss), went_on, tir, stop (a STOP_* reason or WENT_ON; -1 on a miss), mat (the material index of the hit
    triangle, < 0: the defaults; -2 on a miss), tex (the base colour came from a texture lookup), n_ok (the shading normal is finite))."""
    rays0 = aov_ref.camera_rays(cam, W, H, n_samples, pixel_ids)
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
    log = []
    step = 0
    while active.size:
        rays = np.concatenate([o[active], d[active]], 1).astype(F32)
        hit, t, u, v, prim = S.intersect_n(rays, use_bvh=False)
        entry = dict(idx=active.copy(), rays=rays, hit=hit.copy(), t=t.copy(), prim=prim.copy(), kind=np.full(active.size, -1), went_on=np.zeros(active.size, bool),
                     tir=np.zeros(active.size, bool), stop=np.full(active.size, -1), mat=np.full(active.size, -2), tex=np.zeros(active.size, bool),
                     n_ok=np.zeros(active.size, bool))
        log.append(entry)
        if step == 0:
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
        dist[a] = dist[a] + t[hit]
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
        # the rays that go on
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
            wi[refl] = reflect(wo[refl], vn[refl])
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
        hi = np.nonzero(hit)[0]
        entry["kind"][hi] = kind
        entry["went_on"][hi] = go
        entry["tir"][hi] = (kind == GLASS) & ~through & go
        entry["stop"][hi] = np.where(go, WENT_ON, np.where(emits, STOP_EMITTER, np.where(step == max_follow, STOP_CAP, np.where(~n_ok, STOP_BAD_NORMAL, np.where(
            kind == NONE, STOP_CLASSIFIED_NONE, STOP_NON_FINITE_DIRECTION)))))
        entry["mat"][hi] = mi
        entry["tex"][hi] = look
        entry["n_ok"][hi] = n_ok
        active = a[go]
        step += 1
    return dict(contrib=out.reshape(shape + (8,)), log=log, shape=shape)


def aov(S, flat, env, cam, W, H, n_samples, max_follow, roughness_max, pixel_ids=None, materials=None, want_log=False):
    """The follow-mode guide buffers: (n_pixels, 8) float32 in list order, or with pixel_ids None the whole frame as (H, W, 8) in framebuffer
    order (row 0 = y = H-1), as Context.render_aov_follow returns it."""
    whole = pixel_ids is None
    ids = np.arange(W * H) if whole else np.asarray(pixel_ids)
    r = samples(S, flat, env, cam, W, H, n_samples, max_follow, roughness_max, ids, materials)
    c = r["contrib"]
    acc = np.zeros((ids.size, 8), F32)
    for k in range(n_samples):  # float32, in sample order from 0
        acc = acc + c[:, k]
    out = acc * orc.dm("div", F32(1.0), F32(n_samples))[0]
    out = out.reshape(H, W, 8)[::-1].copy() if whole else out
    return (out, r) if want_log else out
