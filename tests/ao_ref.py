"""pt_trace_ao (include/mi355pt.h "ray queries: ambient occlusion") restated in numpy from the ORIGINAL flat scene
(scene_io.flatten_scene) and the oracle only: oracle.Scene.intersect_n(..., use_bvh=False) for the primary rays and, with tmax = thi,
for the occlusion rays; orc.rng_init, rng_next, onb, to_world and sample_cosine_hemisphere for the stream and the directions;
tests/surface_ref.py's interp3, cross3 and unit3 and tests/aov_ref.py's dot3 for the surface.  Nothing here reads the library under test.

The work is split so that one pass over the stream serves several settings: the stream of a ray depends on (index, seed) only, so the
first K' <= K directions of a ray are its directions at n_rays = K', and the radius only changes the bound of the second brute force.
  prepare(S, flat, rays, truth, flags, seed, K)   steps 1-4 up to the directions: the records without ao, p, nf, (m, K, 3) directions
  finish(S, prep, K', radius)                      the occlusion brute force and step 5 -> (n,) DTYPE records
  compared(S, flat, rays, truth, prep, K')         which records a bit-for-bit comparison takes (below)
  ao(...)                                          prepare + finish

COMPARED RECORDS.  The closest hit is defined inside the domain of "validation hooks": no ray that grazes a triangle below
ray_battery.MIN_SIN_GRAZING.  Cosine sampling from surface points leaves it now and then, so a record is left out if its primary ray or
one of its K' occlusion rays has ray_battery.sin_grazing below that bound against the triangle the brute force reports as THAT ray's
closest hit with no bound.  The rule reads the restatement and the brute force, never the code under test.

MUTATIONS are the wrong readings of the definition that tests/test_trace_ao_host.py shows to change a compared record."""
import numpy as np

import aov_ref
import oracle as orc
import ray_battery as rb
import surface_ref

F32 = np.float32
interp3, cross3, unit3, dot3 = surface_ref.interp3, surface_ref.cross3, surface_ref.unit3, aov_ref.dot3
MUTATIONS = ("no_facing_flip", "draws_swapped", "seed_words_swapped", "radius_ignored", "stream_restarts_per_k")
SHADING_NORMAL = 1
K_TMAX = F32(1e10)
DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("n", "<f4", (3,)), ("ao", "<f4")])
assert DTYPE.itemsize == 32


def thi_of(radius):
    """radius < 1e10f ? radius : 1e10f"""
    r = F32(radius)
    return r if r < K_TMAX else K_TMAX


def _directions(nf, index, seed, K, mutation):
    """(K, 3) directions of one ray: its stream, the frame of nf once, two draws per ray (r1 then r2)."""
    t, b = orc.onb(nf)
    state = orc.rng_init(seed, index) if mutation == "seed_words_swapped" else orc.rng_init(index, seed)
    first = state
    out = np.zeros((K, 3), F32)
    for k in range(K):
        if mutation == "stream_restarts_per_k":
            state = first
        r1, state = orc.rng_next(state)
        r2, state = orc.rng_next(state)
        w = orc.sample_cosine_hemisphere(r2, r1) if mutation == "draws_swapped" else orc.sample_cosine_hemisphere(r1, r2)
        out[k] = orc.to_world(t, b, nf, w)
    return out


def prepare(S, flat, rays, truth, flags, seed, K, mutation=None):
    """truth: (hit, t, u, v, prim) of S.intersect_n(rays, use_bvh=False).  Returns dict(base: (n,) records with ao = 1, traced: indices of
    the rays that trace occlusion rays, p (m, 3), nf (m, 3), dirs (m, K, 3), K)."""
    assert mutation is None or mutation in MUTATIONS
    rays = np.asarray(rays, F32)
    hit, t, u, v, prim = (np.asarray(a) for a in truth)
    base = np.zeros(hit.shape[0], DTYPE)  # a miss: {+0, +0, +0, -1}, {+0, +0, +0, 1.0f}
    base["prim"], base["ao"] = -1, 1.0
    idx = np.nonzero(hit)[0]
    pr = prim[idx]
    bx, by = u[idx].astype(F32), v[idx].astype(F32)
    bw = F32(1.0) - bx - by
    pos = np.asarray(flat["positions"], F32).reshape(-1, 3, 3)[pr]
    nrm = np.asarray(flat["normals"], F32).reshape(-1, 3, 3)[pr]
    p = interp3(bw, bx, by, pos[:, 0], pos[:, 1], pos[:, 2])
    if flags & SHADING_NORMAL:
        n = unit3(interp3(bw, bx, by, nrm[:, 0], nrm[:, 1], nrm[:, 2]))
    else:
        n = unit3(cross3(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]))
    zero = (n == 0).all(1)
    flip = dot3(n, rays[idx, 3:6]) > 0
    if mutation == "no_facing_flip":
        flip = np.zeros_like(flip)
    nf = np.where(flip[:, None], -n, n).astype(F32)
    nf[zero] = 0.0
    base["t"][idx], base["u"][idx], base["v"][idx], base["prim"][idx], base["n"][idx] = t[idx], bx, by, pr, nf
    tr = ~zero
    traced = idx[tr]
    dirs = np.zeros((traced.size, K, 3), F32)
    for j, (i, f) in enumerate(zip(traced, nf[tr])):
        dirs[j] = _directions(f, int(i), int(seed), K, mutation)
    return dict(base=base, traced=traced, p=np.ascontiguousarray(p[tr]), nf=np.ascontiguousarray(nf[tr]), dirs=dirs, K=K)


def occlusion_rays(prep, K):
    """(m * K, 6): the occlusion rays of the traced records at n_rays = K, record by record."""
    assert 1 <= K <= prep["K"]
    m = prep["traced"].size
    return np.concatenate([np.repeat(prep["p"][:, None, :], K, 1), prep["dirs"][:, :K]], 2).reshape(m * K, 6).astype(F32)


def finish(S, prep, K, radius, mutation=None):
    out = prep["base"].copy()
    m = prep["traced"].size
    if m:
        thi = K_TMAX if mutation == "radius_ignored" else thi_of(radius)
        occ = S.intersect_n(occlusion_rays(prep, K), tmin=1e-3, tmax=float(thi), use_bvh=False)[0]
        clear = (~occ).reshape(m, K).sum(1)
        out["ao"][prep["traced"]] = clear.astype(F32) * (F32(1.0) / F32(K))
    return out


def ao(S, flat, rays, truth, K, flags, radius, seed, mutation=None):
    return finish(S, prepare(S, flat, rays, truth, flags, seed, K, mutation), K, radius, mutation)


def compared(S, flat, rays, truth, prep, K):
    """(n,) bool: the records a bit-for-bit comparison takes (module docstring)."""
    rays = np.asarray(rays, F32)
    pos = np.asarray(flat["positions"], F32).reshape(-1, 3, 3)
    hit, prim = np.asarray(truth[0]), np.asarray(truth[4])
    ok = np.ones(hit.shape[0], bool)
    h = np.nonzero(hit)[0]
    ok[h] = rb.sin_grazing(rays[h], pos[prim[h]]) >= rb.MIN_SIN_GRAZING
    m = prep["traced"].size
    if m:
        r = occlusion_rays(prep, K)
        far = S.intersect_n(r, use_bvh=False)  # no bound: the closest hit of the occlusion ray
        g = np.ones(r.shape[0], bool)
        fh = np.nonzero(far[0])[0]
        g[fh] = rb.sin_grazing(r[fh], pos[far[4][fh]]) >= rb.MIN_SIN_GRAZING
        ok[prep["traced"]] &= g.reshape(m, K).all(1)
    return ok


def differ(a, b):
    """Per record: any of the 32 bytes differs."""
    return (a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)).any(1)
