"""What tests/test_trace_rays_host.py (CPU) and tests/test_gpu_trace_rays.py (GPU) share: the ray battery of tests/ray_battery.py with its
brute-force truth, computed once per scene and process and never changed, as pt_ray / pt_ray_hit records.

A battery ray is COMPARED when it lies where the closest hit is defined (include/mi355pt.h "validation hooks"): classes 1-6 whole, class 7
(far origins) up to ray_battery.DOMAIN_EXTENTS; the only rays left out are the OUTSIDE classes 8 and 9 and the farther origins of class 7.
Every comparison is bit for bit: t, u, v as uint32, the id as int32, a miss is {+0, +0, +0, -1}."""
import numpy as np

import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B

N_PER_CLASS = 2000
K_TMAX = np.float32(1e10)
TMAX_SCENES = ("rects", "cornell")  # the scenes of the per-ray tmax cases
_cache = {}


def thi_of(tmax):
    """The definition's bound: tmax < 1e10f ? tmax : 1e10f (NaN and +inf give 1e10f)."""
    t = np.asarray(tmax, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(t < K_TMAX, t, K_TMAX).astype(np.float32)


def hits_of(truth):
    """(hit, t, u, v, prim) of oracle.Scene.intersect_n -> HIT_DTYPE records as the library stores them."""
    hit, t, u, v, prim = truth
    out = np.zeros(hit.shape[0], B.HIT_DTYPE)
    out["t"], out["u"], out["v"] = np.where(hit, t, 0), np.where(hit, u, 0), np.where(hit, v, 0)
    out["prim"] = np.where(hit, prim, -1)
    return out


def same(got, want, mask=None):
    """Per ray: the 16 bytes of a hit record, or the occlusion byte, equal."""
    eq = got.view(np.uint8).reshape(got.shape[0], -1) == want.view(np.uint8).reshape(want.shape[0], -1)
    eq = eq.all(1)
    return eq if mask is None else (eq | ~mask)


def assert_same(got, want, mask, what, rays=None, cls=None):
    ok = same(got, want, mask)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: %d of %d compared rays differ; first: ray %d%s got %r want %r%s" % (
            what, int((~ok).sum()), int(mask.sum()) if mask is not None else got.shape[0], i, "" if cls is None else " class %d" % cls[i], got[i], want[i],
            "" if rays is None else " %r" % (rays[i].tolist(),)))


def compared(tris, rays, cls):
    """Mask of the battery rays that are compared (module docstring)."""
    ext = rb.origin_extents(rays, rb.scene_measure(tris))
    return np.isin(cls, (1, 2, 3, 4, 5, 6)) | ((cls == 7) & (ext <= rb.DOMAIN_EXTENTS))


def battery(orc, name, watertight=False):
    """dict(tris, rays (n, 6), cls, mask, S (oracle scene), truth (intersect_n's tuple, brute force), hits (HIT_DTYPE), occ (uint8))."""
    key = (name, bool(watertight))
    if key not in _cache:
        tris = rb.make_scene(name)
        S = rb.oracle_scene(orc, tris)
        host = B.Context(-1)
        rb.upload(host, tris)
        t4 = rb.trees_of(host.export_trees())[1]
        host.close()
        used = t4.ref != -1
        planes = np.stack([t4.lo[used], t4.hi[used]], 1) if t4.n_nodes else None
        # (the rays are those of tests/test_gpu_ray_probes.py: same seed, same planes, class 2 from the Moeller-Trumbore hits)
        rays, cls = rb.make_rays(tris, np.random.default_rng(4242), N_PER_CLASS, planes=planes, hit_fn=lambda r: S.intersect_n(r, use_bvh=True)[:2])
        if watertight:
            S.set_watertight(True)
        truth = S.intersect_n(rays, use_bvh=False)
        for a in truth:
            a.setflags(write=False)
        rays.setflags(write=False)
        _cache[key] = dict(tris=tris, rays=rays, cls=cls, mask=compared(tris, rays, cls), S=S, truth=truth, hits=hits_of(truth), occ=truth[0].astype(np.uint8))
    return _cache[key]


def closed_case(orc, mesh="ico1280"):
    """The closed icosphere, 2000 rays from strictly inside aimed at its shared edges and vertices, and the oracle's two answers."""
    tris, centre, half = rb.make_closed_mesh(mesh)
    rays = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(99), 2000)["edges_and_vertices"]
    S = rb.oracle_scene(orc, tris)
    mt = S.intersect_n(rays, use_bvh=False)
    S.set_watertight(True)
    wt = S.intersect_n(rays, use_bvh=False)
    return tris, rays, mt, wt


def moved_scene(name="soup1"):
    """(triangles, the same triangles deformed): what pt_update_vertices gets in both files."""
    tris = rb.make_scene(name)
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    P = tris.astype(np.float64)
    moved = P + 0.03 * ext * np.sin(3.0 * P[..., [1, 2, 0]] / ext + 0.5)
    return tris, moved.astype(np.float32)


_tmax_cache = {}


def tmax_cases(orc, name):
    """The per-ray bounds of the definition on a battery, with the oracle's answers, for the CPU twin and the GPU calls alike: a list of
    (label, pt_ray records, HIT_DTYPE expectations, occlusion bytes, mask or None).  Five bounds that are the same for every ray - +inf,
    NaN, 1e10, -1, 1e-3 - with one brute-force pass per distinct thi; then, on a sample of 240 compared rays that hit, the ray's own
    bound: half its t, exactly its t (the same hit comes back), nextafter(t, 0) (that hit is gone), one brute force per ray."""
    if name in _tmax_cache:
        return _tmax_cache[name]
    bt = battery(orc, name)
    S, rays, mask = bt["S"], bt["rays"], bt["mask"]
    hit, t = bt["truth"][0], bt["truth"][1]
    cases = []
    for tmax in (np.inf, np.nan, 1e10, -1.0, 1e-3):
        thi = float(thi_of(tmax))
        want = bt["truth"] if thi == 1e10 else S.intersect_n(rays, tmin=1e-3, tmax=thi, use_bvh=False)
        if thi < 1e10:
            assert not want[0].any(), "no hit has 1e-3 < t <= %g" % thi
        cases.append(("tmax %r" % tmax, B.make_rays(rays, tmax), hits_of(want), want[0].astype(np.uint8), mask))
    idx = np.nonzero(hit & mask)[0]
    idx = idx[np.random.default_rng(7).permutation(idx.size)[:240]]
    assert idx.size >= 100
    kinds = np.arange(idx.size) % 3
    tm = np.where(kinds == 0, t[idx] * np.float32(0.5), np.where(kinds == 1, t[idx], np.nextafter(t[idx], np.float32(0)))).astype(np.float32)
    want = np.zeros(idx.size, B.HIT_DTYPE)
    for j, (i, b) in enumerate(zip(idx, tm)):
        ok, tt, uu, vv, pp = S.intersect(rays[i, :3], rays[i, 3:], tmin=1e-3, tmax=float(b), use_bvh=False)
        want[j] = (np.float32(tt), np.float32(uu), np.float32(vv), pp) if ok else (0, 0, 0, -1)
    assert same(want[kinds == 1], bt["hits"][idx][kinds == 1]).all(), "a bound of exactly the hit's t keeps the hit (the oracle says so)"
    assert not same(want[kinds == 2], bt["hits"][idx][kinds == 2]).any(), "one float below it the hit is gone"
    cases.append(("per-ray tmax (half t, t, nextafter(t, 0))", B.make_rays(rays[idx], tm), want, (want["prim"] >= 0).astype(np.uint8), None))
    # all eight kinds of bound mixed in ONE call, so that neighbouring lanes of a wave carry different bounds
    k8 = np.arange(idx.size) % 8
    mixed = np.select([k8 == 0, k8 == 1, k8 == 2, k8 == 3, k8 == 4], [np.inf, np.nan, 1e10, -1.0, 1e-3], tm).astype(np.float32)
    full = bt["hits"][idx]
    wm = want.copy()  # k8 >= 5: the ray's own bound, as above
    wm[k8 <= 2] = full[k8 <= 2]
    wm[(k8 == 3) | (k8 == 4)] = (0, 0, 0, -1)
    cases.append(("eight kinds of bound in one call", B.make_rays(rays[idx], mixed), wm, (wm["prim"] >= 0).astype(np.uint8), None))
    _tmax_cache[name] = cases
    return cases
