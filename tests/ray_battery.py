"""Scenes, rays and tree helpers shared by tests/test_tree_structure.py (CPU) and tests/test_gpu_ray_probes.py (GPU).

One seeded generator for the RAY BATTERY: seven classes of rays chosen to sit where a traversal goes wrong (and an eighth that lies
outside the domain on which the closest hit is defined, which the tests count but never assert) - zero and denormal
direction components, origins and ray lines exactly on box planes / edges / corners of the product's own node arrays, rays through
vertices and along shared edges, edge-grazing and nearly coplanar rays, far origins on both sides of the distance up to which the fma
slab form is claimed.  Every ray is finite and its direction has unit length to float32 rounding (the product normalises): nothing
here can make a walk spin.

Also: the hierarchy read-back turned into parent maps (`TreePaths`), the structure checks both files run on it, and a float32 numpy
emulation of the product's slab tests (`slab_margin`); closed meshes with rays from inside and the battery as the exact-geometry
referee takes it (tests/exact_hit.py, tests/test_exact_hit.py, tests/test_gpu_exact_hit.py).
"""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")

# outside the domain of the definition, counted only: 8 = rays coplanar with a general triangle up to rounding, 9 = rays aimed at an edge at a
# grazing angle below 1e-2 rad (the hit is displaced along the ray by (placement error) / sin(angle): more than the padding)
OUTSIDE = (8, 9)
OUTSIDE_NAMES = {8: "coplanar (outside the domain)", 9: "grazing below 1e-2 rad (outside the domain)"}
CLASSES = {1: "uniform", 2: "secondary", 3: "zero components", 4: "box planes", 5: "vertices and edges", 6: "grazing", 7: "far origins"}
FAR_EXTENTS = (3.0, 7.0, 10.0, 41.0, 43.0, 300.0, 3000.0)
K_TMIN = np.float32(1e-3)
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# scenes: every scene is one triangle soup (n, 3, 3) float32; only the geometry matters here
# ---------------------------------------------------------------------------------------------------------------------
def mesh_of(tris):
    v = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    return dict(vertices=v, normals=np.tile(np.float32([0, 1, 0]), (v.shape[0], 1)), texcoords=np.zeros((0, 2), np.float32),
                indices=np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3))


def _soup_of(entities):
    return np.concatenate([m["vertices"][m["indices"]].astype(np.float32) for m, _ in entities]).reshape(-1, 3, 3)


def rect_scene(rng, n=120):
    """Axis-aligned rectangles: a regular wall of them (shared edges and vertices), random ones, coincident copies."""
    t = []
    g = np.linspace(-1.0, 1.0, 7)
    for i in range(6):
        for j in range(6):  # a wall in the plane z = 0.25: neighbours share edges and corners exactly
            a, b, c, d = (g[i], g[j], 0.25), (g[i + 1], g[j], 0.25), (g[i + 1], g[j + 1], 0.25), (g[i], g[j + 1], 0.25)
            t += [[a, b, c], [a, c, d]]
    for _ in range(n):
        ax = int(rng.integers(0, 3))
        lo, hi = np.sort(rng.uniform(-1, 1, (2, 3)), axis=0)
        lo[ax] = hi[ax] = float(rng.choice([-1.0, 0.0, 0.5, rng.uniform(-1, 1)]))
        a, b = (ax + 1) % 3, (ax + 2) % 3
        p = [lo.copy(), lo.copy(), hi.copy(), lo.copy()]
        p[1][a] = hi[a]
        p[3][b] = hi[b]
        t += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
        if rng.random() < 0.2:
            t += [[p[0], p[1], p[2]]]  # coincident copy: the lower id wins
    return np.asarray(t, np.float32)


def strip_scene(n=3000):
    """The sliver strip of test_bvh_depth_cap: SAH builds a deep, unbalanced tree over it."""
    x = np.arange(n + 1, dtype=np.float32) ** 2 * 1e-3
    v = np.stack([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 1e-3, 0 * x], 1)], 1).reshape(-1, 3)
    idx = np.array([[2 * i, 2 * i + 2, 2 * i + 1] for i in range(n)], np.int32)
    return v[idx].astype(np.float32)


def scene_names():
    return ["cornell", "rects", "one_leaf", "soup1", "soup2", "soup3", "soup_offset30", "strip", "dragon", "car"]


def make_scene(name):
    """(n, 3, 3) float32 triangles of the named scene."""
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    if name == "cornell":
        return _soup_of(scene_io.load_scene_dir(ASSETS, "cornell-box")["entities"])
    if name == "rects":
        return rect_scene(np.random.default_rng(11))
    if name == "one_leaf":
        return np.float32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0.5], [1, 0, 0.5], [0, 1, 0.5]], [[2, 0, 0], [2, 1, 0], [2, 0, 1]]])
    if name.startswith("soup"):
        from test_gpu_fuzz import _random_scene  # the fuzz suite's soups: coincident, degenerate, huge triangles, needles, offsets

        if name == "soup_offset30":  # a soup 30 extents away from the origin: the padding grows with max |coordinate|
            t = _soup_of(_random_scene(np.random.default_rng(20260407))[0]).astype(np.float64)
            ext = float((t.reshape(-1, 3).max(0) - t.reshape(-1, 3).min(0)).max())
            return (t + np.array([30.0, -17.0, 23.0]) * ext).astype(np.float32)
        return _soup_of(_random_scene(np.random.default_rng({"soup1": 20260405, "soup2": 20260411, "soup3": 20260419}[name]))[0])
    if name == "strip":
        return strip_scene()
    if name == "dragon":  # reduced C4 stand-in: 24 000 + 4 triangles
        return _soup_of([(m, 0) for _, m in procedural.dragon_standin(n_u=300, n_v=40)])
    if name == "car":  # reduced C5 stand-in (~17 000 triangles)
        return _soup_of([(m, 0) for _, m in procedural.car_standin(detail=0.1)])
    raise KeyError(name)


def upload(ctx, tris):
    from owl_path_tracer_amd.pyhost import scene_io

    ctx.upload_scene([(mesh_of(tris), 0)], [scene_io.MAT_DEFAULT])


def oracle_scene(orc, tris, leaf_size=4):
    from owl_path_tracer_amd.pyhost import scene_io

    return orc.Scene(scene_io.flatten_scene([(mesh_of(tris), 0)], [("a", scene_io.MAT_DEFAULT, "")]), leaf_size=leaf_size)


# ---------------------------------------------------------------------------------------------------------------------
# the ray battery
# ---------------------------------------------------------------------------------------------------------------------
def _unit32(d):
    """Normalised in float32, as the product does (directions of unit length to float32 rounding)."""
    d = np.asarray(d, np.float32)
    n = np.sqrt((d * d).sum(-1, dtype=np.float32), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (d / n[..., None]).astype(np.float32)


def _rand_dirs(rng, n):
    return _unit32(rng.normal(0, 1, (n, 3)))


def _bary_points(rng, tris, n):
    """Points on random triangles, computed in float32 (what a bounce origin looks like)."""
    k = rng.integers(0, tris.shape[0], n)
    u = rng.random(n).astype(np.float32)
    v = (rng.random(n).astype(np.float32) * (F32(1) - u)).astype(np.float32)
    w = (F32(1) - u - v).astype(np.float32)
    t = tris[k]
    return (w[:, None] * t[:, 0] + u[:, None] * t[:, 1] + v[:, None] * t[:, 2]).astype(np.float32), k


def make_rays(tris, rng, n=2000, planes=None, hit_fn=None):
    """rays (N, 6) float32 and their class (N,) of CLASSES.  `planes`: (m, 2, 3) lo / hi boxes taken from the product's node arrays
    (class 4; the scene box is always among them).  `hit_fn(rays) -> (hit, t)`: lets class 2 start on the hit points of class 1."""
    tris = np.asarray(tris, np.float32)
    P = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max()) or 1.0
    ctr = 0.5 * (lo + hi)
    out, cls = [], []

    def add(c, o, d):
        o = np.asarray(o, np.float32).reshape(-1, 3)
        d = np.asarray(d, np.float32).reshape(-1, 3)
        out.append(np.concatenate([o, d], 1))
        cls.append(np.full(o.shape[0], c, np.int32))

    def inside(m):
        return (lo + rng.random((m, 3)) * (hi - lo))

    def around(m, k=2.0):
        return (lo - k * ext + rng.random((m, 3)) * (hi - lo + 2 * k * ext))

    # 1. uniform origins inside and up to 2 extents outside the scene box, random directions
    o1 = np.concatenate([inside(n // 2), around(n - n // 2)]).astype(np.float32)
    d1 = _rand_dirs(rng, n)
    add(1, o1, d1)

    # 2. secondary-like: origins ON surfaces, directions random / reflected / back along the incoming ray (t near kTMin)
    pts, k = _bary_points(rng, tris, n // 2)
    if hit_fn is not None:
        hit, t = hit_fn(np.concatenate([o1, d1], 1))
        hp = (o1[hit] + t[hit, None] * d1[hit]).astype(np.float32)[: n // 2]
        pts = np.concatenate([pts, hp])
        inc = np.concatenate([_rand_dirs(rng, n // 2), d1[hit][: n // 2]])
        k = np.concatenate([k, rng.integers(0, tris.shape[0], hp.shape[0])])
    else:
        inc = _rand_dirs(rng, pts.shape[0])
    nrm = np.cross(tris[k, 1].astype(np.float64) - tris[k, 0], tris[k, 2].astype(np.float64) - tris[k, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    refl = inc - 2.0 * (inc * nrm).sum(1, keepdims=True) * nrm
    add(2, pts, _rand_dirs(rng, pts.shape[0]))
    add(2, pts, _unit32(refl))
    add(2, pts, -inc)

    # 3. direction components exactly +0 / -0 on one and on two axes, denormal and 1e-20-sized ones; origins inside, outside and
    #    exactly on a slab plane of that axis (a coordinate of the scene box or of a vertex)
    m = n // 6
    for val in (0.0, -0.0, 1e-40, -1e-40, 1e-20, -1e-20):
        for two in (False, True):
            d = rng.normal(0, 1, (m, 3))
            ax = rng.integers(0, 3, m)
            d[np.arange(m), ax] = 0.0
            if two:
                d[np.arange(m), (ax + 1) % 3] = 0.0
            d = _unit32(d)
            d[np.arange(m), ax] = F32(val)
            if two:
                d[np.arange(m), (ax + 1) % 3] = F32(-val if rng.random() < 0.5 else val)
            o = np.concatenate([inside(m // 3), around(m // 3, 0.5), inside(m - 2 * (m // 3))]).astype(np.float32)
            on = np.arange(2 * (m // 3), m)  # exactly on a plane of the zero axis
            vals = np.concatenate([lo[None], hi[None], P[rng.integers(0, P.shape[0], 16)]]).astype(np.float32)
            o[on, ax[on]] = vals[rng.integers(0, vals.shape[0], on.size), ax[on]]
            add(3, o, d)

    # 4. origins and ray lines exactly on box planes, edges and corners of the node arrays, both rows of every axis, root included
    boxes = np.concatenate([np.stack([lo, hi])[None].astype(np.float32)] + ([np.asarray(planes, np.float32)] if planes is not None and len(planes) else []))
    boxes = boxes[np.isfinite(boxes).all((1, 2))]
    m = n // 4
    for fixed in (1, 2, 3):
        b = boxes[rng.integers(0, boxes.shape[0], m)]
        row = rng.integers(0, 2, (m, 3))
        corner = np.where(row == 0, b[:, 0], b[:, 1]).astype(np.float32)  # a corner of the box: lo or hi row per axis
        o = (b[:, 0] + rng.random((m, 3)).astype(np.float32) * (b[:, 1] - b[:, 0])).astype(np.float32)
        ax = rng.integers(0, 3, m)
        keep = np.zeros((m, 3), bool)
        for j in range(fixed):
            keep[np.arange(m), (ax + j) % 3] = True
        o = np.where(keep, corner, o).astype(np.float32)
        add(4, o, _rand_dirs(rng, m))
        d = rng.normal(0, 1, (m, 3))
        d[keep] = 0.0  # the ray line stays in the plane / runs along the edge
        d[np.arange(m), (ax + 2) % 3] += np.where(d[np.arange(m), (ax + 2) % 3] == 0, 1.0, 0.0)
        back = (o.astype(np.float64) - _unit32(d) * ext * rng.uniform(0.0, 1.5, (m, 1)))
        back = np.where(keep, corner, back).astype(np.float32)
        add(4, back, _unit32(d))
        add(4, o, _unit32(ctr - o + 1e-9))

    # 5. rays through vertices and along (shared) edges, in the plane of a triangle, along needles
    m = n // 4
    k = rng.integers(0, tris.shape[0], m)
    o = around(m, 1.0).astype(np.float32)
    vtx = tris[k, rng.integers(0, 3, m)]
    add(5, o, _unit32(vtx - o))
    e0 = rng.integers(0, 3, m)
    a, b = tris[k, e0], tris[k, (e0 + 1) % 3]
    mid = (a + (b - a) * rng.random((m, 1)).astype(np.float32)).astype(np.float32)
    add(5, o, _unit32(mid - o))
    ed = (b - a).astype(np.float32)
    ok = (ed != 0).any(1)
    is_flat = ((tris[:, 0] == tris[:, 1]) & (tris[:, 0] == tris[:, 2])).any(1)[k]
    along_o, along_d = (a - ed * rng.uniform(0.1, 2.0, (m, 1)).astype(np.float32)), _unit32(ed)
    # along an edge (needles: along their axis).  Such a ray lies in its triangle's plane: for an axis-aligned triangle det is exactly 0
    # (rejected, ties between the neighbours of a shared edge cannot arise); for a general one it is coplanar only up to rounding
    # - class 8, outside the domain of the definition (see below)
    add(5, along_o[ok & is_flat], along_d[ok & is_flat])
    add(8, along_o[ok & ~is_flat], along_d[ok & ~is_flat])
    # exactly in the plane of an AXIS-ALIGNED triangle: det is exactly 0 and the triangle is rejected.  (A ray within rounding of the
    # plane of a general triangle is outside the definition's domain: det is tiny but not 0, Moeller-Trumbore's t, u, v are noise and
    # can place a "hit" outside the triangle's box - DESIGN 2.1; class 6 goes down to 1e-4 rad.)
    flat = np.nonzero(((tris[:, 0] == tris[:, 1]) & (tris[:, 0] == tris[:, 2])).any(1))[0]
    if flat.size:
        kf = flat[rng.integers(0, flat.size, m)]
        axf = np.argmax((tris[kf, 0] == tris[kf, 1]) & (tris[kf, 0] == tris[kf, 2]), axis=1)
        dpl = rng.normal(0, 1, (m, 3))
        dpl[np.arange(m), axf] = 0.0
        dpl = _unit32(dpl)
        opl = (tris[kf].mean(1, dtype=np.float64) - dpl * ext * rng.uniform(0.2, 1.5, (m, 1))).astype(np.float32)
        opl[np.arange(m), axf] = tris[kf, 0][np.arange(m), axf]
        add(5, opl, dpl)
    # 8. (OUTSIDE the domain, counted and never asserted) rays in the plane of a general triangle up to rounding: det is tiny but not 0,
    #    t, u, v are rounding noise and the "hit" can lie outside the triangle's padded box, so which triangle wins depends on the hierarchy
    cen = tris[k].mean(1, dtype=np.float64)
    e1, e2 = (tris[k, 1] - tris[k, 0]).astype(np.float64), (tris[k, 2] - tris[k, 0]).astype(np.float64)
    ang = rng.uniform(0, 2 * np.pi, (m, 1))
    inpl = np.cos(ang) * e1 + np.sin(ang) * e2
    okp = (np.linalg.norm(inpl, axis=1) > 0) & ~is_flat
    dpl = _unit32(inpl[okp])
    add(8, (cen[okp] - dpl * ext * rng.uniform(0.2, 1.5, (okp.sum(), 1))).astype(np.float32), dpl)

    # 6. edge-grazing and nearly coplanar rays: aimed within +-k x 1e-6 extents of an edge, grazing angles 0.3 .. 1e-4 rad; those below
    #    1e-2 rad are class 9: measured on the oracle itself, 1 ray in ~160 000 at 1e-4 rad gets a hit placed 5 paddings outside its
    #    triangle's box, and walk and brute force then disagree
    m = n // 6
    for theta in (0.3, 0.1, 0.03, 0.01, 1e-3, 1e-4):
        k = rng.integers(0, tris.shape[0], m)
        t = tris[k].astype(np.float64)
        e0 = rng.integers(0, 3, m)
        a, b, c = t[np.arange(m), e0], t[np.arange(m), (e0 + 1) % 3], t[np.arange(m), (e0 + 2) % 3]
        nrm = np.cross(b - a, c - a)
        ln = np.linalg.norm(nrm, axis=1)
        good = ln > 1e-30
        nrm = nrm / np.maximum(ln, 1e-300)[:, None]
        edge = (b - a) / np.maximum(np.linalg.norm(b - a, axis=1), 1e-300)[:, None]
        inward = np.cross(nrm, edge)
        kk = rng.choice([-10.0, -5.0, -2.0, -1.0, 0.0, 1.0, 2.0, 5.0, 10.0], m)
        target = a + (b - a) * rng.random((m, 1)) + inward * (kk * 1e-6 * ext)[:, None]
        ang = rng.uniform(0, 2 * np.pi, (m, 1))
        tdir = np.cos(ang) * edge + np.sin(ang) * inward
        d = np.cos(theta) * tdir - np.sin(theta) * nrm * rng.choice([-1.0, 1.0], (m, 1))
        d32 = _unit32(d)
        o = target - d32.astype(np.float64) * ext * rng.uniform(0.05, 3.0, (m, 1))
        add(6 if theta >= 1e-2 else 9, o[good], d32[good])

    # 7. far origins aimed at the scene
    m = n // 7
    for far in FAR_EXTENTS:
        target, _ = _bary_points(rng, tris, m)
        d = _rand_dirs(rng, m)
        add(7, (target.astype(np.float64) - d.astype(np.float64) * far * ext).astype(np.float32), d)

    rays = np.concatenate(out).astype(np.float32)
    cls = np.concatenate(cls)
    d = rays[:, 3:]
    # finite, and unit length to float32 rounding - up to the tiny components set on purpose
    ok = np.isfinite(rays).all(1) & (np.abs((d.astype(np.float64) ** 2).sum(1) - 1.0) < 1e-5)
    return np.ascontiguousarray(rays[ok]), cls[ok]


DOMAIN_EXTENTS = 10.0  # the closest hit is DEFINED (independent of the hierarchy) for origins within this many extents: DESIGN 2.1
FMA_EXTENTS = 41.94304  # walk_params: beyond pad x 2^22 the product switches to the subtracting slab form


def scene_measure(tris):
    """E = max(scene extent, largest |coordinate| of the scene): the boxes are padded by 1e-5 E (pt_bvh_build), walk_params measures
    the camera's distance in it.  Taken from the triangles, not from the pad a context reports: that is under test."""
    P = np.asarray(tris, np.float64).reshape(-1, 3)
    return float(max((P.max(0) - P.min(0)).max(), np.abs(P).max()))


def origin_extents(rays, E):
    """Largest |origin coordinate| of each ray in units of E (scene_measure).  Moeller-Trumbore places a hit with an error that
    grows with the distance to the origin (some 2^-24 x distance x 14 in the worst case seen in 2.4 M rays), the boxes are padded by
    1e-5 E: beyond ~10 E a triangle test can accept a hit that lies outside the padded box, and brute force and ANY hierarchy - the
    oracle's own included - start to disagree (measured: 0 of 1.8 M rays at 10 / 20 / 30 E, 1 of 300 000 at 41 E, 5e-5 at 100 E,
    7e-4 at 3 000 E)."""
    return np.abs(rays[:, :3].astype(np.float64)).max(1) / float(E)


def bands(rays, E, cls=None):
    """(inside the domain, between the domain and the fma form's reach, beyond the fma form's reach); class 8 is in none of them"""
    e = origin_extents(rays, E)
    if cls is not None:
        e = np.where(np.isin(cls, OUTSIDE), np.nan, e)
    with np.errstate(invalid="ignore"):
        return e <= DOMAIN_EXTENTS, (e > DOMAIN_EXTENTS) & (e <= FMA_EXTENTS), e > FMA_EXTENTS


# ---------------------------------------------------------------------------------------------------------------------
# the trees read back from a context
# ---------------------------------------------------------------------------------------------------------------------
def leaf_range(ref):
    code = ~np.asarray(ref, np.int64) & 0xffffffff
    return code >> 3, code & 7


class Tree:
    """One of the three hierarchies as flat slot arrays: slot s of node i = index i * width + s, with lo / hi (n, 3), ref (n,)."""

    def __init__(self, name, lo, hi, ref, root, width):
        self.name, self.lo, self.hi, self.ref, self.root, self.width = name, lo, hi, ref, int(root), width
        self.n_nodes = ref.size // width


def trees_of(ex):
    nd, n4, n8 = ex["nodes"], ex["nodes4"], ex["nodes8"]
    t2 = Tree("binary", np.ascontiguousarray(nd["lo"].transpose(0, 2, 1)).reshape(-1, 3), np.ascontiguousarray(nd["hi"].transpose(0, 2, 1)).reshape(-1, 3),
              np.stack([nd["left"], nd["right"]], 1).reshape(-1), ex["root"], 2)
    t4 = Tree("quad", np.ascontiguousarray(n4["lo"].transpose(0, 2, 1)).reshape(-1, 3), np.ascontiguousarray(n4["hi"].transpose(0, 2, 1)).reshape(-1, 3),
              n4["child"].reshape(-1), ex["root4"], 4)
    t8 = Tree("oct", n8["c"]["lo"].reshape(-1, 3), n8["c"]["hi"].reshape(-1, 3), n8["c"]["ref"].reshape(-1), ex["root8"], 8)
    return t2, t4, t8


def check_structure(ex, wide_leaves=1):
    """The structure the walks rely on, asserted on a read-back: returns a dict of measured figures."""
    tris = ex["tris"]
    n_slots = tris.size
    real = tris["id"] != 0x7fffffff
    ids = np.sort(tris["id"][real])
    assert np.array_equal(ids, np.arange(ids.size)), "every triangle id exactly once in the leaf-ordered records"
    V = np.stack([tris["p0"], tris["p1"], tris["p2"]], 1)  # (slots, 3, 3)
    vlo, vhi = V.min(1), V.max(1)
    pad = np.float32(ex["pad"])
    assert pad > 0 and np.isfinite(pad)
    sub = {}  # per tree: the vertex box below every slot
    out = {}
    for T in trees_of(ex):
        if T.n_nodes == 0:
            # no node array: the root is a leaf (tiny scene) - or the tree was too deep for this walk and the product does not use it
            if T.name == "binary" or T.root < -1:
                first, count = leaf_range(T.root)
                assert T.root < -1 and first == 0 and count == real.sum() == n_slots
            out[T.name] = dict(nodes=0, depth=0)
            continue
        assert 0 <= T.root < T.n_nodes
        seen_node = np.zeros(T.n_nodes, np.int32)
        seen_node[T.root] += 1
        seen_tri = np.zeros(n_slots, np.int32)
        internal = T.ref >= 0
        empty = T.ref == -1
        leaf = T.ref < -1
        assert (T.ref[internal] < T.n_nodes).all(), "child reference out of range"
        np.add.at(seen_node, T.ref[internal], 1)
        assert (seen_node == 1).all(), "every node referenced exactly once (the root by the root reference)"
        first, count = leaf_range(T.ref[leaf])
        assert (count >= 1).all() and (first + count <= n_slots).all()
        for f, c in zip(first, count):
            seen_tri[f:f + c] += 1
        assert (seen_tri[real] == 1).all(), "every real triangle slot in exactly one leaf"
        assert np.isposinf(T.lo[empty]).all() and np.isposinf(T.hi[empty]).all(), "an empty slot carries the never-hit box"
        assert T.name != "binary" or not empty.any()
        # vertex box below every slot, and the depth, bottom-up (children have larger indices than parents in no particular order: recurse)
        slo = np.full((T.ref.size, 3), np.inf, np.float32)
        shi = np.full((T.ref.size, 3), -np.inf, np.float32)
        depth = np.zeros(T.n_nodes, np.int32)
        order, stack = [], [T.root]
        while stack:
            i = stack.pop()
            order.append(i)
            stack += [int(r) for r in T.ref[i * T.width:(i + 1) * T.width] if r >= 0]
        assert len(order) == T.n_nodes
        for i in reversed(order):
            d = 0
            for s in range(i * T.width, (i + 1) * T.width):
                r = int(T.ref[s])
                if r >= 0:
                    slo[s] = slo[r * T.width:(r + 1) * T.width].min(0)
                    shi[s] = shi[r * T.width:(r + 1) * T.width].max(0)
                    d = max(d, int(depth[r]))
                elif r < -1:
                    f, c = (int(x) for x in leaf_range(r))
                    m = real[f:f + c]
                    if m.any():
                        slo[s] = vlo[f:f + c][m].min(0)
                        shi[s] = vhi[f:f + c][m].max(0)
            depth[i] = d + 1
        used = ~empty
        has = np.isfinite(slo).all(1) & used
        assert np.isfinite(T.lo[used]).all() and np.isfinite(T.hi[used]).all() and (T.lo[used] <= T.hi[used]).all()
        # every slot's box holds every vertex below it, with the full pad (float32 subtraction as the builders do it)
        assert (T.lo[has] <= (slo[has] - pad).astype(np.float32)).all() and (T.hi[has] >= (shi[has] + pad).astype(np.float32)).all(), \
            "%s tree: a slot's box does not contain its subtree with the full pad" % T.name
        sub[T.name] = (slo, shi)
        measured = int(depth[T.root])
        want = {"binary": ex["depth"], "quad": ex["depth4"], "oct": ex["depth8"]}[T.name]
        assert measured == want, "%s tree: depth field %d, measured %d" % (T.name, want, measured)
        out[T.name] = dict(nodes=T.n_nodes, depth=measured)
    # quad / oct slot boxes ARE binary boxes: the collapse stores boxes of the binary tree, it does not recompute them
    t2 = trees_of(ex)[0]
    if t2.n_nodes:
        binset = set(map(bytes, np.concatenate([t2.lo, t2.hi], 1)))
        for T in trees_of(ex)[1:]:
            if T.n_nodes == 0:
                continue
            used = T.ref != -1
            rows = np.concatenate([T.lo, T.hi], 1)[used]
            missing = [r for r in map(bytes, rows) if r not in binset]
            # (a wide leaf of the oct tree takes the box of the binary subtree it replaces: a binary slot's box as well)
            assert not missing, "%s tree: %d slot boxes are not boxes of the binary tree" % (T.name, len(missing))
    return out


class TreePaths:
    """For each leaf-order triangle slot: the chain of slots (boxes) from its leaf up to the root, for one Tree."""

    def __init__(self, T, n_slots):
        self.T = T
        self.leaf_slot = np.full(n_slots, -1, np.int64)  # triangle slot -> slot index of its leaf
        self.parent_slot = np.full(max(T.n_nodes, 1), -1, np.int64)  # node -> slot index that references it (-1: root)
        if T.n_nodes == 0:
            return
        internal = np.nonzero(T.ref >= 0)[0]
        self.parent_slot[T.ref[internal]] = internal
        for s in np.nonzero(T.ref < -1)[0]:
            f, c = (int(x) for x in leaf_range(T.ref[s]))
            self.leaf_slot[f:f + c] = s

    def levels(self, tri_slots):
        """Yields the slot index per query at each level, leaf first; -1 where the chain has ended."""
        cur = self.leaf_slot[tri_slots].copy()
        while (cur >= 0).any():
            yield cur
            node = np.where(cur >= 0, cur // self.T.width, 0)
            cur = np.where(cur >= 0, self.parent_slot[node], -1)


# ---------------------------------------------------------------------------------------------------------------------
# the product's slab tests, emulated in float32
# ---------------------------------------------------------------------------------------------------------------------
PT_INV_MAX = np.float32(1e18)


def ray_inv_variants(d):
    """ray_inv (pt_trace.h) for the correctly rounded reciprocal and its two float32 neighbours - v_rcp_f32 is within 1 ulp -
    each clamped to +-PT_INV_MAX as the product clamps."""
    d = np.asarray(d, np.float32)
    with np.errstate(divide="ignore", over="ignore"):
        r0 = np.divide(np.float32(1.0), d, dtype=np.float32)
    out = []
    for r in (np.nextafter(r0, np.float32(-np.inf)), r0, np.nextafter(r0, np.float32(np.inf))):
        out.append(np.clip(r, -PT_INV_MAX, PT_INV_MAX).astype(np.float32))
    return out


MIN_SIN_GRAZING = 1e-2  # slab emulation: below this sine of the angle between ray and triangle plane the hit's t is not a usable bound


def sin_grazing(rays, tri_vertices):
    """|d . n| for the unit normal n of each ray's triangle (n, 3, 3)."""
    t = np.asarray(tri_vertices, np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    return np.abs((rays[:, 3:].astype(np.float64) * n).sum(1))


def slab_margin(lo, hi, o, inv, tbest, exact, octant):
    """The slab test of node4_step (octant = True: entry / exit rows by the sign of inv) or box_test / box_test_fma (min / max of the two
    distances) on boxes lo, hi (n, 3) for rays o, inv (n, 3), best hit tbest (n,).  float32 throughout; the fma of the fma form is the
    float64 sum of the exact float64 product and the addend, rounded to float32 (Python 3.10 has no math.fma: two roundings instead
    of one, which can differ from a true fma by one float32 ulp in rare halfway cases).
    Returns (passes, margin in ulps of the far distance)."""
    lo, hi, o, inv = (np.asarray(x, np.float32) for x in (lo, hi, o, inv))
    with np.errstate(over="ignore", invalid="ignore"):
        if exact:
            t0 = ((lo - o).astype(np.float32) * inv).astype(np.float32)
            t1 = ((hi - o).astype(np.float32) * inv).astype(np.float32)
        else:
            no = (-(o * inv).astype(np.float32)).astype(np.float64)
            t0 = (lo.astype(np.float64) * inv.astype(np.float64) + no).astype(np.float32)
            t1 = (hi.astype(np.float64) * inv.astype(np.float64) + no).astype(np.float32)
        if octant:
            neg = np.signbit(inv)
            en, exi = np.where(neg, t1, t0), np.where(neg, t0, t1)
        else:
            en, exi = np.fmin(t0, t1), np.fmax(t0, t1)
        tn = np.fmax(np.fmax(en[:, 0], en[:, 1]), np.fmax(en[:, 2], K_TMIN))
        tf = np.fmin(np.fmin(exi[:, 0], exi[:, 1]), np.fmin(exi[:, 2], np.asarray(tbest, np.float32)))
        tfp = (tf * np.float32(1.0000004)).astype(np.float32)
        ok = tn <= tfp
        margin = (tfp.astype(np.float64) - tn.astype(np.float64)) / np.spacing(np.abs(tf)).astype(np.float64)
    return ok, margin


# ---------------------------------------------------------------------------------------------------------------------
# closed meshes with shared float32 vertices, rays from strictly inside: exact geometry says every such ray hits
# ---------------------------------------------------------------------------------------------------------------------
def icosphere(sub):
    """Unit icosphere, (20 x 4^sub, 3, 3) float32; neighbours share bit-identical float32 vertices."""
    p = (1 + 5 ** 0.5) / 2
    V = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    for _ in range(sub):
        cache, F2 = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]

        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.array(V, np.float32)[np.array(F)]


CLOSED_RADIUS = 1.7
CLOSED_OFFSET = 13.6  # 4 extents of the icosphere


def closed_mesh_names():
    return ["box", "ico320", "ico1280", "ico1280_offset"]


def make_closed_mesh(name):
    """((n, 3, 3) float32 triangles, centre, half-width of the cube of origins strictly inside)."""
    if name == "box":
        lo, hi = np.float32([-1.25, -0.5, -2.0]), np.float32([0.75, 1.5, 1.0])
        c = np.array([[lo[0] if (i & 1) == 0 else hi[0], lo[1] if (i & 2) == 0 else hi[1], lo[2] if (i & 4) == 0 else hi[2]] for i in range(8)], np.float32)
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        F = [f for a, b, cc, d in quads for f in ((a, b, cc), (a, cc, d))]
        return c[np.array(F)], 0.5 * (lo.astype(np.float64) + hi), 0.6
    sub, off = {"ico320": (2, 0.0), "ico1280": (3, 0.0), "ico1280_offset": (3, CLOSED_OFFSET)}[name]
    tris = (icosphere(sub) * np.float32(CLOSED_RADIUS) + np.float32(off)).astype(np.float32)
    return tris, np.full(3, float(np.float32(off))), 0.6


CLOSED_SETS = ("random", "edges_and_vertices")


def closed_mesh_rays(tris, centre, half, rng, n):
    """{set name: (n, 6) float32 rays} from origins strictly inside: random directions; aimed at points on shared edges, a quarter of
    them at vertices."""
    o = (centre + rng.uniform(-half, half, (n, 3))).astype(np.float32)
    out = {"random": np.concatenate([o, _rand_dirs(rng, n)], 1)}
    k, e = rng.integers(0, tris.shape[0], n), rng.integers(0, 3, n)
    a, b = tris[k, e].astype(np.float64), tris[k, (e + 1) % 3].astype(np.float64)
    s = rng.random((n, 1))
    s[: n // 4] = 0.0
    o = (centre + rng.uniform(-half, half, (n, 3))).astype(np.float32)
    out["edges_and_vertices"] = np.concatenate([o, _unit32(a + (b - a) * s - o)], 1)
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# how many rays per class the exact referee (tests/exact_hit.py) takes on a scene: it visits every (ray, triangle) pair in numpy
# ---------------------------------------------------------------------------------------------------------------------
REFEREE_PAIRS = int(os.environ.get("PT_REFEREE_PAIRS", "12000000"))
REFEREE_MIN_RAYS = 120


def referee_rays_per_class(n_tris, n_per_class):
    """PT_PROBE_RAYS per class where the scene is small, fewer on large ones (a battery has ~10.5 n rays), never below 120: with
    120 every class and every far-origin distance is still drawn."""
    return int(min(n_per_class, max(REFEREE_MIN_RAYS, REFEREE_PAIRS // (11 * max(1, n_tris)))))


_referee_cache = {}


def referee_battery(orc, name, n_per_class):
    """Scene, the battery's rays (same seed and planes as the other two files; fewer per class on large scenes) and the referee's
    tables for them, once per scene and process: dict(tris, rays, cls, tables, n, seconds)."""
    import time

    import exact_hit
    from owl_path_tracer_amd.pyhost import binding as B

    key = (name, n_per_class)
    if key not in _referee_cache:
        tris = make_scene(name)
        n = referee_rays_per_class(tris.shape[0], n_per_class)
        S = oracle_scene(orc, tris)
        host = B.Context(-1)
        host.set_option("leaf_size", 4)
        host.set_option("wide_leaves", 1)
        upload(host, tris)
        t4 = trees_of(host.export_trees())[1]
        host.close()
        used = t4.ref != -1
        planes = np.stack([t4.lo[used], t4.hi[used]], 1) if t4.n_nodes else None
        rays, cls = make_rays(tris, np.random.default_rng(4242), n, planes=planes, hit_fn=lambda r: S.intersect_n(r, use_bvh=True)[:2])
        t0 = time.time()
        tables = exact_hit.Tables(tris, rays)
        _referee_cache[key] = dict(tris=tris, rays=rays, cls=cls, tables=tables, n=n, S=S, seconds=time.time() - t0)
    return _referee_cache[key]
