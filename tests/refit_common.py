"""Scenes, movements and the box definition shared by tests/test_refit_host.py (CPU) and tests/test_gpu_refit.py (GPU).

A SCENE here is a list of (mesh dict, material index) as Context.upload_scene takes it.  Every scene ends in a small SLIVER MESH: flat
triangles of base 1 and height h over it, h on both sides of the sliver threshold (height <= 1e-5 of the longest edge: never hit,
collapsed to a point at upload and at every update), and triangles with NaN / infinite corners.  The movement rolls the list of
heights, so that with every update some triangles cross the threshold in each direction.

THE MOVEMENT (moved(scene, k)), three parts: a smooth wobble of every vertex, a rigid shift of one mesh by about 3 extents (so that
the extent, hence the pad of every box, changes), and the sliver mesh with its heights rolled by k.  k = 0 is the scene itself.

THE DEFINITION (expected_boxes): the box of a slot is the float32 min / max over the vertices of the collapsed triangles below it, then
one float32 -/+ pad, pad = float32(ext) * float32(1e-5), ext = the largest of the scene's extents and absolute coordinates; an empty
slot is {+inf, +inf}.  Computed in numpy from triangle records by id, on whatever topology the read-back shows.
"""
import os

import numpy as np

import ray_battery as rb
from owl_path_tracer_amd.pyhost import scene_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
F32 = np.float32
PAD_ID = 0x7fffffff
ARRAYS = ("nodes", "nodes4", "nodes8", "tris")
# heights over a base of length 1: the threshold is 1e-5 (|e1 x e2|^2 <= 1e-10 max|e|^4)
SLIVER_HEIGHTS = (0.5e-5, 0.98e-5, 0.9999e-5, 1.0001e-5, 1.02e-5, 2e-5, 1e-3, 0.25)


def sliver_mesh(k=0, scale=0.3, at=(0.0, 0.0, 0.0)):
    """len(SLIVER_HEIGHTS) flat triangles with the heights rolled by k, then four triangles with non-finite corners (NaN first corner,
    infinite middle corner, all corners non-finite, one finite corner last).  Unindexed: 3 vertices per triangle."""
    hs = np.roll(np.asarray(SLIVER_HEIGHTS, np.float64), k)
    t = []
    for i, h in enumerate(hs):
        a = 0.7 * i  # every triangle in its own rotated frame, stacked along y
        ex, ez = np.array([np.cos(a), 0.0, np.sin(a)]), np.array([-np.sin(a), 0.0, np.cos(a)])
        o = np.array([0.0, 0.1 * i, 0.0])
        t.append([o, o + ex, o + 0.5 * ex + h * ez])
    t = np.asarray(t, np.float64) * scale + np.asarray(at, np.float64)
    nan, inf = np.nan, np.inf
    p = np.asarray(at, np.float64)
    bad = [[[nan, 0, 0], p + [0.1, 0, 0], p + [0, 0.1, 0]], [p, [inf, 1, 1], p + [0, 0.1, 0.1]], [[nan] * 3, [nan, inf, 0], [-inf] * 3],
           [[inf, 0, 0], [0, nan, 0], p + [0.2, 0.2, 0.2]]]
    v = np.concatenate([t, np.asarray(bad, np.float64)]).reshape(-1, 3).astype(F32)
    return dict(vertices=v, normals=np.tile(F32([0, 1, 0]), (v.shape[0], 1)), texcoords=np.zeros((0, 2), F32), indices=np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3),
                sliver=True, _scale=scale, _at=tuple(at))


def _finite_sliver_mesh(k=0, scale=0.3, at=(0.0, 0.0, 0.0)):
    """The sliver mesh without its non-finite and huge triangles: for the scenes the oracle renders or traces."""
    m = sliver_mesh(k, scale, at)
    n = 3 * len(SLIVER_HEIGHTS)
    return dict(m, vertices=m["vertices"][:n], normals=m["normals"][:n], indices=m["indices"][: n // 3], finite_only=True)


def _soup(tris):
    return rb.mesh_of(np.asarray(tris, F32))


def _with_unreferenced(mesh, extra):
    """The mesh with vertices nobody indexes appended (huge and non-finite ones): they must not move the pad."""
    extra = np.asarray(extra, F32).reshape(-1, 3)
    return dict(mesh, vertices=np.concatenate([mesh["vertices"], extra]).astype(F32), normals=np.concatenate([mesh["normals"], np.tile(F32([0, 1, 0]), (extra.shape[0], 1))]).astype(F32))


def scene_names():
    return ["one_tri", "two_tris", "meshes", "rects", "cornell"]


def make_scene(name):
    """(entities, number of materials, index of the mesh the movement shifts).  one_tri has no sliver mesh (its root is a leaf code:
    no node at all); two_tris neither (one node at leaf size 1)."""
    if name == "one_tri":
        return [(_soup([[[0, 0, 0], [1, 0, 0], [0, 1, 0.5]]]), 0)], 1, 0
    if name == "two_tris":
        return [(_soup([[[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[2, 0, 0], [2, 1, 0], [2, 0, 1]]]), 0)], 1, 0
    if name == "meshes":
        # four meshes with different vertex bases: an icosphere with unreferenced huge / non-finite vertices, a mesh of 0 triangles that
        # still has vertices, a few rectangles, the sliver mesh
        ico = _with_unreferenced(_soup(rb.icosphere(1) * F32(0.8) + F32([0.3, 1.0, -0.2])), [[1e30, -1e30, 1e25], [np.nan, 0, 0], [np.inf, -np.inf, 1], [3e38, 3e38, -3e38]])
        none = dict(vertices=F32([[5, 5, 5], [np.nan, 1, 1], [1e20, 0, 0]]), normals=np.tile(F32([0, 1, 0]), (3, 1)), texcoords=np.zeros((0, 2), F32), indices=np.zeros((0, 3), np.int32))
        rects = _soup(rb.rect_scene(np.random.default_rng(5), n=12))
        return [(ico, 0), (none, 0), (rects, 0), (sliver_mesh(at=(-1.5, -0.5, 0.5)), 0)], 1, 0
    if name == "rects":
        return [(_soup(rb.rect_scene(np.random.default_rng(11))), 0), (_finite_sliver_mesh(at=(0.1, 0.2, 0.6)), 0)], 1, 1
    if name == "soup2":
        return [(_soup(rb.make_scene("soup2")), 0), (_finite_sliver_mesh(at=(0.1, 0.2, 0.6)), 0)], 1, 1
    if name == "cornell":  # 17 974 triangles (the sphere: 17 952): every level of the tree spans several blocks of the refit kernels
        sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
        ents = list(sc["entities"])
        # the light hangs a quarter unit below the ceiling here: the wobble bends the ceiling's two large triangles and the small light
        # differently, and a light that ends up above the ceiling leaves a black frame, which shows nothing
        light = [i for i, (_, mid) in enumerate(ents) if sc["materials"][mid][0] == "light"][0]
        ents[light] = (dict(ents[light][0], vertices=(ents[light][0]["vertices"] - F32([0, 0.25, 0])).astype(F32)), ents[light][1])
        ents.append((_finite_sliver_mesh(scale=0.2, at=(-0.5, 0.3, 0.2)), 0))
        return ents, len(sc["materials"]), 0  # the movement shifts the box (10 triangles, material 0)
    raise KeyError(name)


def cornell_materials():
    """The Cornell box's (name, 17 floats, texture name) list: the scene "cornell" above uses these material indices."""
    return scene_io.load_scene_dir(ASSETS, "cornell-box")["materials"]


CORNELL_ENV = dict(color=(1, 1, 1), intensity=0.0)


def cornell_camera(W, H, make):
    """make = B.to_camera_data or the oracle's"""
    c = scene_io.load_scene_dir(ASSETS, "cornell-box")["camera"]
    return make(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)


def soup_of(entities):
    """(n, 3, 3) float32 triangles in global id order (entity order, then face order)."""
    parts = [m["vertices"][m["indices"]].astype(F32).reshape(-1, 3, 3) for m, _ in entities if m["indices"].shape[0]]
    return np.concatenate(parts) if parts else np.zeros((0, 3, 3), F32)


def extent_of(entities):
    """Extent of the finite vertices that triangles use (float64; the scale of the movement only)."""
    P = soup_of(entities).reshape(-1, 3).astype(np.float64)
    P = P[np.isfinite(P).all(1) & (np.abs(P) < 1e20).all(1)]
    return float((P.max(0) - P.min(0)).max()) if P.size else 1.0


def moved(scene, k, amp=0.03, with_normals=False):
    """Update k of the scene: the list of mesh dicts for Context.update_vertices (same counts as the upload), k = 0 the uploaded arrays.
    amp: wobble amplitude in extents.  with_normals: the normals move as well (rotated about y by 0.3 k rad, still of unit length)."""
    entities, _, shift = scene
    ext = extent_of(entities)
    out = []
    for i, (m, _) in enumerate(entities):
        if m.get("sliver"):
            new = (_finite_sliver_mesh if m.get("finite_only") else sliver_mesh)(k, m["_scale"], m["_at"])
            v = new["vertices"]
        else:
            v = m["vertices"].astype(np.float64)
            if k:
                with np.errstate(invalid="ignore", over="ignore"):
                    w = amp * ext * np.sin(v[:, [1, 2, 0]] * (2.0 / ext) + 0.9 * k + np.arange(3))
                    v = np.where(np.isfinite(v) & (np.abs(v) < 1e20), v + w, v)
                if i == shift:
                    v = v + np.array([3.0, 0.4, -2.5]) * ext * (1 if k % 2 else -1)
            v = v.astype(F32)
        d = dict(m, vertices=v)
        if with_normals and not m.get("sliver"):
            a = 0.3 * k
            R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            d["normals"] = (m["normals"].astype(np.float64) @ R.T).astype(F32)
        out.append(d)
    return out


def as_entities(scene, meshes):
    """The moved meshes as an entity list for a fresh upload_scene."""
    return [(m, mid) for m, (_, mid) in zip(meshes, scene[0])]


def materials_of(scene):
    return [scene_io.MAT_DEFAULT] * scene[1]


def upload(ctx, scene, meshes=None, **kw):
    ctx.upload_scene(as_entities(scene, meshes) if meshes is not None else scene[0], kw.pop("materials", None) or materials_of(scene), **kw)


def same_arrays(a, b, what, keys=ARRAYS):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), "%s: array '%s' differs" % (what, k)
    for k in ("root", "root4", "root8", "depth", "depth4", "depth8", "max_leaf"):
        assert a[k] == b[k], "%s: %s" % (what, k)


def tris_by_id(ex):
    """The live triangle records sorted by id."""
    t = ex["tris"]
    t = t[t["id"] != PAD_ID]
    return t[np.argsort(t["id"], kind="stable")]


def point_triangles(ex):
    t = tris_by_id(ex)
    return int(((t["p0"] == t["p1"]) & (t["p0"] == t["p2"])).all(1).sum())


def expected_pad(V):
    """pad of the definition from collapsed triangles V (n, 3, 3) float32: float32 arithmetic throughout."""
    if V.shape[0] == 0:
        return F32(0)
    P = V.reshape(-1, 3)
    mn, mx = P.min(0), P.max(0)
    ext = F32(0)
    for a in range(3):
        ext = max(ext, F32(mx[a] - mn[a]), F32(abs(mn[a])), F32(abs(mx[a])))
    return F32(F32(ext) * F32(1e-5))


def expected_boxes(ex, V):
    """For the three trees of a read-back: (tree, expected lo, expected hi) per slot, from the definition.  V: collapsed triangles by id
    (from a FRESH upload of the same vertices), so nothing here comes from the refit under test but the topology."""
    tris = ex["tris"]
    live = tris["id"] != PAD_ID
    Vs = np.zeros((tris.size, 3, 3), F32)
    Vs[live] = V[tris["id"][live]]
    vlo, vhi = Vs.min(1), Vs.max(1)
    pad = expected_pad(V)
    out = []
    for T in rb.trees_of(ex):
        if T.n_nodes == 0:
            continue
        slo = np.full((T.ref.size, 3), np.inf, F32)
        shi = np.full((T.ref.size, 3), -np.inf, F32)
        order, stack = [], [T.root]
        while stack:
            i = stack.pop()
            order.append(i)
            stack += [int(r) for r in T.ref[i * T.width:(i + 1) * T.width] if r >= 0]
        for i in reversed(order):
            for s in range(i * T.width, (i + 1) * T.width):
                r = int(T.ref[s])
                if r >= 0:
                    slo[s] = slo[r * T.width:(r + 1) * T.width].min(0)
                    shi[s] = shi[r * T.width:(r + 1) * T.width].max(0)
                elif r < -1:
                    f, c = (int(x) for x in rb.leaf_range(r))
                    m = live[f:f + c]
                    slo[s] = vlo[f:f + c][m].min(0)
                    shi[s] = vhi[f:f + c][m].max(0)
        used = T.ref != -1
        lo = np.where(used[:, None], (slo - pad).astype(F32), F32(np.inf))
        hi = np.where(used[:, None], (shi + pad).astype(F32), F32(np.inf))
        reach = np.zeros(T.ref.size, bool)  # slots of nodes the root reaches (the sibling-pair layout leaves holes)
        for i in order:
            reach[i * T.width:(i + 1) * T.width] = True
        out.append((T, lo, hi, reach, pad))
    return out


def assert_boxes(ex, V, what):
    """Every slot's box equals the definition bit for bit (by value should the pad be 0: only then can the sign of a zero show)."""
    pad = expected_pad(V)
    assert F32(ex["pad"]).view(np.uint32) == pad.view(np.uint32), "%s: pad %r, definition %r" % (what, ex["pad"], pad)
    for T, lo, hi, reach, _ in expected_boxes(ex, V):
        for got, want, row in ((T.lo, lo, "lo"), (T.hi, hi, "hi")):
            g, w = np.ascontiguousarray(got[reach]), np.ascontiguousarray(want[reach])
            bad = (g != w) if pad == 0 else (g.view(np.uint32) != w.view(np.uint32))
            assert not bad.any(), "%s: %s tree, %d %s planes differ from the definition; first slot %d: %r, want %r" % (
                what, T.name, bad.sum(), row, np.nonzero(bad.any(1))[0][0], g[bad.any(1)][0].tolist(), w[bad.any(1)][0].tolist())
