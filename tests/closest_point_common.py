"""Scenes, point sets and checks shared by tests/test_closest_point_host.py (CPU) and tests/test_gpu_closest_point.py (GPU):
pt_closest_point, nearest-surface queries for the caller's points.

SCENES: Cornell, the textured cube of assets/, the closed icosphere of tests/ray_battery.py with points outside and inside it, and every
scene of tests/ray_battery.py.  All of them satisfy the premise of the definition (the computed q of a triangle lies inside that
triangle's padded leaf box) on the points used here - premise() asserts it, nothing is left out.
POINT SETS, seeded, radius = +inf: points in the scene's box; points out to 5 extents around it; points ON vertices, ON the midpoints
of edges (the midpoint in float32: on a shared edge up to rounding) and in vertex regions (a vertex pushed away from its triangle's
centroid: for a closed mesh every incident triangle then reports that vertex as q - the same dd bit for bit, an exact tie).
A case is computed once per process and handed out read-only; want() is tests/closest_point_ref.py's vectorised restatement over the
case's `ref` points - a size the restatement does in seconds - and the GPU file draws more points of the same kinds for the twin."""
import os

import numpy as np

import closest_point_ref as R
import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

F32 = np.float32
BATTERY = tuple(rb.scene_names())
SCENES = ("cornell", "cube", "ico_out", "ico_in") + tuple(n for n in BATTERY if n != "cornell")
REF_PAIRS = 3_000_000  # (point, triangle) pairs the restatement visits per case, at most
_cases, _want = {}, {}


def scene_tris(name):
    if name == "cube":
        return rb._soup_of(scene_io.load_scene_dir(rb.ASSETS, "cube")["entities"])
    if name in ("ico_out", "ico_in"):
        return rb.make_closed_mesh("ico1280")[0]
    return rb.make_scene(name)


def points_of(name, tris, n, seed):
    """n points of the five kinds, (n, 3) float32."""
    rng = np.random.default_rng(seed)
    P = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max()) or 1.0
    k = max(1, n // 5)
    if name == "ico_in":
        c = 0.5 * (lo + hi)
        box = c + rng.uniform(-0.9, 0.9, (2 * k, 3)) * rb.CLOSED_RADIUS / np.sqrt(3.0)
        far = box[k:]
        box = box[:k]
    else:
        box = lo + rng.random((k, 3)) * (hi - lo)
        far = lo - 5.0 * ext + rng.random((k, 3)) * (hi - lo + 10.0 * ext)
    t = tris[rng.integers(0, tris.shape[0], k)]
    c = rng.integers(0, 3, k)
    vtx = t[np.arange(k), c]
    t = tris[rng.integers(0, tris.shape[0], k)]
    c = rng.integers(0, 3, k)
    mid = ((t[np.arange(k), c] + t[np.arange(k), (c + 1) % 3]) * F32(0.5)).astype(F32)
    t = tris[rng.integers(0, tris.shape[0], n - 4 * k)].astype(np.float64)
    c = rng.integers(0, 3, t.shape[0])
    v = t[np.arange(t.shape[0]), c]
    away = v - t.mean(1)
    away /= np.maximum(np.linalg.norm(away, axis=1, keepdims=True), 1e-300)
    reg = v + away * ext * rng.uniform(0.01, 0.5, (t.shape[0], 1)) * (-1.0 if name == "ico_in" else 1.0) * (0.2 if name == "ico_in" else 1.0)
    return np.ascontiguousarray(np.concatenate([box, far, vtx, mid, reg]), F32)


def case(name):
    """dict(name, tris (n, 3, 3) as uploaded, T (the same after the sliver rule, id order), ref (POINT_DTYPE), extent, E, upload(ctx))."""
    if name in _cases:
        return _cases[name]
    tris = np.ascontiguousarray(scene_tris(name), F32)
    T = R.triangles(tris)
    n_ref = int(np.clip(REF_PAIRS // max(1, tris.shape[0]), 120, 2000))
    ref = B.make_points(points_of(name, tris, n_ref, 20261021))
    for a in (tris, T, ref):
        a.setflags(write=False)
    P = tris.reshape(-1, 3).astype(np.float64)
    _cases[name] = dict(name=name, tris=tris, T=T, ref=ref, extent=float(np.ptp(P, axis=0).max()), E=rb.scene_measure(tris), upload=lambda ctx, tris=tris: rb.upload(ctx, tris))
    return _cases[name]


def want(name):
    if name not in _want:
        c = case(name)
        w = R.closest(c["T"], c["ref"])
        w.setflags(write=False)
        _want[name] = w
    return _want[name]


def more_points(name, n, seed=7):
    """n further points of the same kinds for the comparisons that need no restatement."""
    return B.make_points(points_of(name, case(name)["tris"], n, seed))


def needle_scene():
    """((52, 3, 3) triangles, (n, 3) points): 50 needles (height 1e-6 over a base of 1: collapsed by the sliver rule) scattered over a
    quad at z = -3 (ids 50 and 51), and points on the needles' first corners - where they collapse to - and within 0.2 of the needles."""
    i = np.arange(50, dtype=np.float64)
    b = np.stack([i, 3.0 * (i % 5), 2.0 * (i % 7)], 1)
    needles = np.stack([b, b + [1, 0, 0], b + [0.5, 1e-6, 0]], 1)
    quad = [[[-1, -1, -3], [51, -1, -3], [51, 13, -3]], [[-1, -1, -3], [51, 13, -3], [-1, 13, -3]]]
    tris = np.concatenate([needles, quad]).astype(F32)
    rng = np.random.default_rng(2)
    x = (b[rng.integers(0, 50, 3000)] + np.stack([rng.uniform(0, 1, 3000), rng.uniform(-0.2, 0.2, 3000), rng.uniform(0.0, 0.2, 3000)], 1)).astype(F32)
    x[:50] = tris[:50, 0]
    return tris, x


def assert_same(got, wanted, what):
    bad = R.differ(got, wanted)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d records differ; first: point %d\n got  %r\n want %r" % (what, int(bad.sum()), bad.size, i, got[i], wanted[i]))


# ---------------------------------------------------------------------------------------------------------------------
# the premise: q inside the padded leaf box of its triangle, from the hierarchy the context holds
# ---------------------------------------------------------------------------------------------------------------------
def leaf_boxes(ctx, n_tris):
    """(lo, hi) (n_tris, 3) by global id: the quad tree's box of the leaf that holds the triangle; None where the root is a leaf (no
    box is ever tested: the premise is vacuous)."""
    ex = ctx.export_trees()
    T4 = rb.trees_of(ex)[1]
    if T4.n_nodes == 0:
        return None
    lt = ex["tris"]
    real = lt["id"] != R.NO_ID
    slot_of = np.full(n_tris, -1, np.int64)
    slot_of[lt["id"][real]] = np.nonzero(real)[0]
    assert (slot_of >= 0).all()
    ls = rb.TreePaths(T4, lt.size).leaf_slot[slot_of]
    assert (ls >= 0).all()
    return T4.lo[ls], T4.hi[ls]


def premise(ctx, c, pts, rec, n_all=24):
    """Asserts the premise for the winner of every point (rec: the records of pts) and for EVERY triangle on a seeded subsample of
    n_all points.  Returns (pairs checked, False if vacuous)."""
    boxes = leaf_boxes(ctx, c["T"].shape[0])
    if boxes is None:
        return 0, False
    blo, bhi = boxes
    found = rec["prim"] >= 0
    w = rec["prim"][found]
    q = rec["q"][found]
    ok = ((q >= blo[w]) & (q <= bhi[w])).all(1)
    assert ok.all(), "%s: the winner's q lies outside its padded leaf box for %d of %d points" % (c["name"], (~ok).sum(), ok.size)
    sub = np.random.default_rng(99).choice(pts.shape[0], min(n_all, pts.shape[0]), replace=False)
    r = R.tri_all(c["T"], pts["p"][sub].astype(F32))
    gone = R.collapsed(c["T"])
    inside = ((r["q"] >= blo[None]) & (r["q"] <= bhi[None])).all(2) | gone[None]
    assert inside.all(), "%s: q of %d (point, triangle) pairs lies outside the triangle's padded leaf box" % (c["name"], (~inside).sum())
    return int(ok.size + inside.size), True
