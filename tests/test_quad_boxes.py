"""The box invariant of the octant-ordered slab test (pt_trace.h, node4_step): the quad-node step takes the lo row of an axis as the
entry plane for a positive reciprocal direction and the hi row for a negative one, which equals the per-axis min / max only when every
non-empty slot has a finite box with lo <= hi.  pt_debug_quad_info checks every slot of the host-built quad nodes (and that empty slots
carry {+inf, +inf}); these scenes push the builder at slivers, degenerate and NaN / infinite vertices."""
import numpy as np
import pytest

from owl_path_tracer_amd.pyhost import binding as B

MAT = np.zeros((1, 17), np.float32)
MAT[0, :3] = 0.7


def _mesh(tri_xyz):
    """(n, 3, 3) triangle corners -> an unindexed mesh dict"""
    v = np.ascontiguousarray(np.asarray(tri_xyz, np.float32).reshape(-1, 3))
    n = np.zeros_like(v)
    n[:, 1] = 1.0
    return dict(vertices=v, normals=n, texcoords=np.zeros((v.shape[0], 2), np.float32), indices=np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3))


def _check(tris, leaf=4):
    ctx = B.Context(-1)
    ctx.set_option("leaf_size", leaf)
    ctx.upload_scene([(_mesh(tris), 0)], MAT)
    q = ctx.quad_info()  # raises PtError when a slot breaks the invariant
    assert q["triangles"] == len(tris)
    assert q["leaf_slots"] + q["internal_slots"] + q["empty_slots"] == 4 * q["quad_nodes"]
    ctx.close()
    return q


def _random_tris(rng, n, scale=1.0):
    c = rng.uniform(-10, 10, (n, 1, 3))
    return c + rng.normal(0, scale, (n, 3, 3))


@pytest.mark.parametrize("leaf", [1, 2, 4])
def test_random_scene_boxes_are_ordered(leaf):
    _check(_random_tris(np.random.default_rng(7), 600), leaf)


def test_flat_and_axis_aligned_triangles():
    """triangles in the planes x = c, y = c, z = c: one axis of their boxes has lo == hi up to the padding"""
    rng = np.random.default_rng(11)
    t = _random_tris(rng, 300)
    for a in range(3):
        t[a::3, :, a] = np.round(t[a::3, :1, a])
    _check(t)


def test_slivers_points_and_needles():
    rng = np.random.default_rng(3)
    t = _random_tris(rng, 200)
    t[0::4, 1] = t[0::4, 0]                                     # degenerate: two equal corners
    t[1::4, 1:] = t[1::4, :1]                                   # a point
    t[2::4, 2] = t[2::4, 0] + 1e-7 * (t[2::4, 1] - t[2::4, 0])  # needle, collapsed by the sliver rule
    t[3::4, 2] = 0.5 * (t[3::4, 0] + t[3::4, 1])                # collinear
    _check(t)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nan_and_infinite_vertices(bad):
    """a triangle with a NaN or infinite coordinate collapses to its first finite corner, or to the origin when it has none
    (pt_collapse_sliver): the boxes stay finite"""
    rng = np.random.default_rng(5)
    t = _random_tris(rng, 120)
    t[0::6, 1, 0] = bad
    t[1::6, 2, 1] = bad
    t[2::6, 1:, 2] = bad
    t[3::6, 0, 0] = bad
    t[4::6, :2, 1] = bad
    t[5::12, :, 2] = bad
    _check(t)


def test_far_and_tiny_coordinates():
    rng = np.random.default_rng(9)
    t = np.concatenate([_random_tris(rng, 100, 1e-4) * 1e5, _random_tris(rng, 100, 1e-6) * 1e-3])
    _check(t)
