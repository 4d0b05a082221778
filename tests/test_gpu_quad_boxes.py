"""The box invariant of the octant-ordered slab test (pt_trace.h, node4_step) for trees built by the device builders (bvh_builder 1:
LBVH, 2: PLOC): every non-empty quad slot has a finite box with lo <= hi (pt_debug_quad_info fails otherwise).  The host builder is
covered by tests/test_quad_boxes.py."""
import numpy as np
import pytest

from owl_path_tracer_amd.pyhost import binding as B
pytestmark = pytest.mark.gpu

MAT = np.zeros((1, 17), np.float32)
MAT[0, :3] = 0.7


def _mesh(tri_xyz):
    v = np.ascontiguousarray(np.asarray(tri_xyz, np.float32).reshape(-1, 3))
    n = np.zeros_like(v)
    n[:, 1] = 1.0
    return dict(vertices=v, normals=n, texcoords=np.zeros((v.shape[0], 2), np.float32), indices=np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3))


def _random_tris(rng, n):
    return rng.uniform(-10, 10, (n, 1, 3)) + rng.normal(0, 1.0, (n, 3, 3))


def _scenes():
    rng = np.random.default_rng(21)
    plain = _random_tris(rng, 2000)
    odd = _random_tris(rng, 2000)
    odd[0::8, 1] = odd[0::8, 0]
    odd[1::8, 2] = odd[1::8, 0] + 1e-7 * (odd[1::8, 1] - odd[1::8, 0])
    odd[2::8, 1, 0] = np.nan
    odd[3::8, 0, 1] = np.inf
    odd[4::8, :, 2] = -np.inf
    for a in range(3):
        odd[5 + a::24, :, a] = np.round(odd[5 + a::24, :1, a])
    return {"plain": plain, "odd": odd}


@pytest.mark.parametrize("builder", [1, 2])
@pytest.mark.parametrize("leaf", [1, 4])
def test_device_built_quad_boxes_are_ordered(cornell, builder, leaf):
    ctx = B.Context(0)
    try:
        ctx.set_option("bvh_builder", builder)
        ctx.set_option("leaf_size", leaf)
        ctx.upload_scene(cornell["entities"], [m for _, m, _ in cornell["materials"]])
        q = ctx.quad_info()
        assert q["triangles"] == 17974
        for name, t in _scenes().items():
            ctx.upload_scene([(_mesh(t), 0)], MAT)
            q = ctx.quad_info()
            assert q["triangles"] == len(t), name
            assert q["leaf_slots"] + q["internal_slots"] + q["empty_slots"] == 4 * q["quad_nodes"], name
    finally:
        ctx.close()
