"""pt_trace_ao in the middle of a context's life: ONE context, a fixed sequence of pt_render, pt_set_materials, pt_update_vertices and
option changes with an ambient-occlusion call after each, blocking and on caller streams by turns, every AO call held to the CPU twin
of a FRESH host-only context in the model's state (so nothing stale on the context under test can agree with itself) on the records
tests/ao_ref.py's rule compares, and the renders around it to each other where the state is the same."""
import numpy as np
import pytest

import ao_common as AC
import ao_ref
import async_common as AS
import ray_battery as rb
import surface_common as SC
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io
from test_gpu_trace_ao import DevAo

pytestmark = pytest.mark.gpu


def _mask(orc, tris, rays, cls, K, flags, seed, wt):
    S = rb.oracle_scene(orc, tris)
    S.set_watertight(bool(wt))
    flat = SC.battery_flat(tris)
    truth = S.intersect_n(rays, use_bvh=False)
    prep = ao_ref.prepare(S, flat, rays, truth, flags, seed, K)
    return TC.compared(tris, rays, cls) & ao_ref.compared(S, flat, rays, truth, prep, K)


def _fresh_twin(tris, rec, prm, wt):
    h = B.Context(-1)
    h.set_option("watertight", wt)
    rb.upload(h, tris)
    out = h.trace_ao_host(rec, prm)
    h.close()
    return out


def test_ao_between_renders_and_scene_changes(orc):
    tris, moved = TC.moved_scene()
    bt = TC.battery(orc, "soup1")
    rays, cls = bt["rays"][:1500], bt["cls"][:1500]
    rec = B.make_rays(rays)
    ctx = B.Context(0)
    ctx.set_option("dynamic", 1)
    ctx.upload_scene([(rb.mesh_of(tris), 0)], [scene_io.MAT_DEFAULT], env=B.make_env(color=(1, 1, 1), intensity=1.0))
    P = tris.reshape(-1, 3).astype(np.float64)
    c = 0.5 * (P.min(0) + P.max(0))
    ext = float(np.ptp(P, axis=0).max())
    W, H = 40, 30
    cam = B.to_camera_data(list(c + [0, 0, 2.0 * ext]), list(c), [0, 1, 0], 40.0, W, H)
    red = scene_io.material(base_color=(1.0, 0.2, 0.2))
    state = dict(tris=tris, wt=0)
    d = DevAo(rec)
    step = [0]

    def ao(K, flags, radius, seed, device):
        step[0] += 1
        prm = B.ao_default_params(n_rays=K, flags=flags, radius=radius, seed=seed)
        if device:
            ctx.trace_ao_device(d.rays, d.n, d.out, prm, stream=AS.stream(step[0] % 2))
            ctx.synchronize()
            got, tail = d.read()
            got = got.copy()
            assert (tail == AS.FILL).all()
        else:
            got = ctx.trace_ao(rec, prm)
        what = "call %d (K=%d flags=%d radius=%g seed=%d, %s, watertight %d)" % (step[0], K, flags, radius, seed, "device" if device else "blocking", state["wt"])
        m = _mask(orc, state["tris"], rays, cls, K, flags, seed, state["wt"])
        AC.assert_same(got, _fresh_twin(state["tris"], rec, prm, state["wt"]), m, what)
        AC.assert_same(got, ctx.trace_ao_host(rec, prm), m, what + ", the context's own twin")
        return got

    try:
        a0 = ao(4, 0, 0.25 * ext, 1, False)
        r0, _ = ctx.render(cam, W, H, 4, 4)
        a1 = ao(4, 0, 0.25 * ext, 1, True)
        assert not ao_ref.differ(a0, a1).any(), "a render in between changes nothing"
        r1, _ = ctx.render(cam, W, H, 4, 4)
        assert (r0.view(np.uint32) == r1.view(np.uint32)).all(), "nor does AO change a render"
        ctx.set_materials(np.stack([red]).astype(np.float32))
        a2 = ao(4, 0, 0.25 * ext, 1, True)
        assert not ao_ref.differ(a0, a2).any(), "materials are not read"
        ctx.render(cam, W, H, 4, 4)
        ctx.update_vertices([rb.mesh_of(moved)])
        state["tris"] = moved
        a3 = ao(6, 1, float("inf"), 2, False)
        ctx.render(cam, W, H, 4, 4)
        a4 = ao(4, 0, 0.25 * ext, 1, True)
        assert ao_ref.differ(a0, a4).any(), "the deformation changes records"
        ctx.set_option("watertight", 1)
        state["wt"] = 1
        ao(3, 0, 0.5 * ext, 3, True)
        ctx.set_option("watertight", 0)
        state["wt"] = 0
        ctx.update_vertices([rb.mesh_of(tris)])
        state["tris"] = tris
        a6 = ao(4, 0, 0.25 * ext, 1, False)
        assert not (ao_ref.differ(a0, a6) & _mask(orc, tris, rays, cls, 4, 0, 1, 0)).any(), "back in the first state"
        assert a3.shape == a0.shape
    finally:
        AS.destroy_streams()
        d.free()
        ctx.close()
