"""pt_trace_closest / pt_trace_occluded on the GPU, ray by ray against the oracle's brute force (include/mi355pt.h "ray queries").

Every comparison is bit for bit on the rays tests/trace_rays_common.py compares (classes 1-6, class 7 up to DOMAIN_EXTENTS); the truth is
computed once per scene and shared with tests/test_trace_rays_host.py.
* both calls, blocking and device forms, for n = 1, 63, 64, 65, 130 (partial waves, a tail) and the 2000-per-class battery of every scene;
* the per-ray tmax cases of the CPU file (+inf, NaN, 1e10, -1, 1e-3, half t, exactly t, nextafter(t, 0)) through both calls and forms;
* the lane refill: ranges of thousands of rays per wave (option "rays_grid"), and the battery tiled past the resident waves on the library's
  own grid, each at "rays_refill" default, 0, 16 and 63 against the oracle and byte-identical to each other;
* "box_exact" 0 and 1; "watertight" on the closed icosphere;
* the sliver strip, whose quad walk needs more stack than LDS holds (asserted with probe op 32: aux > 12 for compared battery rays): the HBM overflow column;
* after pt_update_vertices; a pt_render before and after the calls; one ordering leg over two caller streams; pt_get_stats."""
import ctypes as C
import os

import numpy as np
import pytest

import async_common as AS
import ray_battery as rb
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

pytestmark = pytest.mark.gpu

ROOT = rb.ROOT
ASSETS = os.path.join(ROOT, "assets")


class DevRays:
    """n rays in HBM and room for both results, every output byte 0xA5 until a call writes it."""

    def __init__(self, rec):
        self.n = rec.shape[0]
        self.sizes = (self.n * 32, self.n * 16, self.n)
        self.p = [C.c_void_p() for _ in self.sizes]
        for p, b in zip(self.p, self.sizes):
            AS._ok(AS.hip().hipMalloc(C.byref(p), max(b, 16)), "hipMalloc")
            AS._ok(AS.hip().hipMemset(p, AS.FILL, max(b, 16)), "hipMemset")
        AS._ok(AS.hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        AS.to_device(self.p[0].value, rec)
        self.rays, self.hits, self.occ = (p.value for p in self.p)

    def read(self):
        hits, occ = np.empty(self.n, B.HIT_DTYPE), np.empty(self.n, np.uint8)
        AS._ok(AS.hip().hipMemcpy(hits.ctypes.data_as(C.c_void_p), self.p[1], self.sizes[1], AS.D2H), "hipMemcpy")
        AS._ok(AS.hip().hipMemcpy(occ.ctypes.data_as(C.c_void_p), self.p[2], self.sizes[2], AS.D2H), "hipMemcpy")
        return hits, occ

    def free(self):
        for p in self.p:
            if p.value:
                AS.hip().hipFree(p)
                p.value = None


def _ctx(tris, **opts):
    ctx = B.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    rb.upload(ctx, tris)
    return ctx


def _all_four(ctx, rec):
    """(closest, occluded) of the blocking forms and of the device forms on the context's own stream."""
    hits, occ = ctx.trace_closest(rec), ctx.trace_occluded(rec)
    d = DevRays(rec)
    try:
        ctx.trace_closest_device(d.rays, d.n, d.hits)
        ctx.trace_occluded_device(d.rays, d.n, d.occ)
        ctx.synchronize()
        dh, do = d.read()
    finally:
        d.free()
    return hits, occ, dh, do


def _check(ctx, rec, want_hits, want_occ, mask, what, rays=None, cls=None):
    hits, occ, dh, do = _all_four(ctx, rec)
    TC.assert_same(hits, want_hits, mask, what + ": pt_trace_closest", rays, cls)
    TC.assert_same(occ, want_occ, mask, what + ": pt_trace_occluded", rays, cls)
    assert TC.same(dh, hits).all() and TC.same(do, occ).all(), what + ": the device forms store what the blocking forms return"
    assert (occ <= 1).all()
    return hits, occ


@pytest.mark.parametrize("name", rb.scene_names())
def test_battery_against_brute_force(orc, name):
    bt = TC.battery(orc, name)
    ctx = _ctx(bt["tris"])
    _check(ctx, B.make_rays(bt["rays"]), bt["hits"], bt["occ"], bt["mask"], name, bt["rays"], bt["cls"])
    ctx.close()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_small_counts(orc, n):
    bt = TC.battery(orc, "soup1")
    idx = np.nonzero(bt["mask"])[0][:: max(1, int(bt["mask"].sum()) // n)][:n]  # spread over the classes
    assert idx.size == n
    ctx = _ctx(bt["tris"])
    _check(ctx, B.make_rays(bt["rays"][idx]), bt["hits"][idx], bt["occ"][idx], None, "n = %d" % n, bt["rays"][idx])
    assert ctx.stats()["grid"] == (n + 63) // 64
    ctx.close()


@pytest.mark.parametrize("name", TC.TMAX_SCENES)
def test_per_ray_tmax(orc, name):
    """+inf, NaN, 1e10, -1, 1e-3, half the ray's t, exactly its t, nextafter(t, 0) - the cases of tests/test_trace_rays_host.py through
    both calls in both forms."""
    bt = TC.battery(orc, name)
    ctx = _ctx(bt["tris"])
    for label, rec, want_hits, want_occ, mask in TC.tmax_cases(orc, name):
        _check(ctx, rec, want_hits, want_occ, mask, "%s: %s" % (name, label))
    ctx.close()


def test_n_zero_is_ok_and_launches_nothing(orc):
    ctx = _ctx(rb.make_scene("one_leaf"))
    none = np.zeros(0, B.RAY_DTYPE)
    assert ctx.trace_closest(none).shape == (0,) and ctx.trace_occluded(none).shape == (0,)
    ctx.trace_closest_device(0, 0, 0)
    ctx.trace_occluded_device(0, 0, 0)
    ctx.synchronize()
    ctx.close()


REFILLS = (0, 16, 63)  # a new batch only when the whole wave is done / an intermediate value / whenever a lane is idle


def _refill_sweep(ctx, rec, want_hits, want_occ, mask, what, ranges_longer_than):
    """Both calls, blocking and device forms, at the default and at REFILLS, each against the oracle; every wave's range is longer than
    `ranges_longer_than` rays (from pt_get_stats: grid * that < n), so lanes ARE refilled - with a range of 64 rays the first round hands
    every ray out and no setting matters."""
    n = rec.shape[0]
    base = None
    for r in (None,) + REFILLS:
        if r is not None:
            ctx.set_option("rays_refill", r)
        hits, occ = _check(ctx, rec, want_hits, want_occ, mask, "%s, rays_refill %s" % (what, "default" if r is None else r))
        grid = ctx.stats()["grid"]
        assert grid * ranges_longer_than < n and grid < (n + 63) // 64, "precondition: a wave's range is longer than %d rays (grid %d, %d rays)" % (ranges_longer_than, grid, n)
        if base is None:
            base = (hits, occ)
        assert TC.same(hits, base[0]).all() and TC.same(occ, base[1]).all(), "rays_refill = %s changes a result" % r  # every ray, compared or not


def test_refill_on_long_ranges(orc):
    """Option "rays_grid" = 5: five waves share the battery, some 4000 rays - 66 blocks - each, so a wave refills its lanes thousands of
    times; the mixed per-ray bounds ride along, so a refilled lane must take its OWN ray's bound."""
    for name in ("dragon", "strip"):
        bt = TC.battery(orc, name)
        ctx = _ctx(bt["tris"], rays_grid=5, **(dict(leaf_size=1) if name == "strip" else {}))  # (strip: refills next to lanes whose stack is in HBM)
        _refill_sweep(ctx, B.make_rays(bt["rays"]), bt["hits"], bt["occ"], bt["mask"], name + ", five waves", 3000)
        ctx.close()
    bt = TC.battery(orc, "cornell")
    label, rec, want_hits, want_occ, mask = TC.tmax_cases(orc, "cornell")[-1]
    ctx = _ctx(bt["tris"], rays_grid=1)  # one wave, 240 rays with eight kinds of bound
    _refill_sweep(ctx, rec, want_hits, want_occ, mask, "cornell, one wave, " + label, 128)
    ctx.close()


def test_refill_on_the_grid_of_the_occupancy_query(orc):
    """No option: the battery tiled until there are more 64-ray blocks than resident waves, so the library's own grid gives every wave
    several blocks.  The expectations are the battery's, tiled."""
    bt = TC.battery(orc, "soup1")
    ctx = _ctx(bt["tris"])
    ctx.trace_occluded(B.make_rays(bt["rays"]))
    n1 = bt["rays"].shape[0]
    assert ctx.stats()["grid"] == (n1 + 63) // 64  # one block per wave: the battery alone refills nothing
    resident = 256 * 32  # more waves than any gfx950 part keeps resident (256 CUs x 32 wave slots); the precondition below is what counts
    tiles = (2 * 64 * resident + n1 - 1) // n1
    rec = np.tile(B.make_rays(bt["rays"]), tiles)
    _refill_sweep(ctx, rec, np.tile(bt["hits"], tiles), np.tile(bt["occ"], tiles), np.tile(bt["mask"], tiles), "soup1 x %d" % tiles, 64)
    ctx.close()


@pytest.mark.parametrize("exact", (0, 1))
def test_box_exact(orc, exact):
    for name in ("rects", "soup_offset30"):
        bt = TC.battery(orc, name)
        ctx = _ctx(bt["tris"], box_exact=exact)
        _check(ctx, B.make_rays(bt["rays"]), bt["hits"], bt["occ"], bt["mask"], "%s, box_exact %d" % (name, exact), bt["rays"], bt["cls"])
        ctx.close()


def test_watertight_on_the_closed_mesh(orc):
    tris, rays, mt, wt = TC.closed_case(orc)
    assert wt[0].all()
    rec = B.make_rays(rays)
    ctx = _ctx(tris, watertight=1)
    _, occ = _check(ctx, rec, TC.hits_of(wt), wt[0].astype(np.uint8), None, "closed mesh, watertight", rays)
    assert (occ == 1).all(), "no aimed ray leaves a closed mesh under the watertight test"
    ctx.set_option("watertight", 0)
    _check(ctx, rec, TC.hits_of(mt), mt[0].astype(np.uint8), None, "closed mesh, Moeller-Trumbore", rays)
    ctx.close()
    bt = TC.battery(orc, "rects", watertight=True)  # and the battery of one scene under the watertight test
    ctx = _ctx(bt["tris"], watertight=1)
    _check(ctx, B.make_rays(bt["rays"]), bt["hits"], bt["occ"], bt["mask"], "rects, watertight", bt["rays"], bt["cls"])
    ctx.close()


def test_overflow_column_is_walked(orc):
    """The sliver strip: probe op 32 says that battery rays push past the 12 LDS levels of the stack, so their walks use the wave's HBM
    overflow column.  One triangle per leaf, as tests/test_gpu_ray_probes.py uploads the strip for the same purpose: the deepest tree
    the scene gives."""
    bt = TC.battery(orc, "strip")
    ctx = _ctx(bt["tris"], leaf_size=1)
    depth4 = ctx.export_trees()["depth4"]
    assert 3 * depth4 + 1 > B.PT_LDS_STACK
    aux = ctx.debug_eval("quad_ovf", bt["rays"], 6)[:, 5]  # probe op 32: the deepest stack level of each ray's walk
    deep = aux > B.PT_LDS_STACK
    print("deepest stack entry %d; %d of %d battery rays go past LDS entry %d, %d of them compared" % (aux.max(), deep.sum(), aux.size, B.PT_LDS_STACK, (deep & bt["mask"]).sum()))
    assert (deep & bt["mask"]).any(), "precondition: no compared battery ray's walk goes past LDS entry %d" % B.PT_LDS_STACK
    _check(ctx, B.make_rays(bt["rays"]), bt["hits"], bt["occ"], bt["mask"], "strip, leaf_size 1", bt["rays"], bt["cls"])
    assert ctx.stats()["stack_entries"] == 3 * depth4 + 1
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    rays = TC.battery(orc, "soup1")["rays"]
    cls = TC.battery(orc, "soup1")["cls"]
    truth = rb.oracle_scene(orc, moved).intersect_n(rays, use_bvh=False)
    mask = TC.compared(moved, rays, cls)
    ctx = _ctx(tris, dynamic=1)
    ctx.update_vertices([rb.mesh_of(moved)])
    hits, occ = _check(ctx, B.make_rays(rays), TC.hits_of(truth), truth[0].astype(np.uint8), mask, "after pt_update_vertices", rays, cls)
    ctx.close()
    fresh = _ctx(moved)
    assert TC.same(fresh.trace_closest(rays), hits, mask).all() and TC.same(fresh.trace_occluded(rays), occ, mask).all()
    fresh.close()


def _cornell():
    sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
    ctx = B.Context(0)
    ctx.upload_scene(sc["entities"], [m for _, m, _ in sc["materials"]], env=B.make_env(color=(1, 1, 1), intensity=0.0))
    c = sc["camera"]
    W = H = 48
    return ctx, B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H), W, H


def test_render_state_is_untouched(orc):
    bt = TC.battery(orc, "cornell")
    rec = B.make_rays(bt["rays"][:3000])
    ctx, cam, W, H = _cornell()
    before, _ = ctx.render(cam, W, H, 8, 8)
    ctx.trace_closest(rec)
    ctx.trace_occluded(rec)
    after, _ = ctx.render(cam, W, H, 8, 8)
    assert (before.view(np.uint32) == after.view(np.uint32)).all()
    ctx.close()


def test_ordering_over_two_caller_streams(orc):
    """pt_render_device on stream A, pt_trace_closest_device on stream B, then a blocking pt_trace_occluded, with no pt_synchronize in
    between: each equals its stand-alone result."""
    bt = TC.battery(orc, "cornell")
    rec = B.make_rays(bt["rays"])
    ctx, cam, W, H = _cornell()
    spp, depth = 64, 8
    alone_rgb, _ = ctx.render(cam, W, H, spp, depth)
    alone_hits, alone_occ = ctx.trace_closest(rec), ctx.trace_occluded(rec)
    TC.assert_same(alone_hits, bt["hits"], bt["mask"], "cornell with its materials")
    fb, d = AS.DeviceFrame(W, H), DevRays(rec)
    try:
        ctx.render_device(cam, W, H, spp, depth, fb.rgb, None, stream=AS.stream(0))
        ctx.trace_closest_device(d.rays, d.n, d.hits, stream=AS.stream(1))
        occ = ctx.trace_occluded(rec)  # blocking: behind both, and the context is idle when it returns
        rgb, _ = fb.read()
        hits, _ = d.read()
        ctx.synchronize()
    finally:
        AS.destroy_streams()
        fb.free()
        d.free()
    assert (rgb.view(np.uint32) == alone_rgb.view(np.uint32)).all(), "the frame on stream A"
    assert TC.same(hits, alone_hits).all(), "the closest hits on stream B"
    assert TC.same(occ, alone_occ).all(), "the blocking occlusion query"
    ctx.close()


def test_stats_are_the_ray_kernels(orc):
    bt = TC.battery(orc, "rects")
    ctx = _ctx(bt["tris"])
    depth4 = ctx.export_trees()["depth4"]
    for fn in (ctx.trace_closest, ctx.trace_occluded):
        fn(B.make_rays(bt["rays"]))
        st = ctx.stats()
        assert st["launches"] == 1 and st["kernel_ms"] > 0
        assert st["block"] == 64 and st["lds_bytes"] == B.PT_LDS_STACK * 64 * 4 and 0 < st["vgprs"] <= 128
        assert 1 <= st["grid"] <= (bt["rays"].shape[0] + 63) // 64 and st["stack_entries"] == 3 * depth4 + 1
    ctx.synchronize()
    ctx.close()
