"""pt_trace_surface on the GPU (include/mi355pt.h "ray queries: the surface at the hit"): the blocking and the device form against the
CPU twin and against tests/surface_ref.py, bit for bit on the 80 bytes of every compared record; the first 16 bytes against
pt_trace_closest of the same context on every ray.

* n = 1, 63, 64, 65, 130 on the textured cube (partial waves, a tail), grid = ceil(n / 64);
* the 64 x 48 centre tables and the probe tables of Cornell, the cube, mirror_wall and tir; every scene of the ray battery;
* the lane refill: "rays_grid" = 2 (a wave owns thousands of rays) at "rays_refill" default, 0, 16 and 63, byte-identical to each other;
* "box_exact" 0 and 1; "watertight" 0 and 1 on the closed icosphere; the sliver strip, whose walk needs the HBM overflow column; the
  per-ray tmax cases; after pt_set_materials and after pt_update_vertices;
* pt_trace_closest_device then pt_trace_surface_device on two caller streams without a synchronize; a pt_render before and after;
* n == 0 launches nothing, bytes past n * 80 stay untouched, pt_get_stats reports the surface kernel's launch."""
import ctypes as C
import os

import numpy as np
import pytest

import async_common as AS
import ray_battery as rb
import surface_common as SC
import surface_ref
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(rb.ROOT, "assets")
TAIL = 256  # bytes behind the records, which no call may touch


class DevSurface:
    """n rays in HBM, room for n pt_ray_hit and for n pt_surface + TAIL bytes, every output byte 0xA5 until a call writes it."""

    def __init__(self, rec):
        self.n = rec.shape[0]
        self.sizes = (max(self.n * 32, 16), max(self.n * 16, 16), self.n * 80 + TAIL)
        self.p = [C.c_void_p() for _ in self.sizes]
        for p, b in zip(self.p, self.sizes):
            AS._ok(AS.hip().hipMalloc(C.byref(p), b), "hipMalloc")
            AS._ok(AS.hip().hipMemset(p, AS.FILL, b), "hipMemset")
        AS._ok(AS.hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.n:
            AS.to_device(self.p[0].value, rec)
        self.rays, self.hits, self.out = (p.value for p in self.p)

    def read(self):
        """(the n surface records, the TAIL bytes behind them, the n closest hits)"""
        raw, hits = np.empty(self.sizes[2], np.uint8), np.empty(self.n, B.HIT_DTYPE)
        AS._ok(AS.hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), self.p[2], self.sizes[2], AS.D2H), "hipMemcpy")
        if self.n:
            AS._ok(AS.hip().hipMemcpy(hits.ctypes.data_as(C.c_void_p), self.p[1], self.n * 16, AS.D2H), "hipMemcpy")
        return raw[:self.n * 80].view(B.SURFACE_DTYPE), raw[self.n * 80:], hits

    def free(self):
        for p in self.p:
            if p.value:
                AS.hip().hipFree(p)
                p.value = None


def _opts(ctx, opts):
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def _ctx_scene(name, **opts):
    ctx = _opts(B.Context(0), opts)
    SC.upload(ctx, SC.scene(name), B)
    return ctx


def _ctx_soup(tris, **opts):
    ctx = _opts(B.Context(0), opts)
    rb.upload(ctx, tris)
    return ctx


def _both(ctx, rec):
    """The blocking form's records; the device form on the context's own stream stores the same bytes and leaves the tail alone."""
    got = ctx.trace_surface(rec)
    d = DevSurface(rec)
    try:
        ctx.trace_surface_device(d.rays, d.n, d.out)
        ctx.synchronize()
        dev, tail, _ = d.read()
    finally:
        d.free()
    assert not surface_ref.differ(dev, got).any(), "the device form stores what the blocking form returns"
    assert (tail == AS.FILL).all(), "bytes past n * 80 were written"
    return got


def _check(ctx, rec, want, mask, what):
    """Both forms against the twin on EVERY ray's first 16 bytes and pt_trace_closest, against the twin's 80 bytes and (want given)
    the restatement's on the compared rays."""
    got = _both(ctx, rec)
    twin = ctx.trace_surface_host(rec)
    assert TC.same(SC.first16(got), ctx.trace_closest(rec)).all(), what + ": the first 16 bytes are pt_trace_closest's, on all rays"
    SC.assert_same(got, twin, mask, what + ": pt_trace_surface vs the twin")
    if want is not None:
        SC.assert_same(got, want, mask, what + ": pt_trace_surface vs the restatement")
    return got


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_small_counts(orc, n):
    case = SC.table_case(orc, "cube", "centres", 64, 48)
    idx = np.arange(case["rec"].shape[0])[:: case["rec"].shape[0] // n][:n]
    assert idx.size == n
    ctx = _ctx_scene("cube")
    got = _check(ctx, case["rec"][idx], case["want"][idx], None, "cube, n = %d" % n)
    assert ctx.stats()["grid"] == (n + 63) // 64
    assert n < 63 or ((got["prim"] >= 0).any() and (got["prim"] < 0).any())
    ctx.close()


@pytest.mark.parametrize("name", SC.SCENES)
def test_whole_tables(orc, name):
    ctx = _ctx_scene(name)
    for nm, kind, W, H in SC.GPU_TABLES:
        if nm == name:
            case = SC.table_case(orc, name, kind, W, H)
            _check(ctx, case["rec"], case["want"], None, "%s %s %dx%d" % (name, kind, W, H))
    ctx.close()


@pytest.mark.parametrize("name", rb.scene_names())
def test_battery(orc, name):
    case = SC.battery_case(orc, name)
    ctx = _ctx_soup(case["tris"])
    _check(ctx, case["rec"], case["want"], case["mask"], name)
    ctx.close()


def test_refill_on_long_ranges(orc):
    """Option "rays_grid" = 2: two waves share the battery, thousands of rays each, so a wave refills its lanes again and again and a
    lane retires through the record fetch next to lanes that are still walking."""
    case = SC.battery_case(orc, "dragon")
    ctx = _ctx_soup(case["tris"], rays_grid=2)
    base = None
    for r in (None, 0, 16, 63):
        if r is not None:
            ctx.set_option("rays_refill", r)
        got = _check(ctx, case["rec"], case["want"], case["mask"], "dragon, two waves, rays_refill %s" % ("default" if r is None else r))
        assert ctx.stats()["grid"] == 2 and case["rec"].shape[0] > 2 * 3000
        base = got if base is None else base
        assert not surface_ref.differ(got, base).any(), "rays_refill = %s changes a record" % r  # every ray, compared or not
    ctx.close()


@pytest.mark.parametrize("exact", (0, 1))
def test_box_exact(orc, exact):
    for name in ("rects", "soup_offset30"):
        case = SC.battery_case(orc, name)
        ctx = _ctx_soup(case["tris"], box_exact=exact)
        _check(ctx, case["rec"], case["want"], case["mask"], "%s, box_exact %d" % (name, exact))
        ctx.close()


def test_watertight_on_the_closed_mesh(orc):
    tris, rays, mt, wt = TC.closed_case(orc)
    assert wt[0].all()
    flat, rec = SC.battery_flat(tris), B.make_rays(rays)
    ctx = _ctx_soup(tris, watertight=1)
    got = _check(ctx, rec, surface_ref.surface(flat, wt), None, "closed mesh, watertight")
    assert (got["prim"] >= 0).all(), "no aimed ray leaves a closed mesh under the watertight test"
    ctx.set_option("watertight", 0)
    _check(ctx, rec, surface_ref.surface(flat, mt), None, "closed mesh, Moeller-Trumbore")
    ctx.close()


def test_overflow_column_is_walked(orc):
    """The sliver strip with one triangle per leaf, as tests/test_gpu_trace_rays.py uploads it: its quad walk needs more stack than LDS
    holds, so lanes retire with their stack in the wave's HBM column."""
    case = SC.battery_case(orc, "strip")
    ctx = _ctx_soup(case["tris"], leaf_size=1)
    depth4 = ctx.export_trees()["depth4"]
    assert 3 * depth4 + 1 > B.PT_LDS_STACK
    _check(ctx, case["rec"], case["want"], case["mask"], "strip, leaf_size 1")
    assert ctx.stats()["stack_entries"] == 3 * depth4 + 1
    ctx.close()


@pytest.mark.parametrize("name", TC.TMAX_SCENES)
def test_per_ray_tmax(orc, name):
    bt = TC.battery(orc, name)
    ctx = _ctx_soup(bt["tris"])
    for label, rec, want_hits, _, mask in TC.tmax_cases(orc, name):
        got = _check(ctx, rec, None, mask, "%s: %s" % (name, label))
        TC.assert_same(SC.first16(got), want_hits, mask, "%s: %s, against the oracle" % (name, label))
    ctx.close()


def test_after_set_materials(orc):
    case = SC.table_case(orc, "mirror_wall", "centres", 64, 48)
    ctx = _ctx_scene("mirror_wall")
    before = _check(ctx, case["rec"], case["want"], None, "mirror_wall")
    mats = SC.emitting_wall()
    mats[1, :3] = np.float32([0.125, 0.25, 0.5])
    ctx.set_materials(mats)
    after = _check(ctx, case["rec"], surface_ref.surface(case["flat"], case["truth"], materials=mats), None, "mirror_wall after pt_set_materials")
    assert surface_ref.differ(before, after).any()
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    bt = TC.battery(orc, "soup1")
    rec = B.make_rays(bt["rays"])
    mask = TC.compared(moved, bt["rays"], bt["cls"])
    truth = rb.oracle_scene(orc, moved).intersect_n(bt["rays"], use_bvh=False)
    ctx = _ctx_soup(tris, dynamic=1)
    before = ctx.trace_surface(rec)
    ctx.update_vertices([rb.mesh_of(moved)])
    got = _check(ctx, rec, surface_ref.surface(SC.battery_flat(moved), truth), mask, "after pt_update_vertices")
    assert surface_ref.differ(before, got).any(), "the deformation changes records"
    ctx.close()
    fresh = _ctx_soup(moved)
    assert SC.same(fresh.trace_surface(rec), got, mask).all()
    fresh.close()


def _cornell():
    sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
    ctx = B.Context(0)
    ctx.upload_scene(sc["entities"], [m for _, m, _ in sc["materials"]], env=B.make_env(color=(1, 1, 1), intensity=0.0))
    c = sc["camera"]
    W = H = 48
    return ctx, B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H), W, H


def test_render_state_is_untouched(orc):
    rec = B.make_rays(TC.battery(orc, "cornell")["rays"][:3000])
    ctx, cam, W, H = _cornell()
    before, _ = ctx.render(cam, W, H, 8, 8)
    ctx.trace_surface(rec)
    after, _ = ctx.render(cam, W, H, 8, 8)
    assert (before.view(np.uint32) == after.view(np.uint32)).all()
    ctx.close()


def test_ordering_over_two_caller_streams(orc):
    """pt_trace_closest_device on stream A, then pt_trace_surface_device on stream B with no pt_synchronize in between: both use the
    context's one walk workspace, and each equals its stand-alone result."""
    case = SC.battery_case(orc, "dragon")
    rec = case["rec"]
    ctx = _ctx_soup(case["tris"])
    alone_hits, alone = ctx.trace_closest(rec), ctx.trace_surface(rec)
    d = DevSurface(rec)
    try:
        ctx.trace_closest_device(d.rays, d.n, d.hits, stream=AS.stream(0))
        ctx.trace_surface_device(d.rays, d.n, d.out, stream=AS.stream(1))
        ctx.synchronize()
        got, tail, hits = d.read()
    finally:
        AS.destroy_streams()
        d.free()
    assert TC.same(hits, alone_hits).all(), "the closest hits on stream A"
    assert not surface_ref.differ(got, alone).any() and (tail == AS.FILL).all(), "the surface records on stream B"
    ctx.close()


def test_n_zero_launches_nothing_and_stats_are_the_surface_kernels(orc):
    case = SC.battery_case(orc, "rects")
    ctx = _ctx_soup(case["tris"])
    depth4 = ctx.export_trees()["depth4"]
    ctx.trace_surface(case["rec"])
    st = ctx.stats()
    assert st["launches"] == 1 and st["kernel_ms"] > 0
    assert st["block"] == 64 and st["lds_bytes"] == B.PT_LDS_STACK * 64 * 4 and 0 < st["vgprs"] <= 128
    assert 1 <= st["grid"] <= (case["rec"].shape[0] + 63) // 64 and st["stack_entries"] == 3 * depth4 + 1
    ctx.synchronize()
    none = np.zeros(0, B.RAY_DTYPE)
    assert ctx.trace_surface(none).shape == (0,)
    d = DevSurface(none)
    try:
        ctx.trace_surface_device(d.rays, 0, d.out)
        ctx.trace_surface_device(0, 0, 0)
        ctx.synchronize()
        _, tail, _ = d.read()
    finally:
        d.free()
    assert (tail == AS.FILL).all(), "n == 0 wrote to the output"
    ctx.close()
