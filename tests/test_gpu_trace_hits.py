"""pt_trace_hits on the GPU (include/mi355pt.h "ray queries: the first K hits"): the blocking and the device form against the CPU twin on
every ray and against the oracle-derived rule of tests/hits_ref.py on the compared ones, bit for bit on the K * 16 bytes of every ray.

* n = 1, 63, 64, 65, 130 on the cube at K = 4 (partial waves, a tail), grid = ceil(n / 64), the bytes past n * K * 16 untouched;
* every scene of the ray battery and the constructed stacks of tests/hits_common.py, K = 1, 3, 16; the doubled stack by construction;
* K = 1 against pt_trace_closest of the same context on every ray, and entry 0 of K = 4;
* the lane refill: "rays_grid" = 2 at "rays_refill" default, 0, 16 and 63 on the dragon at K = 4, byte-identical to each other;
* "box_exact" 0 and 1; "watertight" 0 and 1 on the closed icosphere; the sliver strip, whose walk needs the HBM overflow column; the
  per-ray tmax cases; after pt_update_vertices;
* pt_trace_closest_device then pt_trace_hits_device on two caller streams without a synchronize; a pt_render before and after;
* n == 0 launches nothing; pt_get_stats reports the hits kernel's launch, whose LDS grows with K."""
import ctypes as C
import os

import numpy as np
import pytest

import async_common as AS
import hits_common as HC
import ray_battery as rb
import surface_common as SC
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(rb.ROOT, "assets")
TAIL = 256  # bytes behind the records, which no call may touch


class DevHits:
    """n rays in HBM, room for n pt_ray_hit and for n * K pt_ray_hit + TAIL bytes, every output byte AS.FILL until a call writes it."""

    def __init__(self, rec, K):
        self.n, self.K = rec.shape[0], K
        self.sizes = (max(self.n * 32, 16), max(self.n * 16, 16), self.n * K * 16 + TAIL)
        self.p = [C.c_void_p() for _ in self.sizes]
        for p, b in zip(self.p, self.sizes):
            AS._ok(AS.hip().hipMalloc(C.byref(p), b), "hipMalloc")
            AS._ok(AS.hip().hipMemset(p, AS.FILL, b), "hipMemset")
        AS._ok(AS.hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.n:
            AS.to_device(self.p[0].value, np.ascontiguousarray(rec))
        self.rays, self.hits, self.out = (p.value for p in self.p)

    def read(self):
        """(the (n, K) lists, the TAIL bytes behind them, the n closest hits)"""
        raw, hits = np.empty(self.sizes[2], np.uint8), np.empty(self.n, B.HIT_DTYPE)
        AS._ok(AS.hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), self.p[2], self.sizes[2], AS.D2H), "hipMemcpy")
        if self.n:
            AS._ok(AS.hip().hipMemcpy(hits.ctypes.data_as(C.c_void_p), self.p[1], self.n * 16, AS.D2H), "hipMemcpy")
        return raw[:self.n * self.K * 16].view(B.HIT_DTYPE).reshape(self.n, self.K), raw[self.n * self.K * 16:], hits

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


def _both(ctx, rec, K):
    """The blocking form's lists; the device form on the context's own stream stores the same bytes and leaves the tail alone."""
    got = ctx.trace_hits(rec, K)
    d = DevHits(rec, K)
    try:
        ctx.trace_hits_device(d.rays, d.n, d.out, K)
        ctx.synchronize()
        dev, tail, _ = d.read()
    finally:
        d.free()
    assert got.shape == (rec.shape[0], K)
    assert HC.same_lists(dev, got).all(), "the device form stores what the blocking form returns"
    assert (tail == AS.FILL).all(), "bytes past n * K * 16 were written"
    return got


def _check(ctx, rec, K, what, case=None):
    """Both forms against the twin on EVERY ray, and (case given) against the rule on the compared rays."""
    got = _both(ctx, rec, K)
    HC.assert_same_lists(got, ctx.trace_hits_host(rec, K), None, what + ", K = %d: pt_trace_hits vs the twin, every ray" % K, rec)
    if case is not None:
        HC.assert_rule(case, got, what + ", K = %d: pt_trace_hits vs the rule" % K)
    return got


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_small_counts(orc, n):
    table = SC.table_case(orc, "cube", "centres", 64, 48)["rec"]
    idx = np.arange(table.shape[0])[:: table.shape[0] // n][:n]
    assert idx.size == n
    ctx = B.Context(0)
    SC.upload(ctx, SC.scene("cube"), B)
    got = _check(ctx, table[idx], 4, "cube, n = %d" % n)
    assert ctx.stats()["grid"] == (n + 63) // 64
    assert TC.same(np.ascontiguousarray(got[:, 0]), ctx.trace_closest(table[idx])).all()
    assert n < 63 or ((got["prim"][:, 1] >= 0).any() and (got["prim"][:, 0] < 0).any()), "rays through both faces of the cube, and rays past it"
    ctx.close()


@pytest.mark.parametrize("name", HC.names())
def test_cases(orc, name):
    c = HC.case(orc, name)
    ctx = _ctx(c["tris"])
    closest = ctx.trace_closest(c["rec"])
    for K in HC.GPU_KS:
        got = _check(ctx, c["rec"], K, name, c)
        if K == 1:
            assert TC.same(got.reshape(-1), closest).all(), "K = 1 is pt_trace_closest of the same context, on every ray"
        if name == "stack_doubled":
            HC.assert_same_lists(got, HC.doubled_expectation(c, K), None, "stack_doubled, K = %d: the lists by construction" % K, c["rec"])
    l4 = _both(ctx, c["rec"], 4)
    assert TC.same(np.ascontiguousarray(l4[:, 0]), closest).all(), "entry 0 of K = 4 is pt_trace_closest's record, on every ray"
    ctx.close()


def test_refill_on_long_ranges(orc):
    """Option "rays_grid" = 2: two waves share the battery, thousands of rays each, so a wave refills its lanes again and again and a
    lane retires through its K stores next to lanes that are still walking and inserting."""
    c = HC.case(orc, "dragon")
    ctx = _ctx(c["tris"], rays_grid=2)
    base = None
    for r in (None, 0, 16, 63):
        if r is not None:
            ctx.set_option("rays_refill", r)
        got = _check(ctx, c["rec"], 4, "dragon, two waves, rays_refill %s" % ("default" if r is None else r), c)
        assert ctx.stats()["grid"] == 2 and c["rec"].shape[0] > 2 * 3000
        base = got if base is None else base
        assert HC.same_lists(got, base).all(), "rays_refill = %s changes a list" % r  # every ray, compared or not
    ctx.close()


@pytest.mark.parametrize("exact", (0, 1))
def test_box_exact(orc, exact):
    for name in ("rects", "soup_offset30"):
        c = HC.case(orc, name)
        ctx = _ctx(c["tris"], box_exact=exact)
        _check(ctx, c["rec"], 4, "%s, box_exact %d" % (name, exact), c)
        ctx.close()


def test_watertight_on_the_closed_mesh(orc):
    tris, rays, mt, wt = TC.closed_case(orc)
    assert wt[0].all()
    rec = B.make_rays(rays)
    ctx = _ctx(tris, watertight=1)
    for K in (1, 4):
        got = _check(ctx, rec, K, "closed mesh, watertight")
        TC.assert_same(np.ascontiguousarray(got[:, 0]), TC.hits_of(wt), None, "closed mesh, watertight, K = %d: entry 0 vs the oracle" % K, rays)
    assert (got["prim"][:, 0] >= 0).all(), "no aimed ray leaves a closed mesh under the watertight test"
    ctx.set_option("watertight", 0)
    got = _check(ctx, rec, 4, "closed mesh, Moeller-Trumbore")
    TC.assert_same(np.ascontiguousarray(got[:, 0]), TC.hits_of(mt), None, "closed mesh, Moeller-Trumbore: entry 0 vs the oracle", rays)
    ctx.close()


def test_overflow_column_is_walked(orc):
    """The sliver strip with one triangle per leaf, as tests/test_gpu_trace_rays.py uploads it: its quad walk needs more stack than LDS
    holds, so lanes walk with their stack in the wave's HBM column while their list sits behind the LDS part."""
    c = HC.case(orc, "strip")
    ctx = _ctx(c["tris"], leaf_size=1)
    depth4 = ctx.export_trees()["depth4"]
    assert 3 * depth4 + 1 > B.PT_LDS_STACK
    for K in (4, 16):
        _check(ctx, c["rec"], K, "strip, leaf_size 1", c)
    assert ctx.stats()["stack_entries"] == 3 * depth4 + 1
    ctx.close()


@pytest.mark.parametrize("name", TC.TMAX_SCENES)
def test_per_ray_tmax(orc, name):
    bt = TC.battery(orc, name)
    ctx = _ctx(bt["tris"])
    for label, rec, want_hits, _, mask in TC.tmax_cases(orc, name):
        got = _check(ctx, rec, 4, "%s: %s" % (name, label))
        TC.assert_same(np.ascontiguousarray(got[:, 0]), want_hits, mask, "%s: %s, entry 0 against the oracle" % (name, label))
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    c = HC.case(orc, "soup1")
    rec = c["rec"]
    mask = TC.compared(moved, TC.battery(orc, "soup1")["rays"], TC.battery(orc, "soup1")["cls"])
    ctx = _ctx(tris, dynamic=1)
    before = ctx.trace_hits(rec, 4)
    ctx.update_vertices([rb.mesh_of(moved)])
    got = _check(ctx, rec, 4, "after pt_update_vertices")
    assert not HC.same_lists(before, got).all(), "the deformation changes lists"
    ctx.close()
    fresh = _ctx(moved)
    HC.assert_same_lists(fresh.trace_hits(rec, 4), got, mask, "a refit scene against a fresh upload", rec)
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
    ctx.trace_hits(rec, 16)
    after, _ = ctx.render(cam, W, H, 8, 8)
    assert (before.view(np.uint32) == after.view(np.uint32)).all()
    ctx.close()


def test_ordering_over_two_caller_streams(orc):
    """pt_trace_closest_device on stream A, then pt_trace_hits_device on stream B with no pt_synchronize in between: both use the
    context's one walk workspace, and each equals its stand-alone result."""
    c = HC.case(orc, "dragon")
    rec = c["rec"]
    ctx = _ctx(c["tris"])
    alone_hits, alone = ctx.trace_closest(rec), ctx.trace_hits(rec, 4)
    d = DevHits(rec, 4)
    try:
        ctx.trace_closest_device(d.rays, d.n, d.hits, stream=AS.stream(0))
        ctx.trace_hits_device(d.rays, d.n, d.out, 4, stream=AS.stream(1))
        ctx.synchronize()
        got, tail, hits = d.read()
    finally:
        AS.destroy_streams()
        d.free()
    assert TC.same(hits, alone_hits).all(), "the closest hits on stream A"
    assert HC.same_lists(got, alone).all() and (tail == AS.FILL).all(), "the lists on stream B"
    ctx.close()


def test_n_zero_launches_nothing_and_stats_are_the_hits_kernels(orc):
    c = HC.case(orc, "rects")
    ctx = _ctx(c["tris"])
    depth4 = ctx.export_trees()["depth4"]
    words = 4  # a list entry is the record itself, {t, u, v, id}
    lds = {}
    for K in (1, 4, 16):
        ctx.trace_hits(c["rec"], K)
        st = ctx.stats()
        assert st["launches"] == 1 and st["kernel_ms"] > 0
        assert st["block"] == 64 and 0 < st["vgprs"] <= 128
        assert st["lds_bytes"] == (B.PT_LDS_STACK + K * words) * 64 * 4, "the stack, then K entries per lane"
        assert 1 <= st["grid"] <= (c["rec"].shape[0] + 63) // 64 and st["stack_entries"] == 3 * depth4 + 1
        lds[K] = st["lds_bytes"]
    assert lds[1] < lds[4] < lds[16], "the LDS of a launch grows with K"
    ctx.synchronize()
    launches = ctx.stats()["launches"]
    none = np.zeros(0, B.RAY_DTYPE)
    assert ctx.trace_hits(none, 16).shape == (0, 16)
    d = DevHits(none, 16)
    try:
        ctx.trace_hits_device(d.rays, 0, d.out, 16)
        ctx.trace_hits_device(0, 0, 0, 16)
        ctx.synchronize()
        _, tail, _ = d.read()
    finally:
        d.free()
    assert (tail == AS.FILL).all(), "n == 0 wrote to the output"
    assert ctx.stats()["launches"] == launches, "n == 0 launched a kernel"
    ctx.close()
