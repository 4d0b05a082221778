"""pt_trace_ao on the GPU (include/mi355pt.h "ray queries: ambient occlusion"): the blocking and the device form against the CPU twin and
against tests/ao_ref.py, bit for bit on the 32 bytes of every compared record (tests/ao_common.py: the records whose primary and
occlusion rays stay inside the closest-hit domain); the first 16 bytes against pt_trace_closest of the same context on every ray.

* n = 1, 63, 64, 65, 130 on the textured cube at K = 1 and 5 (partial waves, a tail), grid = ceil(n / 64), the tail bytes untouched;
* the 64 x 48 tables of Cornell and the cube at K = 16; the icosphere from inside and outside under "watertight" 0 and 1;
* the lane refill: "rays_grid" = 2 (a wave owns 1536 rays) at "rays_refill" default, 0, 16 and 63 with K = 4: byte-identical to each
  other on every ray, and to the twin - a lane in its occlusion phase and a refilled lane sit in one wave;
* "box_exact" 0 and 1: identical bytes; the sliver strip, whose walk needs the HBM overflow column, at K = 2;
* fused against composed: clear of pt_trace_ao_device equals the zero count of pt_trace_occluded_device over the twin's occlusion rays;
* pt_trace_surface_device then pt_trace_ao_device on two caller streams without a synchronize; a pt_render before and after;
* n == 0 launches nothing, pt_get_stats reports the AO kernel's launch."""
import ctypes as C
import os

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

pytestmark = pytest.mark.gpu

ASSETS = os.path.join(rb.ROOT, "assets")
TAIL = 256  # bytes behind the records, which no call may touch
SEED = AC.SEEDS[1]


class DevAo:
    """n rays in HBM, room for n pt_ao_hit + TAIL bytes and for `extra` more bytes, every output byte 0xA5 until a call writes it."""

    def __init__(self, rec, extra=16):
        self.n = rec.shape[0]
        self.sizes = (max(self.n * 32, 16), self.n * 32 + TAIL, max(extra, 16))
        self.p = [C.c_void_p() for _ in self.sizes]
        for p, b in zip(self.p, self.sizes):
            AS._ok(AS.hip().hipMalloc(C.byref(p), b), "hipMalloc")
            AS._ok(AS.hip().hipMemset(p, AS.FILL, b), "hipMemset")
        AS._ok(AS.hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.n:
            AS.to_device(self.p[0].value, rec)
        self.rays, self.out, self.extra = (p.value for p in self.p)

    def read(self):
        """(the n records, the TAIL bytes behind them)"""
        raw = np.empty(self.sizes[1], np.uint8)
        AS._ok(AS.hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), self.p[1], self.sizes[1], AS.D2H), "hipMemcpy")
        return raw[:self.n * 32].view(B.AO_DTYPE), raw[self.n * 32:]

    def read_extra(self, dtype, count):
        out = np.empty(count, dtype)
        AS._ok(AS.hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p[2], out.nbytes, AS.D2H), "hipMemcpy")
        return out

    def free(self):
        for p in self.p:
            if p.value:
                AS.hip().hipFree(p)
                p.value = None


def _ctx(c, **opts):
    ctx = B.Context(0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    c["upload"](ctx)
    return ctx


def _both(ctx, rec, prm):
    """The blocking form's records; the device form on the context's own stream stores the same bytes and leaves the tail alone."""
    got = ctx.trace_ao(rec, prm)
    d = DevAo(rec)
    try:
        ctx.trace_ao_device(d.rays, d.n, d.out, prm)
        ctx.synchronize()
        dev, tail = d.read()
    finally:
        d.free()
    assert not ao_ref.differ(dev, got).any(), "the device form stores what the blocking form returns"
    assert (tail == AS.FILL).all(), "bytes past n * 32 were written"
    return got


def _check(ctx, rec, prm, want, mask, what):
    """Both forms: the first 16 bytes against pt_trace_closest on EVERY ray, the 32 bytes against the twin and (want given) the
    restatement on the compared records."""
    got = _both(ctx, rec, prm)
    twin = ctx.trace_ao_host(rec, prm)
    bad = ao_ref.differ(got, twin)
    print("%s: %d rays, %d differ from the twin, %d of them compared" % (what, got.shape[0], bad.sum(), (bad & mask).sum() if mask is not None else bad.sum()))
    assert TC.same(AC.first16(got), ctx.trace_closest(rec)).all(), what + ": the first 16 bytes are pt_trace_closest's, on all rays"
    AC.assert_same(got, twin, mask, what + ": pt_trace_ao vs the twin")
    if want is not None:
        AC.assert_same(got, want, mask, what + ": pt_trace_ao vs the restatement")
    return got


@pytest.mark.parametrize("K", (1, 5))
@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_small_counts(orc, n, K):
    c = AC.case(orc, "cube")
    total = c["rec"].shape[0]
    idx = np.arange(total)[:: total // n][:n]
    assert idx.size == n
    # the stream of a ray follows its index in THIS call: the restatement is made for these n rays
    rays, truth = c["rays"][idx], tuple(a[idx] for a in c["truth"])
    prep = ao_ref.prepare(c["S"], c["flat"], rays, truth, 0, SEED, K)
    mask = ao_ref.compared(c["S"], c["flat"], rays, truth, prep, K)
    assert mask.all(), "the cube is axis-aligned: no record is left out"
    ctx = _ctx(c)
    got = _check(ctx, np.ascontiguousarray(c["rec"][idx]), AC.params(c, K, 0, "quarter", SEED), ao_ref.finish(c["S"], prep, K, AC.radius_of(c, "quarter")), mask,
                 "cube, n = %d, K = %d" % (n, K))
    assert ctx.stats()["grid"] == (n + 63) // 64
    assert n < 63 or ((got["prim"] >= 0).any() and (got["prim"] < 0).any())
    ctx.close()


@pytest.mark.parametrize("name", ("cornell", "cube"))
def test_whole_tables(orc, name):
    c = AC.case(orc, name)
    ctx = _ctx(c)
    for flags, which in ((0, "inf"), (1, "quarter")):
        got = _check(ctx, c["rec"], AC.params(c, 16, flags, which, SEED), AC.want(c, 16, flags, which, SEED), AC.mask(c, 16, flags, SEED),
                     "%s K=16 flags=%d radius=%s" % (name, flags, which))
        assert name == "cube" or len(np.unique(got["ao"])) > 4  # (the cube is convex and alone: nothing occludes it)
    ctx.close()


@pytest.mark.parametrize("wt", (0, 1))
@pytest.mark.parametrize("name", AC.ICO)
def test_icosphere(orc, name, wt):
    c = AC.case(orc, name, watertight=bool(wt))
    K, flags, which, seed = 4, wt, "inf" if name == "ico_in" else "quarter", 5
    prep = ao_ref.prepare(c["S"], c["flat"], c["rays"], c["truth"], flags, seed, K)
    mask = ao_ref.compared(c["S"], c["flat"], c["rays"], c["truth"], prep, K)
    assert (~mask).sum() <= AC.MAX_LEFT_OUT * mask.size
    ctx = _ctx(c, watertight=wt)
    got = _check(ctx, c["rec"], AC.params(c, K, flags, which, seed), ao_ref.finish(c["S"], prep, K, AC.radius_of(c, which)), mask, "%s, watertight %d" % (name, wt))
    if name == "ico_in" and wt:
        assert (got["prim"] >= 0).all(), "no ray leaves a closed mesh under the watertight test"
    ctx.close()


def test_refill_on_long_ranges(orc):
    """Option "rays_grid" = 2: two waves share the table, 1536 rays and 5 x 1536 walks each, so a wave refills its lanes again and again
    while other lanes are in their occlusion phase."""
    c = AC.case(orc, "cornell")
    K, flags, which = 4, 0, "quarter"
    prm = AC.params(c, K, flags, which, SEED)
    ctx = _ctx(c, rays_grid=2)
    base = None
    for r in (None, 0, 16, 63):
        if r is not None:
            ctx.set_option("rays_refill", r)
        got = _check(ctx, c["rec"], prm, AC.want(c, K, flags, which, SEED), AC.mask(c, K, flags, SEED), "cornell, two waves, rays_refill %s" % ("default" if r is None else r))
        assert ctx.stats()["grid"] == 2
        base = got if base is None else base
        assert not ao_ref.differ(got, base).any(), "rays_refill = %s changes a record" % r  # every ray, compared or not
    ctx.close()
    full = _ctx(c)
    assert not ao_ref.differ(full.trace_ao(c["rec"], prm), base).any(), "the grid changes a record"
    assert full.stats()["grid"] == (c["rec"].shape[0] + 63) // 64
    full.close()


def test_box_exact(orc):
    c = AC.case(orc, "cornell")
    K, flags, which = 4, 1, "inf"
    out = []
    for exact in (0, 1):
        ctx = _ctx(c, box_exact=exact)
        out.append(_check(ctx, c["rec"], AC.params(c, K, flags, which, SEED), AC.want(c, K, flags, which, SEED), AC.mask(c, K, flags, SEED), "cornell, box_exact %d" % exact))
        ctx.close()
    assert not (ao_ref.differ(out[0], out[1]) & AC.mask(c, K, flags, SEED)).any(), "the slab form changes a compared record"


def test_overflow_column_is_walked(orc):
    """The sliver strip with one triangle per leaf, as tests/test_gpu_trace_rays.py uploads it: its quad walk needs more stack than LDS
    holds, so primary and occlusion walks run with their stack in the wave's HBM column."""
    bt = SC.battery_case(orc, "strip")
    K, seed = 2, 9
    S = rb.oracle_scene(orc, bt["tris"])
    prep = ao_ref.prepare(S, bt["flat"], bt["rays"], bt["truth"], 0, seed, K)
    mask = bt["mask"] & ao_ref.compared(S, bt["flat"], bt["rays"], bt["truth"], prep, K)
    ctx = B.Context(0)
    ctx.set_option("leaf_size", 1)
    rb.upload(ctx, bt["tris"])
    depth4 = ctx.export_trees()["depth4"]
    assert 3 * depth4 + 1 > B.PT_LDS_STACK
    _check(ctx, bt["rec"], B.ao_default_params(n_rays=K, seed=seed), ao_ref.finish(S, prep, K, np.inf), mask, "strip, leaf_size 1")
    assert ctx.stats()["stack_entries"] == 3 * depth4 + 1
    ctx.synchronize()  # PT_E_HIP here would be a walk out of its bounds
    ctx.close()


def test_fused_against_composed_on_the_device(orc):
    c = AC.case(orc, "cornell")
    K = 16
    prm = AC.params(c, K, 0, "quarter", SEED)
    ctx = _ctx(c)
    _, ao_rays = ctx.trace_ao_host(c["rec"], prm, return_rays=True)
    n = c["rec"].shape[0]
    d, e = DevAo(c["rec"]), DevAo(np.ascontiguousarray(ao_rays.reshape(-1)), extra=n * K)
    try:
        ctx.trace_ao_device(d.rays, n, d.out, prm)
        ctx.trace_occluded_device(e.rays, n * K, e.extra)
        ctx.synchronize()
        got, _ = d.read()
        occ = e.read_extra(np.uint8, n * K).reshape(n, K)
    finally:
        d.free()
        e.free()
    assert set(np.unique(occ)) <= {0, 1}
    assert ((occ == 0).sum(1) == AC.clear_of(got, K)).all(), "one kernel and the composition count the same rays, on every record"
    ctx.close()


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
    ctx.trace_ao(rec, B.ao_default_params(n_rays=4))
    after, _ = ctx.render(cam, W, H, 8, 8)
    assert (before.view(np.uint32) == after.view(np.uint32)).all()
    ctx.close()


def test_ordering_over_two_caller_streams(orc):
    """pt_trace_surface_device on stream A, then pt_trace_ao_device on stream B with no pt_synchronize in between: both use the
    context's one walk workspace, and each equals its stand-alone result."""
    c = AC.case(orc, "cornell")
    rec, n = c["rec"], c["rec"].shape[0]
    prm = AC.params(c, 8, 0, "inf", SEED)
    ctx = _ctx(c)
    alone_surface, alone = ctx.trace_surface(rec), ctx.trace_ao(rec, prm)
    d = DevAo(rec, extra=n * 80)
    try:
        ctx.trace_surface_device(d.rays, n, d.extra, stream=AS.stream(0))
        ctx.trace_ao_device(d.rays, n, d.out, prm, stream=AS.stream(1))
        ctx.synchronize()
        got, tail = d.read()
        surf = d.read_extra(B.SURFACE_DTYPE, n)
    finally:
        AS.destroy_streams()
        d.free()
    assert (surf.view(np.uint8) == alone_surface.view(np.uint8)).all(), "the surface records on stream A"
    assert not ao_ref.differ(got, alone).any() and (tail == AS.FILL).all(), "the AO records on stream B"
    ctx.close()


def test_n_zero_launches_nothing_and_stats_are_the_ao_kernels(orc):
    c = AC.case(orc, "cornell")
    ctx = _ctx(c)
    depth4 = ctx.export_trees()["depth4"]
    ctx.trace_ao(c["rec"], B.ao_default_params(n_rays=2))
    st = ctx.stats()
    assert st["launches"] == 1 and st["kernel_ms"] > 0
    assert st["block"] == 64 and st["lds_bytes"] == B.PT_LDS_STACK * 64 * 4 and 0 < st["vgprs"] <= 128
    assert 1 <= st["grid"] <= (c["rec"].shape[0] + 63) // 64 and st["stack_entries"] == 3 * depth4 + 1
    ctx.synchronize()
    none = np.zeros(0, B.RAY_DTYPE)
    assert ctx.trace_ao(none).shape == (0,)
    d = DevAo(none)
    try:
        ctx.trace_ao_device(d.rays, 0, d.out)
        ctx.trace_ao_device(0, 0, 0)
        ctx.synchronize()
        _, tail = d.read()
    finally:
        d.free()
    assert (tail == AS.FILL).all(), "n == 0 wrote to the output"
    ctx.close()
