"""pt_closest_point on the GPU (include/mi355pt.h "point queries: the nearest surface"): the blocking and the device form against the CPU
twin and against tests/closest_point_ref.py, bit for bit on the 32 bytes of EVERY record (tests/closest_point_common.py: scenes and
point sets; no record is left out).

* n = 1, 63, 64, 65, 130 on the textured cube (partial waves, a tail), grid = ceil(n / 64), the bytes past n * 32 untouched;
* 20 000 points a scene on Cornell, the cube, the icosphere from outside and inside and every scene of tests/ray_battery.py against the
  twin, and the case's reference points against the restatement;
* the lane refill: "rays_grid" = 2 (a wave owns ~10 000 points) at "rays_refill" default, 0, 16 and 63: byte-identical to each other
  and to the twin, and the full grid stores the same;
* exact ties (a mesh uploaded twice; vertex regions of a closed mesh), the radius cases, the needle scene;
* the deep strip at one triangle per leaf: the walk's stack runs into the wave's HBM overflow column;
* after pt_update_vertices; two caller streams; right behind a pt_render_device with no synchronize; a pt_render before and after;
* n == 0 launches nothing, pt_get_stats reports the point kernel's launch."""
import ctypes as C
import os

import numpy as np
import pytest

import async_common as AS
import closest_point_common as PC
import closest_point_ref as R
import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

pytestmark = pytest.mark.gpu

F32 = np.float32
TAIL = 256  # bytes behind the records, which no call may touch
N_SCENE = 20000


class DevPoints:
    """n points in HBM and room for n pt_point_hit + TAIL bytes, every output byte 0xA5 until a call writes it."""

    def __init__(self, pts):
        self.n = pts.shape[0]
        self.sizes = (max(self.n * 16, 16), self.n * 32 + TAIL)
        self.p = [C.c_void_p() for _ in self.sizes]
        for p, b in zip(self.p, self.sizes):
            AS._ok(AS.hip().hipMalloc(C.byref(p), b), "hipMalloc")
            AS._ok(AS.hip().hipMemset(p, AS.FILL, b), "hipMemset")
        AS._ok(AS.hip().hipDeviceSynchronize(), "hipDeviceSynchronize")
        if self.n:
            AS.to_device(self.p[0].value, pts)
        self.pts, self.out = (p.value for p in self.p)

    def read(self):
        """(the n records, the TAIL bytes behind them)"""
        raw = np.empty(self.sizes[1], np.uint8)
        AS._ok(AS.hip().hipMemcpy(raw.ctypes.data_as(C.c_void_p), self.p[1], self.sizes[1], AS.D2H), "hipMemcpy")
        return raw[:self.n * 32].view(B.POINT_HIT_DTYPE), raw[self.n * 32:]

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


def _both(ctx, pts, stream=None):
    """The blocking form's records; the device form stores the same bytes and leaves the tail alone."""
    got = ctx.closest_point(pts)
    d = DevPoints(pts)
    try:
        ctx.closest_point_device(d.pts, d.n, d.out, stream=stream)
        ctx.synchronize()  # PT_E_HIP here would be a walk out of its bounds
        dev, tail = d.read()
    finally:
        d.free()
    assert not R.differ(dev, got).any(), "the device form stores what the blocking form returns"
    assert (tail == AS.FILL).all(), "bytes past n * 32 were written"
    return got


def _check(ctx, pts, what, want=None, twin=None):
    got = _both(ctx, pts)
    PC.assert_same(got, ctx.closest_point_host(pts) if twin is None else twin, what + ": pt_closest_point vs the twin")
    if want is not None:
        PC.assert_same(got, want, what + ": pt_closest_point vs the restatement")
    return got


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_small_counts(n):
    c = PC.case("cube")
    pts = np.ascontiguousarray(c["ref"][:: c["ref"].shape[0] // n][:n])
    assert pts.shape[0] == n
    ctx = _ctx(c["tris"])
    _check(ctx, pts, "cube, n = %d" % n, R.closest(c["T"], pts))
    assert ctx.stats()["grid"] == (n + 63) // 64
    ctx.close()


@pytest.mark.parametrize("name", PC.SCENES)
def test_scene(name):
    c = PC.case(name)
    ctx = _ctx(c["tris"])
    _check(ctx, c["ref"], name + ", reference points", PC.want(name))
    got = _check(ctx, PC.more_points(name, N_SCENE), "%s, %d points" % (name, N_SCENE))
    assert (got["prim"] >= 0).all() and len(np.unique(got["feature"])) >= 4
    ctx.close()


def test_refill_on_long_ranges():
    """Option "rays_grid" = 2: two waves share the points, ~10 000 each, so a wave refills its lanes again and again."""
    c = PC.case("cornell")
    pts = PC.more_points("cornell", N_SCENE)
    ctx = _ctx(c["tris"], rays_grid=2)
    base, twin = None, ctx.closest_point_host(pts)
    for r in (None, 0, 16, 63):
        if r is not None:
            ctx.set_option("rays_refill", r)
        got = _check(ctx, pts, "cornell, two waves, rays_refill %s" % ("default" if r is None else r), twin=twin)
        assert ctx.stats()["grid"] == 2
        base = got if base is None else base
        assert not R.differ(got, base).any(), "rays_refill = %s changes a record" % r
    ctx.close()
    full = _ctx(c["tris"])
    assert not R.differ(full.closest_point(pts), base).any(), "the grid changes a record"
    assert full.stats()["grid"] > 2
    full.close()


def test_exact_ties():
    tris = rb.make_closed_mesh("ico320")[0]
    n = tris.shape[0]
    ctx = B.Context(0)
    ctx.upload_scene([(rb.mesh_of(tris), 0), (rb.mesh_of(tris), 0)], [scene_io.MAT_DEFAULT])
    pts = B.make_points(PC.points_of("twice", tris, 4000, 11))
    got = _check(ctx, pts, "a mesh uploaded twice", R.closest(R.triangles(np.concatenate([tris, tris])), pts))
    assert (got["prim"] >= 0).all() and (got["prim"] < n).all(), "every record is a tie between id and id + n: the lower one wins"
    ctx.close()
    # vertex regions of the closed icosphere: five or six triangles report the same vertex
    c = PC.case("ico_out")
    v = c["T"][np.random.default_rng(5).integers(0, c["T"].shape[0], 3000), 0]
    pts = B.make_points((v.astype(np.float64) * 1.5).astype(F32))
    ctx = _ctx(c["tris"])
    got = _check(ctx, pts, "vertex regions")
    assert (got["q"] == v).all() and (got["feature"] >= 1).all() and (got["feature"] <= 3).all()
    PC.assert_same(got[:300], R.closest(c["T"], pts[:300]), "vertex regions vs the restatement")
    ctx.close()


def test_radii():
    tris = F32([[[-4, -4, 0], [4, -4, 0], [0, 6, 0]]])
    half, below = F32(0.5), np.nextafter(F32(0.5), F32(0))
    radii = F32([np.inf, np.nan, 1e10, 3e38, 0.5, below, -1.0, -np.inf, -0.0, 0.0, 1e-3, 0.49, 0.51])
    pts = B.make_points(np.tile(F32([0.25, 0.5, 0.5]), (radii.size, 1)), radii)
    ctx = _ctx(tris)
    got = _check(ctx, pts, "radii, the root is a leaf", R.closest(R.triangles(tris), pts))
    assert (got["prim"] == 0).tolist() == [True, True, True, True, True, False, False, False, False, False, False, False, True]
    ctx.close()
    # the same radii through a real walk: Cornell's points, a radius each, from nothing found to everything
    c = PC.case("cornell")
    pts = np.array(PC.more_points("cornell", 6000))
    rng = np.random.default_rng(8)
    pts["radius"] = (c["extent"] * 10.0 ** rng.uniform(-3, 1, pts.shape[0])).astype(F32)
    pts["radius"][::7] = F32(-1.0)
    pts["radius"][1::7] = F32(np.nan)
    ctx = _ctx(c["tris"])
    got = _check(ctx, pts, "cornell, a radius per point")
    assert (got["prim"][::7] == -1).all() and (got["prim"][1::7] >= 0).all()
    found = got["prim"] >= 0
    assert 0.2 < found.mean() < 0.95 and (got["dist"][found] <= R.bound(pts["radius"][found])[0]).all()
    # a point at exactly its radius from the surface is found, one float below it is not
    on = np.array(pts[found][:2000])
    on["radius"] = got["dist"][found][:2000]
    at = ctx.closest_point(on)
    PC.assert_same(at, ctx.closest_point_host(on), "radius = the reported distance")
    assert (at["prim"] >= 0).any() and (at["prim"] < 0).any()  # dist = sqrt_(dd) rounds: dist * dist is dd or a neighbour of it, either side
    ctx.close()


def test_slivers_are_never_reported():
    tris, x = PC.needle_scene()
    pts = B.make_points(x)
    ctx = _ctx(tris)
    got = _check(ctx, pts, "needles", R.closest(R.triangles(tris), pts))
    assert (got["prim"] >= 50).all() and (got["dist"] >= 3.0).all()
    ctx.close()
    only = _ctx(tris[:50])
    got = _check(only, pts, "needles alone")
    assert (got["prim"] == -1).all()
    only.close()


def test_overflow_column_is_walked():
    """The strip of tests/ray_battery.py at one triangle per leaf: the walk of a point with radius +inf enters every slot on its way
    down (best is 1e20 until the first leaf), three pushes a level, more entries than the LDS part of a lane's stack holds."""
    c = PC.case("strip")
    ctx = _ctx(c["tris"], leaf_size=1)
    depth4 = ctx.export_trees()["depth4"]
    assert 2 * depth4 > B.PT_LDS_STACK, "two pushes a level already pass the %d entries kept in LDS" % B.PT_LDS_STACK
    _check(ctx, c["ref"], "strip, leaf_size 1", PC.want("strip"))
    _check(ctx, PC.more_points("strip", N_SCENE), "strip, leaf_size 1, %d points" % N_SCENE)
    assert ctx.stats()["stack_entries"] == 3 * depth4 + 1
    ctx.close()


def test_after_update_vertices():
    tris = rb.make_scene("soup2")
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    P = tris.astype(np.float64)
    moved = (P + 0.03 * ext * np.sin(3.0 * P[..., [1, 2, 0]] / ext + 0.5)).astype(F32)
    pts = PC.more_points("soup2", 5000)
    ctx = _ctx(tris, dynamic=1)
    before = ctx.closest_point(pts)
    ctx.update_vertices([rb.mesh_of(moved)])
    got = _both(ctx, pts)
    fresh = B.Context(-1)
    rb.upload(fresh, moved)
    want = fresh.closest_point_host(pts)
    fresh.close()
    assert R.differ(want, before).any()
    PC.assert_same(got, want, "after pt_update_vertices vs a fresh upload's twin")
    PC.assert_same(got, ctx.closest_point_host(pts), "after pt_update_vertices vs the context's own twin")
    ctx.close()


def _cornell():
    sc = scene_io.load_scene_dir(rb.ASSETS, "cornell-box")
    ctx = B.Context(0)
    ctx.upload_scene(sc["entities"], [m for _, m, _ in sc["materials"]], env=B.make_env(color=(1, 1, 1), intensity=0.0))
    c = sc["camera"]
    W = H = 48
    return ctx, B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H), W, H


def test_streams_and_render_state():
    """Two launches over two caller streams with no synchronize between them (they share the context's one walk workspace); one right
    behind a pt_render_device; and a pt_render before and after all of it is bit-identical."""
    pts_a, pts_b = PC.more_points("cornell", 6000, seed=21), PC.more_points("cornell", 7000, seed=22)
    ctx, cam, W, H = _cornell()
    before, _ = ctx.render(cam, W, H, 8, 8)
    alone_a, alone_b = ctx.closest_point(pts_a), ctx.closest_point(pts_b)
    PC.assert_same(alone_a, ctx.closest_point_host(pts_a), "cornell as its own entities")
    a, b = DevPoints(pts_a), DevPoints(pts_b)
    frame = AS.DeviceFrame(W, H)
    try:
        ctx.closest_point_device(a.pts, a.n, a.out, stream=AS.stream(0))
        ctx.closest_point_device(b.pts, b.n, b.out, stream=AS.stream(1))
        ctx.synchronize()
        got_a, tail_a = a.read()
        got_b, tail_b = b.read()
        assert not R.differ(got_a, alone_a).any() and (tail_a == AS.FILL).all(), "the records on stream A"
        assert not R.differ(got_b, alone_b).any() and (tail_b == AS.FILL).all(), "the records on stream B"
        ctx.render_device(cam, W, H, 8, 8, frame.rgb, stream=AS.stream(0))
        ctx.closest_point_device(b.pts, b.n, b.out, stream=AS.stream(1))
        ctx.synchronize()
        rgb, _ = frame.read()
        got_b, _ = b.read()
        assert (rgb.view(np.uint32) == before.view(np.uint32)).all(), "the frame in flight"
        assert not R.differ(got_b, alone_b).any(), "the records behind the frame"
    finally:
        AS.destroy_streams()
        a.free()
        b.free()
        frame.free()
    after, _ = ctx.render(cam, W, H, 8, 8)
    assert (before.view(np.uint32) == after.view(np.uint32)).all()
    ctx.close()


def test_n_zero_launches_nothing_and_stats_are_the_point_kernels():
    c = PC.case("cornell")
    ctx = _ctx(c["tris"])
    depth4 = ctx.export_trees()["depth4"]
    ctx.closest_point(c["ref"])
    st = ctx.stats()
    assert st["launches"] == 1 and st["kernel_ms"] > 0
    assert st["block"] == 64 and st["lds_bytes"] in (B.PT_LDS_STACK * 64 * 4, 2 * B.PT_LDS_STACK * 64 * 4) and 0 < st["vgprs"] <= 128
    assert 1 <= st["grid"] <= (c["ref"].shape[0] + 63) // 64 and st["stack_entries"] == 3 * depth4 + 1
    ctx.synchronize()
    none = np.zeros(0, B.POINT_DTYPE)
    assert ctx.closest_point(none).shape == (0,)
    d = DevPoints(none)
    try:
        ctx.closest_point_device(d.pts, 0, d.out)
        ctx.closest_point_device(0, 0, 0)
        ctx.synchronize()
        _, tail = d.read()
    finally:
        d.free()
    assert (tail == AS.FILL).all(), "n == 0 wrote to the output"
    ctx.close()
