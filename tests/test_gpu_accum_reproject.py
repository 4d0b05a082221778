"""Reprojection of the accumulation on the GPU (pt_accum_reproject, pt_accum_reproject_device; kernel: csrc/pt_accum_reproject.hip).  Every
comparison is bit for bit.  Scene: Cornell at 40 x 30 and 70 x 45, depth 4, environment use_auto = 1 (test_gpu_accum's); adds of 2 + 3 + 2
first, so n = 7 and n_half = 3; guides from pt_render_aov at n = 1.

1. The moved state: pt_debug_accum_state and pt_accum_read (rgb, RGBA8, noise, samples) after pt_accum_reproject == the twin
   pt_debug_accum_reproject_host applied to the state before == the restatement tests/accum_reproject_ref.py; identical cameras, a 10
   degree orbit, a sideways step and an old camera that looks away; cap 0 and 4.  On the orbit between a quarter and all but a quarter of
   the pixels keep history, otherwise the leg would show nothing.  pt_get_stats shows the one launch.
2. Identical camera, no cap: the state is unchanged, and one more uniform add gives bit for bit the state of the same accumulation that
   never had the call: the RNG streams are untouched.
3. A selecting add after the orbit, threshold at the median noise: active_pixels >= the number of pixels with n == 0, and each of those
   then has n = n_samples.
4. pt_accum_add_device -> pt_render_aov_device(new camera) -> pt_accum_reproject_device -> pt_accum_add_device -> pt_accum_denoise_device
   on ONE caller's stream with no synchronize in between equals the blocking sequence.
5. Shard 0 of world 2: pixels whose source lies in the other shard come out reset; equals the twin with the mask.
6. Refused by name with the accumulation intact: no accumulation, a shard changed after begin, bad parameters.  A pt_render after a
   reproject is bit for bit the pt_render before, and pt_accum_begin afterwards reaches pt_render(N) again."""
import ctypes as C

import numpy as np
import pytest

import accum_reproject_common as RC
import aov_common as AC
import async_common as AS
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
DEPTH = 4
ENV = dict(use_auto=True, intensity=1.0)
_ctx = {}


def scene():
    return dict(AC.scene("cornell"), env=ENV)


def gpu():
    """ONE context for the whole module (its stream and one caller stream stay below four hardware queues)."""
    if "ctx" not in _ctx:
        _ctx["ctx"] = B.Context(0)
        AC.upload(_ctx["ctx"], scene(), B)
        _ctx["host"] = B.Context(-1)
    return _ctx["ctx"]


def host():
    gpu()
    return _ctx["host"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    AS.destroy_streams()
    for k in ("ctx", "host"):
        if k in _ctx:
            _ctx[k].close()
    _ctx.clear()


def cams(kind, W, H):
    """The orbit is one of 10 degrees: with the default tolerances the twin keeps the history of 0.64 (40 x 30) and 0.59 (70 x 45) of the pixels
    there (0.89 and 0.90 at 2 degrees, which would leave too few fresh pixels to show anything)."""
    return RC.pair(kind, scene()["camera"], W, H, deg=10.0)


def P(n, thr=0.0):
    return B.accum_default_params(n_samples=n, noise_threshold=thr)


def begin_7_3(ctx, cam, W, H):
    ctx.accum_begin(cam, W, H, DEPTH)
    for k in (2, 3, 2):
        ctx.accum_add(P(k))


def snapshot(ctx):
    """dict of the state and the read-back, as the twin returns them"""
    rd, st = ctx.accum_read(), ctx.accum_state()
    return dict(st, rgb=rd["rgb"], rgba8=rd["rgba8"], noise=rd["noise"], samples=rd["samples"])


def blob(snap):
    return [np.ascontiguousarray(snap[k]).tobytes() for k in sorted(snap)]


@pytest.mark.parametrize("cap", [0, 4])
@pytest.mark.parametrize("kind", ["identical", "orbit", "sideways", "away"])
@pytest.mark.parametrize("W,H", [(40, 30), (70, 45)])
def test_moved_state_equals_the_twin(orc, W, H, kind, cap):
    ctx = gpu()
    old, new = cams(kind, W, H)
    prev, cur = ctx.render_aov(old, W, H, 1), ctx.render_aov(new, W, H, 1)
    prm = B.reproject_default_params(max_history=cap)
    begin_7_3(ctx, old, W, H)
    try:
        before = snapshot(ctx)
        assert (before["n"] == 7).all() and (before["n_half"] == 3).all()
        info0 = ctx.accum_info()
        ctx.accum_reproject(new, prev, cur, prm)
        stats = ctx.stats()
        after = snapshot(ctx)
        info1 = ctx.accum_info()
    finally:
        ctx.accum_end()
    twin = host().accum_reproject_host(old, new, prev, cur, before, None, prm)
    want = RC.ref(old, new, prev, cur, before, None, prm)
    RC.assert_state(twin, want, "twin vs restatement")
    RC.assert_state(after, twin, "pt_accum_reproject vs the twin")
    assert (after["samples"] == twin["n"]).all()
    share = float(want["has"].mean())
    print("%dx%d %s: %.3f of the pixels keep history" % (W, H, kind, share))
    if kind == "identical":
        assert share == 1
    if kind == "orbit":
        assert 0.25 <= share <= 0.75
    if kind == "sideways":
        assert 0 < share < 1
    if kind == "away":
        assert share == 0 and (after["n"] == 0).all() and np.isposinf(after["noise"]).all() and (after["rgba8"] == 0).all()
    if cap == 4 and share > 0:
        assert (after["n"][want["has"]] == 4).all() and (after["n_half"][want["has"]] == 1).all()
    assert stats["launches"] == 1 and stats["kernel_ms"] > 0 and stats["block"] == 256 and stats["lds_bytes"] == 0 and 0 < stats["vgprs"] <= 64, stats
    assert stats["grid"] == (W * H + 255) // 256, stats
    for k in ("adds", "samples_total", "owned_pixels", "width", "height"):
        assert info0[k] == info1[k], k


def test_identical_camera_leaves_state_and_streams_alone():
    W, H = 40, 30
    ctx = gpu()
    cam, same_cam = cams("identical", W, H)
    aov = ctx.render_aov(cam, W, H, 1)
    begin_7_3(ctx, cam, W, H)
    try:
        before = snapshot(ctx)
        ctx.accum_add(P(3))
        plain = snapshot(ctx)
    finally:
        ctx.accum_end()
    begin_7_3(ctx, cam, W, H)
    try:
        ctx.accum_reproject(same_cam, aov, aov, None)  # (one buffer twice)
        assert blob(snapshot(ctx)) == blob(before), "identical cameras, no cap: nothing may change"
        ctx.accum_reproject(same_cam, aov, aov, None)  # ... and back into the first set of buffers
        assert blob(snapshot(ctx)) == blob(before)
        ctx.accum_add(P(3))
        assert blob(snapshot(ctx)) == blob(plain), "the add after a reproject draws what it would have drawn without it"
    finally:
        ctx.accum_end()
    rgb, rgba8 = ctx.render(cam, W, H, 10, DEPTH, want_rgba8=True)
    assert RC.same(plain["rgb"], rgb).all() and (plain["rgba8"] == rgba8).all()


def test_a_selecting_add_takes_the_pixels_without_history():
    W, H = 70, 45
    ctx = gpu()
    old, new = cams("orbit", W, H)
    prev, cur = ctx.render_aov(old, W, H, 1), ctx.render_aov(new, W, H, 1)
    begin_7_3(ctx, old, W, H)
    try:
        ctx.accum_reproject(new, prev, cur, None)
        rd = ctx.accum_read()
        fresh = rd["samples"] == 0
        assert fresh.any() and np.isposinf(rd["noise"][fresh]).all()
        finite = rd["noise"][np.isfinite(rd["noise"]) & (rd["noise"] > 0)]
        ctx.accum_add(P(5, thr=float(np.median(finite))))
        info = ctx.accum_info()
        after = ctx.accum_read()["samples"]
        assert info["active_pixels"] >= int(fresh.sum()) and info["active_pixels"] < W * H
        assert (after[fresh] == 5).all()
        assert set(np.unique(after)) <= {5, 7, 12}
    finally:
        ctx.accum_end()


def test_one_stream_no_synchronize():
    W, H = 40, 30
    ctx = gpu()
    old, new = cams("orbit", W, H)
    prev = ctx.render_aov(old, W, H, 1)
    prm = B.reproject_default_params(max_history=6)
    ctx.accum_begin(old, W, H, DEPTH)
    try:
        ctx.accum_add(P(4))
        ctx.accum_add(P(4))
        cur = ctx.render_aov(new, W, H, 1)
        ctx.accum_reproject(new, prev, cur, prm)
        ctx.accum_add(P(4))
        want, want8 = ctx.accum_denoise(cur, None, want_rgba8=True)
        want_state = snapshot(ctx)
    finally:
        ctx.accum_end()
    s = AS.stream(0, nonblocking=True)
    out, g_prev, g_cur = AS.DeviceFrame(W, H), AS.DeviceFrame(W, H, floats=8), AS.DeviceFrame(W, H, floats=8)
    try:
        AS.to_device(g_prev.rgb, prev)
        ctx.accum_begin(old, W, H, DEPTH)
        ctx.accum_add_device(P(4), None, None, stream=s)
        ctx.accum_add_device(P(4), None, None, stream=s)
        ctx.render_aov_device(new, W, H, 1, g_cur.rgb, stream=s)
        ctx.accum_reproject_device(new, g_prev.rgb, g_cur.rgb, prm, stream=s)
        ctx.accum_add_device(P(4), None, None, stream=s)
        ctx.accum_denoise_device(g_cur.rgb, out.rgb, None, d_out_rgba8=out.rgba8, stream=s)
        ctx.synchronize()
        got, got8 = out.read()
        got_state = snapshot(ctx)
    finally:
        ctx.accum_end()
        out.free()
        g_prev.free()
        g_cur.free()
    RC.assert_state(got_state, want_state, "one caller stream vs the blocking sequence", RC.KEYS + ("samples",))
    assert RC.same(got, want).all() and (got8 == want8).all()
    assert 0 < (got_state["n"] == 4).mean() < 1 and (got_state["n"] == 10).any(), "both kinds of pixel: 8 samples capped at 6 plus 4, and fresh ones"


def test_shard_of_world_two():
    W, H = 70, 45
    ctx = gpu()
    old, new = cams("orbit", W, H)
    prev, cur = ctx.render_aov(old, W, H, 1), ctx.render_aov(new, W, H, 1)
    own = np.zeros(W * H, np.uint8)
    own[B.shard_pixels(W, H, 8, 0, 2)] = 1
    own = np.ascontiguousarray(own.reshape(H, W)[::-1])  # launch order -> framebuffer order
    ctx.set_pixel_shard(0, 2, 8)
    try:
        begin_7_3(ctx, old, W, H)
        before = snapshot(ctx)
        ctx.accum_reproject(new, prev, cur, None)
        after = snapshot(ctx)
    finally:
        ctx.accum_end()
        ctx.set_pixel_shard(0, 1, 16)
    twin = host().accum_reproject_host(old, new, prev, cur, before, own, None)
    RC.assert_state(after, twin, "shard 0 of 2 vs the twin with the mask")
    everywhere = RC.ref(old, new, prev, cur, before, None, None)["has"]
    lost = everywhere & (own != 0) & (twin["n"] == 0)
    assert lost.any(), "some sources must lie in the other shard"
    assert (after["n"][own == 0] == 0).all() and (after["noise"][own == 0].view(U32) == 0).all()


def test_refusals_and_what_comes_after():
    L = B.lib()
    W, H = 40, 30
    ctx = gpu()
    h = ctx._h
    old, new = cams("orbit", W, H)
    prev, cur = ctx.render_aov(old, W, H, 1), ctx.render_aov(new, W, H, 1)
    fp = C.POINTER(C.c_float)
    gp, gc, cam = prev.ctypes.data_as(fp), cur.ctypes.data_as(fp), C.byref(new)
    guides = AS.DeviceFrame(W, H, floats=8)
    dev = C.c_void_p(guides.rgb)
    calls = ((lambda p=None, c=cam, a=gp: L.pt_accum_reproject(h, c, a, gc, p), "pt_accum_reproject"),
             (lambda p=None, c=cam, a=dev: L.pt_accum_reproject_device(h, c, a, dev, p, None), "pt_accum_reproject_device"))
    err = lambda: L.pt_last_error(h).decode()
    try:
        want10, want10_8 = ctx.render(old, W, H, 10, DEPTH, want_rgba8=True)
        ctx.accum_end()
        for call, who in calls:
            assert call() == -1 and who + ": the context has no accumulation (pt_accum_begin not called)" in err(), err()
        begin_7_3(ctx, old, W, H)
        try:
            before = blob(snapshot(ctx))
            ctx.set_pixel_shard(0, 2, 8)
            for call, who in calls:
                assert call() == -1 and who + ": the pixel shard changed after pt_accum_begin" in err(), err()
            ctx.set_pixel_shard(0, 1, 16)
            for call, who in calls:
                assert call(None, None) == -1 and who + ": NULL new_cam" in err(), err()
                assert call(None, cam, None) == -1 and who + ": NULL aov_prev" in err(), err()
                for kw, word in ((dict(reserved=2), "reserved must be 0"), (dict(max_history=1), "max_history 1"), (dict(max_history=-1), "max_history -1"),
                                 (dict(depth_tol=-1.0), "depth_tol"), (dict(albedo_tol=float("nan")), "albedo_tol"), (dict(normal_min=2.0), "normal_min"),
                                 (dict(normal_min=float("nan")), "normal_min")):
                    assert call(C.byref(B.reproject_default_params(**kw))) == -1 and who + ": " + word in err(), (kw, err())
            ctx.synchronize()
            assert blob(snapshot(ctx)) == before, "a refused call changed the accumulation"
            ctx.accum_reproject(new, prev, cur, None)  # ... and with valid arguments it runs
            assert ctx.stats()["launches"] == 1
            assert blob(snapshot(ctx)) != before
            again, again8 = ctx.render(old, W, H, 10, DEPTH, want_rgba8=True)
            assert RC.same(again, want10).all() and (again8 == want10_8).all(), "pt_render after a reproject"
            # before the first add the call only changes the camera: the accumulation then is pt_render's at the new camera
            ctx.accum_begin(old, W, H, DEPTH)
            ctx.accum_reproject(new, prev, cur, None)
            ctx.accum_add(P(4))
            rgb = ctx.accum_add(P(6))[0]
            assert RC.same(rgb, ctx.render(new, W, H, 10, DEPTH)[0]).all(), "a reproject before the first add"
            ctx.accum_begin(old, W, H, DEPTH)
            ctx.accum_add(P(4))
            rgb, rgba8 = ctx.accum_add(P(6), want_rgba8=True)
            assert RC.same(rgb, want10).all() and (rgba8 == want10_8).all(), "pt_accum_begin after a reproject reaches pt_render(N) again"
        finally:
            ctx.accum_end()
            ctx.set_pixel_shard(0, 1, 16)
    finally:
        guides.free()
