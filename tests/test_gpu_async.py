"""The asynchronous entry points on caller streams: pt_render_device, pt_render_batch_device, pt_render_aov_device, and what the library
orders behind a frame in flight (include/mi355pt.h, "one frame's worth of work buffers").

Every comparison is on raw bits against the oracle.  Scene: the Cornell box of tests/refit_common.py, uploaded with option "dynamic".
THE FRAME is 48 x 40 at 64 spp, depth 16 (cost pre-pass, sort, main launch), THE SECOND FRAME 17 x 5 at 8 spp (one unsorted launch).

(a) equivalence: the frame through pt_render_device on NULL, on a non-blocking and on a default-flag caller stream == pt_render == the
    oracle, float and RGBA8; pt_render_batch_device (two cameras) and pt_render_aov_device (against tests/aov_ref.py and the CPU twin) on
    a caller stream; a batch of three frames with "batch_frames" = 2 on a caller stream (two launch sequences of different length: the
    pixel queue changes inside the call); pixel shard 1 of 2 (foreign pixels 0, not the 0xA5 the buffers were filled with); a rank without a tile (16 x 16,
    tile 16, rank 3 of 4: all 0, PT_OK); a counted render whose counters pt_get_stats reads with no pt_synchronize before it.
(b) a state change behind frame A in flight on caller stream s, then frame B on s, the state put back, ONE pt_synchronize: A is the
    oracle's frame of the state before the call, B of the state after it.  b1 pt_set_materials (every base colour changed), b2
    pt_set_environment (colour -> automatic gradient), b3 pt_update_vertices (movement 1; afterwards HBM equals a host-only twin's
    arrays), b4 pt_upload_scene (the `rects` scene: fewer triangles, every buffer reused in place).
(c) two calls with no synchronize between them: c1 two cameras on two streams, c2 the frame on s1 then the second frame on NULL (the
    pixel queue changes in place), c3 the 17 x 5 view on s1 then 96 x 80 on s2 (the work buffers grow), c4 a frame on s1 then the
    blocking pt_render, c5 a frame on s1, pt_render_aov, pt_render_batch_device on s2, c6 a frame on s1 then 1 000 rays through
    pt_debug_eval("closest_hit") against the oracle's closest hits.
(d) FRAME A IS IN FLIGHT when the second call arrives: hipStreamQuery(s) immediately before it must be hipErrorNotReady, or the test
    fails (a correct library never fails these tests; the query only keeps a too-short frame from letting an incorrect one pass).
    Frame A is THE FRAME's view at SPP_A samples, chosen from measurements on an MI355X (profiles/r13_async.json): the smallest of
    64 / 256 / 1024 spp whose kernel_ms is at least 20 x the host time of an enqueue - 64: 11.7 ms against 20 x 0.14 ms, so frame A is
    THE FRAME itself.  The 17 x 5 view of c3 is frame A there and gets SPP_A samples too (7.3 ms): at 8 spp (1.3 ms) it misses the
    factor 20 and could be over before the query; the 8-spp launch is the second frame of c2 and part of (a).

WHICH WAIT A CASE TAKES.  The device-side wait (hipStreamWaitEvent on the ordering event, the stream changes and nothing else does) is
held by c1, c4 and c5 - in c5 the blocking guide pass takes it on the context's stream and leaves the context idle, so the batch on s2
adds none.  The host-side wait is held by b1-b4 (the state changes), c2 (the pixel queue changes: ensure_queue), c3 (the queue changes
and the work buffers grow: ensure), c6 (the probe) and the cut batch of (a).  On one stream throughout - (a), frame B of (b) - the
stream's own order is all there is.

Every test destroys its streams and frees its buffers in a finally, after a pt_synchronize.
"""
import numpy as np
import pytest

import aov_ref
import async_common as A
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B, scene_io

pytestmark = pytest.mark.gpu

W_, H_, SPP, DEPTH = 48, 40, 64, 16
W2, H2, SPP2 = 17, 5, 8
W3, H3 = 96, 80
SPP_A = 64  # (d): profiles/r13_async.json - kernel_ms 11.7 (48 x 40) and 7.3 (17 x 5) against 0.14 ms for the slowest enqueue
COUNTERS = ("samples", "rays", "scatters", "env_misses")
ENV2 = dict(use_auto=True, intensity=1.0)
RECTS_ENV = dict(use_auto=True, intensity=1.0)
RECTS_CAMERA = ([0.3, 0.4, 3.2], [0.0, 0.0, 0.0], [0, 1, 0], 50.0)
THREADS = 16


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what):
    """got = (float frame, RGBA8 frame) as DeviceFrame.read or Context.render returns them; want = the oracle's pair."""
    bad = _bits(got[0]) != _bits(want[0])
    assert not bad.any(), "%s: %d of %d floats differ" % (what, bad.sum(), bad.size)
    bad8 = np.asarray(got[1]) != np.asarray(want[1])
    assert not bad8.any(), "%s: %d of %d RGBA8 pixels differ" % (what, bad8.sum(), bad8.size)


class Box:
    """The module's context with the Cornell box uploaded, and the oracle's frames of every state, each rendered once."""

    def __init__(self, orc):
        self.orc = orc
        self.scene = RC.make_scene("cornell")
        self.materials = RC.cornell_materials()
        self.mats = np.stack([m for _, m, _ in self.materials]).astype(np.float32)
        self.mats2 = self.mats.copy()  # every base colour another one
        self.mats2[:, 0:3] = (0.15 + 0.7 * self.mats[:, [1, 2, 0]]).astype(np.float32)
        assert (self.mats2[:, 0:3] != self.mats[:, 0:3]).any(1).all()
        self.mv = RC.moved(self.scene, 1)
        self.rects = RC.make_scene("rects")
        self.flat = scene_io.flatten_scene(self.scene[0], self.materials)
        named = lambda n: [("m%d" % i, scene_io.MAT_DEFAULT, "") for i in range(n)]
        self._scenes = {"base": lambda: orc.Scene(self.flat),
                        "moved": lambda: orc.Scene(scene_io.flatten_scene(RC.as_entities(self.scene, self.mv), self.materials)),
                        "rects": lambda: orc.Scene(scene_io.flatten_scene(self.rects[0], named(self.rects[1])))}
        self._S, self._want = {}, {}
        c = scene_io.load_scene_dir(RC.ASSETS, "cornell-box")["camera"]
        lf = np.asarray(c["look_from"], np.float64)
        self._views = {1: (c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"]),
                       2: (list(lf + [0.3, 0.2, -0.1]), c["look_at"], c["look_up"], c["vertical_fov"] * 0.8), "rects": RECTS_CAMERA}
        self.ctx = B.Context(0)
        self.ctx.set_option("dynamic", 1)
        self.upload_box()

    def upload_box(self):
        RC.upload(self.ctx, self.scene, materials=list(self.mats), env=B.make_env(**RC.CORNELL_ENV))

    def cam(self, view, W, H, make=None):
        frm, at, up, fov = self._views[view]
        return (make or B.to_camera_data)(list(frm), list(at), list(up), fov, W, H)

    def oracle_scene(self, name):
        if name not in self._S:
            self._S[name] = self._scenes[name]()
        return self._S[name]

    def want(self, state, view, W, H, spp):
        """(float frame, RGBA8 frame, counters) of the oracle, read-only.  state: base | mats2 | env2 | moved | rects."""
        key = (state, view, W, H, spp)
        if key not in self._want:
            orc = self.orc
            S = self.oracle_scene(state if state in ("moved", "rects") else "base")
            env = ENV2 if state == "env2" else RECTS_ENV if state == "rects" else RC.CORNELL_ENV
            if state == "mats2":
                S.set_materials(self.mats2)
            try:
                rgb, rgba8, cnt = S.render(self.cam(view, W, H, orc.to_camera_data), orc.make_env(**env), W, H, spp, DEPTH, threads=THREADS, want_rgba8=True, want_counters=True)
            finally:
                if state == "mats2":
                    S.set_materials(self.mats)
            assert np.isfinite(rgb).all() and rgb.std() > 0.01, "the oracle's frame of %r shows something" % (key,)
            rgb.setflags(write=False)
            rgba8.setflags(write=False)
            self._want[key] = (rgb, rgba8, cnt)
        return self._want[key]

    def want_aov(self, W, H, n):
        key = ("aov", W, H, n)
        if key not in self._want:
            a = aov_ref.aov(self.oracle_scene("base"), self.flat, RC.CORNELL_ENV, self.cam(1, W, H, self.orc.to_camera_data).as_array(), W, H, n)
            a.setflags(write=False)
            self._want[key] = a
        return self._want[key]


@pytest.fixture(scope="module")
def box(orc):
    b = Box(orc)
    yield b
    b.ctx.close()
    A.destroy_streams()


def _require_in_flight(case, s):
    """(d): frame A is still running when the next call arrives."""
    q = A.query(s)
    print("in-flight query, %s: hipStreamQuery = %d" % (case, q))
    assert q == A.HIP_ERROR_NOT_READY, "%s: frame A was over before the next call (hipStreamQuery = %d): the test would show nothing" % (case, q)


class Buffers:
    """The DeviceFrames of one test, all allocated (and filled) BEFORE anything is enqueued - an allocation or a fill may wait for the
    device - and freed, with the streams destroyed, after the test's pt_synchronize."""

    def __init__(self, ctx):
        self.ctx, self.frames = ctx, []

    def frame(self, *a, **kw):
        self.frames.append(A.DeviceFrame(*a, **kw))
        return self.frames[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            self.ctx.synchronize()
        finally:
            for f in self.frames:
                f.free()
            A.destroy_streams()
        return False


# ---------------------------------------------------------------------------------------------------------------------
# (a) equivalence
# ---------------------------------------------------------------------------------------------------------------------
def _stream_of(kind):
    return None if kind == "null" else A.stream(0, nonblocking=(kind == "nonblocking"))


@pytest.mark.parametrize("kind", ["null", "nonblocking", "default_flag"])
def test_a_render_device_equals_render_and_the_oracle(box, kind):
    ctx = box.ctx
    for view, W, H, spp in ((1, W_, H_, SPP), (1, W2, H2, SPP2)):
        want = box.want("base", view, W, H, spp)
        cam = box.cam(view, W, H)
        blocking = ctx.render(cam, W, H, spp, DEPTH, want_rgba8=True)
        with Buffers(ctx) as bufs:
            f = bufs.frame(W, H)
            ctx.render_device(cam, W, H, spp, DEPTH, f.rgb, f.rgba8, stream=_stream_of(kind))
            ctx.synchronize()
            got = f.read()
        _same(got, want, "pt_render_device on the %s stream, %dx%d == the oracle" % (kind, W, H))
        _same(blocking, want, "pt_render, %dx%d == the oracle" % (W, H))


def test_a_batch_device_on_a_caller_stream(box):
    ctx = box.ctx
    frames = [(box.cam(1, W_, H_), None), (box.cam(2, W_, H_), box.mats2)]
    want = [box.want("base", 1, W_, H_, SPP), box.want("mats2", 2, W_, H_, SPP)]
    with Buffers(ctx) as bufs:
        f = bufs.frame(W_, H_, frames=2)
        ctx.render_batch_device(frames, W_, H_, SPP, DEPTH, f.rgb, f.rgba8, stream=A.stream(0))
        ctx.synchronize()
        rgb, rgba8 = f.read()
    for k in (0, 1):
        _same((rgb[k], rgba8[k]), want[k], "pt_render_batch_device on a caller stream, frame %d == the oracle" % k)
    blocking = ctx.render_batch(frames, W_, H_, SPP, DEPTH, want_rgba8=True)
    for k in (0, 1):
        _same((blocking[0][k], blocking[1][k]), want[k], "pt_render_batch, frame %d == the oracle" % k)


def test_a_cut_batch_on_a_caller_stream(box):
    """Three frames, at most two per launch sequence: sequence 1 rewrites the pixel queue (another batch length) behind sequence 0 of
    the same call, on the caller's stream."""
    ctx = box.ctx
    frames = [(box.cam(1, W_, H_), None), (box.cam(2, W_, H_), box.mats2), (box.cam(1, W_, H_), box.mats2)]
    want = [box.want("base", 1, W_, H_, SPP), box.want("mats2", 2, W_, H_, SPP), box.want("mats2", 1, W_, H_, SPP)]
    assert B.plan_batch(W_, H_, 3, 2) == [2, 1]
    try:
        ctx.set_option("batch_frames", 2)
        with Buffers(ctx) as bufs:
            f = bufs.frame(W_, H_, frames=3)
            ctx.render_batch_device(frames, W_, H_, SPP, DEPTH, f.rgb, f.rgba8, stream=A.stream(0))
            ctx.synchronize()
            rgb, rgba8 = f.read()
    finally:
        ctx.set_option("batch_frames", 0)
    for k in range(3):
        _same((rgb[k], rgba8[k]), want[k], "cut batch on a caller stream, frame %d == the oracle" % k)


def _aov_same(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), "%s: %d of %d floats differ" % (what, bad.sum(), bad.size)


def _host_twin_aov(box, W, H, n):
    h = B.Context(-1)
    try:
        RC.upload(h, box.scene, materials=list(box.mats), env=B.make_env(**RC.CORNELL_ENV))
        return h.aov_host(box.cam(1, W, H), W, H, n)
    finally:
        h.close()


def test_a_aov_device_on_a_caller_stream(box):
    ctx, n = box.ctx, 2
    want = box.want_aov(W_, H_, n)
    _aov_same(_host_twin_aov(box, W_, H_, n), want, "pt_debug_aov_host == aov_ref")
    with Buffers(ctx) as bufs:
        f = bufs.frame(W_, H_, floats=8)
        ctx.render_aov_device(box.cam(1, W_, H_), W_, H_, n, f.rgb, stream=A.stream(0))
        ctx.synchronize()
        got, _ = f.read()
    _aov_same(got, want, "pt_render_aov_device on a caller stream == aov_ref")
    assert ctx.stats()["launches"] == 1


def _owned(W, H, tile, rank, world):
    m = np.zeros(W * H, bool)
    m[B.shard_pixels(W, H, tile, rank, world)] = True
    return m.reshape(H, W)[::-1]  # framebuffer order


def test_a_pixel_shard_on_a_caller_stream(box):
    ctx = box.ctx
    want = box.want("base", 1, W_, H_, SPP)
    own = _owned(W_, H_, 16, 1, 2)
    assert own.any() and not own.all()
    try:
        ctx.set_pixel_shard(1, 2, 16)
        with Buffers(ctx) as bufs:
            f = bufs.frame(W_, H_)
            ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP, DEPTH, f.rgb, f.rgba8, stream=A.stream(0))
            ctx.synchronize()
            rgb, rgba8 = f.read()
    finally:
        ctx.set_pixel_shard(0, 1, 16)
    _same((rgb[own], rgba8[own]), (want[0][own], want[1][own]), "rank 1 of 2: owned pixels == the oracle")
    assert (_bits(rgb[~own]) == 0).all() and (rgba8[~own] == 0).all(), "pixels of the other rank must be 0 (the buffers were filled with 0xA5)"


def test_a_rank_without_a_tile_on_a_caller_stream(box):
    ctx = box.ctx
    try:
        ctx.set_pixel_shard(3, 4, 16)  # a 16 x 16 frame is one tile, rank 0's
        assert B.shard_pixels(16, 16, 16, 3, 4).size == 0
        with Buffers(ctx) as bufs:
            f = bufs.frame(16, 16)
            ctx.render_device(box.cam(1, 16, 16), 16, 16, SPP, DEPTH, f.rgb, f.rgba8, stream=A.stream(0))
            ctx.synchronize()  # PT_OK, or it raises
            rgb, rgba8 = f.read()
    finally:
        ctx.set_pixel_shard(0, 1, 16)
    assert (_bits(rgb) == 0).all() and (rgba8 == 0).all()


def test_a_counted_render_stats_without_a_synchronize(box):
    ctx = box.ctx
    want = box.want("base", 1, W_, H_, SPP)
    try:
        ctx.set_option("count", 1)
        with Buffers(ctx) as bufs:
            f = bufs.frame(W_, H_)
            ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP, DEPTH, f.rgb, f.rgba8, stream=A.stream(0))
            st = ctx.stats()  # no pt_synchronize before it
            ctx.synchronize()
            got = f.read()
    finally:
        ctx.set_option("count", 0)
    assert {k: int(st[k]) for k in COUNTERS} == {k: int(want[2][k]) for k in COUNTERS}
    assert st["kernel_ms"] > 0
    _same(got, want, "counted render on a caller stream == the oracle")


# ---------------------------------------------------------------------------------------------------------------------
# (b) a state change behind a frame in flight
# ---------------------------------------------------------------------------------------------------------------------
def _behind_frame_a(box, case, change, restore, state_b, view_b=1):
    """Frame A (state base) on s, the in-flight query, change(), frame B on s, restore(), one pt_synchronize; A and B against the oracle."""
    ctx = box.ctx
    want_a, want_b = box.want("base", 1, W_, H_, SPP_A), box.want(state_b, view_b, W_, H_, SPP)
    assert (_bits(want_b[0]) != _bits(box.want("base", view_b, W_, H_, SPP)[0])).any(), "the state after the call gives another frame"
    cam_a, cam_b = box.cam(1, W_, H_), box.cam(view_b, W_, H_)
    with Buffers(ctx) as bufs:
        fa, fb = bufs.frame(W_, H_), bufs.frame(W_, H_)
        s = A.stream(0)
        try:
            ctx.render_device(cam_a, W_, H_, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s)
            _require_in_flight(case, s)
            change()
            ctx.render_device(cam_b, W_, H_, SPP, DEPTH, fb.rgb, fb.rgba8, stream=s)
        finally:
            restore()
        ctx.synchronize()
        a, b = fa.read(), fb.read()
    _same(a, want_a, "%s: frame A == the oracle's frame of the state BEFORE the call" % case)
    _same(b, want_b, "%s: frame B == the oracle's frame of the state AFTER the call" % case)


def test_b1_set_materials_behind_a_frame(box):
    _behind_frame_a(box, "b1 pt_set_materials", lambda: box.ctx.set_materials(box.mats2), lambda: box.ctx.set_materials(box.mats), "mats2")


def test_b2_set_environment_behind_a_frame(box):
    _behind_frame_a(box, "b2 pt_set_environment", lambda: box.ctx.set_environment(B.make_env(**ENV2)),
                    lambda: box.ctx.set_environment(B.make_env(**RC.CORNELL_ENV)), "env2")


def test_b3_update_vertices_behind_a_frame(box):
    ctx = box.ctx
    back = RC.moved(box.scene, 0)
    _behind_frame_a(box, "b3 pt_update_vertices", lambda: ctx.update_vertices(box.mv), lambda: ctx.update_vertices(back), "moved")
    host = B.Context(-1)  # the twin by itself, as test_gpu_refit.py::test_device_arrays_equal_the_host_twin
    try:
        host.set_option("dynamic", 1)
        RC.upload(host, box.scene, materials=list(box.mats), env=B.make_env(**RC.CORNELL_ENV))
        host.update_vertices(box.mv)
        host.update_vertices(back)
        RC.same_arrays(host.export_trees(), ctx.export_trees(device=True), "b3: HBM against the host twin after the two updates")
    finally:
        host.close()


def test_b4_upload_scene_behind_a_frame(box):
    ctx = box.ctx
    assert RC.soup_of(box.rects[0]).shape[0] < RC.soup_of(box.scene[0]).shape[0]  # every scene buffer is reused in place
    _behind_frame_a(box, "b4 pt_upload_scene", lambda: RC.upload(ctx, box.rects, env=B.make_env(**RECTS_ENV)), box.upload_box, "rects", view_b="rects")
    _same(ctx.render(box.cam(1, W_, H_), W_, H_, SPP, DEPTH, want_rgba8=True), box.want("base", 1, W_, H_, SPP), "b4: the box uploaded again")


# ---------------------------------------------------------------------------------------------------------------------
# (c) two calls, no synchronize between them
# ---------------------------------------------------------------------------------------------------------------------
def test_c1_two_cameras_on_two_streams(box):
    ctx = box.ctx
    want_a, want_b = box.want("base", 1, W_, H_, SPP_A), box.want("base", 2, W_, H_, SPP)
    with Buffers(ctx) as bufs:
        fa, fb = bufs.frame(W_, H_), bufs.frame(W_, H_)
        s1, s2 = A.stream(0), A.stream(1)
        ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s1)
        _require_in_flight("c1 two streams", s1)
        ctx.render_device(box.cam(2, W_, H_), W_, H_, SPP, DEPTH, fb.rgb, fb.rgba8, stream=s2)
        ctx.synchronize()
        a, b = fa.read(), fb.read()
    _same(a, want_a, "c1: camera 1 on s1")
    _same(b, want_b, "c1: camera 2 on s2")


def test_c2_the_pixel_queue_changes_in_place(box):
    ctx = box.ctx
    want_a, want_b = box.want("base", 1, W_, H_, SPP_A), box.want("base", 1, W2, H2, SPP2)
    with Buffers(ctx) as bufs:
        fa, fb = bufs.frame(W_, H_), bufs.frame(W2, H2)
        s1 = A.stream(0)
        ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s1)
        _require_in_flight("c2 queue in place", s1)
        ctx.render_device(box.cam(1, W2, H2), W2, H2, SPP2, DEPTH, fb.rgb, fb.rgba8, stream=None)
        ctx.synchronize()
        a, b = fa.read(), fb.read()
    _same(a, want_a, "c2: 48 x 40 on s1")
    _same(b, want_b, "c2: 17 x 5 on the context's stream")


def test_c3_the_work_buffers_grow(box):
    ctx = box.ctx
    want_a, want_b = box.want("base", 1, W2, H2, SPP_A), box.want("base", 1, W3, H3, SPP)
    with Buffers(ctx) as bufs:
        fa, fb = bufs.frame(W2, H2), bufs.frame(W3, H3)
        s1, s2 = A.stream(0), A.stream(1)
        ctx.render_device(box.cam(1, W2, H2), W2, H2, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s1)
        _require_in_flight("c3 buffers grow", s1)
        ctx.render_device(box.cam(1, W3, H3), W3, H3, SPP, DEPTH, fb.rgb, fb.rgba8, stream=s2)
        ctx.synchronize()
        a, b = fa.read(), fb.read()
    _same(a, want_a, "c3: 17 x 5 on s1")
    _same(b, want_b, "c3: 96 x 80 on s2")


def test_c4_blocking_render_behind_a_frame(box):
    ctx = box.ctx
    want_a, want_b = box.want("base", 1, W_, H_, SPP_A), box.want("base", 2, W_, H_, SPP)
    with Buffers(ctx) as bufs:
        fa = bufs.frame(W_, H_)
        s1 = A.stream(0)
        ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s1)
        _require_in_flight("c4 blocking render", s1)
        b = ctx.render(box.cam(2, W_, H_), W_, H_, SPP, DEPTH, want_rgba8=True)
        ctx.synchronize()
        a = fa.read()
    _same(a, want_a, "c4: the frame on s1")
    _same(b, want_b, "c4: pt_render behind it")


def test_c5_blocking_aov_then_a_batch_on_another_stream(box):
    ctx, n = box.ctx, 2
    frames = [(box.cam(1, W_, H_), None), (box.cam(2, W_, H_), box.mats2)]
    want_a, want_b = box.want("base", 1, W_, H_, SPP_A), [box.want("base", 1, W_, H_, SPP), box.want("mats2", 2, W_, H_, SPP)]
    want_aov = box.want_aov(W_, H_, n)
    with Buffers(ctx) as bufs:
        fa, fb = bufs.frame(W_, H_), bufs.frame(W_, H_, frames=2)
        s1, s2 = A.stream(0), A.stream(1)
        ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s1)
        _require_in_flight("c5 blocking aov, batch", s1)
        aov = ctx.render_aov(box.cam(1, W_, H_), W_, H_, n)
        ctx.render_batch_device(frames, W_, H_, SPP, DEPTH, fb.rgb, fb.rgba8, stream=s2)
        ctx.synchronize()
        a, (rgb, rgba8) = fa.read(), fb.read()
    _same(a, want_a, "c5: the frame on s1")
    _aov_same(aov, want_aov, "c5: pt_render_aov behind it")
    for k in (0, 1):
        _same((rgb[k], rgba8[k]), want_b[k], "c5: frame %d of the batch on s2" % k)


def test_c6_probe_behind_a_frame(box):
    ctx = box.ctx
    want_a = box.want("base", 1, W_, H_, SPP_A)
    rng = np.random.default_rng(1306)
    org = np.asarray(box._views[1][0], np.float64) + rng.uniform(-0.05, 0.05, (1000, 3))
    to = np.asarray(box._views[1][1], np.float64) + rng.uniform(-1.2, 1.2, (1000, 3))
    d = (to - org).astype(np.float32)
    d /= np.sqrt((d * d).sum(1, dtype=np.float32), dtype=np.float32)[:, None]
    rays = np.concatenate([org.astype(np.float32), d], 1)
    hit, t, u, v, prim = box.oracle_scene("base").intersect_n(rays, threads=THREADS)
    assert 0.5 < hit.mean() and np.unique(prim[hit]).size > 20
    with Buffers(ctx) as bufs:
        fa = bufs.frame(W_, H_)
        s1 = A.stream(0)
        ctx.render_device(box.cam(1, W_, H_), W_, H_, SPP_A, DEPTH, fa.rgb, fa.rgba8, stream=s1)
        _require_in_flight("c6 probe", s1)
        out = ctx.debug_eval("closest_hit", rays, 5)
        ctx.synchronize()
        a = fa.read()
    _same(a, want_a, "c6: the frame on s1")
    bad = ((out[:, 0] != 0) != hit) | (np.ascontiguousarray(out[:, 4]).view(np.int32) != prim)
    for k, w in ((1, t), (2, u), (3, v)):
        bad |= hit & (np.ascontiguousarray(out[:, k]).view(np.uint32) != w.view(np.uint32))
    assert not bad.any(), "c6: %d of 1000 closest hits differ from the oracle's" % bad.sum()
