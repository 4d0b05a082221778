"""The guide pass over a ray image on the GPU (pt_render_aov_rays; kernels: csrc/pt_kernel_aov_rays.hip, csrc/pt_kernel_aov_rays_wt.hip =
csrc/pt_aov_follow.h with PT_RAYGEN = 1).  Every comparison is bit for bit on all 8 channels of every pixel.

The reference is the CPU twin pt_debug_aov_rays_host, which tests/test_aov_rays_host.py holds to the numpy restatement on these cases.
The zero-jitter tables (centres, probes) cannot tell one record's jitter from another's; the jittered cases can, and there the GPU is
held to the twin and to the restatement (tests/aov_rays_ref.py) itself.

* GPU == twin over the cases of tests/aov_rays_common.py (four scenes, pixel-centre rays at 20 x 13 and 64 x 48 and 24 x 16 probe rays,
  n = 1 and 3, max_follow 0 and 4), blocking and device forms, "watertight" 0 and 1; pt_get_stats reads as after pt_render_aov.
* GPU == twin == aov_rays_ref over JITTER_CASES: the scrambled and equirect tables of tests/ray_tables.py (every record its own origin,
  direction and jitter, NaN in the reserved floats) on mirror_wall and tir, where followed rays start from jittered ones, at 1 x 1, 7 x 9,
  20 x 13, 130 x 3, 3 x 130 and 64 x 48, n_samples 1, 3 and 16, max_follow 0 and 4, "watertight" 0 and 1 (the restatement under both),
  blocking and device forms, each case first shown to meet the precondition of tests/ray_tables.py in guide buffers;
  both slab forms on a scrambled table; consequence (c) on the device: where coverage at n_samples = 1 says hit, the depth is
  pt_trace_closest's t on table_rays' sample-0 ray.
* The device form on a caller's stream directly behind a pt_render_rays_device of the same table with no synchronize.
* Both slab forms; a shard of world 3 with tile 8 at 20 x 13 (one rank gets a partial block column; pixels not owned are +0); the frame
  after pt_set_materials, pt_set_environment and pt_update_vertices; a 130 x 3 frame (more blocks than rows); 1 x 1 jittered images.
* max_follow = 0 with the pixel-centre table == pt_render_aov_follow(max_follow = 0) through degenerate cameras, on 64 listed pixels.
* A pt_render, a pt_render_rays and an accumulation add around the call are bit-identical to the same calls without it.
* pt_render_rays_device -> pt_render_aov_rays_device -> pt_denoise_device on one stream without a synchronize == pt_debug_denoise_host
  of the two parts.
* A context with a communicator is refused by name."""
import ctypes as C

import numpy as np
import pytest

import aov_rays_common as RC
import aov_rays_ref
import async_common as AS
import ray_image_ref as RR
import refit_common as RF
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import ray_image as RI

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
_state = {}
_twin = {}


def gpu(name):
    """ONE context for the module (its stream and two caller streams stay below four hardware queues), holding scene `name`."""
    if "ctx" not in _state:
        _state["ctx"] = B.Context(0)
    if _state.get("scene") != name:
        RC.upload(_state["ctx"], RC.scene(name), B)
        _state["scene"] = name
    return _state["ctx"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    AS.destroy_streams()
    if "ctx" in _state:
        _state["ctx"].close()
    _state.clear()
    _twin.clear()


def twin(name, kind, W, H, n, k, wt=0):
    """The CPU twin's buffers of a case, (H, W, 8): computed once and handed out read-only."""
    key = (name, kind, W, H, n, k, wt)
    if key not in _twin:
        h = B.Context(-1)
        try:
            RC.upload(h, RC.scene(name), B)
            h.set_option("watertight", wt)
            a = h.aov_rays_host(RC.table(name, kind, W, H, B.to_camera_data), W, H, RC.params(B, n, k, RC.ROUGHNESS_MAX))
        finally:
            h.close()
        a.setflags(write=False)
        _twin[key] = a
    return _twin[key]


def device_table(rays, W, H):
    buf = AS.DeviceFrame(W, H, floats=16)  # 64 bytes per pixel; hipMalloc aligns far beyond 16
    AS.to_device(buf.rgb, rays)
    return buf


def check_stats(st, W, H):
    """As after pt_render_aov: one launch, the guide kernel's geometry, kernel_ms."""
    blocks = ((W + 7) // 8) * ((H + 7) // 8)
    assert st["launches"] == 1 and st["kernel_ms"] > 0 and st["block"] == 64 and 0 < st["vgprs"] <= 128, st
    assert st["lds_bytes"] == RC.lds_bytes_of_the_guide_kernels() and 1 <= st["grid"] <= blocks and st["stack_entries"] > 0, st
    assert st["prepass_spp"] == 0 and st["express_pixels"] == 0 and st["whole_pixels"] == 0, st


@pytest.mark.parametrize("name,kind,W,H,n,k", RC.CASES, ids=lambda v: str(v))
def test_gpu_equals_the_twin(name, kind, W, H, n, k):
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, n, k, RC.ROUGHNESS_MAX)
    table, out = device_table(rays, W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        for wt in (0, 1):
            what = "%s %s %dx%d n=%d max_follow=%d wt=%d" % (name, kind, W, H, n, k, wt)
            want = twin(name, kind, W, H, n, k, wt)
            ctx.set_option("watertight", wt)
            try:
                got = ctx.render_aov_rays(rays, W, H, prm)
                check_stats(ctx.stats(), W, H)
                ctx.render_aov_rays_device(table.rgb, W, H, out.rgb, prm)
                ctx.synchronize()
                check_stats(ctx.stats(), W, H)
            finally:
                ctx.set_option("watertight", 0)
            RC.assert_same(got, want, what + ": blocking form vs twin")
            RC.assert_same(out.read()[0], want, what + ": device form vs twin")
    finally:
        ctx.synchronize()
        table.free()
        out.free()


@pytest.mark.parametrize("name,kind,W,H,n,k", RC.JITTER_CASES, ids=lambda v: str(v))
def test_gpu_equals_the_twin_and_the_restatement_on_jittered_tables(orc, name, kind, W, H, n, k):
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, n, k, RC.ROUGHNESS_MAX)
    RC.precondition(orc, name, kind, W, H, n, k)  # asserted: the case can tell records apart
    table, out = device_table(rays, W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        for wt in (0, 1):
            what = "%s %s %dx%d n=%d max_follow=%d wt=%d" % (name, kind, W, H, n, k, wt)
            want = twin(name, kind, W, H, n, k, wt)
            ctx.set_option("watertight", wt)
            try:
                got = ctx.render_aov_rays(rays, W, H, prm)
                check_stats(ctx.stats(), W, H)
                ctx.render_aov_rays_device(table.rgb, W, H, out.rgb, prm)
                ctx.synchronize()
                check_stats(ctx.stats(), W, H)
            finally:
                ctx.set_option("watertight", 0)
            dev = out.read()[0]
            RC.assert_same(got, want, what + ": blocking form vs twin")
            RC.assert_same(dev, want, what + ": device form vs twin")
            RC.assert_same(got, RC.reference(orc, name, kind, W, H, n, k, wt), what + ": blocking form vs aov_rays_ref")
    finally:
        ctx.synchronize()
        table.free()
        out.free()


def test_both_slab_forms_on_a_scrambled_table():
    name, kind, W, H, n, k = "mirror_wall", "scrambled", 20, 13, 3, 4
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, n, k, RC.ROUGHNESS_MAX)
    table, out = device_table(rays, W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        for be in (0, 1):
            for wt in (0, 1):
                ctx.set_option("box_exact", be)
                ctx.set_option("watertight", wt)
                RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), twin(name, kind, W, H, n, k, wt), "box_exact = %d, watertight = %d, blocking" % (be, wt))
                ctx.render_aov_rays_device(table.rgb, W, H, out.rgb, prm)
                ctx.synchronize()
                RC.assert_same(out.read()[0], twin(name, kind, W, H, n, k, wt), "box_exact = %d, watertight = %d, device" % (be, wt))
    finally:
        for key, v in (("watertight", 0), ("box_exact", -1)):
            ctx.set_option(key, v)
        table.free()
        out.free()


@pytest.mark.parametrize("name", ["cornell", "mirror_wall", "tir"])
def test_consequence_c_on_a_scrambled_table(name):
    """Where coverage at n_samples = 1 says hit, the first-hit depth is pt_trace_closest's t on the ray aov_rays_ref.table_rays gives
    sample 0 of the pixel - the ray query knows nothing of tables, so a pixel that read another record or the other draw shows here
    without any twin."""
    W, H = 20, 13
    ctx = gpu(name)
    t = RC.table(name, "scrambled", W, H, B.to_camera_data)
    rays0 = aov_rays_ref.table_rays(t, W, H, 1, np.arange(W * H))[:, 0]
    got = RI.to_list(ctx.render_aov_rays(t, W, H, B.aov_default_params(n_samples=1, max_follow=0)), W, H)
    hits = ctx.trace_closest(rays0)
    covered = got[:, 3] == 1
    assert covered.sum() > W * H // 4 and ((got[:, 3] == 0) | covered).all()
    assert (covered == (hits["prim"] >= 0)).all()
    assert (got[covered, 7].view(U32) == hits["t"][covered].view(U32)).all()
    assert (got[~covered, 7] == 0).all()


def test_device_form_right_behind_a_render_rays_device():
    name, kind, W, H, n, k = "mirror_wall", "centres", 64, 48, 3, 4
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    want_rgb = ctx.render_rays(rays, W, H, 8, 6, want_rgba8=True)
    table, frame, guides = device_table(rays, W, H), AS.DeviceFrame(W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        s0 = AS.stream(0)
        ctx.render_rays_device(table.rgb, W, H, 8, 6, frame.rgb, frame.rgba8, stream=s0)
        ctx.render_aov_rays_device(table.rgb, W, H, guides.rgb, RC.params(B, n, k, RC.ROUGHNESS_MAX), stream=s0)  # no synchronize between the two
        ctx.synchronize()
        check_stats(ctx.stats(), W, H)
        rgb, rgba = frame.read()
        assert (rgb.view(U32) == want_rgb[0].view(U32)).all() and (rgba == want_rgb[1]).all(), "the ray image in front"
        RC.assert_same(guides.read()[0], twin(name, kind, W, H, n, k), "pt_render_aov_rays_device right behind a pt_render_rays_device")
        # and the other way round, on another stream than the call in front
        ctx.render_aov_rays_device(table.rgb, W, H, guides.rgb, RC.params(B, 1, 0, RC.ROUGHNESS_MAX), stream=AS.stream(1))
        ctx.render_rays_device(table.rgb, W, H, 8, 6, frame.rgb, frame.rgba8, stream=s0)
        ctx.synchronize()
        RC.assert_same(guides.read()[0], twin(name, kind, W, H, 1, 0), "the guides in front of a pt_render_rays_device")
        assert (frame.read()[0].view(U32) == want_rgb[0].view(U32)).all()
    finally:
        ctx.synchronize()
        for b in (table, frame, guides):
            b.free()


def test_both_slab_forms():
    name, kind, n, k = "mirror_wall", "probes", 3, 4
    W, H = RC.PROBE_SIZE
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, n, k, RC.ROUGHNESS_MAX)
    table, out = device_table(rays, W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        for be in (0, 1):
            for wt in (0, 1):
                ctx.set_option("box_exact", be)
                ctx.set_option("watertight", wt)
                RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), twin(name, kind, W, H, n, k, wt), "box_exact = %d, watertight = %d, blocking" % (be, wt))
                ctx.render_aov_rays_device(table.rgb, W, H, out.rgb, prm)
                ctx.synchronize()
                RC.assert_same(out.read()[0], twin(name, kind, W, H, n, k, wt), "box_exact = %d, watertight = %d, device" % (be, wt))
    finally:
        for key, v in (("watertight", 0), ("box_exact", -1)):
            ctx.set_option(key, v)
        table.free()
        out.free()


def test_shard_of_world_3():
    name, kind, W, H, n, k = "mirror_wall", "centres", 20, 13, 3, 4
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, n, k, RC.ROUGHNESS_MAX)
    want = twin(name, kind, W, H, n, k)
    covered = np.zeros((H, W), bool)
    partial_column = False
    try:
        for rank in (0, 1, 2):
            ids = B.shard_pixels(W, H, 8, rank, 3)
            own = np.zeros(W * H, bool)
            own[ids] = True
            partial_column |= bool((np.asarray(ids) % W >= 16).any())  # the block column x = 16..19 of a 20-wide frame
            own = own.reshape(H, W)[::-1]  # launch order -> framebuffer order
            assert own.any() and not (own & covered).any()
            covered |= own
            ctx.set_pixel_shard(rank, 3, 8)
            got = ctx.render_aov_rays(rays, W, H, prm)
            RC.assert_same(got[own], want[own], "rank %d: its pixels" % rank)
            assert (RC.bits(got[~own]) == 0).all(), "rank %d: +0 outside the shard" % rank
    finally:
        ctx.set_pixel_shard(0, 1, 16)
    assert covered.all() and partial_column
    RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), want, "the unsharded frame afterwards")


def test_more_blocks_than_rows_and_one_pixel_images():
    name, W, H = "mirror_wall", 130, 3
    ctx = gpu(name)
    rays = RI.pinhole(RC.camera(RC.scene(name), W, H, B.to_camera_data), W, H)  # jittered
    prm = RC.params(B, 3, 4, RC.ROUGHNESS_MAX)
    h = B.Context(-1)
    try:
        RC.upload(h, RC.scene(name), B)
        RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), h.aov_rays_host(rays, W, H, prm), "130 x 3, pinhole table")
        check_stats(ctx.stats(), W, H)
        p16 = B.aov_default_params(n_samples=16)
        seen = set()
        for i, t in enumerate(RC.jitter_records(B.RAY_GEN_DTYPE)):
            t["org"] = (-0.3, 0.2, 2.5)  # in front of the wall, between the pane and the mirror
            got = ctx.render_aov_rays(t, 1, 1, p16)
            RC.assert_same(got, h.aov_rays_host(t, 1, 1, p16), "1 x 1 image %d" % i)
            seen.add(got.tobytes())
        assert len(seen) == 8
    finally:
        h.close()


def test_after_set_materials_set_environment_and_update_vertices():
    scene = RF.make_scene("cornell")
    materials = RF.cornell_materials()
    mats = np.array([m for _, m, _ in materials], F32)
    for m in mats[1:3]:  # two of the materials become mirrors: the frame holds followed pixels
        m[4], m[7] = 1.0, 0.0
    W, H = 20, 13
    cam = RF.cornell_camera(W, H, B.to_camera_data).as_array()
    rays = RC.fixed_table(np.tile(cam[0:3], (W * H, 1)), RR.pixel_centre_targets(cam, W, H))
    prm = RC.params(B, 3, 4, RC.ROUGHNESS_MAX)
    env = B.make_env(**RF.CORNELL_ENV)

    def fresh(meshes, m, e):
        h = B.Context(-1)
        try:
            RF.upload(h, scene, meshes, materials=list(m), env=e)
            return h.aov_rays_host(rays, W, H, prm)
        finally:
            h.close()

    ctx = B.Context(0)
    try:
        ctx.set_option("dynamic", 1)
        RF.upload(ctx, scene, materials=list(mats), env=env)
        first = ctx.render_aov_rays(rays, W, H, prm)
        RC.assert_same(first, fresh(None, mats, env), "the uploaded state")
        assert (RC.bits(first) != RC.bits(ctx.render_aov_rays(rays, W, H, RC.params(B, 3, 0, RC.ROUGHNESS_MAX)))).any(), "the frame must hold followed pixels"
        mats2 = mats.copy()
        mats2[:, 0:3] = mats[:, [1, 2, 0]] * F32(0.9)  # every base colour turned
        ctx.set_materials(mats2)
        second = ctx.render_aov_rays(rays, W, H, prm)
        RC.assert_same(second, fresh(None, mats2, env), "after pt_set_materials")
        assert (RC.bits(second) != RC.bits(first)).any()
        env2 = B.make_env(use_auto=True, intensity=1.5)
        ctx.set_environment(env2)
        third = ctx.render_aov_rays(rays, W, H, prm)
        RC.assert_same(third, fresh(None, mats2, env2), "after pt_set_environment")
        assert (RC.bits(third) != RC.bits(second)).any()
        mv = RF.moved(scene, 1)
        ctx.update_vertices(mv)
        fourth = ctx.render_aov_rays(rays, W, H, prm)
        RC.assert_same(fourth, fresh(mv, mats2, env2), "after pt_update_vertices")
        assert (RC.bits(fourth) != RC.bits(third)).any()
    finally:
        ctx.close()


def test_first_hit_identity_through_degenerate_cameras():
    """Consequence (a) on the device, against the follow kernel itself: 64 listed pixels, one pt_render_aov_follow per pixel."""
    name, kind, W, H = "mirror_wall", "centres", 20, 13
    ctx = gpu(name)
    orgs, targets = RC.rays_of(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, 3, 0, RC.ROUGHNESS_MAX)
    got = ctx.render_aov_rays(RC.fixed_table(orgs, targets), W, H, prm)
    ids = np.sort(np.random.default_rng(11).choice(W * H, 64, replace=False))
    for i in ids:
        x, y = int(i) % W, int(i) // W
        c12, _ = RR.degenerate_camera(orgs[i], targets[i])
        want = ctx.render_aov_follow(RC.camera_of(B, c12), W, H, prm)
        RC.assert_same(got[H - 1 - y, x], want[H - 1 - y, x], "pixel (%d, %d)" % (x, y))


def test_render_ray_image_and_accumulation_are_untouched():
    name, kind, W, H = "cornell", "centres", 20, 13
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = RC.params(B, 3, 4, RC.ROUGHNESS_MAX)
    want = twin(name, kind, W, H, 3, 4)
    W2, H2 = 37, 23
    cam = RC.camera(RC.scene(name), W2, H2, B.to_camera_data)
    same = lambda a, b: all((x.view(U32) == y.view(U32)).all() for x, y in zip(a, b))
    before = ctx.render(cam, W2, H2, 40, 5, want_rgba8=True)
    before_rays = ctx.render_rays(rays, W, H, 40, 5, want_rgba8=True)
    RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), want, "the guide pass between two renders")
    assert same(ctx.render(cam, W2, H2, 40, 5, want_rgba8=True), before), "pt_render after a pt_render_aov_rays"
    RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), want, "again")
    assert same(ctx.render_rays(rays, W, H, 40, 5, want_rgba8=True), before_rays), "pt_render_rays after a pt_render_aov_rays"
    P = lambda n: B.accum_default_params(n_samples=n, max_pixel_samples=0, noise_threshold=0.0)
    frames = {}
    for between in (False, True):
        ctx.accum_begin(cam, W2, H2, 5)
        try:
            ctx.accum_add(P(8))
            if between:
                RC.assert_same(ctx.render_aov_rays(rays, W, H, prm), want, "the guide pass between two adds")
            ctx.accum_add(P(32))
            frames[between] = ctx.accum_read()
        finally:
            ctx.accum_end()
    for key in ("rgb", "noise"):
        assert (frames[True][key].view(U32) == frames[False][key].view(U32)).all(), key
    for key in ("rgba8", "samples"):
        assert (frames[True][key] == frames[False][key]).all(), key
    assert (frames[True]["rgb"].view(U32) == before[0].view(U32)).all(), "8 + 32 samples: the 40-sample frame"


def test_chain_render_guides_denoise_on_one_stream():
    name, kind, W, H = "mirror_wall", "centres", 64, 48
    ctx = gpu(name)
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    prm = B.aov_default_params(n_samples=4)
    dn = B.denoise_default_params(flags=B.PT_DENOISE_DEMODULATE)
    rgb, _ = ctx.render_rays(rays, W, H, 8, 8)
    aov = ctx.render_aov_rays(rays, W, H, prm)
    h = B.Context(-1)
    try:
        want, want8 = h.denoise_host(rgb, aov, dn, want_rgba8=True)
    finally:
        h.close()
    table, frame, guides = device_table(rays, W, H), AS.DeviceFrame(W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        s = AS.stream(0)
        ctx.render_rays_device(table.rgb, W, H, 8, 8, frame.rgb, None, stream=s)
        ctx.render_aov_rays_device(table.rgb, W, H, guides.rgb, prm, stream=s)
        ctx.denoise_device(frame.rgb, guides.rgb, W, H, frame.rgb, dn, d_out_rgba8=frame.rgba8, stream=s)
        ctx.synchronize()
        got, got8 = frame.read()
        RC.assert_same(guides.read()[0], aov, "the guides of the chain")
    finally:
        ctx.synchronize()
        for b in (table, frame, guides):
            b.free()
    assert (got.view(U32) == want.view(U32)).all(), "%d floats differ" % int((got.view(U32) != want.view(U32)).sum())
    assert (got8 == want8).all()
    assert (got.view(U32) != rgb.view(U32)).any(), "the filter must change the frame"


def test_communicator_is_refused_by_name():
    name, kind, W, H = "cornell", "centres", 20, 13
    rays = RC.table(name, kind, W, H, B.to_camera_data)
    ctx = B.Context(0)
    try:
        RC.upload(ctx, RC.scene(name), B)
        ctx.comm_init_rank(B.comm_unique_id(), 0, 1)
        L = B.lib()
        aov = np.full((H, W, 8), 7.0, F32)
        rc = L.pt_render_aov_rays(ctx._h, rays.ctypes.data, W, H, None, aov.ctypes.data_as(C.POINTER(C.c_float)))
        assert rc == -1 and "pt_render_aov_rays: a context with a communicator renders no ray images yet" in L.pt_last_error(ctx._h).decode()
        rc = L.pt_render_aov_rays_device(ctx._h, 64, W, H, None, 64, None)
        assert rc == -1 and "pt_render_aov_rays_device: a context with a communicator" in L.pt_last_error(ctx._h).decode()
        assert (aov == 7.0).all()
        ctx.comm_destroy()
        RC.assert_same(ctx.render_aov_rays(rays, W, H, RC.params(B, 1, 4, RC.ROUGHNESS_MAX)), twin(name, kind, W, H, 1, 4), "after pt_comm_destroy")
    finally:
        ctx.close()
