"""pt_render_batch on the GPU (run with -m gpu): K frames of one scene - own camera, own material table - in ONE launch sequence.
Every comparison is bit for bit (float frames as uint32, RGBA8 equal, PNG bytes equal): a frame of a batch must be what
pt_set_materials + pt_render gives for it alone on the same context, and the small ones must also be the CPU oracle's frame for that
camera and table.  There is no tolerance to choose: batch, loop and oracle run one arithmetic contract."""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import rccl_stub
from conftest import ASSETS, ROOT
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

PT_MAIN = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
MI = {"metallic": 4, "roughness": 7, "sheen": 9, "clearcoat": 11, "transmission": 14, "transmission_roughness": 15, "emission": 16}  # material_data, device_global.hpp:19-36


@pytest.fixture(scope="module")
def gpu():
    ctx = B.Context(0)
    yield ctx
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bitwise(a, b, what=""):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError("%s: %d of %d values differ; first at %s: %r != %r" % (what, len(bad), same.size, bad[0], a[tuple(bad[0])], b[tuple(bad[0])]))


_CAM_ARGS = {}


def mkcam(look_from, look_at, look_up, vfov, W, H):
    """The product's camera; the oracle builds ITS OWN from the same look-at parameters (_ocam)."""
    cam = B.to_camera_data(look_from, look_at, look_up, vfov, W, H)
    _CAM_ARGS[cam.as_array().tobytes()] = (tuple(look_from), tuple(look_at), tuple(look_up), float(vfov), int(W), int(H))
    return cam


def _ocam(orc, cam):
    return orc.to_camera_data(*_CAM_ARGS[cam.as_array().tobytes()])


def _base(sc):
    return np.stack([m for _, m, _ in sc["materials"]]).astype(np.float32)


def _loop(ctx, frames, W, H, spp, depth, base, want_rgba8=False):
    """The parent's way: pt_set_materials + pt_render per frame.  Returns (frames, rgba8 frames, [stats])."""
    out, out8, sts = [], [], []
    try:
        for cam, mats in frames:
            ctx.set_materials(mats)
            a, a8 = ctx.render(cam, W, H, spp, depth, want_rgba8=want_rgba8)
            out.append(a)
            out8.append(a8)
            sts.append(ctx.stats())
    finally:
        ctx.set_materials(base)
    return np.stack(out), (np.stack(out8) if want_rgba8 else None), sts


def _oracle_frames(orc, flat, frames, env, W, H, spp, depth, want_rgba8=False, textures=None):
    S = orc.Scene(flat)
    out, out8 = [], []
    for cam, mats in frames:
        S.set_materials(mats)
        a, a8, _ = S.render(_ocam(orc, cam), orc.make_env(**env), W, H, spp, depth, want_rgba8=want_rgba8)
        out.append(a)
        out8.append(a8)
    return np.stack(out), (np.stack(out8) if want_rgba8 else None)


def _cornell_frames(cornell, W, H):
    """Three cameras, three tables: an emitter changed (the light dimmer, the sphere glowing), all four lobes on the sphere and the
    box, and the scene's own table from a third viewpoint."""
    base = _base(cornell)
    c = cornell["camera"]
    a = base.copy()
    a[2, MI["emission"]] = 6.0
    a[1, MI["emission"]] = 1.5
    a[1, 0:3] = [0.9, 0.5, 0.2]
    b = base.copy()
    for who in (0, 1):
        b[who, MI["metallic"]] = 0.3
        b[who, MI["clearcoat"]] = 1.0
        b[who, MI["transmission"]] = 0.5
        b[who, MI["transmission_roughness"]] = 0.3
        b[who, MI["sheen"]] = 0.5
    cams = [mkcam(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H), mkcam([2.6, 1.6, 0.9], [0.0, 0.9, 0.0], [0, 1, 0], 55, W, H),
            mkcam([2.2, 0.6, -1.1], [0.0, 1.0, 0.1], [0, 1, 0], 62, W, H)]
    return [(cams[0], a), (cams[1], b), (cams[2], base.copy())], base


CORNELL_ENV = dict(color=(1, 1, 1), intensity=0.0)


def test_batch_of_three_cameras_and_tables(gpu, orc, cornell):
    """Cornell box at a ragged size, K = 3: every frame == its single render == the oracle's whole frame, RGBA8 too; the batch costs
    the launches of ONE single render (pre-pass + main launch), which a hidden loop over frames cannot produce; the context's own
    table is untouched by the batch."""
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**CORNELL_ENV))
    W, H, spp, depth = 61, 47, 64, 16
    frames, base = _cornell_frames(cornell, W, H)
    own_before, _ = gpu.render(frames[0][0], W, H, spp, depth)
    single_launches = gpu.stats()["launches"]
    assert single_launches == 2  # a sorted frame: cost pre-pass + main launch
    got, got8 = gpu.render_batch(frames, W, H, spp, depth, want_rgba8=True)
    st = gpu.stats()
    assert got.shape == (3, H, W, 3) and got8.shape == (3, H, W)
    assert st["launches"] == single_launches, "one launch sequence for the whole batch, not one per frame"
    assert st["kernel_ms"] > 0 and st["kernel_variant"] == 2 and st["vgprs"] <= 128
    own_after, _ = gpu.render(frames[0][0], W, H, spp, depth)  # NO set_materials in between: the context's table is still the scene's
    assert_bitwise(own_after, own_before, "the context's own table after a batch")
    loop, loop8, _ = _loop(gpu, frames, W, H, spp, depth, base, want_rgba8=True)
    want, want8 = _oracle_frames(orc, cornell["flat"], frames, CORNELL_ENV, W, H, spp, depth, want_rgba8=True)
    for f in range(3):
        assert_bitwise(got[f], loop[f], "frame %d: batch == single render" % f)
        assert_bitwise(got[f], want[f], "frame %d: batch == oracle" % f)
        np.testing.assert_array_equal(got8[f], loop8[f])
        np.testing.assert_array_equal(got8[f], want8[f])
    assert len({got[f].tobytes() for f in range(3)}) == 3, "the frames must differ, or nothing per-frame is under test"
    assert not np.array_equal(own_before, got[0])  # frame 0 has the scene's camera but another table
    # a frame that passes no table renders with the context's current one
    mixed, _ = gpu.render_batch([(frames[0][0], None), frames[1]], W, H, spp, depth, n_materials=base.shape[0])
    assert_bitwise(mixed[0], own_before, "materials = NULL: the context's table")
    assert_bitwise(mixed[1], got[1], "a table next to a NULL one")
    # the device-pointer entry point: same frames, asynchronous, left in HBM
    import ctypes as C

    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d, d8 = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d), got.nbytes) == 0 and hip.hipMalloc(C.byref(d8), got8.nbytes) == 0
    try:
        gpu.render_batch_device(frames, W, H, spp, depth, d.value, d8.value)
        gpu.synchronize()
        dev, dev8 = np.empty_like(got), np.empty_like(got8)
        assert hip.hipMemcpy(dev.ctypes.data_as(C.c_void_p), d, dev.nbytes, 2) == 0 and hip.hipMemcpy(dev8.ctypes.data_as(C.c_void_p), d8, dev8.nbytes, 2) == 0
    finally:
        hip.hipFree(d)
        hip.hipFree(d8)
    assert_bitwise(dev, got, "pt_render_batch_device")
    np.testing.assert_array_equal(dev8, got8)
    # the readers describe the launch sequence in ids of the virtual image W x (K * H)
    q, ids, cost = gpu.read_queue(3 * W * H)
    assert q.size == 3 * W * H and np.array_equal(np.sort(q), np.arange(3 * W * H, dtype=np.uint32)) and (cost > 0).all()


OPTION_SETS = [
    ("schedule 0", {"schedule": 0}, {"schedule": 1}, 1),
    ("ring schedule", {"whole": 0}, {"whole": -1}, 2),
    ("whole pixels forced", {"whole": 1}, {"whole": -1}, 2),
    ("no group walk", {"groups": 0}, {"groups": 1}, 2),
    ("group walk always", {"groups": 2}, {"groups": 1}, 2),
    ("fallback instance", {"fallback": 1}, {"fallback": 0}, 2),
    ("binary walk, counted", {"quad": 0, "count": 1}, {"quad": 1, "count": 0}, 2),
    ("spp_per_launch", {"spp_per_launch": 7}, {"spp_per_launch": 0}, 1),
]


@pytest.mark.parametrize("label,opts,reset,launches", OPTION_SETS, ids=[o[0].replace(" ", "_") for o in OPTION_SETS])
def test_batch_through_the_render_paths(gpu, orc, cornell, label, opts, reset, launches):
    """The batch of test_batch_of_three_cameras_and_tables through the render paths the parity suite names; each against the loop on
    the same context with the same options, and against the oracle."""
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**CORNELL_ENV))
    W, H, spp, depth = 61, 47, 40, 16
    frames, base = _cornell_frames(cornell, W, H)
    want, _ = _oracle_frames(orc, cornell["flat"], frames, CORNELL_ENV, W, H, spp, depth)
    try:
        for k, v in opts.items():
            gpu.set_option(k, v)
        got, _ = gpu.render_batch(frames, W, H, spp, depth)
        st = gpu.stats()
        loop, _, sts = _loop(gpu, frames, W, H, spp, depth, base)
    finally:
        for k, v in reset.items():
            gpu.set_option(k, v)
    assert st["launches"] == launches == sts[0]["launches"], (label, st["launches"])
    if "fallback" in opts:
        assert st["kernel_variant"] == 3 and 128 < st["vgprs"] <= 168
    if "whole" in opts:
        assert (st["whole_pixels"] != 0) == (opts["whole"] == 1)
    for f in range(3):
        assert_bitwise(got[f], loop[f], "%s, frame %d: batch == single render" % (label, f))
        assert_bitwise(got[f], want[f], "%s, frame %d: batch == oracle" % (label, f))
    if opts.get("count"):  # the work counters of a counted batch are the sums over its frames
        for k in ("samples", "rays", "scatters", "nan_retries", "env_misses"):
            assert st[k] == sum(s[k] for s in sts), (k, st[k], [s[k] for s in sts])
        assert st["samples"] == 3 * W * H * spp


def test_batch_below_the_prepass_and_counted(gpu, orc, cornell):
    """Below 32 spp there is no cost pre-pass: one launch for the batch.  Counted: the sums of the counted single renders."""
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**CORNELL_ENV))
    W, H, spp, depth = 61, 47, 9, 16
    frames, base = _cornell_frames(cornell, W, H)
    want, _ = _oracle_frames(orc, cornell["flat"], frames, CORNELL_ENV, W, H, spp, depth)
    for count in (0, 1):
        try:
            gpu.set_option("count", count)
            got, _ = gpu.render_batch(frames, W, H, spp, depth)
            st = gpu.stats()
            loop, _, sts = _loop(gpu, frames, W, H, spp, depth, base)
        finally:
            gpu.set_option("count", 0)
        assert st["launches"] == 1 and st["prepass_spp"] == 0
        for f in range(3):
            assert_bitwise(got[f], loop[f], "count=%d frame %d: batch == single render" % (count, f))
            assert_bitwise(got[f], want[f], "count=%d frame %d: batch == oracle" % (count, f))
        if count:
            for k in ("samples", "rays", "scatters", "nan_retries"):
                assert st[k] == sum(s[k] for s in sts), (k, st[k], [s[k] for s in sts])


def test_batch_with_texture_and_environment_map(gpu, orc, cube, scene_io, procedural):
    """A textured cube (the texture slot of a material row is the context's, the caller passes 17 floats) under an environment map
    (the long miss shader), three cameras, the cube's roughness / metallic swept."""
    tex = scene_io.checker_texture()
    envmap = procedural.rgbe_to_ldr_rgba8(procedural.synthetic_sky_rgbe(256, 128))
    env = dict(use_map=True, intensity=1.0, env_map=envmap)
    base = _base(cube)
    gpu.upload_scene(cube["entities"], base, textures=[tex], mesh_textures=[0], env=B.make_env(**env))
    W, H, spp, depth = 75, 50, 36, 6
    c = cube["camera"]
    frames = []
    for k, (frm, rough, metal) in enumerate(((c["look_from"], 0.1, 1.0), ([2.5, 1.5, -1.0], 0.6, 0.5), ([-1.5, 2.0, 2.5], 1.0, 0.0))):
        m = base.copy()
        m[:, MI["roughness"]] = rough
        m[:, MI["metallic"]] = metal
        frames.append((mkcam(frm, c["look_at"], c["look_up"], c["vertical_fov"], W, H), m))
    got, got8 = gpu.render_batch(frames, W, H, spp, depth, want_rgba8=True)
    assert gpu.stats()["launches"] == 2
    loop, loop8, _ = _loop(gpu, frames, W, H, spp, depth, base, want_rgba8=True)
    want, want8 = _oracle_frames(orc, cube["flat"], frames, env, W, H, spp, depth, want_rgba8=True)
    for f in range(3):
        assert_bitwise(got[f], loop[f], "textured cube, frame %d: batch == single render" % f)
        assert_bitwise(got[f], want[f], "textured cube, frame %d: batch == oracle" % f)
        np.testing.assert_array_equal(got8[f], want8[f])
    assert len({got[f].tobytes() for f in range(3)}) == 3


def test_batch_of_one_and_batch_frames_option(gpu, cornell):
    """K = 1 is pt_render.  K = 5 with batch_frames = 2: three launch sequences (2 + 2 + 1), the frames unchanged; the launches add up."""
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**CORNELL_ENV))
    W, H, spp, depth = 61, 47, 40, 16
    three, base = _cornell_frames(cornell, W, H)
    one, one8 = gpu.render_batch(three[:1], W, H, spp, depth, want_rgba8=True)
    assert gpu.stats()["launches"] == 2
    loop, loop8, _ = _loop(gpu, three[:1], W, H, spp, depth, base, want_rgba8=True)
    assert_bitwise(one[0], loop[0], "K = 1 == pt_render")
    np.testing.assert_array_equal(one8[0], loop8[0])
    five = three + [(three[0][0], three[1][1]), (three[2][0], three[0][1])]
    whole, _ = gpu.render_batch(five, W, H, spp, depth)
    assert gpu.stats()["launches"] == 2
    assert B.plan_batch(W, H, 5, 2) == [2, 2, 1]
    try:
        gpu.set_option("batch_frames", 2)
        cut, cut8 = gpu.render_batch(five, W, H, spp, depth, want_rgba8=True)
        st = gpu.stats()
    finally:
        gpu.set_option("batch_frames", 0)
    assert st["launches"] == 6, "three launch sequences of two launches each"
    assert_bitwise(cut, whole, "batch_frames changes no image")
    loop, loop8, _ = _loop(gpu, five, W, H, spp, depth, base, want_rgba8=True)
    assert_bitwise(cut, loop, "five frames in three launch sequences == single renders")
    np.testing.assert_array_equal(cut8, loop8)
    # the readers describe the LAST launch sequence (one frame): ids of a virtual image of one frame
    q, _, _ = gpu.read_queue(5 * W * H)
    assert q.size == W * H and q.max() == W * H - 1


def test_frames_do_not_leak_into_each_other(gpu, orc, cornell):
    """A frame whose table has non-finite base colours (the NaN-retry path: millions of retries, NaN pixels) between two ordinary
    frames leaves them bit-identical to their single renders and to the oracle."""
    env = dict(color=(1, 1, 1), intensity=0.5)
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**env))
    W = H = 64
    spp, depth = 32, 16
    frames, base = _cornell_frames(cornell, W, H)
    bad = base.copy()
    bad[0, 0:2] = np.nan
    bad[3, 0:2] = 3e38
    frames = [frames[0], (frames[1][0], bad), frames[2]]
    try:
        gpu.set_option("count", 1)
        got, _ = gpu.render_batch(frames, W, H, spp, depth)
        st = gpu.stats()
    finally:
        gpu.set_option("count", 0)
    assert st["nan_retries"] > 100_000, "the retry path was really taken"
    assert np.isnan(got[1]).any() and np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
    loop, _, _ = _loop(gpu, frames, W, H, spp, depth, base)
    want, _ = _oracle_frames(orc, cornell["flat"], frames, env, W, H, spp, depth)
    for f in range(3):
        assert_bitwise(got[f], loop[f], "frame %d next to a NaN frame: batch == single render" % f)
        assert_bitwise(got[f], want[f], "frame %d next to a NaN frame: batch == oracle" % f)


def test_one_far_camera_switches_the_whole_sequence(gpu, orc, cornell):
    """One camera beyond the 42-extent switch of the slab test: the whole launch sequence uses the subtracting form; boxes only have
    to be conservative, so every frame equals its single render (which uses the fma form for the near cameras)."""
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**CORNELL_ENV))
    W, H, spp, depth = 96, 72, 40, 16
    frames, base = _cornell_frames(cornell, W, H)
    far = mkcam([3000.0, 1.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0], 0.05, W, H)
    frames = [frames[0], (far, base.copy()), frames[2]]
    got, _ = gpu.render_batch(frames, W, H, spp, depth)
    loop, _, _ = _loop(gpu, frames, W, H, spp, depth, base)
    want, _ = _oracle_frames(orc, cornell["flat"], frames, CORNELL_ENV, W, H, spp, depth)
    assert got[1].max() > 0.0
    for f in range(3):
        assert_bitwise(got[f], loop[f], "frame %d with a far camera in the batch: batch == single render" % f)
        assert_bitwise(got[f], want[f], "frame %d with a far camera in the batch: batch == oracle" % f)


def test_batch_pixel_shards(gpu, cornell):
    """The pixel shard applies per frame.  World 3: the three ranks' batches are disjoint and sum to the full batch, each rank owning
    the same tiles in every frame.  World 8 at 64 x 64: rank 7 owns no tile, returns zeros and launches nothing."""
    gpu.upload_scene(cornell["entities"], _base(cornell), env=B.make_env(**CORNELL_ENV))
    W, H, spp, depth = 80, 56, 36, 16
    frames, base = _cornell_frames(cornell, W, H)
    full, full8 = gpu.render_batch(frames, W, H, spp, depth, want_rgba8=True)
    acc, acc8 = np.zeros_like(full), np.zeros_like(full8)
    try:
        for r in range(3):
            gpu.set_pixel_shard(r, 3, 16)
            part, part8 = gpu.render_batch(frames, W, H, spp, depth, want_rgba8=True)
            assert gpu.stats()["launches"] == 2
            own = np.zeros(W * H, bool)
            own[B.shard_pixels(W, H, 16, r, 3)] = True
            own = own.reshape(H, W)[::-1]  # framebuffer rows are flipped
            for f in range(3):
                assert not part[f][~own].any() and not part8[f][~own].any(), "rank %d wrote outside its tiles in frame %d" % (r, f)
                assert_bitwise(part[f][own], full[f][own], "rank %d, frame %d: its tiles of the full batch" % (r, f))
            acc += part
            acc8 += part8
        assert_bitwise(acc, full, "sum of the three ranks' batches == full batch")
        np.testing.assert_array_equal(acc8, full8)
        assert B.shard_pixels(64, 64, 16, 7, 8).size == 0
        small, _ = _cornell_frames(cornell, 64, 64)
        gpu.set_pixel_shard(7, 8, 16)
        for count in (0, 1):
            gpu.set_option("count", count)
            part, part8 = gpu.render_batch(small, 64, 64, 40, depth, want_rgba8=True)
            st = gpu.stats()
            assert not part.any() and not part8.any() and st["launches"] == 0
            assert not count or st["samples"] == 0
    finally:
        gpu.set_option("count", 0)
        gpu.set_pixel_shard(0, 1, 16)


def _counting_stub_env(tmp_path):
    """PT_RCCL_PATH = tests/stub/count_rccl.cpp (forwards to the stub collective and counts this process's ncclReduce calls)."""
    import shutil as sh

    target = rccl_stub.stub_path()  # skips when g++ or the RCCL header is missing
    so = str(tmp_path / "libcount_rccl.so")
    subprocess.check_call([sh.which("g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rccl_stub.ROCM, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "stub", "count_rccl.cpp"), "-ldl"])
    return dict(os.environ, PT_RCCL_PATH=so, COUNT_RCCL_TARGET=target)


def test_batch_reduce_with_stub_collective(tmp_path):
    """Two processes on one card behind the stub collective (tests/stub/fake_rccl.cpp; it is not RCCL), the pattern of
    tests/test_multi_rank_gpu.py: rank 0's batch == the single-GPU batch, RGBA8 packed on the root although only the root passes
    buffers, and ONE reduce per launch sequence and rank (counted by tests/stub/count_rccl.cpp in front of the stub)."""
    env = _counting_stub_env(tmp_path)
    child = os.path.join(ROOT, "tests", "batch_rank_child.py")
    world = 2
    procs = [subprocess.Popen([sys.executable, child, str(r), str(world), str(tmp_path)], env=env) for r in range(world)]
    t0 = time.time()
    try:
        for p in procs:
            p.wait(timeout=max(1.0, 600 - (time.time() - t0)))
    finally:  # a rank that hangs in a collective must not outlive the test holding the GPU
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), [p.returncode for p in procs]
    import batch_rank_child as child_mod
    from owl_path_tracer_amd.pyhost import scene_io

    sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
    ctx = B.Context(0)
    try:
        ctx.upload_scene(sc["entities"], [m for _, m, _ in sc["materials"]], env=B.make_env(**CORNELL_ENV))
        frames = child_mod.frames_of(sc)
        want, want8 = ctx.render_batch(frames, child_mod.W, child_mod.H, child_mod.SPP, child_mod.DEPTH, want_rgba8=True)
    finally:
        ctx.close()
    for tag in ("one", "cut"):  # one launch sequence; batch_frames = 2: two launch sequences
        np.testing.assert_array_equal(np.load(tmp_path / ("rgb_%s.npy" % tag)).view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(np.load(tmp_path / ("rgba8_%s.npy" % tag)), want8)
    for r in range(world):
        n = json.load(open(tmp_path / ("reduces_%d.json" % r)))
        assert n == {"one": 1, "cut": 2}, "rank %d: reduces per batch %r (one per launch sequence expected)" % (r, n)


def _subset_of_frame(orc, S, cam, env, W, H, spp, depth, n_pix, seed):
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(W * H, n_pix, replace=False)).astype(np.uint32)
    sub = np.zeros((H, W, 3), np.float32)
    S.render(_ocam(orc, cam), orc.make_env(**env), W, H, spp, depth, pixel_list=ids, out=sub)
    return (H - 1 - ids // W), ids % W, sub


def test_c2_batch_of_four_full_size(gpu, orc, cornell):
    """C2 at full size (512 x 512 x 256 spp, depth 16), K = 4: the sphere's metallic at four values.  Every frame == its single
    render; 300 random pixels per frame == the oracle at full spp.  Prints the kernel time of batch and loop (no claim is made here:
    profiles/r07_batch.json holds the measurements)."""
    base = _base(cornell)
    gpu.upload_scene(cornell["entities"], base, env=B.make_env(**CORNELL_ENV))
    W = H = 512
    spp, depth = 256, 16
    c = cornell["camera"]
    cam = mkcam(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
    frames = []
    for v in (0.0, 0.35, 0.7, 1.0):
        m = base.copy()
        m[1, MI["metallic"]] = v
        frames.append((cam, m))
    got, _ = gpu.render_batch(frames, W, H, spp, depth)
    st = gpu.stats()
    assert st["launches"] == 2
    loop, _, sts = _loop(gpu, frames, W, H, spp, depth, base)
    print("C2 x 4: batch kernel_ms=%.1f (%.1f per frame), loop kernel_ms=%s (sum %.1f)" % (st["kernel_ms"], st["kernel_ms"] / 4, ["%.1f" % s["kernel_ms"] for s in sts],
                                                                                          sum(s["kernel_ms"] for s in sts)))
    S = orc.Scene(cornell["flat"])
    for f, (_, m) in enumerate(frames):
        assert_bitwise(got[f], loop[f], "C2 frame %d: batch == single render" % f)
        S.set_materials(m)
        ys, xs, sub = _subset_of_frame(orc, S, cam, CORNELL_ENV, W, H, spp, depth, 300, 70 + f)
        assert_bitwise(got[f][ys, xs], sub[ys, xs], "C2 frame %d: pixel subset at full spp == oracle" % f)
    assert len({got[f].tobytes() for f in range(4)}) == 4


def _sweep_assets(tmp_path):
    """C2 as a three-frame material sweep (the sphere's metallic 0, 0.5, 1) at 200 x 120, 48 spp, as tests/test_host_main.py builds it."""
    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    s = json.load(open(os.path.join(ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[200, 120], max_samples=48)
    s["test"] = dict(name="sweep", material_name="sphere", attribute_name="metallic", material_type=2, values=[0.0, 1.0], step_size=0.5)
    (a / "settings.json").write_text(json.dumps(s))
    return a, ["cornell-box_sweep_metallic(%.1f).png" % v for v in (0.0, 0.5, 1.0)]


def _pt_main(args, env=None):
    return subprocess.run([PT_MAIN] + args, capture_output=True, text=True, timeout=600, env=env)


def test_pt_main_batch_flag(tmp_path):
    """`pt_main --batch 2` on a three-frame sweep (a batch of two and a remainder of one) and `--batch 3` (one batch) write PNGs byte
    for byte those of a run without the flag; `--batch 2 --gpus 2` and `--batch 0` exit 1 with a message."""
    a, names = _sweep_assets(tmp_path)
    ref_dir = tmp_path / "ref"
    os.makedirs(ref_dir)
    r = _pt_main(["--assets", str(a), "--out", str(ref_dir)])
    assert r.returncode == 0, r.stderr[-3000:]
    want = [open(ref_dir / n, "rb").read() for n in names]
    assert len(set(want)) == 3, "the frames of the sweep must differ"
    for k, batches in ((2, 2), (3, 1)):
        d = tmp_path / ("b%d" % k)
        os.makedirs(d)
        r = _pt_main(["--assets", str(a), "--out", str(d), "--batch", str(k)])
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stderr.count("TRACING (batch of") == batches and r.stderr.count("(2 launches)") == batches, r.stderr[-2000:]
        for n, w in zip(names, want):
            assert open(d / n, "rb").read() == w, "--batch %d: %s differs from the run without the flag" % (k, n)
    for flags, word in ((["--batch", "2", "--gpus", "2"], "--gpus"), (["--batch", "2", "--devices", "0,0"], "--devices"), (["--batch", "0"], "positive"), (["--batch"], "missing value")):
        r = _pt_main(["--assets", str(a), "--out", str(tmp_path)] + flags)
        assert r.returncode == 1 and r.stderr.startswith("error: ") and "--batch" in r.stderr and word in r.stderr, (flags, r.stderr[-1000:])


def test_batch_in_the_spilling_build():
    """libmi355pt_spilltest.so squeezes the 128-VGPR instances - the batch ones too - until they spill: a batch must render through the
    batch instance with the larger register budget (kernel_variant 3) and equal the single renders of the same build and the oracle.
    Runs in a child process because the library path is fixed at import."""
    lib = os.path.join(ROOT, "owl-path-tracer_amd", "libmi355pt_spilltest.so")
    assert os.path.exists(lib), "libmi355pt_spilltest.so not built (make -C owl-path-tracer_amd/csrc spilltest; build() makes it)"
    code = r"""
import os, sys, numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "oracle"))
import ptamd; ptamd.load()
from owl_path_tracer_amd.pyhost import binding as B, scene_io
import oracle as orc
assert B.LIB_PATH.endswith("libmi355pt_spilltest.so"), B.LIB_PATH
sc = scene_io.load_scene_dir(os.path.join(%(root)r, "assets"), "cornell-box")
base = np.stack([m for _, m, _ in sc["materials"]]).astype(np.float32)
ctx = B.Context(0)
ctx.upload_scene(sc["entities"], base, env=B.make_env(color=(1, 1, 1), intensity=0.0))
W, H, spp, depth = 61, 47, 40, 16
c = sc["camera"]
views = [(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"]), ([2.6, 1.6, 0.9], [0.0, 0.9, 0.0], [0, 1, 0], 55)]
tables = [base.copy(), base.copy()]
tables[0][1, 4] = 0.25
tables[1][1, 7] = 0.8
frames = [(B.to_camera_data(*v, W, H), t) for v, t in zip(views, tables)]
got, _ = ctx.render_batch(frames, W, H, spp, depth)
st = ctx.stats()
assert st["kernel_variant"] == 3 and 128 < st["vgprs"] <= 168 and st["launches"] == 2, (st["kernel_variant"], st["vgprs"], st["launches"])
S = orc.Scene(scene_io.flatten_scene(sc["entities"], sc["materials"]))
for f, ((cam, t), v) in enumerate(zip(frames, views)):
    ctx.set_materials(t)
    single, _ = ctx.render(cam, W, H, spp, depth)
    assert ctx.stats()["kernel_variant"] == 3
    assert (got[f].view(np.uint32) == single.view(np.uint32)).all(), f
    S.set_materials(t)
    want, _, _ = S.render(orc.to_camera_data(*v, W, H), orc.make_env(color=(1, 1, 1), intensity=0.0), W, H, spp, depth)
    assert (got[f].view(np.uint32) == want.view(np.uint32)).all(), f
print("BATCH_FALLBACK_OK", st["vgprs"])
""" % dict(root=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PT_LIB_PATH=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "BATCH_FALLBACK_OK" in r.stdout, r.stdout + r.stderr
