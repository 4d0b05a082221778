"""The batch forms of the guide pass and the denoiser on the GPU (pt_render_aov_batch, pt_denoise_batch; kernels:
csrc/pt_kernel_aov_follow_batch.hip and csrc/pt_denoise_batch.hip).  Both calls are defined by the single-frame calls, and every
comparison here is bit for bit.

Guide batch
* Batch == loop == twin: the K = 3 frames of batch_guides_common.py (own camera and table each) at 37 x 23 and 24 x 16 (H no multiple of
  8), n = 1 and 3, max_follow 0 and 4: every frame equals pt_set_materials + pt_render_aov_follow on the GPU and the CPU twin;
  max_follow = 0 also equals pt_render_aov.  max_follow 4 differs from 0 in > 20 pixels of frame 0, and in the frame whose mirror is
  diffuse only where the first hit is the glass pane.
* Tiny frames 1 x 1, 7 x 9, 9 x 7, 8 x 8 with K = 5.
* Frames do not leak: another table or camera for frame 1 changes bits in frame 1 only.
* More blocks than waves: 64 x 64, K = 130 on an orbit - K * 64 blocks exceed the grid, so the block loop wraps across frames.
* Option "batch_frames" = 2 with K = 5: same bits, three launches.  "box_exact" 0 / 1 and "quad" = 0: same bits.  "watertight" = 1 is
  refused by name and the next call works.
* Pixel shard at world 3, tile 16: the ranks sum to the full batch, unowned pixels are +0, at 8 x 8 two ranks own nothing.
* Process per rank, world 2, over the counting stub collective: rank 0 == the one-GPU batch, one reduce per launch sequence per rank.
* pt_render_batch_device -> pt_render_aov_batch_device -> pt_denoise_batch_device on one caller stream with no synchronize in between
  equal the three blocking calls; pt_render before == after; pt_update_vertices + guide batch == a fresh upload's.

Denoise batch
* Frames of denoise_common.py stacked with a seed per frame: 37 x 23 K = 3 at L = 1, 5, 8 (taps reach 128 rows: many frames away),
  3 x 2 K = 4, 1 x 1 K = 3, 130 x 19 K = 2, bad guides in one frame only, one sigma at +infinity; flags 0 and 1.  Each frame equals
  pt_denoise of that frame and tests/denoise_ref.py, out_rgba8 included; in place on the host and on device buffers gives the same.
* Another rgb for one frame changes that frame's output only.  "batch_frames" = 2 with K = 5: same bits, 3 * (L + 2) launches."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import async_common as A
import batch_guides_child
import batch_guides_common as BG
import denoise_common as DC
import rccl_stub
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

ROOT = BG.FC.ROOT
F32 = np.float32
RM = 0.3
_ctx = {}
_single = {}


def gpu(name):
    """One uploaded context per scene for the whole module; every test leaves its options, shard and table at their defaults."""
    if name not in _ctx:
        c = B.Context(0)
        BG.upload(c, BG.scene(name), B)
        _ctx[name] = c
    return _ctx[name]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    A.destroy_streams()


def own_table(name):
    return np.stack(BG.scene(name)["mats"]).astype(F32)


def single(name, frame, W, H, n, k, first_hit=False):
    """pt_set_materials(frame's table) + pt_render_aov_follow(frame's camera) on the GPU (first_hit: + pt_render_aov): once per module."""
    key = (name, frame, W, H, n, k, first_hit)
    if key not in _single:
        ctx = gpu(name)
        j, variant = frame
        t = BG.table(name, variant)
        cam = BG.camera(name, j, W, H, B.to_camera_data)
        try:
            if t is not None:
                ctx.set_materials(t)
            a = ctx.render_aov(cam, W, H, n) if first_hit else ctx.render_aov_follow(cam, W, H, BG.params(B, n, k, RM))
        finally:
            if t is not None:
                ctx.set_materials(own_table(name))
        a.setflags(write=False)
        _single[key] = a
    return _single[key]


def _to_device(ptr, a):
    a = np.ascontiguousarray(a)
    assert A.hip().hipMemcpy(C.c_void_p(ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, A.H2D) == 0


# ---- guide batch ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", BG.SIZES)
@pytest.mark.parametrize("name", sorted(BG.FRAMES))
def test_batch_equals_loop_and_twin(name, W, H):
    ctx = gpu(name)
    frs = BG.frames(name, W, H, B)
    for n in (1, 3):
        for k in (0, 4):
            got = ctx.render_aov_batch(frs, W, H, BG.params(B, n, k, RM))
            st = ctx.stats()
            assert got.shape == (3, H, W, 8)
            assert st["launches"] == 1 and st["kernel_ms"] > 0 and st["block"] == 64 and 0 < st["vgprs"] <= 128, st
            for f, frame in enumerate(BG.FRAMES[name]):
                what = "%s %dx%d n=%d max_follow=%d frame %d %r" % (name, W, H, n, k, f, frame)
                BG.assert_same(got[f], single(name, frame, W, H, n, k), what + ": batch vs pt_set_materials + pt_render_aov_follow")
                BG.assert_same(got[f], BG.twin(B, name, frame, W, H, n, k, RM), what + ": batch vs the host twin")
                if k == 0:
                    BG.assert_same(got[f], single(name, frame, W, H, n, k, first_hit=True), what + ": max_follow = 0 vs pt_render_aov")


def test_follow_changes_what_it_should(orc):
    name, W, H, n = "mirror_wall", 37, 23, 1
    ctx = gpu(name)
    frs = BG.frames(name, W, H, B)
    b0 = ctx.render_aov_batch(frs, W, H, BG.params(B, n, 0, RM))
    b4 = ctx.render_aov_batch(frs, W, H, BG.params(B, n, 4, RM))
    changed = (BG.bits(b0) != BG.bits(b4)).any(-1)
    assert changed[0].sum() >= 20, "frame 0: the mirror and the pane are followed"
    f = [v for _, v in BG.FRAMES[name]].index("diffuse")
    _, log = BG.reference(orc, name, BG.FRAMES[name][f], W, H, n, 4, RM, want_log=True)
    e0 = log["log"][0]
    mi = np.asarray(BG.flat(name, "diffuse")["material_index"])[np.maximum(e0["prim"], 0)]
    glass_first = (e0["hit"] & (mi == BG.M_GLASS[name])).reshape(H, W)[::-1]
    assert glass_first.any()
    assert not (changed[f] & ~glass_first).any(), "the frame whose mirror is diffuse changes only where the pane is followed"


@pytest.mark.parametrize("W,H", [(1, 1), (7, 9), (9, 7), (8, 8)])
def test_tiny_frames(W, H):
    name, n, k = "mirror_wall", 3, 4
    which = BG.FRAMES[name] + [(1, "own"), (2, "diffuse")]
    got = gpu(name).render_aov_batch(BG.frames(name, W, H, B, which), W, H, BG.params(B, n, k, RM))
    assert got.shape == (5, H, W, 8)
    for f, frame in enumerate(which):
        BG.assert_same(got[f], BG.twin(B, name, frame, W, H, n, k, RM), "%dx%d frame %d: batch vs the host twin" % (W, H, f))
        BG.assert_same(got[f], single(name, frame, W, H, n, k), "%dx%d frame %d: batch vs the single-frame call" % (W, H, f))


def test_frames_do_not_leak():
    name, W, H = "mirror_wall", 37, 23
    ctx = gpu(name)
    prm = BG.params(B, 1, 4, RM)
    base = ctx.render_aov_batch(BG.frames(name, W, H, B), W, H, prm)
    for what, which in (("table", [(0, "own"), (1, "tinted"), (2, "tinted")]), ("camera", [(0, "own"), (2, "diffuse"), (2, "tinted")])):
        got = ctx.render_aov_batch(BG.frames(name, W, H, B, which), W, H, prm)
        BG.assert_same(got[0], base[0], "another %s for frame 1: frame 0" % what)
        BG.assert_same(got[2], base[2], "another %s for frame 1: frame 2" % what)
        assert (BG.bits(got[1]) != BG.bits(base[1])).any(), what


def test_more_blocks_than_waves():
    name, W, H, K = "ico_map", 64, 64, 130
    ctx = gpu(name)
    frm, at, up, fov = BG.scene(name)["camera"]
    r = math.hypot(frm[0] - at[0], frm[2] - at[2])
    cams = [B.to_camera_data((at[0] + r * math.sin(2 * math.pi * i / K), frm[1], at[2] + r * math.cos(2 * math.pi * i / K)), tuple(at), tuple(up), fov, W, H) for i in range(K)]
    prm = BG.params(B, 1, 4, RM)
    got = ctx.render_aov_batch([(c, None) for c in cams], W, H, prm, n_materials=len(BG.scene(name)["mats"]))
    st = ctx.stats()
    assert st["launches"] == 1 and K * 64 > st["grid"] > 0, st  # 64 blocks per frame: the block loop wraps, a wave serves several frames
    for i, c in enumerate(cams):
        BG.assert_same(got[i], ctx.render_aov_follow(c, W, H, prm), "frame %d of %d" % (i, K))
    assert (BG.bits(got[0]) != BG.bits(got[K // 2])).any()


def test_batch_frames_option():
    name, W, H = "mirror_wall", 37, 23
    ctx = gpu(name)
    which = BG.FRAMES[name] + [(1, "own"), (2, "diffuse")]
    frs = BG.frames(name, W, H, B, which)
    prm = BG.params(B, 3, 4, RM)
    want = ctx.render_aov_batch(frs, W, H, prm)
    assert ctx.stats()["launches"] == 1
    ctx.set_option("batch_frames", 2)
    try:
        assert B.plan_batch(W, H, 5, 2) == [2, 2, 1]
        got = ctx.render_aov_batch(frs, W, H, prm)
        st = ctx.stats()
    finally:
        ctx.set_option("batch_frames", 0)
    BG.assert_same(got, want, "batch_frames = 2 vs one launch sequence")
    assert st["launches"] == 3 and st["kernel_ms"] > 0, st


def test_other_render_options():
    name, W, H = "ico_map", 37, 23
    ctx = gpu(name)
    frs = BG.frames(name, W, H, B)
    prm = BG.params(B, 3, 4, RM)
    want = ctx.render_aov_batch(frs, W, H, prm)
    try:
        for be in (0, 1):
            ctx.set_option("box_exact", be)
            BG.assert_same(ctx.render_aov_batch(frs, W, H, prm), want, "box_exact = %d" % be)
        ctx.set_option("box_exact", -1)
        ctx.set_option("quad", 0)
        BG.assert_same(ctx.render_aov_batch(frs, W, H, prm), want, "quad = 0 (binary walk)")
        assert ctx.stats()["launches"] == 1 and 0 < ctx.stats()["vgprs"] <= 128
        ctx.set_option("quad", 1)
        ctx.set_option("watertight", 1)
        with pytest.raises(B.PtError, match=r"\(-1\)") as e:  # PT_E_INVALID, never frame by frame
            ctx.render_aov_batch(frs, W, H, prm)
        assert "watertight" in str(e.value) and "pt_render_aov_batch" in str(e.value)
        ctx.set_option("watertight", 0)
        BG.assert_same(ctx.render_aov_batch(frs, W, H, prm), want, "after the refusal")
    finally:
        for key, v in (("quad", 1), ("watertight", 0), ("box_exact", -1)):
            ctx.set_option(key, v)


def _owned_mask(W, H, tile, rank, world):
    ids = B.shard_pixels(W, H, tile, rank, world)
    m = np.zeros(W * H, bool)
    m[ids] = True
    return m.reshape(H, W)[::-1]  # framebuffer order


def test_pixel_shard():
    name, W, H = "mirror_wall", 40, 32
    ctx = gpu(name)
    prm = BG.params(B, 2, 4, RM)
    frs, frs8 = BG.frames(name, W, H, B), BG.frames(name, 8, 8, B)
    full, full8 = ctx.render_aov_batch(frs, W, H, prm), ctx.render_aov_batch(frs8, 8, 8, prm)
    total, total8 = np.zeros_like(full), np.zeros_like(full8)
    try:
        empty_ranks = 0
        for rank in range(3):
            ctx.set_pixel_shard(rank, 3, 16)
            part = ctx.render_aov_batch(frs, W, H, prm)
            own = _owned_mask(W, H, 16, rank, 3)
            assert own.any() and not own.all()
            for f in range(3):
                BG.assert_same(part[f][own], full[f][own], "rank %d of 3, frame %d: owned pixels" % (rank, f))
                assert (BG.bits(part[f][~own]) == 0).all(), "rank %d, frame %d: pixels of other ranks must be +0" % (rank, f)
            total = total + part
            part8 = ctx.render_aov_batch(frs8, 8, 8, prm)  # one tile per frame: two of the three ranks own nothing in any frame
            empty_ranks += int((BG.bits(part8) == 0).all())
            total8 = total8 + part8
        BG.assert_same(total, full, "sum of the three ranks")
        BG.assert_same(total8, full8, "8 x 8: sum of the three ranks")
        assert empty_ranks == 2
    finally:
        ctx.set_pixel_shard(0, 1, 16)


def test_process_per_rank_over_the_stub_collective(tmp_path):
    name, W, H, n, k, r = batch_guides_child.CASE
    ctx = gpu(name)
    want = ctx.render_aov_batch(BG.frames(name, W, H, B), W, H, BG.params(B, n, k, r))
    sequences = len(B.plan_batch(W, H, 3, batch_guides_child.BATCH_FRAMES))
    assert sequences == 2
    target = rccl_stub.stub_path()
    so = str(tmp_path / "libcount_rccl.so")
    subprocess.check_call([shutil.which("g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rccl_stub.ROCM, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "stub", "count_rccl.cpp"), "-ldl"])
    env = dict(os.environ, PT_RCCL_PATH=so, COUNT_RCCL_TARGET=target)
    world = 2
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "batch_guides_child.py"), "rank", str(tmp_path), str(rk), str(world)], env=env) for rk in range(world)]
    t0 = time.time()
    try:
        for p in procs:
            p.wait(timeout=max(1.0, 300 - (time.time() - t0)))
    finally:  # a rank that hangs in a collective must not outlive the test holding the GPU
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), [p.returncode for p in procs]
    BG.assert_same(np.load(tmp_path / "rank0.npy"), want, "rank 0 of 2 vs the one-GPU batch")
    for rk in range(world):
        seen = json.load(open(tmp_path / ("reduces_%d.json" % rk)))
        assert seen["reduces"] == sequences and seen["launches"] == sequences, "ONE reduce per launch sequence on rank %d: %r" % (rk, seen)


def test_asynchronous_chain_on_a_caller_stream():
    name, W, H, K, spp, depth = "mirror_wall", 40, 32, 3, 8, 6
    ctx = gpu(name)
    frs = BG.frames(name, W, H, B)
    prm = BG.params(B, 2, 4, RM)
    cam = BG.camera(name, 0, W, H, B.to_camera_data)
    before, _ = ctx.render(cam, W, H, spp, depth)
    rgb, _ = ctx.render_batch(frs, W, H, spp, depth)
    aov = ctx.render_aov_batch(frs, W, H, prm)
    want, want8 = ctx.denoise_batch(rgb, aov, None, want_rgba8=True)
    assert (DC.bits(want) != DC.bits(rgb)).any()
    s = A.stream(0, nonblocking=True)
    frame, guides, out = A.DeviceFrame(W, H, frames=K), A.DeviceFrame(W, H, frames=K, floats=8), A.DeviceFrame(W, H, frames=K)
    try:
        ctx.render_batch_device(frs, W, H, spp, depth, frame.rgb, stream=s)
        ctx.render_aov_batch_device(frs, W, H, guides.rgb, prm, stream=s)
        ctx.denoise_batch_device(frame.rgb, guides.rgb, K, W, H, out.rgb, None, d_out_rgba8=out.rgba8, stream=s)
        after, _ = ctx.render(cam, W, H, spp, depth)  # no synchronize in between: ordered after the chain by the library
        ctx.synchronize()
        got_rgb, _ = frame.read()
        got_aov, _ = guides.read()
        got, got8 = out.read()
    finally:
        for d in (frame, guides, out):
            d.free()
    DC.assert_same(got_rgb, rgb, "pt_render_batch_device on the caller stream")
    BG.assert_same(got_aov, aov, "pt_render_aov_batch_device behind it")
    DC.assert_same(got, want, "pt_denoise_batch_device behind both vs the three blocking calls")
    assert (got8 == want8).all()
    assert (BG.bits(before) == BG.bits(after)).all(), "pt_render after the chain must equal pt_render before it"


def test_update_vertices_then_guide_batch():
    scene = RC.make_scene("cornell")
    W, H = 32, 24
    cam = RC.cornell_camera(W, H, B.to_camera_data)
    env = B.make_env(color=(0.5, 0.25, 1.0), intensity=1.0)
    mats = [m.copy() for _, m, _ in RC.cornell_materials()]
    for m in mats[1:3]:  # two of the materials become mirrors: the moved scene is followed
        m[4], m[7] = 1.0, 0.0
    other = np.stack(mats).astype(F32).copy()
    other[1, 4] = 0.0
    frs = [(cam, None), (cam, other)]
    prm = BG.params(B, 2, 4, RM)
    dyn = B.Context(0)
    try:
        dyn.set_option("dynamic", 1)
        RC.upload(dyn, scene, materials=mats, env=env)
        before = dyn.render_aov_batch(frs, W, H, prm)
        assert (BG.bits(before[0]) != BG.bits(before[1])).any()
        meshes = RC.moved(scene, 1)
        dyn.update_vertices(meshes)
        got = dyn.render_aov_batch(frs, W, H, prm)
        fresh = B.Context(0)
        try:
            RC.upload(fresh, scene, meshes, materials=mats, env=env)
            BG.assert_same(got, fresh.render_aov_batch(frs, W, H, prm), "update vs fresh upload")
            BG.assert_same(got[0], fresh.render_aov_follow(cam, W, H, prm), "frame 0 vs the fresh upload's single frame")
        finally:
            fresh.close()
        assert (BG.bits(got) != BG.bits(before)).any()
    finally:
        dyn.close()


# ---- denoise batch -------------------------------------------------------------------------------------------------------------

DN_CASES = [("37x23_L%d_f%d" % (L, fl), 3, None) for L in (1, 5, 8) for fl in (0, 1)] + [("3x2_L3_f%d" % fl, 4, None) for fl in (0, 1)] + \
           [("1x1_L3_f%d" % fl, 3, None) for fl in (0, 1)] + [("130x19_L2_f%d" % fl, 2, None) for fl in (0, 1)] + \
           [("37x23_L5_f1_badguides", 3, 1), ("29x17_L3_f0_sigma_color_inf", 3, None), ("29x17_L3_f1_sigma_normal_inf", 3, None)]


@pytest.mark.parametrize("cid,K,bad_in", DN_CASES, ids=[c[0] for c in DN_CASES])
def test_denoise_batch_equals_loop_and_restatement(cid, K, bad_in):
    ctx = gpu("mirror_wall")  # (the filter needs no scene; any context will do)
    _, W, H, _, _, _ = DC.case(cid)
    rgb, aov = BG.denoise_stack(cid, K, bad_in)
    p = DC.params(B, cid)
    got, got8 = ctx.denoise_batch(rgb, aov, p, want_rgba8=True)
    st = ctx.stats()
    assert got.shape == (K, H, W, 3) and got8.shape == (K, H, W)
    assert st["launches"] == p.iterations + 2 and st["kernel_ms"] > 0 and st["block"] == 256 and st["vgprs"] > 0 and st["grid"] >= K, st
    for f in range(K):
        want, want8 = BG.denoise_reference(cid, f, bad_in)
        DC.assert_same(got[f], want, "%s frame %d: batch vs denoise_ref" % (cid, f))
        assert (got8[f] == want8).all(), (cid, f)
        one, one8 = ctx.denoise(rgb[f], aov[f], p, want_rgba8=True)
        DC.assert_same(got[f], one, "%s frame %d: batch vs pt_denoise" % (cid, f))
        assert (got8[f] == one8).all(), (cid, f)
    buf = np.array(rgb, F32)
    ctx.denoise_batch(buf, aov, p, in_place=True)
    DC.assert_same(buf, got, "%s: in place" % cid)
    frame, guides = A.DeviceFrame(W, H, frames=K), A.DeviceFrame(W, H, frames=K, floats=8)
    try:
        _to_device(frame.rgb, rgb)
        _to_device(guides.rgb, aov)
        ctx.denoise_batch_device(frame.rgb, guides.rgb, K, W, H, frame.rgb, p, d_out_rgba8=frame.rgba8)
        ctx.synchronize()
        dev, dev8 = frame.read()
    finally:
        frame.free()
        guides.free()
    DC.assert_same(dev, got, "%s: pt_denoise_batch_device in place" % cid)
    assert (dev8 == got8).all()


def test_denoise_frames_do_not_leak():
    cid, K = "37x23_L8_f1", 3  # taps at steps up to 128 rows: five frames away if frames were rows of one image
    ctx = gpu("mirror_wall")
    rgb, aov = BG.denoise_stack(cid, K)
    p = DC.params(B, cid)
    base, _ = ctx.denoise_batch(rgb, aov, p)
    other = np.array(rgb, F32)
    other[1] = BG.denoise_stack(cid, 5)[0][4]
    got, _ = ctx.denoise_batch(other, aov, p)
    DC.assert_same(got[0], base[0], "another rgb for frame 1: frame 0")
    DC.assert_same(got[2], base[2], "another rgb for frame 1: frame 2")
    assert (DC.bits(got[1]) != DC.bits(base[1])).any()


def test_denoise_batch_frames_option():
    cid, K = "37x23_L5_f1", 5
    ctx = gpu("mirror_wall")
    rgb, aov = BG.denoise_stack(cid, K)
    p = DC.params(B, cid)
    want, want8 = ctx.denoise_batch(rgb, aov, p, want_rgba8=True)
    assert ctx.stats()["launches"] == p.iterations + 2
    ctx.set_option("batch_frames", 2)
    try:
        got, got8 = ctx.denoise_batch(rgb, aov, p, want_rgba8=True)
        st = ctx.stats()
    finally:
        ctx.set_option("batch_frames", 0)
    DC.assert_same(got, want, "batch_frames = 2 vs one launch sequence")
    assert (got8 == want8).all()
    assert st["launches"] == 3 * (p.iterations + 2) and st["kernel_ms"] > 0 and st["vgprs"] > 0 and st["block"] == 256, st
