"""The guide pass on the GPU (pt_render_aov; kernel: csrc/pt_aov_first.h).  Every comparison is bit for bit on all 8 channels
of every pixel.

* GPU == tests/aov_ref.py (numpy, from the oracle's building blocks) == the CPU twin pt_debug_aov_host on the cases of aov_common.py
  (textured cube 37 x 23 at n = 1 and 5, Cornell with its emitter 32 x 24 at n = 3, the smooth icospheres under the three miss modes
  24 x 16), each with watertight 0 and 1; frames of 1 x 1 and 9 x 1.
* "box_exact" 0 and 1 and "quad" = 0 give the same buffers; "quad" = 0 with "watertight" = 1 is refused.
* Shard: rank 1 of 3, tile 16, 40 x 40 - owned pixels equal the full frame, the rest is 0, the three ranks sum to the full frame; a rank
  without a tile gives zeros.
* Cross-check through code that involves no restatement: at n = 1, pt_render(spp 1, max_depth 1) equals the albedo where the pixel
  missed or hit an emitter and is 0 elsewhere (Cornell, a camera with >= 10 % misses and >= 5 % light, asserted from the oracle).
* After pt_update_vertices the buffers equal those of a fresh upload; pt_set_materials changes the albedo only.
* pt_render_aov_device leaves the same floats in HBM.
* Two contexts on one card over the stub collective: pt_group_render_aov and the process-per-rank path with world 2 (ONE reduce per
  rank) equal the single-context buffers.
* `pt_main --aov 2`: the albedo PNG decodes to make_rgba of the API's albedo.
* pt_render after pt_render_aov is bit for bit the frame before it; pt_stats describes the guide launch in between."""
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import aov_child
import aov_common as AC
import aov_ref
import rccl_stub
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B, scene_io

pytestmark = pytest.mark.gpu

ROOT = AC.ROOT
ASSETS = AC.ASSETS
PT_MAIN = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
F32 = np.float32
_ctx = {}


def gpu(name):
    """One uploaded context per scene for the whole module; every test leaves its options at their defaults."""
    if name not in _ctx:
        c = B.Context(0)
        AC.upload(c, AC.scene(name), B)
        _ctx[name] = c
    return _ctx[name]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def host_twin(name, W, H, n, wt=0):
    h = B.Context(-1)
    try:
        AC.upload(h, AC.scene(name), B)
        h.set_option("watertight", wt)
        return h.aov_host(AC.camera(AC.scene(name), W, H, B.to_camera_data), W, H, n)
    finally:
        h.close()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("name,W,H,n", AC.CASES)
def test_gpu_equals_restatement_and_twin(orc, name, W, H, n, wt):
    ctx = gpu(name)
    want = AC.reference(orc, name, W, H, n, wt)
    ctx.set_option("watertight", wt)
    try:
        got = ctx.render_aov(AC.camera(AC.scene(name), W, H, B.to_camera_data), W, H, n)
        st = ctx.stats()
    finally:
        ctx.set_option("watertight", 0)
    AC.assert_same(got, want, "%s %dx%d n=%d wt=%d: GPU vs aov_ref" % (name, W, H, n, wt))
    AC.assert_same(host_twin(name, W, H, n, wt), want, "host twin vs aov_ref")
    assert st["launches"] == 1 and st["kernel_ms"] > 0 and st["block"] == 64 and 0 < st["vgprs"] <= 128, st


@pytest.mark.parametrize("W,H", [(1, 1), (9, 1), (1, 9)])
def test_tiny_frames(orc, W, H):
    sc = AC.scene("cube")
    for wt in (0, 1):
        want = AC.reference(orc, "cube", W, H, 3, wt)
        ctx = gpu("cube")
        ctx.set_option("watertight", wt)
        try:
            got = ctx.render_aov(AC.camera(sc, W, H, B.to_camera_data), W, H, 3)
        finally:
            ctx.set_option("watertight", 0)
        AC.assert_same(got, want, "cube %dx%d wt=%d" % (W, H, wt))
        AC.assert_same(host_twin("cube", W, H, 3, wt), want, "twin")


def test_slab_forms_and_binary_walk(orc):
    name, W, H, n = "cornell", 32, 24, 3
    ctx = gpu(name)
    cam = AC.camera(AC.scene(name), W, H, B.to_camera_data)
    want = AC.reference(orc, name, W, H, n, 0)
    want_wt = AC.reference(orc, name, W, H, n, 1)
    try:
        for be in (0, 1):
            ctx.set_option("box_exact", be)
            AC.assert_same(ctx.render_aov(cam, W, H, n), want, "box_exact = %d" % be)
            ctx.set_option("watertight", 1)
            AC.assert_same(ctx.render_aov(cam, W, H, n), want_wt, "box_exact = %d, watertight" % be)
            ctx.set_option("watertight", 0)
        ctx.set_option("box_exact", -1)
        ctx.set_option("quad", 0)
        AC.assert_same(ctx.render_aov(cam, W, H, n), want, "quad = 0 (binary walk)")
        ctx.set_option("watertight", 1)
        with pytest.raises(B.PtError, match=r"\(-1\)") as e:  # PT_E_INVALID, never the other triangle test
            ctx.render_aov(cam, W, H, n)
        assert "watertight" in str(e.value) and "quad" in str(e.value)
        ctx.set_option("quad", 1)
        AC.assert_same(ctx.render_aov(cam, W, H, n), want_wt, "after the refusal")
    finally:
        for k, v in (("quad", 1), ("watertight", 0), ("box_exact", -1)):
            ctx.set_option(k, v)


def _owned_mask(W, H, tile, rank, world):
    ids = B.shard_pixels(W, H, tile, rank, world)
    m = np.zeros(W * H, bool)
    m[ids] = True
    return m.reshape(H, W)[::-1]  # framebuffer order


def test_pixel_shard(orc):
    name, W, H, n = "cornell", 40, 40, 2
    ctx = gpu(name)
    cam = AC.camera(AC.scene(name), W, H, B.to_camera_data)
    full = ctx.render_aov(cam, W, H, n)
    AC.assert_same(full, AC.reference(orc, name, W, H, n, 0), "full frame")
    total = np.zeros_like(full)
    try:
        for rank in range(3):
            ctx.set_pixel_shard(rank, 3, 16)
            part = ctx.render_aov(cam, W, H, n)
            own = _owned_mask(W, H, 16, rank, 3)
            assert own.any() and not own.all()
            AC.assert_same(part[own], full[own], "rank %d of 3: owned pixels" % rank)
            assert (AC.bits(part[~own]) == 0).all(), "rank %d: pixels of other ranks must be +0" % rank
            total = total + part
        AC.assert_same(total, full, "sum of the three ranks")
        ctx.set_pixel_shard(1, 2, 16)  # a 16 x 16 frame is one tile: rank 1 of 2 owns nothing
        empty = ctx.render_aov(AC.camera(AC.scene(name), 16, 16, B.to_camera_data), 16, 16, n)
        assert (AC.bits(empty) == 0).all()
    finally:
        ctx.set_pixel_shard(0, 1, 16)


def test_cross_check_against_the_render_kernel(orc):
    """No restatement involved: a path of depth 1 returns the emission at an emitter, the environment on a miss and nothing elsewhere."""
    name = "cornell_cross"
    W, H = AC.CROSS_SIZE
    sc = AC.scene(name)
    ctx = gpu(name)
    cam = AC.camera(sc, W, H, B.to_camera_data)
    emission = np.asarray(sc["flat"]["materials"])[:, 16]
    for wt in (0, 1):
        # which pixels miss and which see the light: from the oracle, with the shares the test needs to mean something
        S = orc.Scene(sc["flat"], watertight=bool(wt))
        r = aov_ref.samples(S, sc["flat"], sc["env"], AC.camera(sc, W, H, orc.to_camera_data).as_array(), W, H, 1, np.arange(W * H))
        hit, prim = r["hit"][:, 0], r["prim"][:, 0]
        emit = hit & (emission[np.asarray(sc["flat"]["material_index"])[np.maximum(prim, 0)]] > 0)
        assert (~hit).mean() >= 0.10 and emit.mean() >= 0.05, ((~hit).mean(), emit.mean())
        miss_fb, emit_fb = (~hit).reshape(H, W)[::-1], emit.reshape(H, W)[::-1]
        ctx.set_option("watertight", wt)
        try:
            aov = ctx.render_aov(cam, W, H, 1)
            rgb, _ = ctx.render(cam, W, H, 1, 1)
        finally:
            ctx.set_option("watertight", 0)
        assert ((aov[..., 3] == 0) == miss_fb).all()
        want = np.where((miss_fb | emit_fb)[..., None], aov[..., :3], F32(0.0))
        AC.assert_same(rgb, want, "pt_render(spp 1, depth 1) vs albedo, watertight = %d" % wt)
        assert (rgb[emit_fb] > 1).all() and (rgb[miss_fb] == rgb[miss_fb][0]).all() and (rgb[miss_fb][0] > 0).all()


def test_update_vertices():
    scene = RC.make_scene("cornell")
    W, H, n = 32, 24, 2
    cam = RC.cornell_camera(W, H, B.to_camera_data)
    env = B.make_env(color=(0.5, 0.25, 1.0), intensity=1.0)
    mats = [m for _, m, _ in RC.cornell_materials()]
    dyn = B.Context(0)
    try:
        dyn.set_option("dynamic", 1)
        RC.upload(dyn, scene, materials=mats, env=env)
        before = dyn.render_aov(cam, W, H, n)
        for k, with_normals in ((1, False), (2, True)):
            meshes = RC.moved(scene, k, with_normals=with_normals)
            dyn.update_vertices(meshes)
            got = dyn.render_aov(cam, W, H, n)
            fresh, twin = B.Context(0), B.Context(-1)
            try:
                RC.upload(fresh, scene, meshes, materials=mats, env=env)
                RC.upload(twin, scene, meshes, materials=mats, env=env)
                AC.assert_same(got, fresh.render_aov(cam, W, H, n), "update %d vs fresh upload" % k)
                AC.assert_same(got, twin.aov_host(cam, W, H, n), "update %d vs the twin of the fresh upload" % k)
            finally:
                fresh.close()
                twin.close()
            assert (AC.bits(got) != AC.bits(before)).any()
    finally:
        dyn.close()


def test_set_materials_changes_albedo_only():
    name, W, H, n = "cornell", 32, 24, 3
    sc = AC.scene(name)
    ctx = gpu(name)
    cam = AC.camera(sc, W, H, B.to_camera_data)
    a = ctx.render_aov(cam, W, H, n)
    mats = np.stack(sc["mats"]).astype(F32).copy()
    mats[:, 0:3] = mats[:, 0:3] * F32(0.5) + F32(0.125)
    try:
        ctx.set_materials(mats)
        b = ctx.render_aov(cam, W, H, n)
        twin = B.Context(-1)
        try:
            AC.upload(twin, sc, B)
            twin.set_materials(mats)
            AC.assert_same(b, twin.aov_host(cam, W, H, n), "after pt_set_materials: GPU vs twin")
        finally:
            twin.close()
    finally:
        ctx.set_materials(np.stack(sc["mats"]).astype(F32))
    AC.assert_same(b[..., 3:], a[..., 3:], "alpha, normal and depth")
    assert (AC.bits(b[..., :3]) != AC.bits(a[..., :3])).any()
    AC.assert_same(ctx.render_aov(cam, W, H, n), a, "table restored")


def test_render_aov_device():
    name, W, H, n = "ico_map", 24, 16, 2
    ctx = gpu(name)
    cam = AC.camera(AC.scene(name), W, H, B.to_camera_data)
    want = ctx.render_aov(cam, W, H, n)
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), want.nbytes) == 0
    try:
        assert hip.hipMemset(p, 0x55, want.nbytes) == 0
        ctx.render_aov_device(cam, W, H, n, p.value)
        ctx.synchronize()
        got = np.empty_like(want)
        assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), p, want.nbytes, 2) == 0
    finally:
        hip.hipFree(p)
    AC.assert_same(got, want, "pt_render_aov_device")
    assert ctx.stats()["launches"] == 1


def _expected_child_case():
    name, W, H, n = aov_child.CASE
    ctx = gpu(name)
    cam = AC.camera(AC.scene(name), W, H, B.to_camera_data)
    out = {}
    for wt in (0, 1):
        ctx.set_option("watertight", wt)
        try:
            out[wt] = ctx.render_aov(cam, W, H, n)
        finally:
            ctx.set_option("watertight", 0)
    rgb, _ = ctx.render(cam, W, H, 4, 4)
    return out, rgb


def test_group_over_the_stub_collective(tmp_path):
    want, rgb = _expected_child_case()
    rc, out, err = rccl_stub.run_child([sys.executable, os.path.join(ROOT, "tests", "aov_child.py"), "group", str(tmp_path), "0,0"], rccl_stub.stub_env(), 300)
    assert rc == 0, err[-3000:]
    info = json.load(open(tmp_path / "group.json"))
    assert info["size"] == 2
    for wt in (0, 1):
        AC.assert_same(np.load(tmp_path / ("group_wt%d.npy" % wt)), want[wt], "pt_group_render_aov, watertight = %d" % wt)
    AC.assert_same(np.load(tmp_path / "group_rgb.npy"), rgb, "pt_group_render after the guide pass")


def test_process_per_rank_over_the_stub_collective(tmp_path):
    want, _ = _expected_child_case()
    target = rccl_stub.stub_path()
    so = str(tmp_path / "libcount_rccl.so")
    subprocess.check_call([shutil.which("g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rccl_stub.ROCM, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "stub", "count_rccl.cpp"), "-ldl"])
    env = dict(os.environ, PT_RCCL_PATH=so, COUNT_RCCL_TARGET=target)
    world = 2
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "aov_child.py"), "rank", str(tmp_path), str(r), str(world)], env=env) for r in range(world)]
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
    AC.assert_same(np.load(tmp_path / "rank0.npy"), want[0], "rank 0 of 2")
    for r in range(world):
        assert json.load(open(tmp_path / ("reduces_%d.json" % r)))["reduces"] == 1, "ONE reduce per rank"


def test_pt_main_aov_flag(tmp_path):
    from PIL import Image

    W, H, n = 40, 24, 2
    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    s = json.load(open(os.path.join(ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[W, H], max_samples=4, max_path_depth=4, environment_color=[0.3, 0.6, 0.2], environment_intensity=0.75)
    sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
    sphere = [m for _, m, _ in sc["materials"]][1]
    s["test"] = dict(name="g", material_name="sphere", attribute_name="metallic", material_type=2, values=[float(sphere[4]), float(sphere[4])], step_size=1.0)
    (a / "settings.json").write_text(json.dumps(s))
    base = "cornell-box_g_metallic(%.1f)" % float(sphere[4])
    d = tmp_path / "out"
    os.makedirs(d)
    r = subprocess.run([PT_MAIN, "--assets", str(a), "--out", str(d), "--aov", str(n), "--watertight"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ctx = gpu("cornell")  # the same environment (aov_common: colour (0.3, 0.6, 0.2) x 0.75)
    ctx.set_option("watertight", 1)
    try:
        c = sc["camera"]
        g = ctx.render_aov(B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H), W, H, n)
    finally:
        ctx.set_option("watertight", 0)

    def rgba(x):
        q = np.clip(np.nan_to_num((x * F32(256.0)).astype(F32), nan=0.0), 0, 255).astype(np.int64).astype(np.uint32)  # make_rgba: min(255, max(0, int(f * 256)))
        return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(0xFF000000)

    png = lambda tag: np.asarray(Image.open(d / (base + tag))).view(np.uint32).reshape(H, W)
    assert os.path.exists(d / (base + ".png"))
    np.testing.assert_array_equal(png("_albedo.png"), rgba(g[..., :3]))
    np.testing.assert_array_equal(png("_normal.png"), rgba(F32(0.5) * g[..., 4:7] + F32(0.5)))
    far = g[..., 7].max()
    dep = (g[..., 7] / far).astype(F32)
    np.testing.assert_array_equal(png("_depth.png"), rgba(np.stack([dep] * 3, -1)))
    r = subprocess.run([PT_MAIN, "--assets", str(a), "--out", str(d), "--aov", "2", "--batch", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--aov" in r.stderr, r.stderr[-1000:]


def test_render_is_unchanged_by_the_guide_pass():
    name, W, H = "ico_map", 48, 32
    ctx = gpu(name)
    cam = AC.camera(AC.scene(name), W, H, B.to_camera_data)
    a, a8 = ctx.render(cam, W, H, 40, 8, want_rgba8=True)
    st_a = ctx.stats()
    g = ctx.render_aov(cam, W, H, 4)
    st_g = ctx.stats()
    b, b8 = ctx.render(cam, W, H, 40, 8, want_rgba8=True)
    st_b = ctx.stats()
    assert (AC.bits(a) == AC.bits(b)).all() and (a8 == b8).all()
    assert st_g["launches"] == 1 and st_g["kernel_ms"] > 0 and st_g["prepass_ms"] == 0
    for k in ("launches", "vgprs", "lds_bytes", "block", "grid", "stack_entries", "kernel_variant", "prepass_spp", "whole_pixels", "express_pixels"):
        assert st_a[k] == st_b[k], (k, st_a[k], st_b[k])
    assert np.isfinite(g).all()
