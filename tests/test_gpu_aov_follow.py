"""The follow mode of the guide pass on the GPU (pt_render_aov_follow; kernels: csrc/pt_kernel_aov_follow.hip =
csrc/pt_aov_follow.h).  Every comparison is bit for bit on all 8 channels of every pixel.

* GPU == tests/aov_follow_ref.py (numpy) == the CPU twin pt_debug_aov_follow_host over the cases of aov_follow_common.py (four scenes, two
  sizes, n = 1 and 3, max_follow 0 1 2 4, roughness_max 0.3 and 0.2), each with watertight 0 and 1; pt_get_stats: one launch, <= 128 VGPRs.
* Tiny frames 1 x 1, 7 x 9, 9 x 7, 8 x 8: the 8 x 8 block logic and lanes outside the frame.
* Both slab forms and the binary walk ("quad" = 0; with "watertight" = 1 refused by name).
* Pixel shard at world 3, including a rank with no tile at 8 x 8: the ranks sum bit for bit to the full buffers.
* Group and process-per-rank over the stub collective.
* max_follow = 0 equals pt_render_aov on the device.
* pt_render_aov_follow_device on a caller stream followed by pt_render with no synchronize in between; pt_render before == after.
* pt_set_materials turning the mirror diffuse changes exactly the pixels that were followed; pt_update_vertices == a fresh upload.
* `pt_main --aov 2 --follow 4` writes what the library returns."""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import aov_follow_child
import aov_follow_common as FC
import async_common as A
import rccl_stub
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B, scene_io

pytestmark = pytest.mark.gpu

ROOT = FC.ROOT
PT_MAIN = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
F32 = np.float32
_ctx = {}


def gpu(name):
    """One uploaded context per scene for the whole module; every test leaves its options at their defaults."""
    if name not in _ctx:
        c = B.Context(0)
        FC.upload(c, FC.scene(name), B)
        _ctx[name] = c
    return _ctx[name]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    A.destroy_streams()


def host_twin(name, W, H, prm, wt=0, mats=None):
    h = B.Context(-1)
    try:
        FC.upload(h, FC.scene(name), B)
        if mats is not None:
            h.set_materials(mats)
        h.set_option("watertight", wt)
        return h.aov_follow_host(FC.camera(FC.scene(name), W, H, B.to_camera_data), W, H, prm)
    finally:
        h.close()


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("name,W,H,n", FC.FRAMES)
def test_gpu_equals_restatement_and_twin(orc, name, W, H, n, wt):
    ctx = gpu(name)
    cam = FC.camera(FC.scene(name), W, H, B.to_camera_data)
    ctx.set_option("watertight", wt)
    try:
        for k, r in FC.MODES:
            want = FC.reference(orc, name, W, H, n, k, r, wt)
            prm = FC.params(B, n, k, r)
            got = ctx.render_aov_follow(cam, W, H, prm)
            st = ctx.stats()
            what = "%s %dx%d n=%d max_follow=%d roughness_max=%g wt=%d" % (name, W, H, n, k, r, wt)
            FC.assert_same(got, want, what + ": GPU vs aov_follow_ref")
            FC.assert_same(host_twin(name, W, H, prm, wt), want, what + ": host twin vs aov_follow_ref")
            assert st["launches"] == 1 and st["kernel_ms"] > 0 and st["block"] == 64 and 0 < st["vgprs"] <= 128, st
    finally:
        ctx.set_option("watertight", 0)


@pytest.mark.parametrize("W,H", [(1, 1), (7, 9), (9, 7), (8, 8)])
def test_tiny_frames(orc, W, H):
    name = "mirror_wall"
    for wt in (0, 1):
        want = FC.reference(orc, name, W, H, 3, 4, 0.3, wt)
        ctx = gpu(name)
        ctx.set_option("watertight", wt)
        try:
            got = ctx.render_aov_follow(FC.camera(FC.scene(name), W, H, B.to_camera_data), W, H, FC.params(B, 3, 4, 0.3))
        finally:
            ctx.set_option("watertight", 0)
        FC.assert_same(got, want, "%s %dx%d wt=%d" % (name, W, H, wt))


def test_slab_forms_and_binary_walk(orc):
    name, W, H, n, k, r = "ico_map", 37, 23, 3, 4, 0.3
    ctx = gpu(name)
    cam = FC.camera(FC.scene(name), W, H, B.to_camera_data)
    prm = FC.params(B, n, k, r)
    want = FC.reference(orc, name, W, H, n, k, r, 0)
    want_wt = FC.reference(orc, name, W, H, n, k, r, 1)
    try:
        for be in (0, 1):
            ctx.set_option("box_exact", be)
            FC.assert_same(ctx.render_aov_follow(cam, W, H, prm), want, "box_exact = %d" % be)
            ctx.set_option("watertight", 1)
            FC.assert_same(ctx.render_aov_follow(cam, W, H, prm), want_wt, "box_exact = %d, watertight" % be)
            ctx.set_option("watertight", 0)
        ctx.set_option("box_exact", -1)
        ctx.set_option("quad", 0)
        FC.assert_same(ctx.render_aov_follow(cam, W, H, prm), want, "quad = 0 (binary walk)")
        assert ctx.stats()["launches"] == 1 and ctx.stats()["vgprs"] <= 128
        ctx.set_option("watertight", 1)
        with pytest.raises(B.PtError, match=r"\(-1\)") as e:  # PT_E_INVALID, never the other triangle test
            ctx.render_aov_follow(cam, W, H, prm)
        assert "watertight" in str(e.value) and "quad" in str(e.value) and "pt_render_aov_follow" in str(e.value)
        ctx.set_option("quad", 1)
        FC.assert_same(ctx.render_aov_follow(cam, W, H, prm), want_wt, "after the refusal")
    finally:
        for key, v in (("quad", 1), ("watertight", 0), ("box_exact", -1)):
            ctx.set_option(key, v)


def test_argument_errors_on_the_device():
    name = "mirror_wall"
    ctx = gpu(name)
    cam = FC.camera(FC.scene(name), 8, 8, B.to_camera_data)
    for bad in (dict(max_follow=-1), dict(max_follow=9), dict(roughness_max=-0.1), dict(roughness_max=1.5), dict(roughness_max=float("nan")), dict(reserved=1),
                dict(n_samples=0)):
        with pytest.raises(B.PtError, match=r"\(-1\)"):
            ctx.render_aov_follow(cam, 8, 8, B.aov_default_params(**bad))
    fresh = B.Context(0)
    try:
        with pytest.raises(B.PtError, match=r"\(-4\)"):  # PT_E_NO_SCENE
            fresh.render_aov_follow(cam, 8, 8)
    finally:
        fresh.close()
    assert np.isfinite(ctx.render_aov_follow(cam, 8, 8)).all()  # NULL = the defaults


def _owned_mask(W, H, tile, rank, world):
    ids = B.shard_pixels(W, H, tile, rank, world)
    m = np.zeros(W * H, bool)
    m[ids] = True
    return m.reshape(H, W)[::-1]  # framebuffer order


def test_pixel_shard(orc):
    name, W, H, n, k, r = "mirror_wall", 40, 32, 2, 4, 0.3
    ctx = gpu(name)
    prm = FC.params(B, n, k, r)
    cam = FC.camera(FC.scene(name), W, H, B.to_camera_data)
    full = ctx.render_aov_follow(cam, W, H, prm)
    FC.assert_same(full, FC.reference(orc, name, W, H, n, k, r, 0), "full frame")
    cam8 = FC.camera(FC.scene(name), 8, 8, B.to_camera_data)
    full8 = ctx.render_aov_follow(cam8, 8, 8, prm)
    total, total8 = np.zeros_like(full), np.zeros_like(full8)
    try:
        empty_ranks = 0
        for rank in range(3):
            ctx.set_pixel_shard(rank, 3, 16)
            part = ctx.render_aov_follow(cam, W, H, prm)
            own = _owned_mask(W, H, 16, rank, 3)
            assert own.any() and not own.all()
            FC.assert_same(part[own], full[own], "rank %d of 3: owned pixels" % rank)
            assert (FC.bits(part[~own]) == 0).all(), "rank %d: pixels of other ranks must be +0" % rank
            total = total + part
            part8 = ctx.render_aov_follow(cam8, 8, 8, prm)  # one tile: two of the three ranks own nothing
            empty_ranks += int((FC.bits(part8) == 0).all())
            total8 = total8 + part8
        FC.assert_same(total, full, "sum of the three ranks")
        FC.assert_same(total8, full8, "8 x 8: sum of the three ranks")
        assert empty_ranks == 2
    finally:
        ctx.set_pixel_shard(0, 1, 16)


def test_max_follow_0_equals_render_aov():
    for name, W, H, n in (("mirror_wall", 37, 23, 3), ("ico_map", 24, 16, 1)):
        ctx = gpu(name)
        cam = FC.camera(FC.scene(name), W, H, B.to_camera_data)
        for wt in (0, 1):
            ctx.set_option("watertight", wt)
            try:
                FC.assert_same(ctx.render_aov_follow(cam, W, H, FC.params(B, n, 0, 0.3)), ctx.render_aov(cam, W, H, n), "%s wt=%d: max_follow = 0 vs pt_render_aov" % (name, wt))
            finally:
                ctx.set_option("watertight", 0)


def test_follow_device_on_a_caller_stream_then_render():
    name, W, H, n = "mirror_wall", 40, 32, 2
    ctx = gpu(name)
    cam = FC.camera(FC.scene(name), W, H, B.to_camera_data)
    prm = FC.params(B, n, 4, 0.3)
    before, _ = ctx.render(cam, W, H, 8, 6)
    want = ctx.render_aov_follow(cam, W, H, prm)
    f = A.DeviceFrame(W, H, floats=8)
    try:
        ctx.render_aov_follow_device(cam, W, H, f.rgb, prm, stream=A.stream(0))
        after, _ = ctx.render(cam, W, H, 8, 6)  # no synchronize in between: ordered after the pass by the library
        ctx.synchronize()
        got, _ = f.read()
    finally:
        f.free()
    FC.assert_same(got, want, "pt_render_aov_follow_device on a caller stream vs the blocking call")
    assert (FC.bits(before) == FC.bits(after)).all(), "pt_render after the pass must equal pt_render before it"


def test_set_materials_turning_the_mirror_diffuse(orc):
    name, W, H, n, k, r = "mirror_wall", 37, 23, 1, 4, 0.3
    sc = FC.scene(name)
    ctx = gpu(name)
    cam = FC.camera(sc, W, H, B.to_camera_data)
    prm = FC.params(B, n, k, r)
    a = ctx.render_aov_follow(cam, W, H, prm)
    _, log = FC.reference(orc, name, W, H, n, k, r, 0, want_log=True)
    e0 = log["log"][0]
    mi = np.asarray(sc["flat"]["material_index"])[np.maximum(e0["prim"], 0)]
    mirror_first = (e0["hit"] & (mi == FC.M_MIRROR)).reshape(H, W)[::-1]
    assert mirror_first.sum() > 20
    mats = np.stack(sc["mats"]).astype(F32).copy()
    mats[FC.M_MIRROR, 4] = 0.0  # metallic
    try:
        ctx.set_materials(mats)
        b = ctx.render_aov_follow(cam, W, H, prm)
        FC.assert_same(b, host_twin(name, W, H, prm, 0, mats), "after pt_set_materials: GPU vs twin")
    finally:
        ctx.set_materials(np.stack(sc["mats"]).astype(F32))
    changed = (FC.bits(a) != FC.bits(b)).any(-1)
    assert (changed == mirror_first).all(), "exactly the pixels whose first hit was the mirror change"
    FC.assert_same(ctx.render_aov_follow(cam, W, H, prm), a, "table restored")


def test_update_vertices():
    scene = RC.make_scene("cornell")
    W, H = 32, 24
    cam = RC.cornell_camera(W, H, B.to_camera_data)
    env = B.make_env(color=(0.5, 0.25, 1.0), intensity=1.0)
    mats = [m.copy() for _, m, _ in RC.cornell_materials()]
    for m in mats[1:3]:  # two of the materials become mirrors: the moved scene is followed
        m[4], m[7] = 1.0, 0.0
    prm = FC.params(B, 2, 4, 0.3)
    dyn = B.Context(0)
    try:
        dyn.set_option("dynamic", 1)
        RC.upload(dyn, scene, materials=mats, env=env)
        before = dyn.render_aov_follow(cam, W, H, prm)
        assert (FC.bits(before) != FC.bits(dyn.render_aov(cam, W, H, 2))).any(), "the frame must hold followed pixels"
        meshes = RC.moved(scene, 1)
        dyn.update_vertices(meshes)
        got = dyn.render_aov_follow(cam, W, H, prm)
        fresh, twin = B.Context(0), B.Context(-1)
        try:
            RC.upload(fresh, scene, meshes, materials=mats, env=env)
            RC.upload(twin, scene, meshes, materials=mats, env=env)
            FC.assert_same(got, fresh.render_aov_follow(cam, W, H, prm), "update vs fresh upload")
            FC.assert_same(got, twin.aov_follow_host(cam, W, H, prm), "update vs the twin of the fresh upload")
        finally:
            fresh.close()
            twin.close()
        assert (FC.bits(got) != FC.bits(before)).any()
    finally:
        dyn.close()


def _expected_child_case():
    name, W, H, n, k, r = aov_follow_child.CASE
    ctx = gpu(name)
    cam = FC.camera(FC.scene(name), W, H, B.to_camera_data)
    out = {}
    for wt in (0, 1):
        ctx.set_option("watertight", wt)
        try:
            out[wt] = ctx.render_aov_follow(cam, W, H, FC.params(B, n, k, r))
        finally:
            ctx.set_option("watertight", 0)
    return out


def test_group_over_the_stub_collective(tmp_path):
    want = _expected_child_case()
    rc, out, err = rccl_stub.run_child([sys.executable, os.path.join(ROOT, "tests", "aov_follow_child.py"), "group", str(tmp_path), "0,0"], rccl_stub.stub_env(), 300)
    assert rc == 0, err[-3000:]
    assert json.load(open(tmp_path / "group.json"))["size"] == 2
    for wt in (0, 1):
        FC.assert_same(np.load(tmp_path / ("group_wt%d.npy" % wt)), want[wt], "pt_group_render_aov_follow, watertight = %d" % wt)


def test_process_per_rank_over_the_stub_collective(tmp_path):
    want = _expected_child_case()
    target = rccl_stub.stub_path()
    so = str(tmp_path / "libcount_rccl.so")
    subprocess.check_call([shutil.which("g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rccl_stub.ROCM, "include"), "-o", so,
                           os.path.join(ROOT, "tests", "stub", "count_rccl.cpp"), "-ldl"])
    env = dict(os.environ, PT_RCCL_PATH=so, COUNT_RCCL_TARGET=target)
    world = 2
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "aov_follow_child.py"), "rank", str(tmp_path), str(r), str(world)], env=env) for r in range(world)]
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
    FC.assert_same(np.load(tmp_path / "rank0.npy"), want[0], "rank 0 of 2")
    for r in range(world):
        assert json.load(open(tmp_path / ("reduces_%d.json" % r)))["reduces"] == 1, "ONE reduce per rank"


def test_pt_main_follow_flag(tmp_path):
    from PIL import Image

    W, H, n = 40, 24, 2
    assets = os.path.join(ROOT, "assets")
    a = tmp_path / "assets"
    shutil.copytree(assets, a)
    s = json.load(open(os.path.join(assets, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[W, H], max_samples=4, max_path_depth=4, environment_color=[0.3, 0.6, 0.2], environment_intensity=0.75)
    sc = scene_io.load_scene_dir(assets, "cornell-box")
    mats = [m for _, m, _ in sc["materials"]]
    # the sweep sets the sphere's metallic to 1: with its roughness below --follow-roughness the guide ray follows it
    s["test"] = dict(name="g", material_name="sphere", attribute_name="metallic", material_type=2, values=[1.0, 1.0], step_size=1.0)
    (a / "settings.json").write_text(json.dumps(s))
    base = "cornell-box_g_metallic(1.0)"
    d = tmp_path / "out"
    os.makedirs(d)
    r = subprocess.run([PT_MAIN, "--assets", str(a), "--out", str(d), "--aov", str(n), "--follow", "4", "--follow-roughness", "1.0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    mats = np.stack(mats).astype(F32).copy()
    mats[1, 4] = 1.0
    ctx = B.Context(0)
    try:
        ctx.upload_scene(sc["entities"], list(mats), env=B.make_env(color=(0.3, 0.6, 0.2), intensity=0.75))
        c = sc["camera"]
        cam = B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
        g = ctx.render_aov_follow(cam, W, H, B.aov_default_params(n_samples=n, max_follow=4, roughness_max=1.0))
        first = ctx.render_aov(cam, W, H, n)
    finally:
        ctx.close()
    assert (FC.bits(g) != FC.bits(first)).any(), "the frame must hold followed pixels"

    def rgba(x):
        q = np.clip(np.nan_to_num((x * F32(256.0)).astype(F32), nan=0.0), 0, 255).astype(np.int64).astype(np.uint32)  # make_rgba: min(255, max(0, int(f * 256)))
        return q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(0xFF000000)

    png = lambda tag: np.asarray(Image.open(d / (base + tag))).view(np.uint32).reshape(H, W)
    np.testing.assert_array_equal(png("_albedo.png"), rgba(g[..., :3]))
    np.testing.assert_array_equal(png("_normal.png"), rgba(F32(0.5) * g[..., 4:7] + F32(0.5)))
    dep = (g[..., 7] / g[..., 7].max()).astype(F32)
    np.testing.assert_array_equal(png("_depth.png"), rgba(np.stack([dep] * 3, -1)))
    r = subprocess.run([PT_MAIN, "--assets", str(a), "--out", str(d), "--follow", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--follow" in r.stderr, r.stderr[-1000:]
