"""The C++ host entry point (owl-path-tracer_amd/host, binary owl-path-tracer_amd/pt_main): scene ingestion parity with the Python
mirror (both restate parser.cpp / mesh_loader.cpp / application.cpp:166-179), own PNG/HDR codecs, and -- on the GPU box -- the
end-to-end settings.json -> PNG path checked against the oracle."""
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import rccl_stub
from conftest import ASSETS, GOLDEN, ROOT

PT_MAIN = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")


def _run(args, cwd=None, env=None):
    out = subprocess.run([PT_MAIN] + args, cwd=cwd, capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out


def _read_dump(path):
    b = open(path, "rb").read()
    assert b[:4] == b"PTSC"
    p = 4

    def i32():
        nonlocal p
        v = struct.unpack_from("<i", b, p)[0]
        p += 4
        return v

    def string():
        nonlocal p
        n = i32()
        s = b[p:p + n].decode()
        p += n
        return s

    def arr(dtype, n):
        nonlocal p
        a = np.frombuffer(b, dtype, n, p).copy()
        p += a.nbytes
        return a

    cam = arr(np.float32, 10)
    mats = []
    for _ in range(i32()):
        name = string()
        data = arr(np.float32, 17)
        mats.append((name, data, string()))
    meshes = []
    for _ in range(i32()):
        name = string()
        nv, nn, nt, ntri = i32(), i32(), i32(), i32()
        meshes.append((name, dict(vertices=arr(np.float32, nv * 3).reshape(-1, 3), normals=arr(np.float32, nn * 3).reshape(-1, 3),
                                  texcoords=arr(np.float32, nt * 2).reshape(-1, 2), indices=arr(np.int32, ntri * 3).reshape(-1, 3))))
    ents = [(i32(), i32()) for _ in range(i32())]
    return cam, mats, meshes, ents


@pytest.mark.parametrize("cfg,scene", [("c1_cube.json", "cube"), ("c2_cornell-box.json", "cornell-box")])
def test_cpp_ingestion_matches_python_mirror(tmp_path, scene_io, cfg, scene):
    dump = str(tmp_path / "scene.bin")
    out = _run(["--device", "-1", "--assets", ASSETS, "--settings", os.path.join(ASSETS, "configs", cfg), "--dump-scene", dump])
    assert "no render" in out.stderr
    cam, mats, meshes, ents = _read_dump(dump)
    ref = scene_io.load_scene_dir(ASSETS, scene)
    c = ref["camera"]
    np.testing.assert_array_equal(cam, np.float32(c["look_from"] + c["look_at"] + c["look_up"] + [c["vertical_fov"]]))
    assert [(n, f) for n, _, f in mats] == [(n, f) for n, _, f in ref["materials"]]
    for (_, a, _), (_, b, _) in zip(mats, ref["materials"]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    assert [n for n, _ in meshes] == [n for n, _ in ref["meshes"]]
    for (_, a), (_, b) in zip(meshes, ref["meshes"]):
        for k in ("vertices", "normals", "texcoords", "indices"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    mesh_index = {id(m): i for i, (_, m) in enumerate(ref["meshes"])}
    assert ents == [(mesh_index[id(m)], mid) for m, mid in ref["entities"]]


def test_cpp_ingestion_quirks(tmp_path, scene_io):
    # quad face consumed as 3 indices with a 3-stride offset, first-seen normals, 'g' splits shapes, unmatched object vanishes
    a = tmp_path / "assets"
    a.mkdir()
    (a / "q.obj.scene").write_text("o a\nv 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nvn 0 0 1\nvn 0 1 0\nvt 0.25 0.75\nf 1/1/1 2/1/1 3/1/1\nf 2//2 4//2 3//2\n"
                                   "g b\nv 0 0 1\nf -1//1 1//1 2//1\no nomat\nf 1 2 3\n")
    mat = {k: 0.5 for k in ("subsurface", "metallic", "specular", "specular_tint", "roughness", "anisotropic", "sheen", "sheen_tint", "clearcoat",
                            "clearcoat_gloss", "ior", "specular_transmission", "specular_transmission_roughness", "emission")}
    scene = {"camera": {"look_from": [0, 0, 3], "look_at": [0, 0, 0], "look_up": [0, 1, 0], "vertical_fov": 40},
             "materials": [dict(mat, name="b", use_texture=False, filename="", base_color=[1, 0, 0]),
                           dict(mat, name="a", use_texture=True, filename="t.png", base_color=[0, 1, 0])]}
    (a / "q.json").write_text(json.dumps(scene))
    settings = json.load(open(os.path.join(ASSETS, "configs", "c1_cube.json")))
    settings["scene"] = "q"
    (a / "settings.json").write_text(json.dumps(settings))
    dump = str(tmp_path / "d.bin")
    _run(["--device", "-1", "--assets", str(a), "--dump-scene", dump])
    cam, mats, meshes, ents = _read_dump(dump)
    ref = scene_io.load_scene_dir(str(a), "q")
    assert [n for n, _ in meshes] == ["a", "b", "nomat"] == [n for n, _ in ref["meshes"]]
    for (_, x), (_, y) in zip(meshes, ref["meshes"]):
        for k in ("vertices", "normals", "texcoords", "indices"):
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)
    assert meshes[0][1]["normals"].tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 1, 0]]
    assert mats[1][2] == "a-textures/t.png" and mats[1][1][0] == np.float32(0.8)  # textured: base_color stays the default (parser.cpp:32-43)
    assert ents == [(0, 1), (1, 0)]
    # a missing key throws like nlohmann's .get<>()
    del scene["materials"][0]["ior"]
    (a / "q.json").write_text(json.dumps(scene))
    out = subprocess.run([PT_MAIN, "--device", "-1", "--assets", str(a)], capture_output=True, text=True)
    assert out.returncode != 0 and "missing key 'ior'" in out.stderr


def test_png_and_hdr_codecs(tmp_path):
    from PIL import Image

    rng = np.random.default_rng(5)
    for mode, ch in (("RGBA", 4), ("RGB", 3), ("L", 1), ("LA", 2), ("P", 1)):
        a = rng.integers(0, 256, (37, 53, ch), dtype=np.uint8)
        a[:, :20] = a[:, :1]  # runs, so the encoder emits matches and several filter types
        src, dst = str(tmp_path / ("in_%s.png" % mode)), str(tmp_path / ("out_%s.png" % mode))
        img = Image.fromarray(a.squeeze() if ch == 1 else a, "L" if mode == "P" else mode)
        if mode == "P":
            img = img.convert("P", palette=Image.ADAPTIVE, colors=64)
        img.save(src, optimize=(mode == "RGB"))
        _run(["--convert-png", src, dst])
        want = np.asarray(Image.open(src).convert("RGBA"))
        got = np.asarray(Image.open(dst))
        assert got.shape == want.shape and got.dtype == np.uint8
        np.testing.assert_array_equal(got, want, err_msg=mode)
    # Radiance RGBE with RLE scanlines -> stb's 8-bit gamma-2.2 tone map (stb_image.h:1864-1890)
    W, H = 48, 9
    rgbe = rng.integers(1, 256, (H, W, 4), dtype=np.uint8)
    rgbe[..., 3] = rng.integers(120, 136, (H, W))
    rgbe[:, 10:30] = rgbe[:, 10:11]
    rgbe[2, :, 3] = 0
    with open(tmp_path / "e.hdr", "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W))
        for y in range(H):
            f.write(bytes([2, 2, W >> 8, W & 255]))
            for c in range(4):
                row, x = rgbe[y, :, c], 0
                while x < W:
                    run = 1
                    while x + run < W and run < 127 and row[x + run] == row[x]:
                        run += 1
                    if run >= 3:
                        f.write(bytes([128 + run, row[x]]))
                        x += run
                    else:
                        n = min(W - x, 5)
                        f.write(bytes([n]) + bytes(row[x:x + n]))
                        x += n
    _run(["--convert-hdr", str(tmp_path / "e.hdr"), str(tmp_path / "e.png")])
    got = np.asarray(Image.open(tmp_path / "e.png"))
    f1 = np.where(rgbe[..., 3:4] == 0, 0.0, np.ldexp(1.0, rgbe[..., 3:4].astype(np.int32) - 136)).astype(np.float32)
    lin = rgbe[..., :3].astype(np.float32) * f1
    want = np.clip(np.power(lin, np.float32(1 / 2.2)) * 255 + 0.5, 0, 255).astype(np.uint8)
    assert np.abs(got[..., :3].astype(int) - want.astype(int)).max() <= 1  # powf rounding at .5 boundaries
    assert (got[..., 3] == 255).all()


@pytest.mark.gpu
def test_pt_main_end_to_end_matches_oracle(tmp_path, orc, scene_io):
    """assets/settings.json entry point -> PNG, compared with the oracle's RGBA8 image (C1 at full size: cube, 256x256, 16 spp,
    depth 4, textured) plus a two-frame material sweep on the cornell box (file naming of application.hpp:101-105)."""
    from PIL import Image

    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    os.makedirs(a / "cube-textures")
    tex = scene_io.checker_texture()
    Image.fromarray(np.ascontiguousarray(tex[::-1]).view(np.uint8).reshape(64, 64, 4)).save(a / "cube-textures" / "cube.png")  # file row 0 = top
    shutil.copy(os.path.join(ASSETS, "configs", "c1_cube.json"), a / "settings.json")
    out = _run(["--assets", str(a), "--out", str(tmp_path)])
    png = tmp_path / "cube_bench_roughness(0.2).png"
    assert png.exists(), out.stderr
    got = np.asarray(Image.open(png)).view(np.uint32).reshape(256, 256)
    sc = scene_io.load_scene_dir(str(a), "cube")
    S = orc.Scene(scene_io.flatten_scene(sc["entities"], sc["materials"], {0: tex}))
    c = sc["camera"]
    cam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], 256, 256)
    _, want8, _ = S.render(cam, orc.make_env(use_auto=True, intensity=1.0), 256, 256, 16, 4, want_rgba8=True)
    np.testing.assert_array_equal(got, want8)
    # sweep: metallic 0 -> 1 in two steps on the cornell sphere, 64x64
    s = json.load(open(os.path.join(ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[64, 64], max_samples=8)
    s["test"] = dict(name="sweep", material_name="sphere", attribute_name="metallic", material_type=2, values=[0.0, 1.0], step_size=1.0)
    (a / "settings.json").write_text(json.dumps(s))
    _run(["--assets", str(a), "--out", str(tmp_path)])
    sc = scene_io.load_scene_dir(str(a), "cornell-box")
    flat = scene_io.flatten_scene(sc["entities"], sc["materials"])
    S = orc.Scene(flat)
    c = sc["camera"]
    cam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], 64, 64)
    for v in (0.0, 1.0):
        mats = np.stack([m for _, m, _ in sc["materials"]]).copy()
        mats[1, 4] = v
        S.set_materials(mats)
        _, want8, _ = S.render(cam, orc.make_env(color=(1, 1, 1), intensity=0.0), 64, 64, 8, 16, want_rgba8=True)
        got = np.asarray(Image.open(tmp_path / ("cornell-box_sweep_metallic(%.1f).png" % v))).view(np.uint32).reshape(64, 64)
        np.testing.assert_array_equal(got, want8)


def _write_rle_hdr(path, rgbe):
    """Radiance RGBE file with RLE scanlines (the encoding image_buffer.cpp:36-58 reads through stb)."""
    H, W = rgbe.shape[:2]
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W))
        for y in range(H):
            f.write(bytes([2, 2, W >> 8, W & 255]))
            for c in range(4):
                row, x = rgbe[y, :, c], 0
                while x < W:
                    run = 1
                    while x + run < W and run < 127 and row[x + run] == row[x]:
                        run += 1
                    if run >= 3:
                        f.write(bytes([128 + run, row[x]]))
                        x += run
                    else:
                        n = min(W - x, 5)
                        f.write(bytes([n]) + bytes(row[x:x + n]))
                        x += n


def _device_count():
    import torch

    return torch.cuda.device_count()


def _hdr_and_texture_assets(tmp_path, scene_io):
    """A copy of assets/ with the cube's texture PNG, an environment.hdr (RLE RGBE) and settings that use both: (dir, texture, map
    width, map height)."""
    from PIL import Image

    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    os.makedirs(a / "cube-textures")
    tex = scene_io.checker_texture()
    Image.fromarray(np.ascontiguousarray(tex[::-1]).view(np.uint8).reshape(64, 64, 4)).save(a / "cube-textures" / "cube.png")
    # sky gradient + sun + ground, enough dynamic range for the tone map to matter, long runs for the RLE
    EW, EH = 256, 128
    yy, xx = np.mgrid[0:EH, 0:EW]
    lum = np.where(yy < EH // 2, 0.3 + 1.7 * (1 - yy / (EH / 2)), 0.08 + 0.1 * ((xx // 16 + yy // 16) % 2))
    sun = np.exp(-(((xx - 180) / 6.0) ** 2 + ((yy - 24) / 6.0) ** 2)) * 40.0
    rgbf = np.stack([lum * 0.9 + sun, lum * 1.0 + sun * 0.9, lum * 1.3 + sun * 0.6], -1).astype(np.float64)
    m = rgbf.max(-1)
    e = np.ceil(np.log2(np.maximum(m, 1e-30))).astype(np.int32)
    rgbe = np.zeros((EH, EW, 4), np.uint8)
    rgbe[..., :3] = np.clip(rgbf / np.ldexp(1.0, e)[..., None] * 256.0, 0, 255).astype(np.uint8)
    rgbe[..., 3] = (e + 128).astype(np.uint8)
    _write_rle_hdr(a / "environment.hdr", rgbe)
    s = json.load(open(os.path.join(ASSETS, "configs", "c1_cube.json")))
    s.update(buffer_size=[160, 96], max_samples=32, max_path_depth=6, environment_use=True, environment_auto=False, environment_intensity=1.0)
    (a / "settings.json").write_text(json.dumps(s))
    return a, tex, EW, EH


@pytest.mark.gpu
def test_pt_main_environment_hdr_and_texture_end_to_end(tmp_path, orc, scene_io):
    """assets/environment.hdr (RLE RGBE) and a PNG texture through the real entry point on the GPU -
    application.cpp:160 -> image_buffer.cpp:36-58 (stb tone map + vertical flip) -> device.cu:23-39 (miss shader lookup), and
    application.cpp:225-246 -> device.cu:75-94 (texture).  The oracle gets the environment map as the product's own decoder
    produces it (the decoder itself is checked against the stb formula in test_png_and_hdr_codecs)."""
    from PIL import Image

    a, tex, EW, EH = _hdr_and_texture_assets(tmp_path, scene_io)
    out = _run(["--assets", str(a), "--out", str(tmp_path)])
    png = tmp_path / "cube_bench_roughness(0.2).png"
    assert png.exists(), out.stderr
    got = np.asarray(Image.open(png)).view(np.uint32).reshape(96, 160)
    _run(["--convert-hdr", str(a / "environment.hdr"), str(tmp_path / "env.png")])
    env = np.ascontiguousarray(np.asarray(Image.open(tmp_path / "env.png"))[::-1]).view(np.uint32).reshape(EH, EW)  # flip: image_buffer.cpp:50-55
    assert len(np.unique(env)) > 50
    sc = scene_io.load_scene_dir(str(a), "cube")
    S = orc.Scene(scene_io.flatten_scene(sc["entities"], sc["materials"], {0: tex}))
    c = sc["camera"]
    cam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], 160, 96)
    _, want8, st = S.render(cam, orc.make_env(use_map=True, intensity=1.0, env_map=env), 160, 96, 32, 6, want_rgba8=True, want_counters=True)
    assert st["env_misses"] > 1000
    np.testing.assert_array_equal(got, want8)


@pytest.mark.gpu
def test_pt_main_gpus_flag_is_bit_identical(tmp_path):
    """`pt_main --gpus N` (pt_group_*: pixel tiles over N devices + the library's RCCL reduce onto device 0) writes the same PNG
    as the single-context path.  N = 1 always runs; N = 2 and N = all devices when the box has them."""
    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    s = json.load(open(os.path.join(ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[200, 120], max_samples=48)
    (a / "settings.json").write_text(json.dumps(s))
    name = "cornell-box_%s_%s(%.1f).png" % (s["test"]["name"], s["test"]["attribute_name"], s["test"]["values"][0])
    ref_dir = tmp_path / "ref"
    os.makedirs(ref_dir)
    _run(["--assets", str(a), "--out", str(ref_dir)])
    want = open(ref_dir / name, "rb").read()
    nd = _device_count()
    for n in sorted({1, min(2, nd), nd}):
        d = tmp_path / ("g%d" % n)
        os.makedirs(d)
        _run(["--assets", str(a), "--out", str(d), "--gpus", str(n)])
        assert open(d / name, "rb").read() == want, "--gpus %d differs from the single-context image" % n


def _sweep_assets(tmp_path):
    """C2 as a three-frame material sweep (the sphere's metallic 0, 0.5, 1 through pt_set_materials / pt_group_set_materials) at
    200x120, 48 spp: (assets dir, PNG names)."""
    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    s = json.load(open(os.path.join(ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[200, 120], max_samples=48)
    s["test"] = dict(name="sweep", material_name="sphere", attribute_name="metallic", material_type=2, values=[0.0, 1.0], step_size=0.5)
    (a / "settings.json").write_text(json.dumps(s))
    return a, ["cornell-box_sweep_metallic(%.1f).png" % v for v in (0.0, 0.5, 1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["sweep", "hdr_and_texture"])
def test_pt_main_devices_under_stub_collective(tmp_path, scene_io, workload):
    """`pt_main --devices 0,0` / `0,0,0` (and `--gpus 2 --devices 0,0`): the group path with 2 and 3 contexts on one card, the stub
    collective of tests/stub/fake_rccl.cpp standing in for RCCL (it is not RCCL; the real library refuses a device named twice).
    Every PNG must be byte-identical to the single-context run's: a three-frame material sweep on the cornell box (every frame after
    a pt_group_set_materials), and the textured cube under environment.hdr (texture + environment map through clone_scene)."""
    if workload == "sweep":
        a, names = _sweep_assets(tmp_path)
    else:
        a, names = _hdr_and_texture_assets(tmp_path, scene_io)[0], ["cube_bench_roughness(0.2).png"]
    ref_dir = tmp_path / "ref"
    os.makedirs(ref_dir)
    _run(["--assets", str(a), "--out", str(ref_dir)])
    want = [open(ref_dir / n, "rb").read() for n in names]
    assert len(set(want)) == len(want), "the frames of the sweep must differ, or the material swap is not under test"
    env = rccl_stub.stub_env()
    for i, flags in enumerate((["--devices", "0,0"], ["--devices", "0,0,0"], ["--gpus", "2", "--devices", "0,0"])):
        d = tmp_path / ("g%d" % i)
        os.makedirs(d)
        _run(["--assets", str(a), "--out", str(d)] + flags, env=env)
        for n, w in zip(names, want):
            assert open(d / n, "rb").read() == w, "%s: %s differs from the single-context image" % (" ".join(flags), n)


@pytest.mark.parametrize("flags,word", [(["--devices", "0,x"], "--devices"), (["--devices", ""], "--devices"), (["--devices", "0,,1"], "--devices"),
                                        (["--devices", "-1"], "--devices"), (["--devices", "0,0", "--gpus", "3"], "--gpus"),
                                        (["--devices", "0", "--device", "1"], "--device"), (["--device", "-1", "--devices", "0"], "--device"),
                                        (["--devices"], "--devices")])
def test_pt_main_devices_flag_errors(flags, word):
    """A device list that is empty or holds anything but non-negative integers, a count that disagrees with --gpus, and --devices next
    to --device: exit status 1 and a message that names the option (no GPU needed: refused before anything is opened)."""
    out = subprocess.run([PT_MAIN, "--assets", ASSETS, "--settings", os.path.join(ASSETS, "configs", "c1_cube.json")] + flags, capture_output=True, text=True, timeout=120)
    assert out.returncode == 1, out.stderr[-2000:]
    assert out.stderr.startswith("error: ") and word in out.stderr and "--devices" in out.stderr, out.stderr[-2000:]


BENCH_REHEARSAL_LIMIT = 20  # seconds: three times the 6.5 s measured, see test_bench_two_rank_rehearsal


@pytest.mark.gpu
def test_bench_two_rank_rehearsal(tmp_path):
    """bench.py's N = 2 leg as the script itself offers it for a one-GPU box (PT_BENCH_DEVICE + PT_RCCL_PATH, bench.py main()): both
    ranks on device 0 under torch.distributed.run, the stub collective instead of RCCL.  Checked: what the script promises for such
    a run - one JSON line marked "rehearsal", n_gpus 2, a per-rank table whose pixel counts are the two shards - and that the frame it
    dumps has the golden checksum, which test_c4_golden_crc_is_the_oracles ties to the oracle.  No timing number of this run means
    anything (two ranks on one card through files) and none is asserted.  BENCH_REHEARSAL_LIMIT only guards against a hang: the
    command took 5.8 and 6.5 s of wall time as the first thing run on an MI355X box (5.3 to 5.7 s inside the suite; everything it runs -
    bench.py, the process-per-rank driver, the stub's file mode - is as in the parent commit), and the limit is three times the longest."""
    import importlib.util
    import zlib

    try:
        if importlib.util.find_spec("torch.distributed.run") is None:
            raise ImportError
    except ImportError:
        pytest.skip("torch.distributed.run cannot be imported")
    from owl_path_tracer_amd.pyhost import binding as B

    dump = tmp_path / "dump"
    env = rccl_stub.stub_env(PT_BENCH_DEVICE="0")
    rc, so, se = rccl_stub.run_child([sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "bench.py", "--gpus", "2",
                                      "--steps", "1", "--warmup", "0", "--dump-outputs", str(dump)], env, BENCH_REHEARSAL_LIMIT, cwd=ROOT)
    assert rc == 0, so[-2000:] + se[-4000:]
    lines = [json.loads(l) for l in so.splitlines() if l.startswith("{")]
    assert len(lines) == 1, so[-4000:]
    out = lines[0]
    assert out.get("rehearsal") is True and out["n_gpus"] == 2
    W, H = 1920, 1080
    rows = sorted(out["per_rank"], key=lambda r: r["rank"])
    assert [r["rank"] for r in rows] == [0, 1]
    assert [r["pixels"] for r in rows] == [len(B.shard_pixels(W, H, 16, r, 2)) for r in range(2)]
    assert sum(r["pixels"] for r in rows) == W * H
    frame = np.load(dump / "frame.npy")
    assert frame.shape == (H, W, 3) and frame.dtype == np.float32
    crc = zlib.crc32(np.ascontiguousarray(frame, np.float32).tobytes()) & 0xFFFFFFFF  # bench.py: frame_crc
    assert crc == json.load(open(os.path.join(GOLDEN, "c4_frame_crc.json")))["crc32_float3_frame"]
