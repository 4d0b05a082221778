"""Host-side sanitizer runs (round-2 verdict: "no sanitizer run ever touched the hand-written inflate / RLE /
JSON / OBJ parsers").  `make -C owl-path-tracer_amd/csrc asan` builds the library's host code (pt_api.cpp, pt_scene.cpp, pt_render.cpp, pt_guides.cpp, pt_debug.cpp, pt_comm.cpp, pt_bvh.cpp, pt_aov_host.cpp, pt_denoise_host.cpp) with
g++ -fsanitize=address,undefined and stubbed kernel launchers; `make -C owl-path-tracer_amd/host asan` builds the entry point and its
own JSON / OBJ / PNG / Radiance readers the same way.  No GPU: device code cannot be sanitized on this pool, and --device -1 stops
after scene load + BVH build (the reference's counterparts: mesh_loader.cpp:96-98, image_buffer.cpp:27-28, macros.hpp:5-11).

* every truncated or garbled PNG / HDR / OBJ / JSON input must end in an error message and a non-zero exit code (or be accepted) -
  never in a sanitizer report or a signal;
* the CPU tests of the ABI and of the BVH builder run once more against the sanitized library."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ASSETS, ROOT

PKG = os.path.join(ROOT, "owl-path-tracer_amd")
PT_MAIN_ASAN = os.path.join(PKG, "pt_main_asan")
LIB_ASAN = os.path.join(PKG, "libmi355pt_asan.so")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def asan_build():
    try:
        subprocess.check_call(["make", "-C", os.path.join(PKG, "csrc"), "-s", "asan"], timeout=600)
        subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s", "asan"], timeout=600)
    except (subprocess.CalledProcessError, OSError) as e:
        pytest.skip("sanitizer build unavailable: %s" % e)
    return PT_MAIN_ASAN


def _run(binary, args):
    r = subprocess.run([binary] + args, capture_output=True, text=True, timeout=300, env=ENV, errors="replace")
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-3000:]
    assert r.returncode in (0, 1), "exit code %d (a signal or a sanitizer abort): %s" % (r.returncode, text[-3000:])
    return r


def _assets(tmp_path):
    """A small complete assets directory: cube.json + cube.obj.scene + a PNG texture + an RLE environment.hdr + settings."""
    from PIL import Image

    a = tmp_path / "assets"
    (a / "cube-textures").mkdir(parents=True)
    for f in ("cube.json", "cube.obj.scene"):
        shutil.copy(os.path.join(ASSETS, f), a / f)
    rng = np.random.default_rng(7)
    Image.fromarray(rng.integers(0, 255, (32, 32, 4), dtype=np.uint8)).save(a / "cube-textures" / "cube.png")
    rgbe = rng.integers(0, 255, (8, 16, 4), dtype=np.uint8)
    rgbe[:, 4:12, 0] = 9  # runs, so that the file has both RLE packet kinds
    from test_host_main import _write_rle_hdr

    _write_rle_hdr(a / "environment.hdr", rgbe)
    s = json.load(open(os.path.join(ASSETS, "configs", "c1_cube.json")))
    s["environment_use"] = True
    with open(a / "settings.json", "w") as f:
        json.dump(s, f)
    return a


def _variants(data, rng, n_cuts=12, n_flips=12):
    """Truncations at spread-out offsets and copies with a few corrupted bytes."""
    out = []
    for k in range(n_cuts):
        out.append(data[: max(0, (len(data) * k) // n_cuts + int(rng.integers(0, 7)))])
    for _ in range(n_flips):
        b = bytearray(data)
        for _ in range(int(rng.integers(1, 6))):
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append(bytes(b))
    return out


@pytest.mark.parametrize("victim", ["cube-textures/cube.png", "environment.hdr", "cube.obj.scene", "cube.json", "settings.json"])
def test_garbled_inputs_give_errors_not_crashes(tmp_path, asan_build, victim):
    a = _assets(tmp_path)
    base = ["--device", "-1", "--assets", str(a), "--settings", str(a / "settings.json"), "--out", str(tmp_path)]
    ok = _run(asan_build, base)
    assert ok.returncode == 0 and "no render" in ok.stderr, ok.stderr[-2000:]
    good = open(a / victim, "rb").read()
    rng = np.random.default_rng(11)
    n_err = 0
    for blob in _variants(good, rng):
        with open(a / victim, "wb") as f:
            f.write(blob)
        r = _run(asan_build, base)
        n_err += r.returncode != 0
    assert n_err > 0  # at least the empty / half files must be refused
    # hand-made nasties
    nasty = {
        "cube.obj.scene": [b"o cube\nv 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1//1 2//1 99999999//1\n", b"o cube\nf 1 2 3\n", b"o cube\nv 1e999 nan -inf\nf -5//-5 0//0 1//1\n",
                           b"o cube\n" + b"v 0 0 0\n" * 3 + b"vn 0 0 1\nf 1//1 2//1\nf\nf 1/2/3/4/5 2 3\n", b"\x00\xff" * 200],
        "cube.json": [b"{", b"[]", b'{"camera": 5, "materials": "x"}', b'{"materials": [{"name": 7}]}', b'{"a": ' + b"[" * 5000 + b"]" * 5000 + b"}", b'{"a": "\\u12"}', b'{"a": 1e99999}'],
        "settings.json": [b"{}", b'{"fb_size": [0, 0]}', b'{"fb_size": [-4, 100000000]}', b'{"scene": 5}', b'{"max_samples": -1, "max_path_depth": 999}'],
        "environment.hdr": [b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 100000 +X 100000\n", b"#?RADIANCE\n\n-Y 2 +X 8\n\x02\x02\x00\x08\xff\x01", b"#?RGBE\nFORMAT=32-bit_rle_rgbe\n\n+X 4 -Y 4\n" + b"\x01" * 64,
                            b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y -3 +X 4\n"],
        "cube-textures/cube.png": [good[:8] + b"\x00\x00\x00\x0dIHDR" + b"\xff" * 17 + good[33:], good[:33] + b"\x7f\xff\xff\xffIDAT" + good[41:], good[:8] + good[8:33] * 3 + good[33:],
                                   good[:16] + b"\x00\x01\x00\x00\x00\x01\x00\x00" + good[24:]],
    }
    for blob in nasty.get(victim, []):
        with open(a / victim, "wb") as f:
            f.write(blob)
        _run(asan_build, base)


def test_cpu_suite_against_the_sanitized_library(asan_build):
    """tests/test_abi_host.py (ABI surface, host BVH builder vs brute force, quad / oct collapse, sharding, upload validation, the RCCL
    load failure) with libmi355pt_asan.so in place of the product library."""
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    libubsan = subprocess.check_output(["gcc", "-print-file-name=libubsan.so"], text=True).strip()
    env = dict(ENV, PT_LIB_PATH=LIB_ASAN, LD_PRELOAD=libasan + ":" + libubsan)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_abi_host.py"), "-x", "-q", "-p", "no:cacheprovider"], capture_output=True, text=True,
                       timeout=1200, env=env, cwd=ROOT, errors="replace")
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0, text[-4000:]
