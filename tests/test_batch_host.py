"""pt_render_batch without a GPU: the ABI surface, the cut of a batch into launch sequences (pt_debug_plan_batch), the argument errors
of a host-only context, hipcc's resource report for the batch instances of the render kernel, and the same host paths under the
ASan / UBSan build of the library.  (The renders themselves: tests/test_gpu_batch.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import resource_report
from owl_path_tracer_amd.pyhost import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "owl-path-tracer_amd", "csrc")
NEW = ("pt_render_batch", "pt_render_batch_device", "pt_debug_plan_batch")

# The limits of one launch sequence, from the code that sets them (csrc/pt_render.cpp, batch_max_frames): a path slot packs its pixel as
# x | y << 16 and pt_render_device accepts heights up to 65535, so the virtual image has at most 65535 rows; plan_chunks refuses
# n_pixels >= 2^24.
MAX_ROWS = 65535
MAX_PIXELS = (1 << 24) - 1


def test_header_library_and_binding_agree_on_the_batch_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    declared = set(re.findall(r"\b(pt_[a-z0-9_]+)\s*\(", src))
    L = C.CDLL(B.LIB_PATH)
    for n in NEW:
        assert n in declared, "not declared in mi355pt.h: " + n
        assert hasattr(L, n), "not exported: " + n
        assert n in B.EXPORTS, "not in binding.EXPORTS: " + n
    assert re.search(r"typedef struct pt_frame \{\s*pt_camera camera;\s*const float\* materials;", src)
    assert C.sizeof(B.Frame) == 56 and B.Frame.materials.offset == 48  # pt_camera (48 bytes) + one pointer
    assert B.lib().pt_abi_version() == 5  # pt_stats keeps its layout


@pytest.mark.parametrize("W,H,n,cap", [(61, 47, 3, 0), (61, 47, 5, 2), (512, 512, 8, 0), (512, 512, 200, 0), (1920, 1080, 9, 0), (1920, 1080, 40, 3), (1, 1, 7, 0),
                                       (1, 1, 100000, 0), (3, 65535, 4, 0), (65535, 1, 300, 0), (4096, 4095, 3, 0), (200, 120, 1, 0), (200, 120, 1, 5), (7, 33000, 3, 0)])
def test_plan_batch_respects_every_limit(W, H, n, cap):
    seq = B.plan_batch(W, H, n, cap)
    assert sum(seq) == n and all(k >= 1 for k in seq)
    for k in seq:
        assert k * H <= MAX_ROWS, "rows of the virtual image"
        assert k * W * H <= MAX_PIXELS, "pixels of the virtual image"
        assert cap == 0 or k <= cap, "option batch_frames"
    # as few sequences as the limits allow: all but the last are as large as the tightest limit lets them be
    kmax = min(MAX_ROWS // H, MAX_PIXELS // (W * H), cap if cap else n)
    assert all(k == min(kmax, n) for k in seq[:-1]) and len(seq) == -(-n // kmax)


def test_plan_batch_errors():
    pb = B.lib().pt_debug_plan_batch
    assert pb(4096, 4096, 1, 0, None, 0) == -5  # one frame of 2^24 pixels is already beyond a launch sequence: PT_E_LIMIT
    assert pb(4096, 4096, 3, 1, None, 0) == -5
    for bad in ((0, 8, 1, 0), (8, 0, 1, 0), (8, 8, 0, 0), (8, 8, -1, 0), (8, 8, 1, -1), (65536, 8, 1, 0), (8, 65536, 1, 0)):
        assert pb(*bad, None, 0) == -1, bad
    with pytest.raises(B.PtError):
        B.plan_batch(4096, 4096, 2)
    # K = 1 and the size query / short capacity
    assert B.plan_batch(4095, 4096, 1) == [1]
    out = (C.c_int32 * 2)(-7, -7)
    assert pb(64, 64, 10, 3, out, 1) == 4 and out[0] == 3 and out[1] == -7  # at most cap entries are written


def _frames(mats, n):
    cam = B.to_camera_data([2, 1, 2], [0, 0, 0], [0, 1, 0], 50, 8, 8)
    return [(cam, np.stack(mats).astype(np.float32)) for _ in range(n)]


def test_batch_argument_errors_on_a_host_only_context(cube):
    mats = [m for _, m, _ in cube["materials"]]
    fresh = B.Context(-1)
    with pytest.raises(B.PtError, match=r"\(-4\).*no geometries"):  # PT_E_NO_SCENE
        fresh.render_batch(_frames(mats, 2), 8, 8, 1, 4)
    fresh.close()
    ctx = B.Context(-1)
    ctx.upload_scene(cube["entities"], mats, textures=[np.zeros((2, 2), np.uint32)], mesh_textures=[0])
    with pytest.raises(B.PtError, match=r"\(-1\).*at least one frame"):
        ctx.render_batch([], 8, 8, 1, 4, n_materials=len(mats))
    rgb = np.zeros((1, 8, 8, 3), np.float32)
    fp = rgb.ctypes.data_as(C.POINTER(C.c_float))
    assert B.lib().pt_render_batch(ctx._h, None, 2, len(mats), 8, 8, 1, 4, fp, None) == -1  # NULL frames
    assert "frames NULL" in B.lib().pt_last_error(ctx._h).decode()
    arr, n_mat, keep = B._marshal_frames(_frames(mats, 2))
    assert B.lib().pt_render_batch(ctx._h, arr, 0, n_mat, 8, 8, 1, 4, fp, None) == -1
    assert B.lib().pt_render_batch(ctx._h, arr, -3, n_mat, 8, 8, 1, 4, fp, None) == -1
    assert B.lib().pt_render_batch(ctx._h, arr, 2, n_mat, 8, 8, 1, 4, None, None) == -1  # no output buffer
    assert B.lib().pt_render_batch(None, arr, 2, n_mat, 8, 8, 1, 4, fp, None) == -1
    with pytest.raises(B.PtError, match=r"\(-1\).*materials per frame"):
        ctx.render_batch(_frames(mats, 2), 8, 8, 1, 4, n_materials=len(mats) + 1)
    with pytest.raises(B.PtError, match=r"\(-1\).*bad render size"):
        ctx.render_batch(_frames(mats, 2), 8, 0, 1, 4)
    with pytest.raises(B.PtError, match=r"\(-1\).*bad render size"):
        ctx.render_batch(_frames(mats, 2), 8, 8, 1, 64)
    # what a batch cannot do is refused by name
    for key, val, word in (("kernel", 1, "lane-per-pixel"), ("latency", 1, "latency"), ("timeline", 1, "timeline")):
        ctx.set_option(key, val)
        with pytest.raises(B.PtError, match=r"\(-1\).*" + word):
            ctx.render_batch(_frames(mats, 2), 8, 8, 1, 4)
        ctx.set_option(key, 2 if key == "kernel" else 0)
    # a valid call: there is no CPU fallback, for the host-copy and the device-pointer entry point alike
    with pytest.raises(B.PtError, match="no CPU fallback"):
        ctx.render_batch(_frames(mats, 3), 8, 8, 1, 4)
    with pytest.raises(B.PtError, match="no CPU fallback"):
        ctx.render_batch([(f[0], None) for f in _frames(mats, 2)], 8, 8, 1, 4, n_materials=len(mats))  # NULL table = the context's
    with pytest.raises(B.PtError, match="no CPU fallback"):
        ctx.render_batch_device(_frames(mats, 2), 8, 8, 1, 4, 0x1000)
    ctx.set_option("batch_frames", 2)
    ctx.set_option("batch_frames", 0)
    ctx.close()


def test_batch_kernel_instances_need_no_scratch():
    """pt_render_batch refuses a batch instance that spills, as pt_render does for the single-frame ones (plan_frame): every batch
    instance must report ScratchSize 0, there must be exactly the five the launcher selects from (pt_launch_render_batch: product and
    fallback budget, each with the fma and the subtracting slab form, and the instrumented instance), and the batch translation unit
    must not define a second copy of the single-frame kernel."""
    resource_report.assert_ships_with_makefile_flags("pt_kernel_batch")
    report = resource_report.report("asm-batch")[0]
    blocks = re.findall(r"Function Name: (\S*pt_render_batch_kernel\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", report, flags=re.S)
    names = sorted(n for n, _, _ in blocks)
    # <COUNT, WAVES, EXACT> of the five instances pt_launch_render_batch launches (PT_WAVES_PER_EU 4, PT_FALLBACK_WAVES 3, PT_COUNT_WAVES_PER_EU 2)
    want = sorted("_Z22pt_render_batch_kernelILb%dELi%dELb%dEEvPK14PtKernelParams" % t for t in ((0, 4, 0), (0, 4, 1), (0, 3, 0), (0, 3, 1), (1, 2, 0)))
    assert names == want, names
    assert all(int(sz) == 0 for _, _, sz in blocks), blocks
    budget = {"Li4E": 128, "Li3E": 168, "Li2E": 256}
    for n, vg, _ in blocks:
        assert int(vg) <= budget[re.search(r"Li\dE", n).group(0)], (n, vg)
    assert "pt_render_wave_kernel" not in report
    src = open(os.path.join(CSRC, "pt_kernel.hip")).read()
    # (the launcher and the geometry function take the instance from render_instance: the one place that names them)
    pick = src[src.index('static const void* render_instance'):src.index('extern "C" hipError_t pt_launch_render_batch')]
    assert len(re.findall(r"\(const void\*\)PT_RENDER_KERNEL<", pick)) == len(blocks) == 5
    assert "PT_RENDER_KERNEL<" not in src[src.index('extern "C" hipError_t pt_launch_render_batch'):]


def test_batch_host_paths_under_asan():
    """The argument-error and plan tests above once more against libmi355pt_asan.so (g++ -fsanitize=address,undefined, stubbed kernel
    launchers: `make -C csrc asan` must still link with the batch launchers stubbed)."""
    try:
        subprocess.check_call(["make", "-C", CSRC, "-s", "asan"], timeout=600)
    except (subprocess.CalledProcessError, OSError) as e:
        pytest.skip("sanitizer build unavailable: %s" % e)
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    libubsan = subprocess.check_output(["gcc", "-print-file-name=libubsan.so"], text=True).strip()
    preload = ":".join([libasan, libubsan] + [p for p in os.environ.get("LD_PRELOAD", "").split(":") if p])  # the sanitizer runtime comes first
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               PT_LIB_PATH=os.path.join(ROOT, "owl-path-tracer_amd", "libmi355pt_asan.so"), LD_PRELOAD=preload)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider", "-k",
                        "argument_errors or plan_batch or agree_on_the_batch_symbols"], capture_output=True, text=True, timeout=1200, env=env, cwd=ROOT, errors="replace")
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0, text[-4000:]
    assert re.search(r"\b17 passed", text), text[-500:]  # the selected tests ran: 14 plan cases, plan errors, symbols, argument errors
