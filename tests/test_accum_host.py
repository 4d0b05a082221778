"""Progressive accumulation (pt_accum_*; include/mi355pt.h, "progressive accumulation") on the CPU: no GPU needed.

* pt_debug_accum_resolve_host / pt_debug_accum_select_host == tests/accum_ref.py (numpy float32, restated from the header) bit for bit on
  random state arrays: NaN and +-Inf sums, n_half = 0, n = 0, zero and negative sums (the 1e-2 floor), noise exactly at the threshold, the
  cap at n == cap and n == cap - 1, pixels not owned, active and inactive pixels at odd and even passes.
* The exports are in the header and in B.EXPORTS, the ABI is still 5, NULL parameters are the defaults.
* Every refusal a host-only context can reach, by code and message; valid arguments there: PT_E_NO_DEVICE at pt_accum_begin.  (The
  refusals that need an accumulation - a pixel's n about to pass 2^31 - 65536, a changed shard, a new scene - and the communicator's are
  in tests/test_gpu_accum.py.)  `pt_main --adds K` with K > max_samples is refused by pt_main.
* `make asm-accum`: two kernels, 0 scratch.  `make asm asm-wt asm-batch`: every render-kernel instance reports the registers, LDS and
  scratch recorded in tests/golden/render_kernel_resources.json on the commit before this feature - the render kernel was not touched."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import accum_ref
import aov_common as AC
import resource_report
from owl_path_tracer_amd.pyhost import binding as B

ROOT = AC.ROOT
F32, U32 = np.float32, np.uint32
INF, NAN = float("inf"), float("nan")
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_accum_default_params", "pt_accum_begin", "pt_accum_add", "pt_accum_add_device", "pt_accum_read", "pt_accum_info_get", "pt_accum_end",
         "pt_debug_accum_resolve_host", "pt_debug_accum_select_host", "pt_debug_accum_state")


@pytest.fixture(scope="module")
def host():
    ctx = B.Context(-1)
    yield ctx
    ctx.close()


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same(a, b):
    """Bit for bit, any NaN equal to any NaN: which NaN an invalid operation or a NaN operand yields (sign, payload) is the machine's choice
    - x86 SSE, its vectorised loops and gfx950 differ - and the definition only ever tests a NaN with `!=` or `<=`."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def test_error_codes_are_the_headers():
    header = open(B.HEADER_PATH).read()
    for name, v in (("PT_E_INVALID", PT_E_INVALID), ("PT_E_NO_DEVICE", PT_E_NO_DEVICE), ("PT_E_NO_SCENE", PT_E_NO_SCENE)):
        assert re.search(r"\b%s = %d," % (name, v), header), name


def test_exports_abi_and_defaults():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert L.pt_abi_version() == 5 and "#define PT_ABI_VERSION 5" in header
    p = B.accum_default_params()
    assert (p.n_samples, p.max_pixel_samples, p.reserved) == (16, 0, 0) and bits(p.noise_threshold) == 0
    assert C.sizeof(B.AccumParams) == 16 and C.sizeof(B.AccumInfo) == 40
    assert "pt_accum_add_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)


def random_state(seed, N):
    """State arrays as an accumulation can hold them, and as it cannot: every special the definition has to answer."""
    rng = np.random.default_rng(seed)
    sum_ = (rng.random((N, 3)) * rng.choice([0.0, 1e-4, 1.0, 300.0, 1e30], (N, 1))).astype(F32)
    sum_[rng.random((N, 3)) < 0.05] = 0.0
    neg = rng.random(N) < 0.1
    sum_[neg] = -sum_[neg]  # negative and zero sums: the 1e-2 floor
    for v in (NAN, INF, -INF):
        sum_[rng.random((N, 3)) < 0.02] = v
    frac = rng.random((N, 3)).astype(F32)
    seen = (sum_ * frac).astype(F32)
    half = (seen * rng.random((N, 3)).astype(F32)).astype(F32)
    half[rng.random(N) < 0.05] = NAN
    n = rng.choice([0, 1, 2, 7, 8, 16, 31, 32, 33, 1000, 65535, 2 ** 31 - 131072], N).astype(U32)
    n_half = (n * rng.choice([0.0, 0.25, 0.5, 1.0], N)).astype(U32)  # 0: noise stays +inf; n_half == n: a division by zero
    passes = rng.integers(0, 9, N).astype(U32)
    active = (rng.random(N) < 0.6).astype(np.uint8) * rng.choice([1, 255], N).astype(np.uint8)
    owned = (rng.random(N) < 0.85).astype(np.uint8)
    return sum_, seen, half, n, n_half, passes, active, owned


@pytest.mark.parametrize("seed,N,ns", [(1, 1, 1), (2, 63, 8), (3, 4097, 16), (4, 20011, 65535)])
def test_resolve_twin_equals_the_restatement(host, seed, N, ns):
    st = random_state(seed, N)
    before = [np.array(a) for a in st]
    want = accum_ref.resolve(*st, ns)
    got = host.accum_resolve_host(*st, ns)
    for a, b in zip(st, before):
        assert a.tobytes() == b.tobytes(), "the wrapper must not change its inputs"
    for k in ("seen", "half", "rgb", "noise"):
        assert same(got[k], want[k]).all(), (k, int((~same(got[k], want[k])).sum()))
    for k in ("n", "n_half", "passes", "rgba8"):
        assert (got[k] == want[k]).all(), k
    own = st[7] != 0
    if N > 1000:  # the cases are there
        z = got["noise"][own]
        assert np.isinf(z).any() and np.isnan(z).any() and (np.isfinite(z) & (z > 0)).any()
        with np.errstate(all="ignore"):
            lum = (got["rgb"][..., 0] + got["rgb"][..., 1]).astype(F32) + got["rgb"][..., 2]
            assert (own & np.isfinite(got["noise"]) & (lum < F32(1e-2))).any(), "zero and negative sums: the brightness floor divides"
    assert (bits(got["noise"][~own]) == 0).all() and (bits(got["rgb"][~own]) == 0).all() and (got["rgba8"][~own] == 0).all()
    assert (got["n"][~own] == st[3][~own]).all(), "a pixel the context does not own keeps its state"


def test_resolve_by_hand(host):
    """Three adds of one pixel, written out: pass 0 and 2 go to the other half, pass 1 to `half`."""
    o = np.ones(1, np.uint8)
    z3, z1 = np.zeros((1, 3), F32), np.zeros(1, U32)
    s1 = np.array([[8.0, 4.0, 2.0]], F32)
    r = host.accum_resolve_host(s1, z3, z3, z1, z1, z1, o, o, 8)
    assert (r["n"], r["n_half"], r["passes"]) == (8, 0, 1) and np.isinf(r["noise"][0]) and (r["rgb"] == s1 / 8).all() and (r["half"] == 0).all()
    s2 = np.array([[24.0, 8.0, 2.0]], F32)  # the second 8 samples sum to (16, 4, 0)
    r = host.accum_resolve_host(s2, r["seen"], r["half"], r["n"], r["n_half"], r["passes"], o, o, 8)
    assert (r["n"], r["n_half"], r["passes"]) == (16, 8, 2) and (r["half"] == [[16.0, 4.0, 0.0]]).all()
    # a = (2, .5, 0), b = (1, .5, .25): d = 1.25; out = (1.5, .5, .125): l = 2.125
    assert bits(r["noise"])[0] == bits(F32(1.25) / np.sqrt(F32(2.125)))[0]
    held = host.accum_resolve_host(s2, r["seen"], r["half"], r["n"], r["n_half"], r["passes"], np.zeros(1, np.uint8), o, 8)  # not active: nothing moves
    assert all((held[k] == r[k]).all() for k in ("seen", "half", "n", "n_half", "passes", "rgb", "rgba8", "noise"))
    flat = host.accum_resolve_host(np.array([[4.0, 2.0, 0.0]], F32), z3, np.array([[2.0, 1.0, 0.0]], F32), np.array([4], U32), np.array([2], U32), np.array([2], U32),
                                   np.zeros(1, np.uint8), o, 1)
    assert bits(flat["noise"])[0] == 0, "two equal halves: noise +0"
    dark = host.accum_resolve_host(np.array([[1e-3, 0.0, 0.0]], F32), z3, np.array([[1e-3, 0, 0]], F32), np.array([2], U32), np.array([1], U32), np.array([2], U32),
                                   np.zeros(1, np.uint8), o, 1)
    assert bits(dark["noise"])[0] == bits(F32(1e-3) / np.sqrt(F32(1e-2)))[0], "the brightness floor"


@pytest.mark.parametrize("cap,thr", [(0, 0.0), (32, 0.0), (0, 0.25), (32, 0.25), (1, 1e30), (0, INF)])
def test_select_twin_equals_the_restatement(host, cap, thr):
    rng = np.random.default_rng(77)
    N = 5003
    noise = rng.choice(np.array([0.0, -0.0, 0.1, 0.25, np.nextafter(F32(0.25), F32(1)), np.nextafter(F32(0.25), F32(0)), 3.0, INF, -INF, NAN, 1e30], F32), N)
    n = rng.choice(np.array([0, 1, 16, 31, 32, 33, 64, 2 ** 31 - 65537], U32), N)
    owned = (rng.random(N) < 0.8).astype(np.uint8)
    p = B.accum_default_params(max_pixel_samples=cap, noise_threshold=thr)
    got, count = host.accum_select_host(noise, n, owned, p)
    want = accum_ref.select(noise, n, owned, cap, thr)
    assert (got == want).all() and count == int(want.sum())
    own = owned != 0
    assert not got[~own].any()
    if thr == 0.25:
        assert not got[own & (noise == F32(0.25))].any(), "noise exactly at the threshold is done"
        under = own & ((n < cap) if cap else True)
        assert got[under & np.isnan(noise)].all() and got[under & (noise == INF)].all() and got[under & (noise > F32(0.25))].all()
    if cap == 32:
        assert not got[own & (n == 32)].any() and not got[own & (n == 33)].any()
        if thr == 0.0:
            assert got[own & (n == 31)].all()
    if cap == 0 and thr == 0.0:
        assert (got == owned).all()


def test_null_parameters_are_the_defaults(host):
    noise, n, owned = np.array([1.0, INF], F32), np.array([5, 5], U32), np.ones(2, np.uint8)
    a, ca = host.accum_select_host(noise, n, owned, None)
    b, cb = host.accum_select_host(noise, n, owned, B.accum_default_params())
    assert (a == b).all() and ca == cb == 2


def _upload_cube(ctx):
    sc = AC.scene("cube")
    AC.upload(ctx, sc, B)
    return AC.camera(sc, 16, 12, B.to_camera_data)


def test_refusals():
    L = B.lib()
    ctx = B.Context(-1)
    h = ctx._h
    err = lambda: L.pt_last_error(h).decode()
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    out = np.full((12, 16, 3), 7.0, F32)
    out8 = np.full((12, 16), 7, U32)
    o, o8 = out.ctypes.data_as(fp), out8.ctypes.data_as(up)
    P = lambda **kw: C.byref(B.accum_default_params(**kw))
    cam = B.Camera()
    try:
        # no context
        assert L.pt_accum_begin(None, C.byref(cam), 16, 12, 5) == PT_E_INVALID and L.pt_accum_add(None, None, o, o8) == PT_E_INVALID
        assert L.pt_accum_read(None, o, o8, None, None) == PT_E_INVALID and L.pt_accum_end(None) == PT_E_INVALID
        assert L.pt_accum_begin(h, None, 16, 12, 5) == PT_E_INVALID
        # the parameters of an add, before anything else is looked at
        for add, who in ((lambda p: L.pt_accum_add(h, p, o, o8), "pt_accum_add"), (lambda p: L.pt_accum_add_device(h, p, C.c_void_p(16), None, None), "pt_accum_add_device")):
            for kw, word in ((dict(n_samples=0), "n_samples 0 outside 1..65535"), (dict(n_samples=65536), "n_samples 65536 outside 1..65535"), (dict(n_samples=-3), "n_samples -3"),
                             (dict(max_pixel_samples=-1), "max_pixel_samples -1 is negative"), (dict(noise_threshold=-0.5), "noise_threshold -0.5 must be >= 0"),
                             (dict(noise_threshold=NAN), "noise_threshold nan must be >= 0"), (dict(reserved=1), "reserved must be 0")):
                assert add(P(**kw)) == PT_E_INVALID, (who, kw)
                assert who + ":" in err() and word in err(), (who, kw, err())
            # no scene yet
            assert add(None) == PT_E_NO_SCENE and who in err()
        assert L.pt_accum_begin(h, C.byref(cam), 16, 12, 5) == PT_E_NO_SCENE and "pt_accum_begin" in err()
        cam = _upload_cube(ctx)
        # add / read / info without a begin
        for call, who in ((lambda: L.pt_accum_add(h, None, o, o8), "pt_accum_add"), (lambda: L.pt_accum_add_device(h, None, C.c_void_p(16), None, None), "pt_accum_add_device"),
                          (lambda: L.pt_accum_read(h, o, o8, None, None), "pt_accum_read"), (lambda: L.pt_accum_info_get(h, C.byref(B.AccumInfo())), "pt_accum_info_get"),
                          (lambda: L.pt_debug_accum_state(h, None, None, None, None, None), "pt_debug_accum_state")):
            assert call() == PT_E_INVALID, who
            assert who + ":" in err() and "pt_accum_begin not called" in err(), (who, err())
        assert L.pt_accum_end(h) == 0, "PT_OK when there is none"
        # sizes pt_render refuses
        for w, hh, d in ((0, 12, 5), (16, 0, 5), (-1, 12, 5), (65536, 1, 5), (1, 65536, 5), (65535, 65535, 5), (16, 12, -1), (16, 12, 64)):
            assert L.pt_accum_begin(h, C.byref(cam), w, hh, d) == PT_E_INVALID, (w, hh, d)
            assert "pt_accum_begin: bad render size %dx%d depth %d" % (w, hh, d) in err(), err()
        # options an accumulation cannot be combined with, at begin and at an add
        for key, on, off, word in (("kernel", 1, 2, "kernel = 1"), ("latency", 1, 0, "option latency"), ("timeline", 1, 0, "option timeline")):
            ctx.set_option(key, on)
            assert L.pt_accum_begin(h, C.byref(cam), 16, 12, 5) == PT_E_INVALID and "pt_accum_begin:" in err() and word in err(), (key, err())
            assert L.pt_accum_add(h, None, o, o8) == PT_E_INVALID and "pt_accum_add:" in err() and word in err(), (key, err())
            ctx.set_option(key, off)
        # valid arguments: no CPU fallback
        assert L.pt_accum_begin(h, C.byref(cam), 16, 12, 5) == PT_E_NO_DEVICE
        assert L.pt_accum_begin(h, C.byref(cam), 65535, 1, 0) == PT_E_NO_DEVICE and L.pt_accum_begin(h, C.byref(cam), 1, 65535, 63) == PT_E_NO_DEVICE
        assert L.pt_accum_info_get(h, C.byref(B.AccumInfo())) == PT_E_INVALID, "no accumulation came of it"
        assert (out == 7.0).all() and (out8 == 7).all(), "a refused call wrote to the output"
        # the twins refuse what they cannot define
        z = np.zeros(3, F32)
        n = np.zeros(1, U32)
        b = np.ones(1, np.uint8)
        zp, npp, bp = z.ctypes.data_as(fp), n.ctypes.data_as(up), b.ctypes.data_as(C.POINTER(C.c_uint8))
        for ns in (0, 65536):
            assert L.pt_debug_accum_resolve_host(h, 1, zp, zp, zp, npp, npp, npp, bp, bp, ns, zp, npp, zp) == PT_E_INVALID and "n_samples" in err()
        assert L.pt_debug_accum_resolve_host(h, 1, None, zp, zp, npp, npp, npp, bp, bp, 1, zp, npp, zp) == PT_E_INVALID and "NULL" in err()
        assert L.pt_debug_accum_resolve_host(h, -1, zp, zp, zp, npp, npp, npp, bp, bp, 1, zp, npp, zp) == PT_E_INVALID
        assert L.pt_debug_accum_select_host(h, zp, npp, bp, 1, P(noise_threshold=NAN), bp) == PT_E_INVALID and "pt_debug_accum_select_host: noise_threshold" in err()
        assert L.pt_debug_accum_select_host(h, zp, npp, bp, 1, P(reserved=-1), bp) == PT_E_INVALID
        assert L.pt_debug_accum_select_host(h, None, npp, bp, 1, None, bp) == PT_E_INVALID
    finally:
        ctx.close()


def test_pt_main_refuses_more_adds_than_samples():
    pt_main = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
    r = subprocess.run([pt_main, "--device", "-1", "--assets", os.path.join(ROOT, "assets"), "--adds", "1000000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--adds 1000000 exceeds max_samples" in r.stderr, r.stderr[-1000:]
    for extra, word in ((["--adds", "0"], "positive"), (["--adds", "2", "--batch", "2"], "--batch"), (["--adds", "2", "--gpus", "2"], "--gpus")):
        r = subprocess.run([pt_main, "--device", "-1", "--assets", os.path.join(ROOT, "assets")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--adds" in r.stderr and word in r.stderr, r.stderr[-1000:]


def test_accum_kernels_need_no_scratch():
    """From the Makefile's own target (the flags that ship): two kernels, ScratchSize 0, no LDS."""
    rep = resource_report.resources("asm-accum")
    assert len(rep) == 2, sorted(rep)
    for stage in ("resolve", "select"):
        assert sum(("pt_accum_%s_kernel" % stage) in nm for nm in rep) == 1, sorted(rep)
    assert all(v["scratch"] == 0 and v["lds"] == 0 for v in rep.values()), rep


@pytest.mark.parametrize("target", ["asm", "asm-wt", "asm-batch"])
def test_render_kernels_are_the_parents(target):
    """The render kernel has no VGPR to spare (128 of 128): every instance of its three translation units reports what it reported before
    the accumulation existed."""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "render_kernel_resources.json")))["targets"][target]
    got = resource_report.resources(target)
    assert sorted(got) == sorted(want)
    assert sum("pt_render_" in nm for nm in want) == 5, "the product, fallback and instrumented instances"
    if target == "asm":
        assert any("pt_render_wave_kernel" in nm and v["vgprs"] == 128 and v["scratch"] == 0 for nm, v in want.items())
    for nm in want:
        assert got[nm] == want[nm], (nm, got[nm], want[nm])
