"""The variance-guided denoiser (pt_denoise_var, pt_accum_variance, pt_accum_denoise) without a GPU.

* The eight exports are in the header and in B.EXPORTS, the ABI version is still 5, the defaults are 5, 0, 3.0, 0.25, 0.1, 0.2, and the two
  device calls are named in the header's list of asynchronous calls.
* The filter twin pt_debug_denoise_var_host == the numpy restatement tests/denoise_var_ref.py bit for bit - out_var and RGBA8 included, and
  in place - on every frame of denoise_common.CASES with a variance map of the colour's scale that holds 0, 1e-12, 1e31, +Inf, NaN and -1
  (denoise_var_common.py).  The variance twin pt_debug_accum_variance_host == the restatement on flat arrays with n_half = 0, n_half =
  n / 2, (n, n_half) = (7, 3), a sum with Inf, and pixels that are not owned.
* Every refusal by code and message, nothing written; PT_E_NO_DEVICE from the device entry points on the host-only context.
* Four properties that a mistake shared by kernel, twin and restatement would break:
  (a) a constant colour stays constant within test_denoise_host's bound (51 L 2^-24 relative: the colour sums are pt_denoise's);
  (b) variance map 0: kc_p = 1 / 1e-10 = 1e10, so a tap whose colour differs by >= 1e-2 in one channel has e >= 1e-4 * 1e10 = 1e6 and
      weight exp(-1e6) = 0: a frame whose neighbours all differ by that much comes back within 1e-6 relative;
  (c) every sigma +infinity, uniform variance V, L = 1: every tap is taken with w = h, so an interior pixel's v_1 is
      V * sum(h^2) / (sum h)^2 = V * (sum k^2)^2 = V * 0.2734375^2, within 1e-5 relative (25 fma and one division on exact weights);
  (d) variance all VMAX gives, bit for bit, the image of sigma_color = +inf (sigma_color = 1.5, colours below 1e3: ec * kc_p stays far
      below one ulp of every other non-zero term, and alone it is far below the 2^-25 under which exp_ returns exactly 1).
* Quality, figures printed: relRMSE (test_denoise_host's) against the oracle's high-sample frame at 64 x 48, depth 8, accumulations of n
  samples in two equal adds emulated on the oracle (sum = n * R(n), half = sum - n/2 * R(n/2)), the variance from
  pt_debug_accum_variance_host, default parameters without the flag.  The margins were set with the definition, from a float64 numpy draft of it:
    Cornell n = 64:  <= 0.6 x the noisy frame's and <= 0.9 x pt_debug_denoise_host's (draft 0.166 against 0.395 and 0.218);
    Cornell n = 256: <= 0.7 x the noisy frame's (0.110 against 0.189);
    ico_map n = 8 and 64: <= 0.75 x and <= 0.5 x pt_debug_denoise_host's (0.145 against 0.278, 0.065 against 0.276), and the n = 64 figure
    <= 0.6 x the n = 8 figure (0.45 in the draft): the error falls with the samples.
* `make asm-denoise-var` reports exactly four kernels and scratch 0.  `pt_main --denoise-variance` is refused without --adds or --aov."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aov_common as AC
import denoise_common as DC
import denoise_var_common as VC
import denoise_var_ref as VR
import resource_report
from owl_path_tracer_amd.pyhost import binding as B

ROOT = AC.ROOT
F32, U32 = np.float32, np.uint32
INF = float("inf")
PT_E_INVALID, PT_E_NO_DEVICE = -1, -2
NAMES = ("pt_denoise_var_default_params", "pt_denoise_var", "pt_denoise_var_device", "pt_debug_denoise_var_host", "pt_accum_variance", "pt_debug_accum_variance_host",
         "pt_accum_denoise", "pt_accum_denoise_device")


@pytest.fixture(scope="module")
def host():
    ctx = B.Context(-1)
    yield ctx
    ctx.close()


def same(a, b):
    """Bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def test_exports_abi_and_defaults():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    p = B.denoise_var_default_params()
    assert (p.iterations, p.flags) == (5, 0)
    assert [F32(x) for x in (p.sigma_color, p.sigma_normal, p.sigma_depth, p.sigma_albedo)] == [F32(3.0), F32(0.25), F32(0.1), F32(0.2)]
    assert VR.DEFAULTS == dict(iterations=5, flags=0, sigma_color=3.0, sigma_normal=0.25, sigma_depth=0.1, sigma_albedo=0.2)
    asynchronous = re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    for name in ("pt_denoise_var_device", "pt_accum_denoise_device"):
        assert name in asynchronous, name
    assert "standard deviations" in header.lower() or "STANDARD DEVIATIONS" in header


@pytest.mark.parametrize("cid", VC.IDS)
def test_filter_twin_equals_the_restatement(orc, host, cid):
    rgb, var, aov = VC.inputs(cid)
    want, want8, want_v = VC.reference(cid)
    assert np.isfinite(want).all() and (want_v >= 0).all() and (want_v <= VR.VMAX).all()
    p = VC.params(B, cid)
    got, got8, got_v = host.denoise_var_host(rgb, var, aov, p, want_rgba8=True, want_var=True)
    DC.assert_same(got, want, "%s: host twin vs denoise_var_ref" % cid)
    DC.assert_same(got_v, want_v, "%s: out_var" % cid)
    assert (got8 == want8).all(), cid
    buf = np.array(rgb, F32)  # in place: out_rgb = rgb
    res = host.denoise_var_host(buf, var, aov, p, in_place=True)
    assert res[0] is buf and res[2] is None
    DC.assert_same(buf, want, "%s: in place" % cid)
    if rgb.size > 3 and p.iterations > 1:
        assert (DC.bits(want) != DC.bits(np.where(np.isfinite(rgb), rgb, 0))).any(), "the filter must change the frame"


def test_the_cases_cover_what_they_should():
    Ls = {DC.case(c)[3]["iterations"] for c in VC.IDS}
    assert {1, 5, 8} <= Ls
    sizes = {DC.case(c)[1:3] for c in VC.IDS}
    assert (1, 1) in sizes and (130, 19) in sizes
    var = VC.var_map(37, 23, 1)
    flat = var.reshape(-1)
    assert (flat == 0).any() and (flat == F32(1e-12)).any() and (flat == F32(1e31)).any() and np.isposinf(flat).any() and np.isnan(flat).any() and (flat == -1).any()


def test_default_parameters_are_what_null_means(host):
    rgb, aov = DC.frame(21, 13, 5)
    var = VC.var_map(21, 13, 5)
    a, a8, av = host.denoise_var_host(rgb, var, aov, None, want_rgba8=True, want_var=True)
    b, b8, bv = host.denoise_var_host(rgb, var, aov, B.denoise_var_default_params(), want_rgba8=True, want_var=True)
    DC.assert_same(a, b, "NULL parameters")
    DC.assert_same(av, bv, "NULL parameters, out_var")
    assert (a8 == b8).all()
    c, _, _ = host.denoise_var_host(rgb, var, aov, B.denoise_default_params())  # pt_denoise's defaults are other parameters here
    assert (DC.bits(a) != DC.bits(c)).any()


def _flat_state(rng, N):
    """(sum, half, n, n_half, owned) with the special cases in blocks of N / 6"""
    n = rng.integers(2, 400, N).astype(U32)
    n_half = (n // 2).astype(U32)
    k = N // 6
    n_half[0:k] = 0                       # variance unknown
    n[k:2 * k], n_half[k:2 * k] = 7, 3
    mean = rng.uniform(0.0, 3.0, (N, 3))
    sum_ = (mean * n[:, None]).astype(F32)
    half = (sum_ * (n_half / np.maximum(n, 1))[:, None] + rng.standard_normal((N, 3)) * np.sqrt(np.maximum(n_half, 1))[:, None] * 0.5).astype(F32)
    sum_[2 * k:2 * k + 5, 1] = INF        # a sum with Inf
    sum_[2 * k + 5:2 * k + 9, 2] = np.nan
    half[2 * k + 9:2 * k + 12] = 1e25     # e * e overflows
    n[3 * k:3 * k + 4], n_half[3 * k:3 * k + 4] = 0, 0   # a pixel without samples
    owned = (rng.uniform(size=N) < 0.8).astype(np.uint8)
    owned[:3 * k + 4:7] = 1
    return sum_, half, n, n_half, owned


def test_variance_twin_equals_the_restatement(host):
    sum_, half, n, n_half, owned = _flat_state(np.random.default_rng(11), 600)
    want_rgb, want_var = VR.accum_variance(sum_, half, n, n_half, owned)
    rgb, var = host.accum_variance_host(sum_, half, n, n_half, owned)
    assert same(rgb, want_rgb).all() and same(var, want_var).all()
    own = owned != 0
    assert (var[own & (n_half == 0)] == VR.VMAX).all() and (var[~own].view(U32) == 0).all() and (rgb[~own].view(U32) == 0).all()
    assert not np.isnan(var).any() and (var >= 0).all() and (var <= VR.VMAX).all()
    assert (var[100 * 2 + 9:100 * 2 + 12][own[209:212]] == VR.VMAX).all()
    known = own & (n_half > 0) & np.isfinite(sum_).all(1)
    assert ((var[known] > 0) & (var[known] < VR.VMAX)).mean() > 0.9
    # the estimate means what it says: halves of n/2 samples of variance s^2 each give, on average, s^2 / n
    rng = np.random.default_rng(12)
    N, m, s = 20000, 64, 0.7
    x = rng.standard_normal((N, m, 3)) * s + 2.0
    sm, hf = x.sum(1).astype(F32), x[:, m // 2:].sum(1).astype(F32)
    _, v = host.accum_variance_host(sm, hf, np.full(N, m, U32), np.full(N, m // 2, U32), np.ones(N, np.uint8))
    assert abs(v.astype(np.float64).mean() / (s * s / m) - 1.0) < 0.05


def test_refusals(host):
    L = B.lib()
    W, H = 8, 6
    rgb = np.full((H, W, 3), 0.5, F32)
    var = np.full((H, W, 3), 0.1, F32)
    aov = np.full((H, W, 8), 0.5, F32)
    out = np.full((H, W, 3), 7.0, F32)
    out8 = np.full((H, W), 7, U32)
    outv = np.full((H, W), 7.0, F32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    r, v, g, o, o8, ov = rgb.ctypes.data_as(fp), var.ctypes.data_as(fp), aov.ctypes.data_as(fp), out.ctypes.data_as(fp), out8.ctypes.data_as(up), outv.ctypes.data_as(fp)
    P = lambda **kw: C.byref(B.denoise_var_default_params(**kw))
    h = host._h
    untouched = lambda: (out == 7.0).all() and (out8 == 7).all() and (outv == 7.0).all()

    def refused(args, word):
        assert L.pt_debug_denoise_var_host(*args) == PT_E_INVALID, word
        err = L.pt_last_error(h).decode()
        assert "pt_debug_denoise_var_host" in err and word in err, (word, err)

    assert L.pt_debug_denoise_var_host(None, r, v, g, W, H, None, o, o8, ov) == PT_E_INVALID
    refused((h, None, v, g, W, H, None, o, o8, ov), "NULL rgb")
    refused((h, r, None, g, W, H, None, o, o8, ov), "NULL var")
    refused((h, r, v, None, W, H, None, o, o8, ov), "NULL aov")
    refused((h, r, v, g, W, H, None, None, o8, ov), "NULL out_rgb")
    for w, hh in ((0, H), (W, 0), (-1, H), (W, -3), (65536, 1), (1, 65536), (65535, 65535)):
        refused((h, r, v, g, w, hh, None, o, o8, ov), "bad frame size %dx%d" % (w, hh))
    for it in (0, 9, -1):
        refused((h, r, v, g, W, H, P(iterations=it), o, o8, ov), "iterations %d outside 1..8" % it)
    for fl in (2, 3, 0x100, -2):
        refused((h, r, v, g, W, H, P(flags=fl), o, o8, ov), "unknown flag bits")
    for name in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"):
        for x in (0.0, -1.0, float("nan"), -INF):
            refused((h, r, v, g, W, H, P(**{name: x}), o, o8, ov), name)
    assert untouched(), "a refused call wrote to an output"
    # no CPU fallback behind the device entry points: valid arguments PT_E_NO_DEVICE, invalid ones PT_E_INVALID by name
    p16 = C.c_void_p(16)
    assert L.pt_denoise_var(h, r, v, g, W, H, None, o, o8) == PT_E_NO_DEVICE
    assert L.pt_denoise_var_device(h, p16, p16, p16, W, H, None, p16, None, None) == PT_E_NO_DEVICE
    assert L.pt_denoise_var(h, r, None, g, W, H, None, o, o8) == PT_E_INVALID and "pt_denoise_var: NULL var" in L.pt_last_error(h).decode()
    assert L.pt_denoise_var(h, r, v, g, W, H, P(iterations=9), o, o8) == PT_E_INVALID and "pt_denoise_var: iterations 9" in L.pt_last_error(h).decode()
    assert L.pt_denoise_var_device(h, p16, None, p16, W, H, None, p16, None, None) == PT_E_INVALID and "pt_denoise_var_device: NULL d_var" in L.pt_last_error(h).decode()
    assert L.pt_denoise_var_device(h, p16, p16, p16, 0, H, None, p16, None, None) == PT_E_INVALID
    assert L.pt_denoise_var(None, r, v, g, W, H, None, o, o8) == PT_E_INVALID
    # a host-only context has no accumulation: refused by name
    for call, who in ((lambda: L.pt_accum_denoise(h, g, None, o, o8), "pt_accum_denoise"), (lambda: L.pt_accum_denoise_device(h, p16, None, p16, None, None), "pt_accum_denoise_device"),
                      (lambda: L.pt_accum_variance(h, o), "pt_accum_variance")):
        assert call() == PT_E_INVALID, who
        assert who + ": the context has no accumulation" in L.pt_last_error(h).decode(), L.pt_last_error(h).decode()
    assert L.pt_accum_denoise(None, g, None, o, o8) == PT_E_INVALID and L.pt_accum_variance(None, o) == PT_E_INVALID
    assert untouched()
    # the variance twin
    n = np.full(4, 4, U32)
    s3 = np.zeros((4, 3), F32)
    own = np.ones(4, np.uint8)
    o3, v3 = np.full((4, 3), 7.0, F32), np.full((4, 3), 7.0, F32)
    bp = C.POINTER(C.c_uint8)
    args = [h, 4, s3.ctypes.data_as(fp), s3.ctypes.data_as(fp), n.ctypes.data_as(up), n.ctypes.data_as(up), own.ctypes.data_as(bp), o3.ctypes.data_as(fp), v3.ctypes.data_as(fp)]
    for k in range(2, 9):
        bad = list(args)
        bad[k] = None
        assert L.pt_debug_accum_variance_host(*bad) == PT_E_INVALID and "pt_debug_accum_variance_host: NULL array" in L.pt_last_error(h).decode(), k
    for cnt in (-1, 2 ** 31):
        bad = list(args)
        bad[1] = cnt
        assert L.pt_debug_accum_variance_host(*bad) == PT_E_INVALID and "n_pixels" in L.pt_last_error(h).decode()
    assert (o3 == 7.0).all() and (v3 == 7.0).all()
    assert L.pt_debug_accum_variance_host(*args) == 4
    # all of these are allowed
    assert L.pt_debug_denoise_var_host(h, r, v, g, W, H, P(sigma_color=INF, sigma_depth=INF, iterations=8, flags=1), o, None, None) == W * H
    assert np.isfinite(out).all() and (out != 7.0).all()


def _bound(L):
    return 51.0 * L * 2.0 ** -24


@pytest.mark.parametrize("L", [1, 5, 8])
def test_constant_colour_stays_constant(host, L):
    rng = np.random.default_rng(140 + L)
    W, H = 41, 27
    aov = DC.guides(rng, W, H)
    var = VC.var_map(W, H, L)
    col = np.array([0.7, 3.25, 1e-3], F32)
    rgb = np.broadcast_to(col, (H, W, 3)).copy()
    for impl in (lambda: host.denoise_var_host(rgb, var, aov, B.denoise_var_default_params(iterations=L))[0], lambda: VR.denoise_var(rgb, var, aov, iterations=L)[0]):
        out = impl().astype(np.float64)
        rel = np.abs(out - col.astype(np.float64)) / col.astype(np.float64)
        print("L = %d: largest relative deviation %.3g (bound %.3g)" % (L, rel.max(), _bound(L)))
        assert rel.max() <= _bound(L)


def test_variance_zero_keeps_pixels_that_differ_from_their_neighbours(host):
    W, H = 37, 23
    rng = np.random.default_rng(150)
    ys, xs = np.mgrid[0:H, 0:W]
    # the red channel walks through 0.5 + 0.02 * ((x + 3 y) mod 31): any two pixels within 16 steps of each other in x and y differ by >= 0.02
    # unless (dx + 3 dy) is a multiple of 31; the green one breaks those ties with 0.02 * ((5 x + y) mod 37)
    rgb = np.stack([0.5 + 0.02 * ((xs + 3 * ys) % 31), 0.5 + 0.02 * ((5 * xs + ys) % 37), np.full((H, W), 0.25)], -1).astype(F32)
    for s in (1, 2, 4, 8, 16):  # the premise: every tap of every iteration differs from its centre by >= 1e-2 in some channel
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * s, xs + dx * s
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                if (dx or dy) and inside.any():
                    d = np.abs(rgb[np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)].astype(np.float64) - rgb).max(-1)
                    assert d[inside].min() >= 1e-2, (s, dx, dy)
    aov = DC.guides(rng, W, H)
    var = np.zeros((H, W, 3), F32)
    for out in (host.denoise_var_host(rgb, var, aov, B.denoise_var_default_params())[0], VR.denoise_var(rgb, var, aov)[0]):
        rel = np.abs(out.astype(np.float64) - rgb) / rgb
        print("variance 0: largest relative change %.3g" % rel.max())
        assert rel.max() <= 1e-6


def test_uniform_variance_shrinks_by_the_kernels_own_factor(host):
    W, H, V = 19, 13, 0.37
    rgb, aov = DC.frame(W, H, 160)
    var = np.full((H, W, 3), V / 3.0, F32)
    p = dict(iterations=1, sigma_color=INF, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
    vin = float((F32(V / 3.0) + F32(V / 3.0)) + F32(V / 3.0))
    for v1 in (host.denoise_var_host(rgb, var, aov, B.denoise_var_default_params(**p), want_var=True)[2], VR.denoise_var(rgb, var, aov, **p)[2]):
        inner = v1[2:-2, 2:-2].astype(np.float64)
        rel = np.abs(inner / (vin * 0.2734375 ** 2) - 1.0)
        print("uniform variance: largest relative deviation of v_1 %.3g" % rel.max())
        assert rel.max() <= 1e-5
        assert (v1[0, 0] > v1[2, 2]), "at a corner fewer taps average"


def test_unknown_variance_is_filtered_by_the_guides_alone(host):
    cid = "37x23_L3_f0"  # not a case of CASES: its frame, L = 3
    rgb, aov = DC.frame(37, 23, 170)
    rgb = np.clip(np.where(np.isfinite(rgb), rgb, 0), -900, 900).astype(F32)
    assert np.abs(rgb).max() < 1e3
    var = np.full((37 * 23 * 3,), VR.VMAX, F32).reshape(23, 37, 3)
    for flags in (0, 1):
        a = host.denoise_var_host(rgb, var, aov, B.denoise_var_default_params(iterations=3, flags=flags, sigma_color=1.5), want_rgba8=True)
        b = host.denoise_var_host(rgb, np.zeros_like(var), aov, B.denoise_var_default_params(iterations=3, flags=flags, sigma_color=INF), want_rgba8=True)
        DC.assert_same(a[0], b[0], "variance VMAX vs sigma_color = +inf (%s, flags %d)" % (cid, flags))
        assert (a[1] == b[1]).all()
        c = VR.denoise_var(rgb, var, aov, iterations=3, flags=flags, sigma_color=1.5)
        DC.assert_same(c[0], b[0], "the restatement, variance VMAX vs sigma_color = +inf")
        assert (DC.bits(a[0]) != DC.bits(rgb)).any()


# ---- quality ------------------------------------------------------------------------------------------------------------------
QW, QH, QDEPTH = 64, 48, 8
_q = {}


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def _scene(orc, name):
    if name not in _q:
        sc = AC.scene(name)
        ctx = B.Context(-1)
        try:
            AC.upload(ctx, sc, B)
            aov = ctx.aov_host(AC.camera(sc, QW, QH, B.to_camera_data), QW, QH, 1)
        finally:
            ctx.close()
        _q[name] = dict(S=orc.Scene(sc["flat"]), cam=AC.camera(sc, QW, QH, orc.to_camera_data), env=orc.make_env(**sc["env"]), aov=aov, frames={})
    return _q[name]


def _render(orc, name, n):
    q = _scene(orc, name)
    if n not in q["frames"]:
        q["frames"][n] = q["S"].render(q["cam"], q["env"], QW, QH, n, QDEPTH)[0]
    return q["frames"][n]


def _figures(orc, host, name, n, n_ref):
    """relRMSE of (the noisy frame, pt_debug_denoise_host, pt_debug_denoise_var_host) for an accumulation of n samples in two equal adds"""
    key = (name, n)
    if key not in _q:
        q = _scene(orc, name)
        ref, full, first = _render(orc, name, n_ref), _render(orc, name, n), _render(orc, name, n // 2)
        sum_ = (F32(n) * full).astype(F32)
        half = (sum_ - (F32(n // 2) * first).astype(F32)).astype(F32)  # the samples of the second add
        N = QW * QH
        rgb, var = host.accum_variance_host(sum_.reshape(N, 3), half.reshape(N, 3), np.full(N, n, U32), np.full(N, n - n // 2, U32), np.ones(N, np.uint8))
        rgb, var = rgb.reshape(QH, QW, 3), var.reshape(QH, QW, 3)
        fixed = host.denoise_host(rgb, q["aov"], B.denoise_default_params())[0]
        guided = host.denoise_var_host(rgb, var, q["aov"], B.denoise_var_default_params())[0]
        _q[key] = (rel_rmse(rgb, ref), rel_rmse(fixed, ref), rel_rmse(guided, ref))
        print("%s n = %d: relRMSE noisy %.3f, pt_denoise %.3f, variance-guided %.3f" % ((name, n) + _q[key]))
    return _q[key]


def test_quality_cornell(orc, host):
    noisy, fixed, guided = _figures(orc, host, "cornell", 64, 2048)
    assert guided <= 0.6 * noisy and guided <= 0.9 * fixed, (noisy, fixed, guided)
    noisy, fixed, guided = _figures(orc, host, "cornell", 256, 2048)
    assert guided <= 0.7 * noisy, (noisy, fixed, guided)


def test_quality_icospheres(orc, host):
    n8, f8, g8 = _figures(orc, host, "ico_map", 8, 1024)
    n64, f64, g64 = _figures(orc, host, "ico_map", 64, 1024)
    assert g8 <= 0.75 * f8, (n8, f8, g8)
    assert g64 <= 0.5 * f64, (n64, f64, g64)
    assert g64 <= 0.6 * g8, (g8, g64)


# ---- build and tool -----------------------------------------------------------------------------------------------------------
def test_denoise_var_kernels_need_no_scratch():
    """From the Makefile's own target (the flags that ship): exactly four kernels, each with ScratchSize 0."""
    blocks = resource_report.report("asm-denoise-var")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 4, names
    for kernel in ("pt_accum_variance_kernel", "pt_denoise_var_prepare_kernel", "pt_denoise_var_iter_kernel", "pt_denoise_var_finish_kernel"):
        assert sum(kernel in nm for nm in names) == 1, names
    assert all(int(sz) == 0 for _, _, sz in blocks), blocks


def test_pt_main_refuses_denoise_variance_without_adds_or_guides():
    pt_main = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
    for extra, word in ((["--denoise-variance"], "--adds"), (["--denoise-variance", "--aov", "1"], "--adds"), (["--denoise-variance", "--aov", "1", "--adds", "1"], "--adds"),
                        (["--denoise-variance", "--adds", "2"], "--aov"), (["--denoise-variance", "--adds", "2", "--aov", "1", "--denoise"], "--denoise ")):
        r = subprocess.run([pt_main, "--device", "-1", "--assets", os.path.join(ROOT, "assets")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--denoise-variance" in r.stderr and word in r.stderr, (extra, r.stderr[-1000:])
