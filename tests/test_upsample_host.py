"""The upsampling (pt_upsample: joint bilateral upsampling of a low-resolution frame under full-resolution guides) without a GPU.

* The five exports exist in the header, the library and EXPORTS, the ABI version is still 5, the default parameters are the header's,
  the struct is 24 bytes, pt_upsample_device is in the header's list of asynchronous calls.
* The CPU twin pt_debug_upsample_host == the numpy restatement tests/upsample_ref.py bit for bit on every case of upsample_common.py
  (NaNs compared as NaNs: by their bits), out_rgba8 included; both branches of step 5 are taken.
* Every refusal by code and message, nothing written; pt_upsample / pt_upsample_device on a host-only context: PT_E_NO_DEVICE.
* `make asm-upsample`: no kernel needs scratch.  `pt_main --upsample` without --aov, or with --batch, is refused.
* Properties that a mistake shared by kernel, twin and restatement would break:
  (a) a constant colour comes back within a relative (2 taps^2 + 2) 2^-24 without the flag: at most taps^2 fma and taps^2 additions
      form the two sums, the product b = bx * by perturbs numerator and denominator alike, and one division;
  (b) without the flag every output component lies inside the range of that component over the (sanitised) input, widened by the same
      bound relative to the range's largest magnitude (a weighted mean with positive weights);
  (c) every sigma at +infinity, flag 0, taps 2: plain bilinear interpolation (float64, edge pixels repeated) within 4 x 2^-24 of the
      largest input magnitude;
  (d) equal sizes, identical guides, flag 0, taps 2: the sanitised input bit for bit (+ 0.0f: the one fma turns a -0.0f into +0.0f);
  (e) two half-planes with perpendicular normals and different constant colours, the edge on a low-pixel boundary, W = 2 w: en = 2,
      kn = 16, so a tap across the edge weighs at most e^-32 = 1.3e-14 of its tent weight and each side keeps its colour within 1e-6.
* Quality on the oracle's frames: aov_common's Cornell and textured cube, 32 x 24 at 256 spp -> 64 x 48, depth 8, guides from
  pt_debug_aov_host at n = 4 at both sizes, against the oracle's 1024-spp frame at 64 x 48: relRMSE of the twin at the defaults
  <= 0.8 x (Cornell) and <= 0.65 x (cube) that of the same twin as plain bilinear (every sigma +inf, flag 0, taps 2).  A numpy draft of
  the definition gave: Cornell bilinear 0.585, defaults 0.369, taps 2 0.429; cube bilinear 0.131, defaults 0.062, taps 2 0.066."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import aov_common as AC
import denoise_common as DC
import resource_report
import upsample_common as UC
import upsample_ref
from owl_path_tracer_amd.pyhost import binding as B

ROOT = AC.ROOT
F32 = np.float32
INF = float("inf")
PT_E_INVALID, PT_E_NO_DEVICE = -1, -2
NAMES = ("pt_upsample_default_params", "pt_upsample", "pt_upsample_device", "pt_debug_upsample_host")
BILINEAR = dict(taps=2, flags=0, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)


@pytest.fixture(scope="module")
def host():
    ctx = B.Context(-1)
    yield ctx
    ctx.close()


def test_exports_abi_and_defaults():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert L.pt_abi_version() == 5
    p = B.upsample_default_params()
    assert (p.taps, p.flags, p.reserved) == (4, B.PT_UPSAMPLE_DEMODULATE, 0) and B.PT_UPSAMPLE_DEMODULATE == 1
    assert [F32(x) for x in (p.sigma_normal, p.sigma_depth, p.sigma_albedo)] == [F32(0.25), F32(0.1), F32(0.2)]
    assert C.sizeof(B.UpsampleParams) == 24
    assert re.search(r"#define PT_UPSAMPLE_DEMODULATE 1\b", header)
    assert "pt_upsample_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_upsample_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)


@pytest.mark.parametrize("cid", UC.IDS)
def test_host_twin_equals_the_restatement(orc, host, cid):
    rgb, g_lo, g_hi = UC.inputs(cid)
    want, want8 = UC.reference(cid)
    p = UC.params(B, cid)
    got, got8 = host.upsample_host(rgb, g_lo, g_hi, p, want_rgba8=True)
    UC.assert_same(got, want, "%s: host twin vs upsample_ref" % cid)
    assert (got8 == want8).all(), cid
    if "badguides" not in cid:
        assert np.isfinite(want).all()


def test_both_branches_of_step_5_are_taken(orc):
    for cid in UC.IDS:
        UC.reference(cid)
    guided = [cid for cid in UC.IDS if UC.BRANCHES[cid]["guided"] > 0]
    fallback = [cid for cid in UC.IDS if UC.BRANCHES[cid]["fallback"] > 0 and "badguides" not in cid]
    print("guided in %d cases, fallback (finite guides) in %d: %s" % (len(guided), len(fallback), [(c, UC.BRANCHES[c]["fallback"]) for c in fallback][:6]))
    assert guided and fallback
    assert any(UC.BRANCHES[cid]["fallback"] > 0 for cid in UC.IDS if "badguides" in cid)


def test_default_parameters_are_what_null_means(host):
    rgb, g_lo, g_hi = UC.frame(11, 7, 21, 13, 5)
    a, a8 = host.upsample_host(rgb, g_lo, g_hi, None, want_rgba8=True)
    b, b8 = host.upsample_host(rgb, g_lo, g_hi, B.upsample_default_params(), want_rgba8=True)
    UC.assert_same(a, b, "NULL parameters")
    assert (a8 == b8).all()


def test_refusals(host):
    L = B.lib()
    w, h, W, H = 4, 3, 8, 6
    rgb = np.full((h, w, 3), 0.5, F32)
    g_lo = np.full((h, w, 8), 0.5, F32)
    g_hi = np.full((H, W, 8), 0.5, F32)
    out = np.full((H, W, 3), 7.0, F32)
    out8 = np.full((H, W), 7, np.uint32)
    fp = C.POINTER(C.c_float)
    r, gl, gh, o, o8 = rgb.ctypes.data_as(fp), g_lo.ctypes.data_as(fp), g_hi.ctypes.data_as(fp), out.ctypes.data_as(fp), out8.ctypes.data_as(C.POINTER(C.c_uint32))
    P = lambda **kw: C.byref(B.upsample_default_params(**kw))
    hd = host._h

    def refused(args, word):
        assert L.pt_debug_upsample_host(*args) == PT_E_INVALID, word
        msg = L.pt_last_error(hd).decode()
        assert word in msg and "pt_debug_upsample_host" in msg, (word, msg)

    assert L.pt_debug_upsample_host(None, r, gl, w, h, gh, W, H, None, o, o8) == PT_E_INVALID
    refused((hd, None, gl, w, h, gh, W, H, None, o, o8), "NULL rgb_lo")
    refused((hd, r, None, w, h, gh, W, H, None, o, o8), "NULL aov_lo")
    refused((hd, r, gl, w, h, None, W, H, None, o, o8), "NULL aov_hi")
    refused((hd, r, gl, w, h, gh, W, H, None, None, o8), "NULL out_rgb")
    for ww, hh in ((0, h), (w, 0), (-1, h), (w, -3), (65536, 1), (1, 65536)):
        refused((hd, r, gl, ww, hh, gh, W, H, None, o, o8), "bad low frame size %dx%d" % (ww, hh))
    for WW, HH in ((0, H), (W, 0), (-1, H), (W, -3), (65536, 8), (8, 65536), (65535, 65535)):
        refused((hd, r, gl, w, h, gh, WW, HH, None, o, o8), "bad frame size %dx%d" % (WW, HH))
    refused((hd, r, gl, W + 1, h, gh, W, H, None, o, o8), "is larger than the frame")
    refused((hd, r, gl, w, H + 1, gh, W, H, None, o, o8), "is larger than the frame")
    for t in (0, 1, 3, 5, 8, -2):
        refused((hd, r, gl, w, h, gh, W, H, P(taps=t), o, o8), "taps %d is not 2 or 4" % t)
    for fl in (2, 3, 0x100, -2):
        refused((hd, r, gl, w, h, gh, W, H, P(flags=fl), o, o8), "unknown flag bits")
    for name in ("sigma_normal", "sigma_depth", "sigma_albedo"):
        for v in (0.0, -1.0, float("nan"), -INF):
            refused((hd, r, gl, w, h, gh, W, H, P(**{name: v}), o, o8), name)
    for v in (1, -1):
        refused((hd, r, gl, w, h, gh, W, H, P(reserved=v), o, o8), "reserved")
    assert (out == 7.0).all() and (out8 == 7).all(), "a refused call wrote to the output"
    # no CPU fallback behind the device entry points: valid arguments PT_E_NO_DEVICE, invalid ones PT_E_INVALID by name
    v16 = C.c_void_p(16)
    assert L.pt_upsample(hd, r, gl, w, h, gh, W, H, None, o, o8) == PT_E_NO_DEVICE
    assert L.pt_upsample_device(hd, v16, v16, w, h, v16, W, H, None, v16, None, None) == PT_E_NO_DEVICE
    assert L.pt_upsample(hd, None, gl, w, h, gh, W, H, None, o, o8) == PT_E_INVALID and "pt_upsample: NULL rgb_lo" in L.pt_last_error(hd).decode()
    assert L.pt_upsample(hd, r, gl, w, h, gh, W, H, P(taps=3), o, o8) == PT_E_INVALID and "pt_upsample: taps 3" in L.pt_last_error(hd).decode()
    assert L.pt_upsample_device(hd, v16, None, w, h, v16, W, H, None, v16, None, None) == PT_E_INVALID and "pt_upsample_device: NULL d_aov_lo" in L.pt_last_error(hd).decode()
    assert L.pt_upsample_device(hd, v16, v16, W + 1, h, v16, W, H, None, v16, None, None) == PT_E_INVALID and "pt_upsample_device" in L.pt_last_error(hd).decode()
    assert L.pt_upsample(None, r, gl, w, h, gh, W, H, None, o, o8) == PT_E_INVALID
    assert (out == 7.0).all() and (out8 == 7).all()
    assert L.pt_debug_upsample_host(hd, r, gl, w, h, gh, W, H, P(sigma_depth=INF, taps=2, flags=1), o, None) == W * H  # all of these are allowed
    assert np.isfinite(out).all() and (out != 7.0).all()


def test_upsample_kernels_need_no_scratch():
    """From the Makefile's own target (the flags that ship): the two kernels report ScratchSize 0."""
    blocks = resource_report.report("asm-upsample")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 2, names
    assert sum("pt_upsample_prepare_kernel" in nm for nm in names) == 1 and sum("pt_upsample_kernel" in nm for nm in names) == 1, names
    assert all(int(sz) == 0 for _, _, sz in blocks), blocks


def test_pt_main_refuses_upsample_without_guides_or_with_a_batch():
    pt_main = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
    for extra, word in ((["--upsample", "2"], "--aov"), (["--aov", "1", "--upsample", "2", "--batch", "2"], "--batch"), (["--aov", "1", "--upsample", "9"], "2..8"),
                        (["--aov", "1", "--upsample", "1"], "2..8")):
        r = subprocess.run([pt_main, "--device", "-1", "--assets", os.path.join(ROOT, "assets")] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--upsample" in r.stderr and word in r.stderr, r.stderr[-1000:]


def _bound(taps):
    return (2.0 * taps * taps + 2.0) * 2.0 ** -24


@pytest.mark.parametrize("taps", [2, 4])
def test_constant_colour_stays_constant(orc, host, taps):
    rng = np.random.default_rng(40 + taps)
    w, h, W, H = 17, 11, 41, 27
    g_hi = DC.guides(rng, W, H)
    g_lo = UC.low_guides(rng, g_hi, w, h)
    col = np.array([0.7, 3.25, 1e-3], F32)
    rgb = np.broadcast_to(col, (h, w, 3)).copy()
    for impl in (lambda: host.upsample_host(rgb, g_lo, g_hi, B.upsample_default_params(taps=taps, flags=0))[0],
                 lambda: upsample_ref.upsample(rgb, g_lo, g_hi, taps=taps, flags=0)[0]):
        out = impl().astype(np.float64)
        rel = np.abs(out - col.astype(np.float64)) / col.astype(np.float64)
        print("taps = %d: largest relative deviation %.3g (bound %.3g)" % (taps, rel.max(), _bound(taps)))
        assert rel.max() <= _bound(taps)


@pytest.mark.parametrize("cid", [c for c in UC.IDS if "_f0" in c])
def test_output_stays_inside_the_input_range(host, cid):
    rgb, g_lo, g_hi = UC.inputs(cid)
    p = UC.params(B, cid)
    out, _ = host.upsample_host(rgb, g_lo, g_hi, p)
    clean = np.where(np.isfinite(rgb), rgb, F32(0.0)).astype(np.float64)
    for k in range(3):
        lo, hi = clean[..., k].min(), clean[..., k].max()
        slack = _bound(p.taps) * max(abs(lo), abs(hi))
        assert lo - slack <= out[..., k].min() and out[..., k].max() <= hi + slack, (cid, k, lo, hi, out[..., k].min(), out[..., k].max())


def _bilinear64(c, W, H):
    """Plain bilinear interpolation of c (h, w, 3) to W x H in float64, edge pixels repeated.  The sample positions are the definition's
    (step 2, in float32: they are part of it, and a position off by x * 2^-24 moves the value by more than the bound on the arithmetic);
    everything from tx, ty on is float64."""
    h, w = c.shape[:2]
    c = c.astype(np.float64)
    fx = ((np.arange(W).astype(F32) + F32(0.5)) * (F32(w) / F32(W)) - F32(0.5)).astype(np.float64)
    fy = ((np.arange(H).astype(F32) + F32(0.5)) * (F32(h) / F32(H)) - F32(0.5)).astype(np.float64)
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    tx, ty = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    top = c[ya][:, xa] * (1 - tx) + c[ya][:, xb] * tx
    bot = c[yb][:, xa] * (1 - tx) + c[yb][:, xb] * tx
    return top * (1 - ty) + bot * ty


@pytest.mark.parametrize("size", [(20, 15, 50, 37), (35, 23, 70, 45), (9, 1, 37, 1), (3, 2, 7, 5)])
def test_every_sigma_off_is_bilinear_interpolation(orc, host, size):
    w, h, W, H = size
    rng = np.random.default_rng(900 + W)
    g_hi = DC.guides(rng, W, H)
    g_lo = UC.low_guides(rng, g_hi, w, h)
    rgb = rng.uniform(-3.0, 3.0, (h, w, 3)).astype(F32)
    want = _bilinear64(rgb, W, H)
    scale = float(np.abs(rgb).max())
    for out in (host.upsample_host(rgb, g_lo, g_hi, B.upsample_default_params(**BILINEAR))[0], upsample_ref.upsample(rgb, g_lo, g_hi, **BILINEAR)[0]):
        err = np.abs(out.astype(np.float64) - want).max() / scale
        print("%dx%d -> %dx%d: largest deviation from float64 bilinear %.3g of the largest input (bound %.3g)" % (w, h, W, H, err, 4 * 2.0 ** -24))
        assert err <= 4 * 2.0 ** -24


@pytest.mark.parametrize("cid", ["37x23_to_37x23_t2_f0", "1x1_to_1x1_t2_f0"])
def test_equal_sizes_and_identical_guides_give_the_input_back(host, cid):
    rgb, _, g_hi = UC.inputs(cid)
    out, out8 = host.upsample_host(rgb, g_hi, g_hi, UC.params(B, cid), want_rgba8=True)
    clean = np.where(np.isfinite(rgb), rgb, F32(0.0)).astype(F32) + F32(0.0)  # (-0.0f -> +0.0f: fma_(1, c, +0))
    UC.assert_same(out, clean, "identity")
    assert (out8 == upsample_ref.make_rgba(clean)).all()


def test_an_edge_in_the_normals_is_kept(orc, host):
    w, h, W, H = 24, 10, 48, 20
    a, b = np.array([0.9, 0.2, 0.4], F32), np.array([0.1, 0.6, 2.0], F32)

    def planes(n_x, n_y, edge):
        left = np.arange(n_x) < edge
        g = np.zeros((n_y, n_x, 8), F32)
        g[..., 0:3] = 0.5
        g[..., 3] = 1.0
        g[:, left, 4:7], g[:, ~left, 4:7] = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
        g[..., 7] = 2.0
        return g, left

    g_lo, left_lo = planes(w, h, 10)
    g_hi, left = planes(W, H, 20)
    rgb = np.zeros((h, w, 3), F32)
    rgb[:, left_lo], rgb[:, ~left_lo] = a, b
    for taps in (2, 4):
        for flags in (0, 1):
            for out in (host.upsample_host(rgb, g_lo, g_hi, B.upsample_default_params(taps=taps, flags=flags))[0], upsample_ref.upsample(rgb, g_lo, g_hi, taps=taps, flags=flags)[0]):
                for side, colour in ((left, a), (~left, b)):
                    rel = np.abs(out[:, side].astype(np.float64) - colour) / colour
                    assert rel.max() <= 1e-6, (taps, flags, rel.max())


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


@pytest.mark.parametrize("name,factor,draft", [("cornell", 0.8, (0.585, 0.369, 0.429)), ("cube", 0.65, (0.131, 0.062, 0.066))])
def test_quality_against_the_high_sample_frame(orc, host, name, factor, draft):
    w, h, W, H = 32, 24, 64, 48
    sc = AC.scene(name)
    S = orc.Scene(sc["flat"])
    cam = AC.camera(sc, W, H, orc.to_camera_data)  # ONE camera for both sizes
    env = orc.make_env(**sc["env"])
    lo, _, _ = S.render(cam, env, w, h, 256, 8)
    ref, _, _ = S.render(cam, env, W, H, 1024, 8)
    ctx = B.Context(-1)
    try:
        AC.upload(ctx, sc, B)
        bcam = AC.camera(sc, W, H, B.to_camera_data)
        g_lo, g_hi = ctx.aov_host(bcam, w, h, 4), ctx.aov_host(bcam, W, H, 4)
    finally:
        ctx.close()
    bil = rel_rmse(host.upsample_host(lo, g_lo, g_hi, B.upsample_default_params(**BILINEAR))[0], ref)
    dflt = rel_rmse(host.upsample_host(lo, g_lo, g_hi, None)[0], ref)
    taps2 = rel_rmse(host.upsample_host(lo, g_lo, g_hi, B.upsample_default_params(taps=2))[0], ref)
    print("%s: relRMSE bilinear %.3f, defaults %.3f, taps 2 %.3f (the draft: %.3f, %.3f, %.3f)" % ((name, bil, dflt, taps2) + draft))
    assert dflt <= factor * bil, (bil, dflt)
