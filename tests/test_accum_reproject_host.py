"""Reprojection of the accumulation (pt_accum_reproject) without a GPU.  Every comparison is bit for bit unless it says otherwise.

* The four exports are in the header, the library and B.EXPORTS, the ABI version is still 5, the defaults are 0, 0, 0.05, 0.9, 0.1 and the
  device call is named in the header's list of asynchronous calls.
* The twin pt_debug_accum_reproject_host == the numpy restatement tests/accum_reproject_ref.py on synthetic frames: guides of
  denoise_common.guides (depths 1..6), a seeded state with n in 0..400 and n_half in {0, n / 2, (7, 3)}; sizes 1 x 1, 9 x 1, 40 x 30,
  70 x 45, 130 x 19; identical cameras, a 2 degree orbit, a sideways step of a third of the frame, an old camera that looks the other way
  (all reset) and, at 40 x 30, a roll by 90 degrees; max_history 0 and 4 - (7, 3) becomes (4, 1) - and (400, 1) under a cap of 2, which
  gives n_half = 0 and half = +0; the owned mask of shard 1 of 2; guides with NaN normals, +Inf depths and alpha 0 (sky to sky, sky to
  surface); each tolerance switched off in turn.
* Three properties a mistake shared by twin and restatement would break:
  (a) identical cameras, one guide buffer, no cap, finite guides: every array comes back unchanged.  It needs every pixel to map onto
      itself; a float32 numpy draft of steps 1 to 3 measured |fx - (px + 0.5)| <= 0.018 for a 40 degree Cornell-style camera, depths 0.01
      to 500 and sizes up to 1920 x 1080, so qx == px everywhere.
  (b) the new camera = the old one moved sideways by d in front of a fronto-parallel plane at distance z: every surviving pixel's source is
      round(d W / (|h| z)) columns away (+-1 at the rounding boundary) in the same row; 2.19798 columns for d = 0.1, z = 3, fov 40, W = 64.
  (c) under the cap, sum / n of a capped pixel equals the uncapped one within 2 ulp at max_history = 4 (a power of two: f = 4 fl(1 / n)
      exactly, so the two are in fact equal) and within 6 ulp at 6 and 100 (four roundings against two, each <= 2^-24 relative, an ulp
      >= 2^-24 relative), and 0 < n_half < n or n_half == 0.
* Every refusal by code and message, nothing written; the twin's refusals mirror the call's.
* `make asm-accum-reproject` reports exactly one kernel and scratch 0.
* Quality on the oracle's Cornell at 64 x 48, depth 8, environment use_auto = 1: the state at camera A emulated as sum = 32 R_A(32) with the
  half from R_A(16) (as test_denoise_var_host does), reprojected by the twin to camera B, a 2 degree orbit, with the guide twin's guides at
  n = 1; then 4 R_B(4) is added.  Against the oracle's 2048-spp frame at B, relRMSE over the pixels that kept history must be strictly
  below that of R_B(4) alone over the same pixels (the ideal ratio is sqrt(4 / 36) = 0.33), and at least half of the pixels keep history
  (the restatement alone says so).  Both figures are printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import accum_reproject_common as RC
import accum_reproject_ref as RR
import aov_common as AC
import denoise_common as DC
import resource_report
from owl_path_tracer_amd.pyhost import binding as B

ROOT = AC.ROOT
F32, U32 = np.float32, np.uint32
INF = float("inf")
PT_E_INVALID, PT_E_NO_DEVICE = -1, -2
NAMES = ("pt_accum_reproject_default_params", "pt_accum_reproject", "pt_accum_reproject_device", "pt_debug_accum_reproject_host")
VIEW = ([0.3, 0.4, 4.0], [0.0, 0.1, 0.0], [0, 1, 0], 40.0)
SIZES = [(1, 1), (9, 1), (40, 30), (70, 45), (130, 19)]
OFF = dict(depth_tol=INF, normal_min=-INF, albedo_tol=INF)


@pytest.fixture(scope="module")
def host():
    ctx = B.Context(-1)
    yield ctx
    ctx.close()


def P(**kw):
    return B.reproject_default_params(**kw)


def guides(rng, W, H, bad=False):
    """denoise_common's guides with unit normals, as the guide pass gives them (a pixel then passes the normal test against itself)"""
    g = DC.guides(rng, W, H, bad)
    g[..., 4:7] /= np.linalg.norm(g[..., 4:7].astype(np.float64), axis=-1, keepdims=True).astype(F32)
    return g


def frame(W, H, seed, bad=False):
    rng = np.random.default_rng(seed)
    return guides(rng, W, H, bad), guides(rng, W, H, bad), RC.random_state(rng, W, H)


def check(host, old, new, prev, cur, state, owned=None, params=None, what=""):
    want = RC.ref(old, new, prev, cur, state, owned, params)
    got = host.accum_reproject_host(old, new, prev, cur, state, owned, params)
    RC.assert_state(got, want, what)
    return want


def test_exports_abi_and_defaults():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    p = B.reproject_default_params()
    assert (p.max_history, p.reserved) == (0, 0)
    assert [F32(x) for x in (p.depth_tol, p.normal_min, p.albedo_tol)] == [F32(0.05), F32(0.9), F32(0.1)]
    assert RR.DEFAULTS == dict(max_history=0, reserved=0, depth_tol=0.05, normal_min=0.9, albedo_tol=0.1)
    assert C.sizeof(B.pt_reproject_params) == 20
    asynchronous = re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_accum_reproject_device" in asynchronous
    assert "No temporal stage" not in open(os.path.join(ROOT, "DESIGN.md")).read()


@pytest.mark.parametrize("cap", [0, 4])
@pytest.mark.parametrize("kind", ["identical", "orbit", "sideways", "away"])
@pytest.mark.parametrize("W,H", SIZES)
def test_twin_equals_the_restatement(orc, host, W, H, kind, cap):
    old, new = RC.pair(kind, VIEW, W, H, depth=3.5)  # (a sideways step sized for the guides' depths, 1..6)
    prev, cur, state = frame(W, H, 1000 + W + 7 * cap)
    if kind == "identical":
        cur = prev
    for name, prm in (("defaults", P(max_history=cap)), ("tests off", P(max_history=cap, **OFF))):
        want = check(host, old, new, prev, cur, state, None, prm, "%dx%d %s cap %d, %s" % (W, H, kind, cap, name))
        share = want["has"].mean()
        if kind == "away":
            assert share == 0 and (want["n"] == 0).all() and np.isposinf(want["noise"]).all()
        if kind == "identical":
            assert share == 1
        if name == "tests off" and W * H > 100:
            if kind == "orbit":
                assert 0.25 < share < 1.0, share
            if kind == "sideways":
                assert 0.05 < share < 0.95, share
        if cap == 4 and share > 0:
            seven = want["has"] & (want["n"] == 4) & (want["n_half"] == 1)
            assert (want["n"] <= 4).all() and (W * H < 100 or seven.any()), "(7, 3) must arrive as (4, 1)"


@pytest.mark.parametrize("cap", [0, 4])
def test_twin_roll_by_ninety_degrees(orc, host, cap):
    W, H = 40, 30
    old, new = RC.pair("roll", VIEW, W, H)
    prev, cur, state = frame(W, H, 77)
    want = check(host, old, new, prev, cur, state, None, P(max_history=cap, **OFF), "roll")
    # the rolled frame shows the middle 30 x 30 of the old one's 40 columns; its own outer columns look past the old frame's top and bottom
    assert 0.5 < want["has"].mean() < 0.9 and not want["has"][:, 0].any() and want["has"][:, W // 2].all()


def test_twin_cap_that_empties_the_half_buffer(orc, host):
    W, H = 40, 30
    old, new = RC.pair("orbit", VIEW, W, H)
    prev, cur, state = frame(W, H, 78)
    state["n"][:], state["n_half"][:] = 400, 1
    want = check(host, old, new, prev, cur, state, None, P(max_history=2, **OFF), "(400, 1) under a cap of 2")
    has = want["has"]
    assert has.any() and (want["n"][has] == 2).all() and (want["n_half"] == 0).all() and (want["half"].view(U32) == 0).all() and np.isposinf(want["noise"]).all()


def test_twin_with_the_mask_of_a_shard(orc, host):
    W, H = 70, 45
    own = np.zeros(W * H, np.uint8)
    own[B.shard_pixels(W, H, 8, 1, 2)] = 1
    own = np.ascontiguousarray(own.reshape(H, W)[::-1])  # launch order -> framebuffer order
    assert 0.3 < own.mean() < 0.7
    for kind in ("identical", "orbit", "sideways"):
        old, new = RC.pair(kind, VIEW, W, H, depth=3.5)
        prev, cur, state = frame(W, H, 79)
        want = check(host, old, new, prev, cur, state, own, P(**OFF), "shard 1 of 2, " + kind)
        everywhere = RC.ref(old, new, prev, cur, state, None, P(**OFF))
        assert not want["has"][own == 0].any()
        for k in RC.KEYS:
            assert (np.ascontiguousarray(want[k])[own == 0].view(U32) == 0).all(), k
        if kind != "identical":
            assert (everywhere["has"] & (own != 0) & ~want["has"]).any(), "some sources must lie in the other shard"


def test_twin_on_bad_guides_and_sky(orc, host):
    W, H = 40, 30
    prev, cur, state = frame(W, H, 80, bad=True)
    assert np.isnan(cur).any() and np.isinf(prev).any()
    cur[:8, :, 3] = 0.0    # sky in the new frame: over surface in the old one ...
    prev[:4, :, 3] = 0.0   # ... and over sky
    prev[20:24, :, 3] = 0.0  # surface in the new frame over sky in the old one
    prev[0, :5, 0] = np.nan  # a NaN albedo fails its test even between two sky pixels
    for kind in ("identical", "orbit"):
        old, new = RC.pair(kind, VIEW, W, H)
        for prm in (P(), P(**OFF)):
            want = check(host, old, new, prev, cur, state, None, prm, "bad guides, " + kind)
        if kind == "identical":  # with every test off only the classes decide - and NaN: every comparison must be TRUE
            has = want["has"]
            sc, sp = RR.is_surface(cur), RR.is_surface(prev)
            nan_normal = np.isnan(cur[..., 4:7]).any(-1) | np.isnan(prev[..., 4:7]).any(-1)
            nan_albedo = np.isnan(cur[..., 0:3]).any(-1) | np.isnan(prev[..., 0:3]).any(-1)
            assert (has == ((sc == sp) & ~nan_albedo & ~(sc & nan_normal))).all()
            for what, m in (("sky to sky", ~sc & ~sp), ("sky over surface", ~sc & sp), ("surface over sky", sc & ~sp), ("NaN normal between surfaces", sc & sp & nan_normal),
                            ("NaN albedo between skies", ~sc & ~sp & nan_albedo), ("+Inf depth makes a sky pixel", np.isinf(cur[..., 7]) & (cur[..., 3] >= 0.5))):
                assert m.any(), what


@pytest.mark.parametrize("off", ["depth_tol", "normal_min", "albedo_tol"])
def test_each_tolerance_switched_off_in_turn(orc, host, off):
    W, H = 70, 45
    old, new = RC.pair("orbit", VIEW, W, H)
    prev, cur, state = frame(W, H, 82)
    base = check(host, old, new, prev, cur, state, None, P(), "defaults")
    one = check(host, old, new, prev, cur, state, None, P(**{off: OFF[off]}), off + " off")
    assert (one["has"] | ~base["has"]).all(), "switching a test off cannot lose history"
    others = {k: v for k, v in OFF.items() if k != off}
    only = check(host, old, new, prev, cur, state, None, P(**others), "only " + off)
    free = check(host, old, new, prev, cur, state, None, P(**OFF), "all off")
    assert only["has"].sum() < free["has"].sum(), "the test alone must reject something on random guides"


# ---- properties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(40, 30), (70, 45), (130, 19), (320, 180)])
def test_identical_cameras_change_nothing(orc, host, W, H):
    rng = np.random.default_rng(90 + W)
    cam, same_cam = RC.pair("identical", ([0.0, 1.0, 3.4], [0.0, 1.0, 0.0], [0, 1, 0], 40.0), W, H)
    aov = guides(rng, W, H)
    aov[..., 7] = np.exp(rng.uniform(np.log(0.01), np.log(500.0), (H, W)))
    state = RC.random_state(rng, W, H)
    for impl in (lambda: host.accum_reproject_host(cam, same_cam, aov, aov, state, None, None), lambda: RC.ref(cam, same_cam, aov, aov, state)):
        out = impl()
        RC.assert_state(out, state, "identical cameras", RC.STATE)
    res = host.accum_resolve_host(state["sum"].reshape(-1, 3), state["sum"].reshape(-1, 3), state["half"].reshape(-1, 3), state["n"].ravel(), state["n_half"].ravel(),
                                  state["passes"].ravel(), np.zeros(W * H, np.uint8), np.ones(W * H, np.uint8), 1)
    for k in ("rgb", "rgba8", "noise"):
        assert RC.same(np.ascontiguousarray(out[k]).reshape(res[k].shape), res[k]).all(), k


def test_sideways_step_in_front_of_a_plane(orc, host):
    W, H, d, z, fov = 64, 48, 0.1, 3.0, 40.0
    frm, at = np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.0])
    old = RC.look(frm, at, [0, 1, 0], fov, W, H)
    step = np.array([d, 0.0, 0.0])
    new = RC.look(frm + step, at + step, [0, 1, 0], fov, W, H)
    hlen = float(np.linalg.norm(np.array(list(old.horizontal), np.float64)))
    shift = d * W / (hlen * z)
    print("expected shift %.5f columns" % shift)
    assert abs(shift - 2.19798) < 1e-4
    ys, xs = np.mgrid[0:H, 0:W]
    o, llc, hor, ver = old.as_array().astype(np.float64).reshape(4, 3)
    dirs = llc + hor * ((xs + 0.5) / W)[..., None] + ver * ((H - 1 - ys + 0.5) / H)[..., None] - o
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    aov = np.zeros((H, W, 8), F32)
    aov[..., 0:3] = 0.5
    aov[..., 3] = 1.0
    aov[..., 6] = 1.0
    aov[..., 7] = z / -dirs[..., 2]  # the plane z = -3: the same buffer under both cameras
    state = RC.random_state(np.random.default_rng(95), W, H)
    state["passes"] = (xs + W * ys + 1).astype(U32)  # every pixel names itself
    for out in (host.accum_reproject_host(old, new, aov, aov, state, None, None), RC.ref(old, new, aov, aov, state)):
        has = out["passes"] != 0
        src = out["passes"].astype(np.int64) - 1
        dx, dy = src % W - xs, src // W - ys
        assert (dy[has] == 0).all() and (np.abs(dx[has] - round(shift)) <= 1).all() and (dx[has] == round(shift)).mean() > 0.9
        assert has[:, :W - 4].all() and not has[:, W - 1].any(), "the columns that the step pushes out lose their history, no others"


@pytest.mark.parametrize("cap,ulps", [(4, 2), (6, 6), (100, 6)])
def test_the_cap_keeps_the_pixel_value(orc, host, cap, ulps):
    W, H = 70, 45
    cam, same_cam = RC.pair("identical", VIEW, W, H)
    rng = np.random.default_rng(96)
    aov = guides(rng, W, H)
    state = RC.random_state(rng, W, H)
    for impl in (lambda p: host.accum_reproject_host(cam, same_cam, aov, aov, state, None, p), lambda p: RC.ref(cam, same_cam, aov, aov, state, None, p)):
        free, capped = impl(P()), impl(P(max_history=cap))
        hit = state["n"] > cap
        assert hit.any() and (capped["n"][hit] == cap).all() and (capped["n"][~hit] == state["n"][~hit]).all()
        a, b = capped["rgb"][hit].astype(np.float64), free["rgb"][hit].astype(np.float64)
        err = np.abs(a - b) / np.spacing(np.abs(free["rgb"][hit]).astype(F32)).astype(np.float64)
        print("cap %d: largest deviation of sum / n %.2f ulp (bound %d)" % (cap, err.max(), ulps))
        assert err.max() <= ulps
        nh, n = capped["n_half"][hit].astype(np.int64), capped["n"][hit].astype(np.int64)
        assert (((nh > 0) & (nh < n)) | (nh == 0)).all()
        RC.assert_state({k: capped[k][~hit] for k in RC.KEYS}, {k: free[k][~hit] for k in RC.KEYS}, "pixels under the cap")


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(host):
    L = B.lib()
    W, H = 8, 6
    h = host._h
    cam, cam2 = RC.pair("orbit", VIEW, W, H)
    aov = np.full((H, W, 8), 0.5, F32)
    st = dict(sum=np.full((H, W, 3), 7.0, F32), half=np.full((H, W, 3), 7.0, F32), n=np.full((H, W), 7, U32), n_half=np.full((H, W), 7, U32), passes=np.full((H, W), 7, U32))
    out = np.full((H, W, 3), 7.0, F32)
    out8 = np.full((H, W), 7, U32)
    noise = np.full((H, W), 7.0, F32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    g = aov.ctypes.data_as(fp)
    arrays = [st["sum"].ctypes.data_as(fp), st["half"].ctypes.data_as(fp), st["n"].ctypes.data_as(up), st["n_half"].ctypes.data_as(up), st["passes"].ctypes.data_as(up),
              out.ctypes.data_as(fp), out8.ctypes.data_as(up), noise.ctypes.data_as(fp)]
    untouched = lambda: all((v == 7).all() for v in list(st.values()) + [out, out8, noise])
    c1, c2 = C.byref(cam), C.byref(cam2)
    bad_params = [(dict(reserved=1), "reserved must be 0"), (dict(max_history=1), "max_history 1"), (dict(max_history=-3), "max_history -3"), (dict(depth_tol=-0.1), "depth_tol"),
                  (dict(depth_tol=float("nan")), "depth_tol"), (dict(albedo_tol=-1.0), "albedo_tol"), (dict(albedo_tol=float("nan")), "albedo_tol"),
                  (dict(normal_min=float("nan")), "normal_min"), (dict(normal_min=1.5), "normal_min")]

    def refused(rc, who, word):
        err = L.pt_last_error(h).decode()
        assert rc == PT_E_INVALID and who in err and word in err, (rc, who, word, err)

    who = "pt_debug_accum_reproject_host"
    twin = lambda *a: L.pt_debug_accum_reproject_host(*a)
    assert twin(None, c1, c2, W, H, g, g, None, None, *arrays) == PT_E_INVALID
    refused(twin(h, None, c2, W, H, g, g, None, None, *arrays), who, "NULL old_cam")
    refused(twin(h, c1, None, W, H, g, g, None, None, *arrays), who, "NULL new_cam")
    refused(twin(h, c1, c2, W, H, None, g, None, None, *arrays), who, "NULL aov_prev")
    refused(twin(h, c1, c2, W, H, g, None, None, None, *arrays), who, "NULL aov_cur")
    for k in range(len(arrays)):
        bad = list(arrays)
        bad[k] = None
        refused(twin(h, c1, c2, W, H, g, g, None, None, *bad), who, "NULL array")
    for w, hh in ((0, H), (W, 0), (-1, H), (65536, 1), (1, 65536), (65535, 65535)):
        refused(twin(h, c1, c2, w, hh, g, g, None, None, *arrays), who, "bad frame size %dx%d" % (w, hh))
    for kw, word in bad_params:
        refused(twin(h, c1, c2, W, H, g, g, None, C.byref(P(**kw)), *arrays), who, word)
    assert untouched(), "a refused call wrote to an array"
    # the calls: a host-only context holds no accumulation, so the arguments alone are judged - valid ones meet PT_E_NO_DEVICE
    p16 = C.c_void_p(16)
    for who, call in (("pt_accum_reproject", lambda cam_, a, b, p: L.pt_accum_reproject(h, cam_, a, b, p)),
                      ("pt_accum_reproject_device", lambda cam_, a, b, p: L.pt_accum_reproject_device(h, cam_, p16 if a else None, p16 if b else None, p, None))):
        refused(call(None, g, g, None), who + ":", "NULL new_cam")
        refused(call(c2, None, g, None), who + ":", "NULL aov_prev")
        refused(call(c2, g, None, None), who + ":", "NULL aov_cur")
        for kw, word in bad_params:
            refused(call(c2, g, g, C.byref(P(**kw))), who + ":", word)
        assert call(c2, g, g, None) == PT_E_NO_DEVICE
        assert call(c2, g, g, C.byref(P(max_history=2, **OFF))) == PT_E_NO_DEVICE
    assert L.pt_accum_reproject(None, c2, g, g, None) == PT_E_INVALID and L.pt_accum_reproject_device(None, c2, p16, p16, None, None) == PT_E_INVALID
    assert untouched()
    # all of these are allowed
    assert twin(h, c1, c2, W, H, g, g, None, C.byref(P(max_history=2, depth_tol=0.0, normal_min=-INF, albedo_tol=0.0)), *arrays) == W * H
    assert twin(h, c1, c2, W, H, g, g, None, C.byref(P(normal_min=1.0, **{k: v for k, v in OFF.items() if k != "normal_min"})), *arrays) == W * H


# ---- build --------------------------------------------------------------------------------------------------------------------
def test_reproject_kernel_needs_no_scratch():
    """From the Makefile's own target (the flags that ship): exactly one kernel, ScratchSize 0."""
    blocks = resource_report.report("asm-accum-reproject")[1]
    assert len(blocks) == 1 and "pt_accum_reproject_kernel" in blocks[0][0], blocks
    assert int(blocks[0][2]) == 0, blocks
    print("pt_accum_reproject_kernel: %s VGPRs" % blocks[0][1])


# ---- quality ------------------------------------------------------------------------------------------------------------------
QW, QH, QDEPTH = 64, 48, 8
ENV = dict(use_auto=True, intensity=1.0)


def rel_rmse(x, ref, mask):
    x, ref = x.astype(np.float64)[mask], ref.astype(np.float64)[mask]
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def test_quality_history_helps_after_an_orbit(orc, host):
    sc = dict(AC.scene("cornell"), env=ENV)
    frm, at, up, fov = sc["camera"]
    view = (frm, at, up, fov)
    cam_a, cam_b = RC.pair("orbit", view, QW, QH)
    ctx = B.Context(-1)
    try:
        AC.upload(ctx, sc, B)
        aov_a, aov_b = ctx.aov_host(cam_a, QW, QH, 1), ctx.aov_host(cam_b, QW, QH, 1)
    finally:
        ctx.close()
    S, env = orc.Scene(sc["flat"]), orc.make_env(**ENV)
    oa, ob = orc.camera_from_array(cam_a.as_array()), orc.camera_from_array(cam_b.as_array())
    render = lambda cam, n: S.render(cam, env, QW, QH, n, QDEPTH)[0]
    ra32, ra16, rb4, ref = render(oa, 32), render(oa, 16), render(ob, 4), render(ob, 2048)
    sum_ = (F32(32) * ra32).astype(F32)
    half = (sum_ - (F32(16) * ra16).astype(F32)).astype(F32)  # the samples of the second add
    full = lambda v: np.full((QH, QW), v, U32)
    state = dict(sum=sum_, half=half, n=full(32), n_half=full(16), passes=full(2))
    want = RC.ref(cam_a, cam_b, aov_a, aov_b, state)
    share = float(want["has"].mean())
    assert share >= 0.5, "the restatement alone: %.3f of the pixels keep history" % share
    moved = host.accum_reproject_host(cam_a, cam_b, aov_a, aov_b, state, None, None)
    RC.assert_state(moved, want, "the twin on the oracle's frames")
    kept = moved["n"] == 32
    assert (kept == want["has"]).all()
    total = (moved["sum"] + (F32(4) * rb4).astype(F32)).astype(F32) / (moved["n"] + U32(4)).astype(F32)[..., None]
    with_history, alone = rel_rmse(total, ref, kept), rel_rmse(rb4, ref, kept)
    print("history kept by %.3f of the pixels; relRMSE over them: 4 spp alone %.4f, 32 reprojected + 4: %.4f (ratio %.3f; ideal 0.333)" % (
        share, alone, with_history, with_history / alone))
    assert with_history < alone
