"""The variance-guided denoiser on the GPU (pt_denoise_var, pt_accum_variance, pt_accum_denoise; kernels: csrc/pt_denoise_var.hip).  Every
comparison is bit for bit.

1. pt_denoise_var == tests/denoise_var_ref.py on every case of denoise_var_common.py (37 x 23 at L = 8 makes the taps leave the frame,
   70 x 45 and 130 x 19 cross the 64-wide tile), RGBA8 included, in place, and pt_get_stats describes the filter (launches = L + 2);
   pt_denoise_var_device in place on device buffers, on a caller's stream, equals the blocking call.
2. pt_accum_variance == the twin pt_debug_accum_variance_host applied to pt_debug_accum_state.  Scene: Cornell at 40 x 30, depth 4,
   environment use_auto = 1 (test_gpu_accum's).  After one add of 2 samples every pixel is VMAX; after 2 + 3 + 2, n = 7 and n_half = 3 and
   at least half of the pixels have 0 < var < VMAX in all channels (0.79 on the oracle) - otherwise the test would show nothing; after one
   more add with a threshold at the median of the noise map pixels differ in n.
3. pt_accum_denoise == pt_denoise_var(pt_accum_read's rgb, pt_accum_variance's map, the guides of pt_render_aov at n = 1) == the twin
   chain, at 40 x 30 and 70 x 45 with both flags; pt_debug_accum_state is unchanged by the call, launches = L + 3, and one more uniform
   add still gives pt_render(N).
4. pt_accum_add_device -> pt_render_aov_device -> pt_accum_denoise_device on ONE caller's stream with no synchronize in between equals
   the blocking calls.
5. Refused by name with nothing written and the accumulation intact: without an accumulation, and with a shard of world size 2 (where
   pt_accum_variance still works: +0 outside the shard).
6. `pt_main --adds 2 --aov 1 --denoise-variance`: <name>_denoised.png decodes to pt_accum_denoise's RGBA8 image."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import aov_common as AC
import async_common as AS
import denoise_common as DC
import denoise_var_common as VC
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
VMAX = F32(1e30)
DEPTH = 4
ENV = dict(use_auto=True, intensity=1.0)
_ctx = {}


def scene():
    return dict(AC.scene("cornell"), env=ENV)


def gpu():
    """ONE context for the whole module (its stream and one caller stream stay below four hardware queues)."""
    if "ctx" not in _ctx:
        _ctx["ctx"] = B.Context(0)
        AC.upload(_ctx["ctx"], scene(), B)
        _ctx["host"] = B.Context(-1)
    return _ctx["ctx"]


def host():
    gpu()
    return _ctx["host"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    AS.destroy_streams()
    for k in ("ctx", "host"):
        if k in _ctx:
            _ctx[k].close()
    _ctx.clear()


def cam(W, H):
    return AC.camera(scene(), W, H, B.to_camera_data)


def P(n, thr=0.0):
    return B.accum_default_params(n_samples=n, noise_threshold=thr)


def same(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    ok = same(got, want)
    assert ok.all(), "%s: %d of %d floats differ" % (what, int((~ok).sum()), ok.size)


def twin_variance(st, owned=None):
    """pt_debug_accum_variance_host of a pt_debug_accum_state snapshot (framebuffer order is as good as any: the twin is per pixel)"""
    Hh, Ww = st["n"].shape
    N = Hh * Ww
    own = np.ones(N, np.uint8) if owned is None else np.ascontiguousarray(owned, np.uint8).ravel()
    rgb, var = host().accum_variance_host(st["sum"].reshape(N, 3), st["half"].reshape(N, 3), st["n"].ravel(), st["n_half"].ravel(), own)
    return rgb.reshape(Hh, Ww, 3), var.reshape(Hh, Ww, 3)


def snapshot(ctx):
    rd, st = ctx.accum_read(), ctx.accum_state()
    return [rd[k].tobytes() for k in ("rgb", "rgba8", "noise", "samples")] + [st[k].tobytes() for k in ("sum", "half", "n", "n_half", "passes")]


def grid_of(W, H):
    return ((W + 63) // 64) * ((H + 3) // 4)


@pytest.mark.parametrize("cid", VC.IDS)
def test_filter_equals_the_restatement(orc, cid):
    _, W, H = DC.case(cid)[:3]
    rgb, var, aov = VC.inputs(cid)
    want, want8, _ = VC.reference(cid)
    p = VC.params(B, cid)
    ctx = gpu()
    got, got8 = ctx.denoise_var(rgb, var, aov, p, want_rgba8=True)
    st = ctx.stats()
    DC.assert_same(got, want, "%s: GPU vs denoise_var_ref" % cid)
    assert (got8 == want8).all(), cid
    buf = np.array(rgb, F32)
    ctx.denoise_var(buf, var, aov, p, in_place=True)
    DC.assert_same(buf, want, "%s: in place" % cid)
    assert st["launches"] == p.iterations + 2 and st["kernel_ms"] > 0 and st["block"] == 256 and st["vgprs"] > 0 and st["lds_bytes"] == 0 and st["grid"] == grid_of(W, H), st


def test_filter_on_device_buffers_and_a_caller_stream(orc):
    cid = "70x45_L3_f1"
    _, W, H = DC.case(cid)[:3]
    rgb, var, aov = VC.inputs(cid)
    want, want8, _ = VC.reference(cid)
    p = VC.params(B, cid)
    ctx = gpu()
    s = AS.stream(0, nonblocking=True)
    frame, vmap, guides = AS.DeviceFrame(W, H), AS.DeviceFrame(W, H), AS.DeviceFrame(W, H, floats=8)
    try:
        AS.to_device(frame.rgb, rgb)
        AS.to_device(vmap.rgb, var)
        AS.to_device(guides.rgb, aov)
        ctx.denoise_var_device(frame.rgb, vmap.rgb, guides.rgb, W, H, frame.rgb, p, d_out_rgba8=frame.rgba8, stream=s)  # in place
        ctx.synchronize()
        got, got8 = frame.read()
        st = ctx.stats()
    finally:
        frame.free()
        vmap.free()
        guides.free()
    DC.assert_same(got, want, "pt_denoise_var_device in place on a caller's stream")
    assert (got8 == want8).all()
    assert st["launches"] == p.iterations + 2 and st["kernel_ms"] > 0, st


def test_variance_of_the_accumulation():
    W, H = 40, 30
    ctx = gpu()
    ctx.accum_begin(cam(W, H), W, H, DEPTH)
    try:
        ctx.accum_add(P(2))
        var = ctx.accum_variance()
        assert (var == VMAX).all(), "no half buffer yet: every pixel unknown"
        assert_same(var, twin_variance(ctx.accum_state())[1], "variance after one add")
        ctx.accum_add(P(3))
        ctx.accum_add(P(2))
        st = ctx.accum_state()
        assert (st["n"] == 7).all() and (st["n_half"] == 3).all()
        var = ctx.accum_variance()
        rgb_t, var_t = twin_variance(st)
        assert_same(var, var_t, "variance after 2 + 3 + 2")
        rd = ctx.accum_read()
        assert_same(rd["rgb"], rgb_t, "the twin's colour is resolve's image")
        known = ((var > 0) & (var < VMAX)).all(-1).mean()
        print("pixels with 0 < var < VMAX in every channel: %.3f" % known)
        assert known >= 0.5
        finite = rd["noise"][np.isfinite(rd["noise"]) & (rd["noise"] > 0)]
        ctx.accum_add(P(4, thr=float(np.median(finite))))
        st = ctx.accum_state()
        assert set(np.unique(st["n"])) == {7, 11}, np.unique(st["n"])
        var = ctx.accum_variance()
        assert_same(var, twin_variance(st)[1], "variance after an adaptive add: pixels differ in n")
    finally:
        ctx.accum_end()


@pytest.mark.parametrize("W,H", [(40, 30), (70, 45)])
def test_accum_denoise_against_its_parts(W, H):
    ctx = gpu()
    c = cam(W, H)
    want16, want16_8 = ctx.render(c, W, H, 16, DEPTH, want_rgba8=True)
    aov = ctx.render_aov(c, W, H, 1)
    ctx.accum_begin(c, W, H, DEPTH)
    try:
        ctx.accum_add(P(4))
        ctx.accum_add(P(6))
        before = snapshot(ctx)
        rd, st = ctx.accum_read(), ctx.accum_state()
        var = ctx.accum_variance()
        rgb_t, var_t = twin_variance(st)
        for flags in (0, 1):
            p = B.denoise_var_default_params(flags=flags)
            got, got8 = ctx.accum_denoise(aov, p, want_rgba8=True)
            stats = ctx.stats()
            assert snapshot(ctx) == before, "pt_accum_denoise changed the accumulation"
            parts, parts8 = ctx.denoise_var(rd["rgb"], var, aov, p, want_rgba8=True)
            twin, twin8, _ = host().denoise_var_host(rgb_t, var_t, aov, p, want_rgba8=True)
            assert_same(got, parts, "pt_accum_denoise vs pt_denoise_var of its parts (flags %d)" % flags)
            assert_same(got, twin, "pt_accum_denoise vs the twin chain (flags %d)" % flags)
            assert (got8 == parts8).all() and (got8 == twin8).all()
            assert (DC.bits(got) != DC.bits(rd["rgb"])).any(), "the filter must change the frame"
            assert stats["launches"] == p.iterations + 3 and stats["kernel_ms"] > 0 and stats["block"] == 256 and stats["lds_bytes"] == 0 and stats["vgprs"] > 0, stats
            assert stats["grid"] == grid_of(W, H), stats
        d0, _ = ctx.accum_denoise(aov, None)  # NULL = the filter's own defaults
        assert_same(d0, ctx.accum_denoise(aov, B.denoise_var_default_params())[0], "NULL parameters")
        rgb, rgba8 = ctx.accum_add(P(6), want_rgba8=True)
        assert_same(rgb, want16, "4 + 6 + 6 with filters in between vs pt_render(16)")
        assert (rgba8 == want16_8).all()
    finally:
        ctx.accum_end()
    again, again8 = ctx.render(c, W, H, 16, DEPTH, want_rgba8=True)
    assert_same(again, want16, "pt_render after the accumulation and its filters")
    assert (again8 == want16_8).all()


def test_add_guides_and_filter_back_to_back_on_a_caller_stream():
    W, H = 40, 30
    ctx = gpu()
    c = cam(W, H)
    ctx.accum_begin(c, W, H, DEPTH)
    try:
        ctx.accum_add(P(4))
        ctx.accum_add(P(4))
        aov = ctx.render_aov(c, W, H, 1)
        want, want8 = ctx.accum_denoise(aov, None, want_rgba8=True)
        s = AS.stream(0, nonblocking=True)
        out, guides = AS.DeviceFrame(W, H), AS.DeviceFrame(W, H, floats=8)
        try:
            ctx.accum_begin(c, W, H, DEPTH)
            ctx.accum_add_device(P(4), None, None, stream=s)
            ctx.accum_add_device(P(4), None, None, stream=s)
            ctx.render_aov_device(c, W, H, 1, guides.rgb, stream=s)
            ctx.accum_denoise_device(guides.rgb, out.rgb, None, d_out_rgba8=out.rgba8, stream=s)
            ctx.synchronize()
            got, got8 = out.read()
            got_aov, _ = guides.read()
            st = ctx.stats()
        finally:
            out.free()
            guides.free()
        AC.assert_same(got_aov, aov, "guides on the caller stream")
        assert_same(got, want, "add -> add -> guides -> filter on one caller stream vs the blocking calls")
        assert (got8 == want8).all()
        assert st["launches"] == 5 + 3, st
    finally:
        ctx.accum_end()


def test_refusals():
    L = B.lib()
    W, H = 40, 30
    ctx = gpu()
    h = ctx._h
    c = cam(W, H)
    aov = ctx.render_aov(c, W, H, 1)
    out = np.full((H, W, 3), 7.0, F32)
    out8 = np.full((H, W), 7, U32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    g, o, o8 = aov.ctypes.data_as(fp), out.ctypes.data_as(fp), out8.ctypes.data_as(up)
    dev = AS.DeviceFrame(W, H)
    guides = AS.DeviceFrame(W, H, floats=8)
    untouched = lambda: (out == 7.0).all() and (out8 == 7).all() and (dev.read()[0].view(U32) == 0xA5A5A5A5).all() and (dev.read()[1] == 0xA5A5A5A5).all()
    calls = ((lambda: L.pt_accum_denoise(h, g, None, o, o8), "pt_accum_denoise"),
             (lambda: L.pt_accum_denoise_device(h, C.c_void_p(guides.rgb), None, C.c_void_p(dev.rgb), C.c_void_p(dev.rgba8), None), "pt_accum_denoise_device"))
    try:
        ctx.accum_end()
        for call, who in calls + ((lambda: L.pt_accum_variance(h, o), "pt_accum_variance"),):
            assert call() == -1, who
            assert who + ": the context has no accumulation (pt_accum_begin not called)" in L.pt_last_error(h).decode(), L.pt_last_error(h).decode()
        ctx.synchronize()
        assert untouched()
        own = np.zeros(W * H, bool)
        own[B.shard_pixels(W, H, 8, 0, 2)] = True
        own = own.reshape(H, W)[::-1]  # launch order -> framebuffer order
        assert 0.3 < own.mean() < 0.7
        ctx.set_pixel_shard(0, 2, 8)
        try:
            ctx.accum_begin(c, W, H, DEPTH)
            ctx.accum_add(P(4))
            ctx.accum_add(P(4))
            before = snapshot(ctx)
            for call, who in calls:
                assert call() == -1, who
                err = L.pt_last_error(h).decode()
                assert who + ": the accumulation's pixel shard (0 of 2) owns" in err and "the filter needs every pixel" in err, err
            ctx.synchronize()
            assert untouched() and snapshot(ctx) == before
            var = ctx.accum_variance()  # the map itself is per shard
            assert_same(var, twin_variance(ctx.accum_state(), own)[1], "variance of a shard")
            assert (var[~own].view(U32) == 0).all() and ((var[own] > 0) & (var[own] < VMAX)).any()
            # the other refusals come after the shard's and before anything is touched
            ctx.set_pixel_shard(0, 1, 16)
            ctx.accum_begin(c, W, H, DEPTH)
            ctx.accum_add(P(4))
            ctx.accum_add(P(4))
            before = snapshot(ctx)
            assert L.pt_accum_denoise(h, None, None, o, o8) == -1 and "pt_accum_denoise: NULL aov" in L.pt_last_error(h).decode()
            assert L.pt_accum_denoise(h, g, None, None, o8) == -1 and "pt_accum_denoise: NULL out_rgb" in L.pt_last_error(h).decode()
            bad = B.denoise_var_default_params(iterations=9)
            assert L.pt_accum_denoise(h, g, C.byref(bad), o, o8) == -1 and "pt_accum_denoise: iterations 9 outside 1..8" in L.pt_last_error(h).decode()
            bad = B.denoise_var_default_params(sigma_color=0.0)
            assert L.pt_accum_denoise_device(h, C.c_void_p(guides.rgb), C.byref(bad), C.c_void_p(dev.rgb), None, None) == -1 and "sigma_color" in L.pt_last_error(h).decode()
            ctx.synchronize()
            assert untouched() and snapshot(ctx) == before
            ctx.accum_denoise(aov, None)  # ... and with valid arguments it runs
            assert snapshot(ctx) == before
        finally:
            ctx.accum_end()
            ctx.set_pixel_shard(0, 1, 16)
    finally:
        dev.free()
        guides.free()


def test_pt_main_denoise_variance_flag(tmp_path):
    from PIL import Image

    from owl_path_tracer_amd.pyhost import scene_io

    W, H = 40, 24
    a = tmp_path / "assets"
    shutil.copytree(AC.ASSETS, a)
    cfg = json.load(open(os.path.join(AC.ASSETS, "configs", "c2_cornell-box.json")))
    cfg.update(buffer_size=[W, H], max_samples=8, max_path_depth=DEPTH, environment_color=[0.3, 0.6, 0.2], environment_intensity=0.75)
    sc = scene_io.load_scene_dir(AC.ASSETS, "cornell-box")
    sphere = [m for _, m, _ in sc["materials"]][1]
    cfg["test"] = dict(name="g", material_name="sphere", attribute_name="metallic", material_type=2, values=[float(sphere[4]), float(sphere[4])], step_size=1.0)
    (a / "settings.json").write_text(json.dumps(cfg))
    base = "cornell-box_g_metallic(%.1f)" % float(sphere[4])
    d = tmp_path / "out"
    os.makedirs(d)
    pt_main = os.path.join(AC.ROOT, "owl-path-tracer_amd", "pt_main")
    r = subprocess.run([pt_main, "--assets", str(a), "--out", str(d), "--adds", "2", "--aov", "1", "--denoise-variance"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    ctx = B.Context(0)
    try:
        AC.upload(ctx, AC.scene("cornell"), B)  # the same environment (aov_common: colour (0.3, 0.6, 0.2) x 0.75)
        c = sc["camera"]
        cm = B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
        ctx.accum_begin(cm, W, H, DEPTH)
        ctx.accum_add(P(4))
        _, rgba = ctx.accum_add(P(4), want_rgba8=True)
        _, out8 = ctx.accum_denoise(ctx.render_aov(cm, W, H, 1), None, want_rgba8=True)
        ctx.accum_end()
    finally:
        ctx.close()
    png = lambda tag: np.asarray(Image.open(d / (base + tag))).view(np.uint32).reshape(H, W)
    np.testing.assert_array_equal(png(".png"), rgba)
    np.testing.assert_array_equal(png("_denoised.png"), out8)
    assert (out8 != rgba).any()
