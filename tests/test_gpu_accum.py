"""Progressive accumulation on the GPU (pt_accum_*; kernels: csrc/pt_accum.hip, render path: csrc/pt_render.cpp accum_frame).  Every comparison
is bit for bit.  Scene: Cornell at 37 x 23 (partial 8 x 8 blocks on both axes), depth 5, environment use_auto = 1, intensity = 1 (with the
black environment 84 % of the pixels of this view are exactly 0 and have noise 0).

1. Uniform adds of 5, 27 and 96 samples (unsorted, unsorted, sorted schedule with its pre-pass): after each, rgb and rgba8 equal pt_render
   at 5, 32 and 128 on the same context, and the last one the oracle.  With "watertight" = 1: 8 + 24 against 32.
2. A pt_render of another size and camera, a pt_render_aov_follow and a pt_denoise between those adds: the accumulation's results do not
   change, and the three calls return what they return on a fresh context.
3. After every add of 8, 8, 16, 16: `half` of pt_debug_accum_state equals the recomputation from the successive `sum` snapshots, noise and
   image equal tests/accum_ref.py of the raw state; the noise map after add 1 is all +inf.
4. Adaptive adds: threshold = the median of the finite noise values > 0 after two uniform adds of 8, then three adds of 16.  The first
   adaptive add holds between a quarter and three quarters of the pixels (emulated on the CPU from the oracle's 8- and 16-spp frames:
   49.8 %); each add's sample-map delta equals the select definition applied to the previous noise map; for every distinct count of the
   final sample map those pixels equal the oracle's render(pixel_list=...) at that count.  A cap of 32 stops every pixel at 32.  A
   threshold of 1e30 after the second add: PT_OK, launches == 0, outputs unchanged.
5. Rank 1 of 3, tile 8: owned pixels equal the unsharded accumulation's, the others are +0 in all four outputs; changing the shard after
   begin makes the next add PT_E_INVALID.
6. pt_accum_add_device on a caller's stream, at once pt_render_device on another stream, then pt_accum_read, no pt_synchronize between.
7. `pt_main --adds 3` writes byte for byte the files `pt_main` writes (37 samples: 12 + 12 + 13), also with --watertight --aov 1 --denoise.
8. The refusals that need an accumulation: a pixel's n about to pass 2^31 - 65536 (reached with 32767 adds of 65535 samples whose active
   set is empty: every pixel is at its cap, so no render kernel runs), a new scene after begin, and every call on a context with a
   communicator (world 1; that leg is not built).  A refused add leaves state and outputs as they were."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import accum_ref
import aov_common as AC
import async_common as AS
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W, H, DEPTH = 37, 23, 5
W2, H2 = 29, 31  # the other frame of the interleaving and stream tests
ENV = dict(use_auto=True, intensity=1.0)
_ctx = {}
_ref = {}


def scene():
    return dict(AC.scene("cornell"), env=ENV)


def gpu():
    """ONE context for the whole module (its stream and two caller streams stay below four hardware queues)."""
    if "ctx" not in _ctx:
        _ctx["ctx"] = B.Context(0)
        AC.upload(_ctx["ctx"], scene(), B)
    return _ctx["ctx"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    AS.destroy_streams()
    if "ctx" in _ctx:
        _ctx["ctx"].close()
    _ctx.clear()
    _ref.clear()


def cam():
    return AC.camera(scene(), W, H, B.to_camera_data)


def cam2():
    return AC.camera(AC.scene("cornell_cross"), W2, H2, B.to_camera_data)


def same(a, b):
    """Bit for bit, any NaN equal to any NaN (which NaN an operation yields is the machine's choice; the definition never looks)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    ok = same(got, want)
    assert ok.all(), "%s: %d of %d floats differ" % (what, int((~ok).sum()), ok.size)


def rendered(n, wt=0):
    """pt_render at n samples on the module's context, once (no accumulation may be between its begin and end when this renders: the
    interleaving test is the one that checks that)."""
    if (n, wt) not in _ref:
        ctx = gpu()
        ctx.set_option("watertight", wt)
        try:
            rgb, rgba8 = ctx.render(cam(), W, H, n, DEPTH, want_rgba8=True)
        finally:
            ctx.set_option("watertight", 0)
        rgb.setflags(write=False)
        rgba8.setflags(write=False)
        _ref[(n, wt)] = (rgb, rgba8)
    return _ref[(n, wt)]


def oracle_scene(orc, wt=False):
    if ("orc", wt) not in _ref:
        _ref[("orc", wt)] = orc.Scene(scene()["flat"], watertight=wt)
    return _ref[("orc", wt)]


def oracle_render(orc, n, pixel_list=None):
    S = oracle_scene(orc)
    rgb, rgba8, _ = S.render(orc.camera_from_array(cam().as_array()), orc.make_env(**ENV), W, H, n, DEPTH, pixel_list=pixel_list, want_rgba8=True)
    return rgb, rgba8


def P(n, cap=0, thr=0.0):
    return B.accum_default_params(n_samples=n, max_pixel_samples=cap, noise_threshold=thr)


def test_uniform_adds(orc):
    for n in (5, 32, 128):
        rendered(n)
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    try:
        total = 0
        for k, (n, launches, sorted_) in enumerate(((5, 1, False), (27, 1, False), (96, 2, True))):
            rgb, rgba8 = ctx.accum_add(P(n), want_rgba8=True)
            st = ctx.stats()
            total += n
            want, want8 = rendered(total)
            assert_same(rgb, want, "after %d samples" % total)
            assert (rgba8 == want8).all(), total
            assert st["launches"] == launches and (st["prepass_spp"] > 0) == sorted_ and st["kernel_ms"] > 0 and st["vgprs"] > 0, st
            info = ctx.accum_info()
            assert (info["adds"], info["owned_pixels"], info["active_pixels"], info["samples_total"]) == (k + 1, W * H, W * H, total * W * H), info
            assert (info["width"], info["height"], info["max_path_depth"]) == (W, H, DEPTH)
        r = ctx.accum_read()
        assert (r["samples"] == 128).all()
        assert_same(r["rgb"], rgb, "pt_accum_read")
        assert (r["rgba8"] == rgba8).all()
    finally:
        ctx.accum_end()
    want, want8 = oracle_render(orc, 128)
    assert_same(rgb, want, "128 samples in three adds vs the oracle")
    assert (rgba8 == want8).all()
    assert (want > 0).mean() > 0.9, "the environment lights the view: (nearly) no pixel is exactly 0"


def test_uniform_adds_watertight():
    want, want8 = rendered(32, wt=1)
    ctx = gpu()
    ctx.set_option("watertight", 1)
    try:
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add(P(8))
        rgb, rgba8 = ctx.accum_add(P(24), want_rgba8=True)
        assert_same(rgb, want, "watertight 8 + 24")
        assert (rgba8 == want8).all()
    finally:
        ctx.accum_end()
        ctx.set_option("watertight", 0)


def _fresh():
    """What the interleaved calls return on a context that never held an accumulation: the 29 x 31 frame from the cross camera, the follow
    guides of the accumulation's view and the denoised 5-sample frame."""
    if "fresh" not in _ref:
        rgb5 = rendered(5)[0]
        ctx = B.Context(0)
        try:
            AC.upload(ctx, scene(), B)
            other = ctx.render(cam2(), W2, H2, 8, 7, want_rgba8=True)
            guides = ctx.render_aov_follow(cam(), W, H)
            clean = ctx.denoise(rgb5, guides, want_rgba8=True)
        finally:
            ctx.close()
        _ref["fresh"] = dict(other=other, guides=guides, clean=clean)
    return _ref["fresh"]


def test_other_calls_between_the_adds():
    for n in (5, 32, 128):
        rendered(n)
    fresh = _fresh()
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    try:
        a5 = ctx.accum_add(P(5), want_rgba8=True)
        other = ctx.render(cam2(), W2, H2, 8, 7, want_rgba8=True)  # another size and camera: rewrites the pixel queue and the work buffers
        a32 = ctx.accum_add(P(27), want_rgba8=True)
        guides = ctx.render_aov_follow(cam(), W, H)
        clean = ctx.denoise(a5[0], guides, want_rgba8=True)
        a128 = ctx.accum_add(P(96), want_rgba8=True)
    finally:
        ctx.accum_end()
    for (rgb, rgba8), n in ((a5, 5), (a32, 32), (a128, 128)):
        assert_same(rgb, rendered(n)[0], "%d samples with other calls in between" % n)
        assert (rgba8 == rendered(n)[1]).all(), n
    assert_same(other[0], fresh["other"][0], "pt_render between two adds")
    assert (other[1] == fresh["other"][1]).all()
    assert_same(guides, fresh["guides"], "pt_render_aov_follow between two adds")
    assert_same(clean[0], fresh["clean"][0], "pt_denoise between two adds")
    assert (clean[1] == fresh["clean"][1]).all()


def test_state_and_estimate():
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    ones = np.ones((H, W), np.uint8)
    model = dict(seen=np.zeros((H, W, 3), F32), half=np.zeros((H, W, 3), F32), n=np.zeros((H, W), U32), n_half=np.zeros((H, W), U32), passes=np.zeros((H, W), U32))
    half = np.zeros((H, W, 3), F32)
    prev_sum = np.zeros((H, W, 3), F32)
    try:
        for k, n in enumerate((8, 8, 16, 16)):
            rgb, rgba8 = ctx.accum_add(P(n), want_rgba8=True)
            st = ctx.accum_state()
            rd = ctx.accum_read()
            if k & 1:  # the samples of every second add, from the snapshots alone
                half = (half + (st["sum"] - prev_sum).astype(F32)).astype(F32)
            prev_sum = st["sum"]
            assert_same(st["half"], half, "half after add %d" % (k + 1))
            r = accum_ref.resolve(st["sum"], model["seen"], model["half"], model["n"], model["n_half"], model["passes"], ones, ones, n)
            model = {key: r[key] for key in model}
            assert_same(st["half"], r["half"], "half vs accum_ref after add %d" % (k + 1))
            for key in ("n", "n_half", "passes"):
                assert (st[key] == r[key]).all(), (key, k)
            assert_same(rd["noise"], r["noise"], "noise after add %d" % (k + 1))
            assert_same(rd["rgb"], r["rgb"], "image after add %d" % (k + 1))
            assert_same(rgb, r["rgb"], "pt_accum_add's image after add %d" % (k + 1))
            assert (rd["rgba8"] == r["rgba8"]).all() and (rgba8 == r["rgba8"]).all()
            assert (rd["samples"] == r["n"]).all()
            if k == 0:
                assert np.isposinf(rd["noise"]).all(), "no half buffer yet"
            else:
                assert np.isfinite(rd["noise"]).all() and (rd["noise"] > 0).mean() > 0.9
        assert (st["n"] == 48).all() and (st["n_half"] == 24).all() and (st["passes"] == 4).all()
    finally:
        ctx.accum_end()


def _ids(mask):
    """framebuffer-order mask (H, W) -> launch ids x + W * y"""
    r, x = np.nonzero(mask)
    return (x + W * (H - 1 - r)).astype(U32)


def test_adaptive_adds(orc):
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    ones = np.ones((H, W), np.uint8)
    try:
        ctx.accum_add(P(8))
        ctx.accum_add(P(8))
        rd = ctx.accum_read()
        finite = rd["noise"][np.isfinite(rd["noise"]) & (rd["noise"] > 0)]
        assert finite.size > 0.9 * W * H
        thr = float(np.median(finite))
        for k in range(3):
            want_active = accum_ref.select(rd["noise"], rd["samples"], ones, 0, thr).astype(bool)
            rgb, _ = ctx.accum_add(P(16, thr=thr))
            info, st = ctx.accum_info(), ctx.stats()
            nxt = ctx.accum_read()
            print("adaptive add %d: %d of %d pixels active" % (k + 1, int(want_active.sum()), W * H))
            if k == 0:
                assert W * H / 4 <= want_active.sum() <= 3 * W * H / 4, want_active.sum()
            assert ((nxt["samples"] - rd["samples"]) == 16 * want_active).all(), "add %d: the sample map's delta is the select definition" % (k + 1)
            assert info["active_pixels"] == want_active.sum() and (st["launches"] > 0) == bool(want_active.any())
            assert_same(nxt["rgb"][~want_active], rd["rgb"][~want_active], "pixels that were not active keep their colour")
            assert_same(nxt["noise"][~want_active], rd["noise"][~want_active], "... and their noise")
            rd = nxt
        counts = sorted(int(c) for c in np.unique(rd["samples"]))
        assert set(counts) <= {16, 32, 48, 64} and len(counts) >= 2, counts
        for c in counts:
            mask = rd["samples"] == c
            want, want8 = oracle_render(orc, c, pixel_list=_ids(mask))
            assert_same(rd["rgb"][mask], want[mask], "the %d pixels with %d samples vs the oracle" % (int(mask.sum()), c))
            assert (rd["rgba8"][mask] == want8[mask]).all(), c
        assert info["samples_total"] == int(rd["samples"].sum())
    finally:
        ctx.accum_end()


def test_cap_and_empty_active_set():
    rendered(32)
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    try:
        for k in range(4):
            ctx.accum_add(P(16, cap=32))
            info, st = ctx.accum_info(), ctx.stats()
            assert info["active_pixels"] == (W * H if k < 2 else 0), (k, info)
            assert (st["launches"] > 0) == (k < 2), (k, st)
        rd = ctx.accum_read()
        assert (rd["samples"] == 32).all(), "a cap of 32 stops every pixel at 32"
        assert_same(rd["rgb"], rendered(32)[0], "capped at 32")
        ctx.accum_begin(cam(), W, H, DEPTH)  # a begin replaces the accumulation
        ctx.accum_add(P(24, cap=32))
        ctx.accum_add(P(24, cap=32))
        ctx.accum_add(P(24, cap=32))
        assert (ctx.accum_read()["samples"] == 48).all(), "n may overshoot the cap by less than n_samples"
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add(P(8))
        ctx.accum_add(P(8))
        before = ctx.accum_read()
        rgb, rgba8 = ctx.accum_add(P(16, thr=1e30), want_rgba8=True)  # PT_OK
        st, info = ctx.stats(), ctx.accum_info()
        after = ctx.accum_read()
        assert st["launches"] == 0 and info["active_pixels"] == 0 and info["adds"] == 3 and info["samples_total"] == 16 * W * H, (st, info)
        for key in ("rgb", "noise"):
            assert_same(after[key], before[key], key)
        assert (after["rgba8"] == before["rgba8"]).all() and (after["samples"] == before["samples"]).all()
        assert_same(rgb, before["rgb"], "the add's own image")
        assert (rgba8 == before["rgba8"]).all()
        assert_same(ctx.accum_add(P(16))[0], rendered(32)[0], "a uniform add after the empty one")
    finally:
        ctx.accum_end()


def test_shard():
    rendered(32)
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    try:
        ctx.accum_add(P(8))
        ctx.accum_add(P(24))
        whole = ctx.accum_read()
    finally:
        ctx.accum_end()
    assert_same(whole["rgb"], rendered(32)[0], "8 + 24")
    own = np.zeros(W * H, bool)
    own[B.shard_pixels(W, H, 8, 1, 3)] = True
    own = own.reshape(H, W)[::-1]  # launch order -> framebuffer order
    assert 0.2 < own.mean() < 0.5
    ctx.set_pixel_shard(1, 3, 8)
    try:
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add(P(8))
        ctx.accum_add(P(24))
        part = ctx.accum_read()
        assert ctx.accum_info()["owned_pixels"] == own.sum()
        for key in ("rgb", "noise"):
            assert_same(part[key][own], whole[key][own], key)
            assert (np.ascontiguousarray(part[key][~own]).view(U32) == 0).all(), key + ": +0 outside the shard"
        for key in ("rgba8", "samples"):
            assert (part[key][own] == whole[key][own]).all() and (part[key][~own] == 0).all(), key
        ctx.set_pixel_shard(2, 3, 8)
        L = B.lib()
        assert L.pt_accum_add(ctx._h, None, None, None) == -1
        assert "pt_accum_add: the pixel shard changed after pt_accum_begin" in L.pt_last_error(ctx._h).decode()
        ctx.set_pixel_shard(1, 3, 8)
        ctx.accum_add(P(16))  # the shard it was begun with: goes on
        assert (ctx.accum_read()["samples"][own] == 48).all()
    finally:
        ctx.accum_end()
        ctx.set_pixel_shard(0, 1, 16)


def test_add_on_a_caller_stream_then_a_render_on_another():
    for n in (8, 128):
        rendered(n)
    want_other = _fresh()["other"]
    ctx = gpu()
    s0, s1 = AS.stream(0), AS.stream(1)
    mine, other = AS.DeviceFrame(W, H), AS.DeviceFrame(W2, H2)
    try:
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add_device(P(8), mine.rgb, mine.rgba8, stream=s0)
        ctx.render_device(cam2(), W2, H2, 8, 7, other.rgb, other.rgba8, stream=s1)
        rd = ctx.accum_read()  # waits on the host; no pt_synchronize before it
        assert_same(rd["rgb"], rendered(8)[0], "pt_accum_read behind an add and a render in flight")
        assert (rd["samples"] == 8).all() and np.isposinf(rd["noise"]).all()
        ctx.synchronize()
        got, got8 = mine.read()
        assert_same(got, rendered(8)[0], "the add's device frame")
        assert (got8 == rendered(8)[1]).all()
        got, got8 = other.read()
        assert_same(got, want_other[0], "pt_render_device right behind the add")
        assert (got8 == want_other[1]).all()
        ctx.accum_add_device(P(24), None, None, stream=s1)
        ctx.accum_add_device(P(96), mine.rgb, None, stream=s0)
        rd = ctx.accum_read()
        assert_same(rd["rgb"], rendered(128)[0], "8 + 24 + 96 on alternating streams")
        ctx.synchronize()
        assert_same(mine.read()[0], rendered(128)[0], "the last add's device frame")
    finally:
        ctx.accum_end()
        ctx.synchronize()
        mine.free()
        other.free()


def test_pt_main_adds_flag(tmp_path):
    pt_main = os.path.join(AC.ROOT, "owl-path-tracer_amd", "pt_main")
    a = tmp_path / "assets"
    shutil.copytree(AC.ASSETS, a)
    s = json.load(open(os.path.join(AC.ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[W, H], max_samples=37, max_path_depth=DEPTH)
    s["test"] = dict(name="g", material_name="sphere", attribute_name="metallic", material_type=2, values=[0.0, 1.0], step_size=1.0)
    (a / "settings.json").write_text(json.dumps(s))
    files = {}
    rich = ["--watertight", "--aov", "1", "--denoise"]
    for tag, extra in (("one", []), ("adds", ["--adds", "3"]), ("rich", rich), ("rich_adds", rich + ["--adds", "3"])):
        d = tmp_path / tag
        os.makedirs(d)
        r = subprocess.run([pt_main, "--assets", str(a), "--out", str(d)] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        files[tag] = {f: open(d / f, "rb").read() for f in sorted(os.listdir(d))}
    assert len(files["one"]) == 2 and all(f.endswith(".png") for f in files["one"]), sorted(files["one"])
    assert files["adds"] == files["one"]
    assert len(files["rich"]) == 10 and files["rich_adds"] == files["rich"], sorted(files["rich"])
    r = subprocess.run([pt_main, "--assets", str(a), "--out", str(tmp_path), "--adds", "38"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "--adds 38 exceeds max_samples = 37" in r.stderr, r.stderr[-1000:]


def _snapshot(ctx):
    rd, st = ctx.accum_read(), ctx.accum_state()
    return [rd[k].tobytes() for k in ("rgb", "rgba8", "noise", "samples")] + [st[k].tobytes() for k in ("sum", "half", "n", "n_half", "passes")]


def test_sample_limit():
    """A pixel's n must stay below 2^31 - 65536 = 2147418112; the library judges it by the sum of the adds' n_samples.  16 + 32767 x 65535 =
    2147385361 fits, one more add of 65535 does not, one of the remaining 32751 does."""
    L = B.lib()
    ctx = gpu()
    ctx.accum_begin(cam(), W, H, DEPTH)
    try:
        ctx.accum_add(P(8, cap=1))
        ctx.accum_add(P(8, cap=1))  # n = 8 >= the cap of 1: nobody is active, from here on an add runs select and resolve only
        assert ctx.accum_info()["active_pixels"] == 0 and (ctx.accum_read()["samples"] == 8).all()
        big = P(65535, cap=1)
        h, ref = ctx._h, __import__("ctypes").byref(big)
        done = 0
        while done < 40000 and L.pt_accum_add(h, ref, None, None) == 0:
            done += 1
        assert done == 32767, done
        err = L.pt_last_error(h).decode()
        assert "pt_accum_add: a pixel would pass 2147418112 samples (2147385361 so far + 65535)" in err, err
        before = _snapshot(ctx)
        info = ctx.accum_info()
        assert info["adds"] == 2 + 32767 and info["active_pixels"] == 0 and info["samples_total"] == 8 * W * H, info
        assert L.pt_accum_add(h, ref, None, None) == -1 and L.pt_accum_add_device(h, ref, None, None, None) == -1
        assert "pt_accum_add_device: a pixel would pass" in L.pt_last_error(h).decode()
        assert _snapshot(ctx) == before and ctx.accum_info() == info, "a refused add touches nothing"
        ctx.accum_add(P(32751, cap=1))  # exactly to the limit
        assert L.pt_accum_add(h, __import__("ctypes").byref(P(1, cap=1)), None, None) == -1
        assert _snapshot(ctx) == before
    finally:
        ctx.accum_end()


def test_new_scene_after_begin():
    rendered(32)
    L = B.lib()
    ctx = B.Context(0)
    try:
        AC.upload(ctx, scene(), B)
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add(P(8))
        before = _snapshot(ctx)
        AC.upload(ctx, scene(), B)  # the same scene again is a new scene all the same
        assert L.pt_accum_add(ctx._h, None, None, None) == -1
        assert "pt_accum_add: a new scene was uploaded after pt_accum_begin; begin again" in L.pt_last_error(ctx._h).decode()
        assert _snapshot(ctx) == before, "the accumulation itself stays readable"
        ctx.set_environment(B.make_env(**ENV))  # (not a new scene)
        assert L.pt_accum_add(ctx._h, None, None, None) == -1
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add(P(8))
        ctx.set_environment(B.make_env(**ENV))
        assert_same(ctx.accum_add(P(24))[0], rendered(32)[0], "a new begin after the upload")
    finally:
        ctx.close()


def test_communicator_is_refused_by_name():
    L = B.lib()
    ctx = B.Context(0)
    try:
        AC.upload(ctx, scene(), B)
        ctx.accum_begin(cam(), W, H, DEPTH)
        ctx.accum_add(P(8))
        ctx.comm_init_rank(B.comm_unique_id(), 0, 1)
        h = ctx._h
        c = cam()
        byref = __import__("ctypes").byref
        for call, who in ((lambda: L.pt_accum_add(h, None, None, None), "pt_accum_add"), (lambda: L.pt_accum_add_device(h, None, None, None, None), "pt_accum_add_device"),
                          (lambda: L.pt_accum_begin(h, byref(c), W, H, DEPTH), "pt_accum_begin")):
            assert call() == -1, who
            err = L.pt_last_error(h).decode()
            assert who + ": a context with a communicator has no accumulation yet" in err, err
        assert ctx.accum_info()["adds"] == 1 and (ctx.accum_read()["samples"] == 8).all(), "what was begun before stays readable and can be ended"
        ctx.accum_end()
        ctx.comm_destroy()
        ctx.accum_begin(c, W, H, DEPTH)
        ctx.accum_add(P(8))
        ctx.accum_end()
    finally:
        ctx.close()
