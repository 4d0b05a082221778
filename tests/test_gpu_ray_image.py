"""pt_render_rays on the GPU (include/mi355pt.h "ray images"): the ray-image instances of the wavefront kernel against the oracle.

Every comparison is bit for bit on out_rgb and out_rgba8 except leg D.  The oracle side is tests/ray_image_ref.py.  Legs A, B, C, E and F
go through the degenerate camera: a ray with zero jitter is the camera {org, L, 0, 0} with dir = fl(L - org), one Scene.render per ray;
the tests choose org and L, never dir.  Legs D2, G, H and I go through the oracle's own ray-image generator, Scene.render_rays, which
tests/test_ray_image_host.py anchors to that camera and to a numpy restatement of the first ray: a jittered frame of any size has an
exact reference.

A. Pinhole through fixed rays: the pixel-centre rays of the scene's camera on Cornell, the textured cube under the automatic environment
   and the glass and metal icospheres under an environment map; 20 x 13 (partial 8 x 8 blocks, more than one wave) and 64 x 48, 4 and
   16 spp, depth 8; every pixel.
B. Probe rays: 24 x 16 unrelated rays - origins anywhere in the scene's box, a seeded few up to 5 extents outside, directions uniform
   on the sphere - so the indexing x + W * y against the flipped output order shows; 8 spp, depth 8 and depth 1.
C. Jitter: eight 1 x 1 images at 64 spp from inside a translated Cornell box, org = 0, |du|, |dv| up to 0.2 |dir|, against Scene.render
   of the camera {0, dir, du, dv}.
D. Jitter over a frame (NOT exact): pinhole(cam, 64, 48) at 256 spp against pt_render(cam) under the metrics and the stated bars of
   tools/tolerance_calibration.py.  The record's three vectors are rounded once each, so a sample's direction differs from the camera's
   by an ulp or so before normalize: same streams, ulp-level arithmetic differences - what the bars were calibrated for.
D2. Its exact twin: pinhole(cam, 64, 48) at 64 spp against Scene.render_rays of that same table.
E. Paths through the host code: blocking and device forms, a caller's stream, right behind a pt_render_device, with and without a cost
   pre-pass, ring and tier schedules, the group walk forced on and off, both slab forms, "count", a shard of world 3, and the frame
   after pt_set_materials and after pt_update_vertices.
F. Nothing else moves: pt_render around a pt_render_rays, an accumulation around one, and the spill-test build (kernel_variant 3).
G. Tables that tell records apart (tests/ray_tables.py): the scrambled table - org, dir, du, dv all per pixel, NaN in the reserved
   floats - and an equirectangular panorama from inside the scene, on Cornell, the cube and ico_map, at 1 x 1, 7 x 9 (under one wave,
   partial blocks), 20 x 13, 64 x 48 (many waves), 130 x 3 (more blocks than rows) and 3 x 130, at 4 spp (no cost pre-pass) and 64 spp
   (pre-pass, sort, tiers), depth 8.  Each case first asserts the precondition on the oracle's frames: the frame differs in at least half
   of its pixels from the frame with the neighbouring record's du / dv, with the jitter zeroed, and with du and dv exchanged - a kernel
   that read another record, a stale one, or swapped the draws cannot pass.
H. Hand-offs: one scrambled 20 x 13 frame at 64 spp under every schedule and walk option that moves samples between slots, chunks and
   launches; the blocking and the device form on the context's and a caller's stream and right behind a pt_render_device; a shard of
   world 3 (owned pixels exact, the others +0, the union the frame); "count" = 1, whose counters are the oracle's.
I. Random scenes: the generator of tests/test_gpu_fuzz.py, each scene under a scrambled table with origins inside its box, frames up to
   40 x 30, 4 to 32 spp, depth 1 to 8; every seed compared, until 32 of the compared frames meet the precondition of leg G.
And the one refusal that needs a device: a context with a communicator."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aov_common as AC
import async_common as AS
import ray_image_ref as RR
import ray_tables as RT
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import ray_image as RI
from owl_path_tracer_amd.pyhost import scene_io

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
DEPTH = 8
SCENES = ("cornell", "cube", "ico_map")
_state = {}
_ref = {}


def gpu(name):
    """ONE context for the module (its stream and two caller streams stay below four hardware queues), holding scene `name`."""
    if "ctx" not in _state:
        _state["ctx"] = B.Context(0)
    if _state.get("scene") != name:
        AC.upload(_state["ctx"], AC.scene(name), B)
        _state["scene"] = name
    return _state["ctx"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    AS.destroy_streams()
    if "ctx" in _state:
        _state["ctx"].close()
    _state.clear()
    _ref.clear()


def oracle_scene(orc, name):
    if ("S", name) not in _ref:
        sc = AC.scene(name)
        _ref[("S", name)] = (orc.Scene(sc["flat"]), orc.make_env(**sc["env"]))
    return _ref[("S", name)]


def assert_frame(got, want, what):
    g, w = np.ascontiguousarray(got[0], F32).view(U32), np.ascontiguousarray(want[0], F32).view(U32)
    bad = (g != w).any(-1)
    assert not bad.any(), "%s: %d of %d pixels differ in out_rgb; first (row, column) %s: got %r, want %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[0][tuple(np.argwhere(bad)[0])], want[0][tuple(np.argwhere(bad)[0])])
    if want[1] is not None:
        assert (got[1] == want[1]).all(), "%s: %d pixels differ in out_rgba8" % (what, int((got[1] != want[1]).sum()))


def pinhole_case(orc, name, W, H, spp, depth=DEPTH):
    """(ray image, the oracle's frame) of the pixel-centre rays of the scene's camera, computed once and handed out read-only."""
    key = ("pin", name, W, H, spp, depth)
    if key not in _ref:
        sc = AC.scene(name)
        cam = AC.camera(sc, W, H, B.to_camera_data).as_array()
        targets = RR.pixel_centre_targets(cam, W, H)
        orgs, dirs = RR.rays_through(np.tile(cam[0:3], (W * H, 1)), targets)
        S, env = oracle_scene(orc, name)
        want = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, spp, depth)
        for a in want:
            a.setflags(write=False)
        _ref[key] = (RI.fixed(orgs, dirs, W, H), want)
    return _ref[key]


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", (4, 16))
@pytest.mark.parametrize("size", ((20, 13), (64, 48)), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", SCENES)
def test_a_pinhole_through_fixed_rays(orc, name, size, spp):
    W, H = size
    rays, want = pinhole_case(orc, name, W, H, spp)
    assert np.isfinite(want[0]).all() and want[0].std() > 0.01
    got = gpu(name).render_rays(rays, W, H, spp, DEPTH, want_rgba8=True)
    assert_frame(got, want, "%s %dx%d %d spp" % (name, W, H, spp))


# ---- B ------------------------------------------------------------------------------------------------------------------
def probe_rays(name, W, H):
    P = AC.scene(name)["flat"]["positions"].reshape(-1, 3).astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(20261020 + SCENES.index(name))
    n = W * H
    orgs = lo + (hi - lo) * rng.random((n, 3))
    far = rng.choice(n, 12, replace=False)  # a seeded few outside, up to 5 extents from the box's centre
    u = rng.normal(size=(12, 3))
    orgs[far] = 0.5 * (lo + hi) + u / np.linalg.norm(u, axis=1, keepdims=True) * ext * rng.uniform(1.0, 5.0, (12, 1))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[far[:6]] = 0.5 * (lo + hi) - orgs[far[:6]]  # half of those look back at the scene
    d[far[:6]] /= np.linalg.norm(d[far[:6]], axis=1, keepdims=True)
    orgs = orgs.astype(F32)
    return orgs, (orgs.astype(np.float64) + d).astype(F32)


@pytest.mark.parametrize("depth", (8, 1))
@pytest.mark.parametrize("name", SCENES)
def test_b_probe_rays(orc, name, depth):
    W, H, spp = 24, 16, 8
    orgs, targets = probe_rays(name, W, H)
    _, dirs = RR.rays_through(orgs, targets)
    S, env = oracle_scene(orc, name)
    want = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, spp, depth)
    lit = want[0].reshape(-1, 3).max(1) > 0
    print("%s depth %d: %d of %d probe pixels are lit, %d distinct" % (name, depth, lit.sum(), lit.size, len({p.tobytes() for p in want[0].reshape(-1, 3)})))
    assert lit.sum() >= 6  # (depth 1 inside a closed mesh is black: the rays from outside that look away see the environment)
    got = gpu(name).render_rays(RI.fixed(orgs, dirs, W, H), W, H, spp, depth, want_rgba8=True)
    assert_frame(got, want, "%s probes, depth %d" % (name, depth))
    # the list view: entry i is ray i
    assert (RI.to_list(got[0], W, H).view(U32) == np.ascontiguousarray(want[0][::-1]).reshape(-1, 3).view(U32)).all()


# ---- C ------------------------------------------------------------------------------------------------------------------
def test_c_jitter_one_pixel_images(orc):
    sc = scene_io.load_scene_dir(AC.ASSETS, "cornell-box")
    P = np.concatenate([m["vertices"] for m, _ in sc["entities"]]).astype(np.float64)
    centre = (0.5 * (P.min(0) + P.max(0))).astype(F32)
    ents = [(dict(m, vertices=(m["vertices"] - centre).astype(F32)), mid) for m, mid in sc["entities"]]
    flat = scene_io.flatten_scene(ents, sc["materials"])
    lo, hi = flat["positions"].reshape(-1, 3).min(0), flat["positions"].reshape(-1, 3).max(0)
    assert (lo < 0).all() and (hi > 0).all(), "the origin lies inside the translated box"
    envk = dict(color=(0.3, 0.6, 0.2), intensity=0.75)
    S, env = orc.Scene(flat), orc.make_env(**envk)
    ctx = B.Context(0)
    try:
        ctx.upload_scene(ents, [m for _, m, _ in sc["materials"]], env=B.make_env(**envk))
        rng = np.random.default_rng(64)
        seen = set()
        for k in range(8):
            d = rng.normal(size=3)
            d = (d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)).astype(F32)
            du, dv = ((v / np.linalg.norm(v) * np.linalg.norm(d) * rng.uniform(0.02, 0.2)).astype(F32) for v in rng.normal(size=(2, 3)))
            t = np.zeros(1, B.RAY_GEN_DTYPE)
            t["dir"], t["du"], t["dv"] = d, du, dv
            rgb, rgba = ctx.render_rays(t, 1, 1, 64, DEPTH, want_rgba8=True)
            want, want8 = RR.oracle_jitter_1x1(orc, S, env, d, du, dv, 64, DEPTH)
            assert (rgb[0, 0].view(U32) == want.view(U32)).all() and rgba[0, 0] == want8, (k, rgb[0, 0], want)
            assert ctx.stats()["prepass_spp"] > 0  # (64 spp: the sorted schedule, on a queue of one pixel)
            seen.add(want.tobytes())
        assert len(seen) == 8
    finally:
        ctx.close()


# ---- D ------------------------------------------------------------------------------------------------------------------
def test_d_jitter_over_a_frame_within_the_stated_bars():
    """Measured on an MI355X (profiles/r22_ray_image.json, "jitter_over_a_frame"): 60.5 % of the 3072 pixels identical, l2_p99 3.5e-7,
    l2_p999 3.7e-4, rel_rmse 1.4e-4, l2_max 3.6e-3, no RGBA8 channel off by more than 1.  The bars are the stated ones of
    tests/test_tolerance_calibration.py, unchanged."""
    sys.path.insert(0, os.path.join(AC.ROOT, "tools"))
    import tolerance_calibration as T

    W, H, spp = 64, 48, 256
    ctx = gpu("cornell")
    cam = AC.camera(AC.scene("cornell"), W, H, B.to_camera_data)
    a, a8 = ctx.render(cam, W, H, spp, DEPTH, want_rgba8=True)
    b, b8 = ctx.render_rays(RI.pinhole(cam, W, H), W, H, spp, DEPTH, want_rgba8=True)
    m = T.metrics(a, a8, b, b8)
    print("pinhole ray image vs pt_render, cornell %dx%d %d spp depth %d: %r" % (W, H, spp, DEPTH, m))
    assert np.isfinite(b).all()
    assert m["l2_p99"] <= 1e-4
    assert m["l2_p999"] <= 0.04
    assert m["rel_rmse"] <= 1e-2


def test_d2_jitter_over_a_frame_exactly(orc):
    """Leg D's table at 64 spp, every pixel bit for bit against the oracle's frame of that same table."""
    W, H, spp = 64, 48, 64
    ctx = gpu("cornell")
    t = RI.pinhole(AC.camera(AC.scene("cornell"), W, H, B.to_camera_data), W, H)
    S, env = oracle_scene(orc, "cornell")
    want = S.render_rays(t, env, W, H, spp, DEPTH, want_rgba8=True)[:2]
    assert np.isfinite(want[0]).all() and want[0].std() > 0.01
    got = ctx.render_rays(t, W, H, spp, DEPTH, want_rgba8=True)
    assert ctx.stats()["prepass_spp"] > 0
    assert_frame(got, want, "pinhole table, cornell %dx%d %d spp" % (W, H, spp))


# ---- E ------------------------------------------------------------------------------------------------------------------
EW, EH = 40, 28


def _device_table(rays):
    buf = AS.DeviceFrame(EW, EH, floats=16)  # 64 bytes per pixel; hipMalloc aligns far beyond 16
    AS.to_device(buf.rgb, rays)
    return buf


def test_e_blocking_and_device_forms_and_streams(orc):
    rays, want4 = pinhole_case(orc, "cornell", EW, EH, 4)
    _, want40 = pinhole_case(orc, "cornell", EW, EH, 40)
    ctx = gpu("cornell")
    got = ctx.render_rays(rays, EW, EH, 4, DEPTH, want_rgba8=True)
    assert ctx.stats()["prepass_spp"] == 0 and ctx.stats()["launches"] == 1
    assert_frame(got, want4, "blocking form, no cost pre-pass")
    got = ctx.render_rays(rays, EW, EH, 40, DEPTH, want_rgba8=True)
    st = ctx.stats()
    assert st["prepass_spp"] > 0 and st["launches"] == 2 and st["kernel_variant"] == 2 and 0 < st["vgprs"] <= 128
    assert_frame(got, want40, "blocking form, cost pre-pass")
    # another frame for the call in front: pt_render at another size
    W2, H2 = 29, 31
    cam2 = AC.camera(AC.scene("cornell"), W2, H2, B.to_camera_data)
    front = ctx.render(cam2, W2, H2, 8, 7, want_rgba8=True)
    table, out, out2 = _device_table(rays), AS.DeviceFrame(EW, EH), AS.DeviceFrame(W2, H2)
    try:
        ctx.render_rays_device(table.rgb, EW, EH, 4, DEPTH, out.rgb, out.rgba8)  # the context's own stream
        ctx.synchronize()
        assert_frame(out.read(), want4, "device form, the context's stream")
        s0, s1 = AS.stream(0), AS.stream(1)
        ctx.render_rays_device(table.rgb, EW, EH, 40, DEPTH, out.rgb, out.rgba8, stream=s0)
        ctx.synchronize()
        assert ctx.stats()["prepass_spp"] > 0
        assert_frame(out.read(), want40, "device form, a caller's stream")
        ctx.render_device(cam2, W2, H2, 8, 7, out2.rgb, out2.rgba8, stream=s1)
        ctx.render_rays_device(table.rgb, EW, EH, 4, DEPTH, out.rgb, None, stream=s0)  # no synchronize between the two
        ctx.synchronize()
        assert_frame(out2.read(), front, "pt_render_device in front of a pt_render_rays_device")
        assert_frame((out.read()[0], None), (want4[0], None), "pt_render_rays_device right behind a pt_render_device")
        # and a blocking ray image right behind a device frame
        ctx.render_device(cam2, W2, H2, 8, 7, out2.rgb, out2.rgba8, stream=s1)
        assert_frame(ctx.render_rays(rays, EW, EH, 4, DEPTH, want_rgba8=True), want4, "pt_render_rays right behind a pt_render_device")
        ctx.synchronize()
        assert_frame(out2.read(), front, "the device frame in front of it")
    finally:
        ctx.synchronize()
        for b in (table, out, out2):
            b.free()


OPTIONS = [("whole", 1, -1), ("whole", 0, -1), ("groups", 2, 1), ("groups", 0, 1), ("schedule", 0, 1), ("box_exact", 1, -1), ("box_exact", 0, -1), ("fallback", 1, 0),
           ("spp_per_launch", 7, 0), ("chunk_spp", 16, 64)]


@pytest.mark.parametrize("key,value,default", OPTIONS, ids=["%s=%d" % o[:2] for o in OPTIONS])
def test_e_schedules_and_walks(orc, key, value, default):
    rays, want = pinhole_case(orc, "cornell", EW, EH, 40)
    ctx = gpu("cornell")
    ctx.set_option(key, value)
    try:
        got = ctx.render_rays(rays, EW, EH, 40, DEPTH, want_rgba8=True)
        st = ctx.stats()
    finally:
        ctx.set_option(key, default)
    assert_frame(got, want, "%s = %d" % (key, value))
    if key == "whole":
        assert (st["whole_pixels"] == EW * EH) == (value == 1) and st["prepass_spp"] > 0
    if key in ("schedule", "spp_per_launch"):
        assert st["prepass_spp"] == 0
    if key == "fallback":
        assert st["kernel_variant"] == 3 and 128 < st["vgprs"] <= 168


def test_e_count(orc):
    ctx = gpu("cornell")
    for spp in (4, 40):
        rays, want = pinhole_case(orc, "cornell", EW, EH, spp)
        ctx.set_option("count", 1)
        try:
            got = ctx.render_rays(rays, EW, EH, spp, DEPTH, want_rgba8=True)
            st = ctx.stats()
        finally:
            ctx.set_option("count", 0)
        assert_frame(got, want, "the instrumented instance, %d spp" % spp)
        assert st["samples"] == EW * EH * spp and st["rays"] >= st["samples"]


def test_e_shard_of_world_3(orc):
    rays, want = pinhole_case(orc, "cornell", EW, EH, 40)
    ctx = gpu("cornell")
    covered = np.zeros((EH, EW), bool)
    try:
        for rank in (0, 2):
            own = np.zeros(EW * EH, bool)
            own[B.shard_pixels(EW, EH, 8, rank, 3)] = True
            own = own.reshape(EH, EW)[::-1]  # launch order -> framebuffer order
            assert 0.2 < own.mean() < 0.5 and not (own & covered).any()
            covered |= own
            ctx.set_pixel_shard(rank, 3, 8)
            rgb, rgba = ctx.render_rays(rays, EW, EH, 40, DEPTH, want_rgba8=True)
            assert (rgb[own].view(U32) == want[0][own].view(U32)).all() and (rgba[own] == want[1][own]).all(), rank
            assert (np.ascontiguousarray(rgb[~own]).view(U32) == 0).all() and (rgba[~own] == 0).all(), "rank %d: +0 outside the shard" % rank
    finally:
        ctx.set_pixel_shard(0, 1, 16)
    assert_frame(ctx.render_rays(rays, EW, EH, 40, DEPTH, want_rgba8=True), want, "the unsharded frame afterwards")


def test_e_after_set_materials_and_update_vertices(orc):
    scene = RC.make_scene("cornell")
    materials = RC.cornell_materials()
    mats = np.array([m for _, m, _ in materials], F32)
    W, H, spp = 20, 13, 16
    cam = RC.cornell_camera(W, H, B.to_camera_data).as_array()
    targets = RR.pixel_centre_targets(cam, W, H)
    orgs, dirs = RR.rays_through(np.tile(cam[0:3], (W * H, 1)), targets)
    rays = RI.fixed(orgs, dirs, W, H)
    env = orc.make_env(**RC.CORNELL_ENV)
    ctx = B.Context(0)
    try:
        ctx.set_option("dynamic", 1)
        RC.upload(ctx, scene, materials=list(mats), env=B.make_env(**RC.CORNELL_ENV))
        S = orc.Scene(scene_io.flatten_scene(scene[0], materials))
        first = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, spp, DEPTH)
        assert_frame(ctx.render_rays(rays, W, H, spp, DEPTH, want_rgba8=True), first, "the uploaded state")
        # another table: every base colour turned
        mats2 = mats.copy()
        mats2[:, 0:3] = mats[:, [1, 2, 0]] * F32(0.9)
        ctx.set_materials(mats2)
        S.set_materials(mats2)
        want = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, spp, DEPTH)
        assert (want[0].view(U32) != first[0].view(U32)).any()
        assert_frame(ctx.render_rays(rays, W, H, spp, DEPTH, want_rgba8=True), want, "after pt_set_materials")
        mv = RC.moved(scene, 1)
        ctx.update_vertices(mv)
        S2 = orc.Scene(scene_io.flatten_scene(RC.as_entities(scene, mv), [(n, m, t) for (n, _, t), m in zip(materials, mats2)]))
        want2 = RR.oracle_pixels(orc, S2, env, orgs, targets, W, H, spp, DEPTH)
        assert (want2[0].view(U32) != want[0].view(U32)).any()
        assert_frame(ctx.render_rays(rays, W, H, spp, DEPTH, want_rgba8=True), want2, "after pt_update_vertices")
    finally:
        ctx.close()


# ---- F ------------------------------------------------------------------------------------------------------------------
def test_f_render_and_accumulation_are_untouched(orc):
    rays, want = pinhole_case(orc, "cornell", EW, EH, 40)
    ctx = gpu("cornell")
    W, H = 37, 23
    cam = AC.camera(AC.scene("cornell"), W, H, B.to_camera_data)
    before = ctx.render(cam, W, H, 40, 5, want_rgba8=True)
    assert_frame(ctx.render_rays(rays, EW, EH, 40, DEPTH, want_rgba8=True), want, "the ray image between two renders")
    assert_frame(ctx.render(cam, W, H, 40, 5, want_rgba8=True), before, "pt_render after a pt_render_rays")
    P = lambda n: B.accum_default_params(n_samples=n, max_pixel_samples=0, noise_threshold=0.0)
    frames = {}
    for between in (False, True):
        ctx.accum_begin(cam, W, H, 5)
        try:
            ctx.accum_add(P(8))
            if between:
                assert_frame(ctx.render_rays(rays, EW, EH, 40, DEPTH, want_rgba8=True), want, "the ray image between two adds")
            ctx.accum_add(P(32))
            frames[between] = ctx.accum_read()
        finally:
            ctx.accum_end()
    for k in ("rgb", "noise"):
        assert (frames[True][k].view(U32) == frames[False][k].view(U32)).all(), k
    for k in ("rgba8", "samples"):
        assert (frames[True][k] == frames[False][k]).all(), k
    assert (frames[True]["rgb"].view(U32) == before[0].view(U32)).all(), "8 + 32 samples: the 40-sample frame"


def test_f_spill_test_build(orc, tmp_path):
    """The build whose 4-wave instances need scratch (libmi355pt_spilltest.so, -DPT_WAVES_PER_EU=5): plan_frame falls back to the larger
    ray-image instance through pt_rayimage_kernel_geometry and leg A's 20 x 13 frame comes out bit for bit.  A child process: the library
    path is fixed at import."""
    lib = os.path.join(AC.ROOT, "owl-path-tracer_amd", "libmi355pt_spilltest.so")
    assert os.path.exists(lib), "libmi355pt_spilltest.so not built (make -C owl-path-tracer_amd/csrc spilltest)"
    W, H, spp = 20, 13, 16
    rays, want = pinhole_case(orc, "cornell", W, H, spp)
    np.save(str(tmp_path / "rays.npy"), rays)
    np.save(str(tmp_path / "rgb.npy"), want[0])
    np.save(str(tmp_path / "rgba.npy"), want[1])
    code = r"""
import os, sys, numpy as np
for p in ("tests", "oracle", ""):
    sys.path.insert(0, os.path.join(%(root)r, p))
import ptamd; ptamd.load()
from owl_path_tracer_amd.pyhost import binding as B
import aov_common as AC
assert B.LIB_PATH.endswith("libmi355pt_spilltest.so"), B.LIB_PATH
ctx = B.Context(0)
AC.upload(ctx, AC.scene("cornell"), B)
rgb, rgba = ctx.render_rays(np.load(os.path.join(%(tmp)r, "rays.npy")), %(W)d, %(H)d, %(spp)d, %(depth)d, want_rgba8=True)
st = ctx.stats()
ctx.close()
assert st["kernel_variant"] == 3 and 128 < st["vgprs"] <= 168, (st["kernel_variant"], st["vgprs"])
want = np.load(os.path.join(%(tmp)r, "rgb.npy"))
assert (rgb.view(np.uint32) == want.view(np.uint32)).all(), int((rgb.view(np.uint32) != want.view(np.uint32)).sum())
assert (rgba == np.load(os.path.join(%(tmp)r, "rgba.npy"))).all()
print("RAY_IMAGE_FALLBACK_OK", st["vgprs"])
""" % dict(root=AC.ROOT, tmp=str(tmp_path), W=W, H=H, spp=spp, depth=DEPTH)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PT_LIB_PATH=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RAY_IMAGE_FALLBACK_OK" in r.stdout, r.stdout + r.stderr

# ---- G ------------------------------------------------------------------------------------------------------------------
G_SIZES = ((1, 1), (7, 9), (20, 13), (64, 48), (130, 3), (3, 130))


def jitter_case(orc, kind, name, W, H, spp, depth=DEPTH, counters=False):
    """(table, the oracle's frame (rgb, rgba8[, counters])) of a table of tests/ray_tables.py, computed once, the precondition asserted on
    the frame that is handed out, read-only."""
    key = ("jit", kind, name, W, H, spp, depth)
    if key not in _ref:
        S, env = oracle_scene(orc, name)
        t = RT.table(kind, name, W, H)
        want = S.render_rays(t, env, W, H, spp, depth, want_rgba8=True, want_counters=True)
        assert np.isfinite(want[0]).all()
        shares = RT.precondition(S, env, t, W, H, spp, depth, want=want[0])
        print("%s %s %dx%d %d spp: differing pixels %s" % (kind, name, W, H, spp, ", ".join("%s %.1f %%" % (k, 100 * v) for k, v in shares.items())))
        for a in want[:2]:
            a.setflags(write=False)
        _ref[key] = (t, want)
    t, want = _ref[key]
    return t, (want if counters else want[:2])


# (a 1 x 1 panorama has du = 0 and dv parallel to dir - no jitter to speak of, tests/ray_tables.py: no equirect case there)
G_CASES = [(name, kind, W, H, spp) for name in SCENES for kind in ("scrambled", "equirect") for (W, H) in G_SIZES if not (kind == "equirect" and W * H == 1)
           for spp in (4, 64)]


@pytest.mark.parametrize("name,kind,W,H,spp", G_CASES, ids=["%s-%s-%dx%d-%d" % c for c in G_CASES])
def test_g_tables_that_tell_records_apart(orc, name, kind, W, H, spp):
    t, want = jitter_case(orc, kind, name, W, H, spp)
    ctx = gpu(name)
    got = ctx.render_rays(t, W, H, spp, DEPTH, want_rgba8=True)
    assert (ctx.stats()["prepass_spp"] > 0) == (spp == 64)
    assert_frame(got, want, "%s table, %s %dx%d %d spp" % (kind, name, W, H, spp))


# ---- H ------------------------------------------------------------------------------------------------------------------
HW, HH, HSPP = 20, 13, 64
HANDOFFS = [("spp_per_launch", 8, 0), ("spp_per_launch", 16, 0), ("chunk_spp", 8, 64), ("whole", 0, -1), ("whole", 1, -1), ("groups", 0, 1), ("groups", 2, 1),
            ("box_exact", 0, -1), ("box_exact", 1, -1), ("fallback", 1, 0), ("slots_per_wave", 64, 0)]


@pytest.mark.parametrize("key,value,default", HANDOFFS, ids=["%s=%d" % o[:2] for o in HANDOFFS])
def test_h_handoffs_on_a_scrambled_table(orc, key, value, default):
    t, want = jitter_case(orc, "scrambled", "cornell", HW, HH, HSPP)
    ctx = gpu("cornell")
    ctx.set_option(key, value)
    try:
        got = ctx.render_rays(t, HW, HH, HSPP, DEPTH, want_rgba8=True)
        st = ctx.stats()
    finally:
        ctx.set_option(key, default)
    assert_frame(got, want, "scrambled table, %s = %d" % (key, value))
    if key == "spp_per_launch":
        assert st["prepass_spp"] == 0  # (the unsorted schedule: chunks of `value` samples)
    if key == "whole":
        assert (st["whole_pixels"] == HW * HH) == (value == 1)
    if key == "fallback":
        assert st["kernel_variant"] == 3
    assert_frame(ctx.render_rays(t, HW, HH, HSPP, DEPTH, want_rgba8=True), want, "the default again after %s = %d" % (key, value))


def test_h_blocking_and_device_forms_and_streams(orc):
    t, want = jitter_case(orc, "scrambled", "cornell", HW, HH, HSPP)
    _, want4 = jitter_case(orc, "scrambled", "cornell", HW, HH, 4)
    ctx = gpu("cornell")
    assert_frame(ctx.render_rays(t, HW, HH, HSPP, DEPTH, want_rgba8=True), want, "blocking form")
    W2, H2 = 29, 31
    cam2 = AC.camera(AC.scene("cornell"), W2, H2, B.to_camera_data)
    front = ctx.render(cam2, W2, H2, 8, 7, want_rgba8=True)
    table = AS.DeviceFrame(HW, HH, floats=16)
    AS.to_device(table.rgb, t)
    out, out2 = AS.DeviceFrame(HW, HH), AS.DeviceFrame(W2, H2)
    try:
        ctx.render_rays_device(table.rgb, HW, HH, HSPP, DEPTH, out.rgb, out.rgba8)
        ctx.synchronize()
        assert_frame(out.read(), want, "device form, the context's stream")
        s0, s1 = AS.stream(0), AS.stream(1)
        ctx.render_rays_device(table.rgb, HW, HH, 4, DEPTH, out.rgb, out.rgba8, stream=s0)
        ctx.synchronize()
        assert_frame(out.read(), want4, "device form, a caller's stream, 4 spp")
        ctx.render_rays_device(table.rgb, HW, HH, HSPP, DEPTH, out.rgb, out.rgba8, stream=s0)
        ctx.synchronize()
        assert_frame(out.read(), want, "device form, a caller's stream")
        ctx.render_device(cam2, W2, H2, 8, 7, out2.rgb, out2.rgba8, stream=s1)
        ctx.render_rays_device(table.rgb, HW, HH, HSPP, DEPTH, out.rgb, out.rgba8, stream=s0)  # no synchronize between the two
        ctx.synchronize()
        assert_frame(out2.read(), front, "pt_render_device in front of a pt_render_rays_device")
        assert_frame(out.read(), want, "pt_render_rays_device right behind a pt_render_device")
    finally:
        ctx.synchronize()
        for b in (table, out, out2):
            b.free()


def test_h_shard_of_world_3(orc):
    t, want = jitter_case(orc, "scrambled", "cornell", HW, HH, HSPP)
    ctx = gpu("cornell")
    covered = np.zeros((HH, HW), bool)
    union = np.zeros((HH, HW, 3), F32)
    union8 = np.zeros((HH, HW), U32)
    try:
        for rank in (0, 1, 2):
            own = np.zeros(HW * HH, bool)
            own[B.shard_pixels(HW, HH, 8, rank, 3)] = True
            own = own.reshape(HH, HW)[::-1]  # launch order -> framebuffer order
            assert own.any() and not (own & covered).any()
            covered |= own
            ctx.set_pixel_shard(rank, 3, 8)
            rgb, rgba = ctx.render_rays(t, HW, HH, HSPP, DEPTH, want_rgba8=True)
            assert (rgb[own].view(U32) == want[0][own].view(U32)).all() and (rgba[own] == want[1][own]).all(), "rank %d: its pixels" % rank
            assert (np.ascontiguousarray(rgb[~own]).view(U32) == 0).all() and (rgba[~own] == 0).all(), "rank %d: +0 outside the shard" % rank
            union[own], union8[own] = rgb[own], rgba[own]
    finally:
        ctx.set_pixel_shard(0, 1, 16)
    assert covered.all()
    assert_frame((union, union8), want, "the union over the ranks")
    assert_frame(ctx.render_rays(t, HW, HH, HSPP, DEPTH, want_rgba8=True), want, "the unsharded frame afterwards")


@pytest.mark.parametrize("spp", (4, HSPP))
def test_h_counters_are_the_oracles(orc, spp):
    t, want = jitter_case(orc, "scrambled", "cornell", HW, HH, spp, counters=True)
    ctx = gpu("cornell")
    ctx.set_option("count", 1)
    try:
        got = ctx.render_rays(t, HW, HH, spp, DEPTH, want_rgba8=True)
        st = ctx.stats()
    finally:
        ctx.set_option("count", 0)
    assert_frame(got, want[:2], "the instrumented instance, %d spp" % spp)
    for k in ("samples", "rays", "scatters", "env_misses", "nan_retries"):
        assert st[k] == want[2][k], (k, st[k], want[2][k])
    assert st["samples"] == HW * HH * spp and st["rays"] > st["samples"]


# ---- I ------------------------------------------------------------------------------------------------------------------
I_TELLING = 32  # cases whose frame tells the records apart (RT.CAP under all three wrong tables) the leg runs until it has compared
I_MOST = 96  # seeds at the most
I_SEED0 = 20261020


def random_case(seed):
    """A scene of tests/test_gpu_fuzz.py's generator (its own seed sequence, untouched) with a frame size, sample count, depth and a
    scrambled table of this test's: origins inside the scene's box, so every ray starts within one extent of the scene, inside the
    closest-hit domain of 10 extents."""
    import test_gpu_fuzz as FZ

    c = FZ.draw_case(seed)
    rng = np.random.default_rng([seed, 1])
    W, H = int(rng.integers(1, 41)), int(rng.integers(1, 31))
    spp = int(rng.choice([4, 7, 16, 32]))
    depth = int(rng.choice([1, 2, 4, 8]))
    P = np.concatenate([m["vertices"] for m, _ in c["ents"]]).astype(np.float64)
    t = RT.scrambled_in_box(P.min(0), P.max(0), W, H, [seed, 2])
    return c, t, W, H, spp, depth


def test_i_random_scenes(orc, scene_io):
    """Every seed from I_SEED0 on is compared bit for bit, none is left out.  A random scene may hide the jitter - a constant environment
    seen directly, a dark scene, one pixel - so the leg goes on until I_TELLING of the frames it compared meet the precondition of
    tests/ray_tables.py on the oracle's frames (at least half of the pixels differ under the neighbouring record's, the zeroed and the
    exchanged jitter): that many frames a kernel reading the wrong record could not have passed.  About every second seed is one."""
    ctx = B.Context(0)
    telling, used, pixels, differing = 0, 0, 0, {k: 0 for k, _ in RT.VARIANTS}
    try:
        while telling < I_TELLING:
            assert used < I_MOST, "only %d of %d random frames tell records apart" % (telling, used)
            seed = I_SEED0 + used
            used += 1
            c, t, W, H, spp, depth = random_case(seed)
            ctx.upload_scene(c["ents"], c["mats"], textures=c["texs"], mesh_textures=c["mesh_tex"], env=B.make_env(**c["env"]))
            got, got8 = ctx.render_rays(t, W, H, spp, depth, want_rgba8=True)
            S = orc.Scene(scene_io.flatten_scene(c["ents"], [("m%d" % i, m, "") for i, m in enumerate(c["mats"])], c["tex_by_mat"]))
            env = orc.make_env(**c["env"])
            want, want8, _ = S.render_rays(t, env, W, H, spp, depth, want_rgba8=True)
            what = "random scene seed=%d (%dx%d, %d spp, depth %d, %d triangles)" % (seed, W, H, spp, depth, sum(len(m["indices"]) for m, _ in c["ents"]))
            same = (got.view(U32) == want.view(U32)) | (np.isnan(got) & np.isnan(want))
            assert same.all(), "%s: %d of %d pixels differ; first (row, column) %s: got %r, want %r" % (
                what, int((~same).any(-1).sum()), W * H, tuple(np.argwhere(~same.all(-1))[0]), got[tuple(np.argwhere(~same.all(-1))[0])], want[tuple(np.argwhere(~same.all(-1))[0])])
            assert (got8 == want8).all(), what + ": RGBA8 differs"
            shares = {k: RT.differing_share(want, S.render_rays(f(t), env, W, H, spp, depth)[0]) for k, f in RT.VARIANTS if not (k == "neighbour" and W * H == 1)}
            telling += int(min(shares.values()) >= RT.CAP)
            pixels += W * H
            for k, v in shares.items():
                differing[k] += v * W * H
    finally:
        ctx.close()
    print("random scenes: %d compared, %d of them tell records apart; of all %d pixels %s differ" % (
        used, telling, pixels, ", ".join("%.1f %% under '%s'" % (100 * v / pixels, k) for k, v in differing.items())))


def test_communicator_is_refused_by_name(orc):
    rays, _ = pinhole_case(orc, "cornell", 20, 13, 4)
    ctx = B.Context(0)
    try:
        AC.upload(ctx, AC.scene("cornell"), B)
        ctx.comm_init_rank(B.comm_unique_id(), 0, 1)
        L = B.lib()
        rgb = np.full((13, 20, 3), 7.0, F32)
        rc = L.pt_render_rays(ctx._h, rays.ctypes.data, 20, 13, 4, DEPTH, rgb.ctypes.data_as(C.POINTER(C.c_float)), None)
        assert rc == -1 and "pt_render_rays: a context with a communicator renders no ray images yet" in L.pt_last_error(ctx._h).decode()
        rc = L.pt_render_rays_device(ctx._h, 64, 20, 13, 4, DEPTH, 64, None, None)
        assert rc == -1 and "pt_render_rays_device: a context with a communicator" in L.pt_last_error(ctx._h).decode()
        assert (rgb == 7.0).all()
        ctx.comm_destroy()
        _, want = pinhole_case(orc, "cornell", 20, 13, 4)
        assert_frame(ctx.render_rays(rays, 20, 13, 4, DEPTH, want_rgba8=True), want, "after pt_comm_destroy")
    finally:
        ctx.close()
