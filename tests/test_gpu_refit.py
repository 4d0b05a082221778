"""pt_update_vertices on the GPU: the refit kernels of csrc/pt_refit.hip, and every render path after them.

Everything is compared on raw bits; scenes, the movement (wobble + one mesh shifted by three extents + slivers across the threshold in
both directions) and helpers are those of tests/refit_common.py and tests/test_refit_host.py.

1. device arrays: after an update, the binary / quad / oct / triangle arrays read back from HBM (PT_TREE_DEVICE) equal the host twin's
   byte for byte - after the identity update (then also the uploaded arrays) and after the moved one; scenes of 1 and 2 triangles, four
   meshes with non-finite and unreferenced vertices, leaf_align padding, and the Cornell box (17 974 triangles: several blocks a level).
2. frames: Cornell 48 x 40 at 64 spp, each path once plain and once counted: update + render == fresh upload of the moved scene + render == the oracle's frame of the
   moved scene - float and RGBA8 frames and the counters samples, rays, scatters, env_misses - through the default path, groups = 2,
   fallback = 1, box_exact = 1, kernel = 1, and watertight = 1 (against the oracle's watertight twin).
3. normals: the smooth textured glass / metal icospheres under an environment map; with new normals passed, and with normals = NULL
   (== a fresh upload of the moved vertices with the old normals).
4. ray probes 30..35 after an update == the oracle's brute force on the moved scene, two battery scenes, every ray inside the domain.
5. four updates and back: the first frame bit for bit, the device arrays the uploaded ones.
6. render_batch of two cameras after an update == the loop of single renders.
7. pt_group_update_vertices, two contexts on one card over the stub collective: the single context's frame after the same update.
"""
import json
import os
import sys

import numpy as np
import pytest

import ray_battery as rb
import rccl_stub
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B, scene_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_, H_, SPP, DEPTH = 48, 40, 64, 16
COUNTERS = ("samples", "rays", "scatters", "env_misses")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_frame(a, b, what):
    bad = _bits(a) != _bits(b)
    assert not bad.any(), "%s: %d of %d floats differ" % (what, bad.sum(), bad.size)


def _ctx(scene, dynamic=1, meshes=None, device=0, **kw):
    ctx = B.Context(device)
    ctx.set_option("dynamic", dynamic)
    opts = {k: kw.pop(k) for k in list(kw) if k in ("leaf_size", "wide_leaves", "leaf_align", "node_pairs")}
    for k, v in opts.items():
        ctx.set_option(k, v)
    RC.upload(ctx, scene, meshes, **kw)
    return ctx


# ---------------------------------------------------------------------------------------------------------------------
# 1. what the kernels wrote
# ---------------------------------------------------------------------------------------------------------------------
DEVICE_CASES = [("one_tri", {}), ("two_tris", dict(leaf_size=1)), ("two_tris", {}), ("meshes", {}), ("meshes", dict(leaf_size=1, wide_leaves=0)), ("meshes", dict(leaf_size=7)),
                ("rects", dict(leaf_align=4)), ("rects", dict(node_pairs=1, leaf_align=3)), ("cornell", {}), ("cornell", dict(leaf_size=1))]


@pytest.mark.parametrize("name,opts", DEVICE_CASES, ids=["%s-%s" % (n, "-".join("%s%d" % kv for kv in o.items()) or "default") for n, o in DEVICE_CASES])
def test_device_arrays_equal_the_host_twin(name, opts):
    scene = RC.make_scene(name)
    ctx = _ctx(scene, **opts)
    host = _ctx(scene, device=-1, **opts)  # the twin by itself, on a context that never saw the device
    uploaded = ctx.export_trees()
    RC.same_arrays(uploaded, ctx.export_trees(device=True), "%s: HBM after the upload" % name)
    for k in (0, 1, 2):
        mv = RC.moved(scene, k)
        ctx.update_vertices(mv)
        host.update_vertices(mv)
        dev = ctx.export_trees(device=True)
        RC.same_arrays(host.export_trees(), dev, "%s, update %d: HBM against the host twin" % (name, k))
        RC.same_arrays(ctx.export_trees(), dev, "%s, update %d: HBM against the context's own host copies (lazy twin)" % (name, k))
        if k == 0:
            RC.same_arrays(uploaded, dev, "%s: HBM after the identity update" % name)
        a, b = ctx.update_info(), host.update_info()
        assert a["pad"].view(np.uint32) == b["pad"].view(np.uint32) == dev["pad"].view(np.uint32)
        assert a["slivers"] == b["slivers"] == RC.point_triangles(dev) and a["levels"] == b["levels"] == uploaded["depth"]
        assert a["h2d_bytes"] == sum(m["vertices"].nbytes + m["normals"].nbytes for m in mv) and (a["device_ms"] > 0 or uploaded["tris"].size == 0)
    ctx.quad_info()
    ctx.oct_info()
    ctx.close()
    host.close()


def test_device_export_flag():
    scene = RC.make_scene("rects")
    ctx = _ctx(scene)
    L = B.lib()
    need = L.pt_debug_export_tree(ctx._h, 1 | B.PT_TREE_DEVICE, None, 0)
    assert need == L.pt_debug_export_tree(ctx._h, 1, None, 0) > 0
    buf = np.zeros(int(need), np.uint8)
    assert L.pt_debug_export_tree(ctx._h, 1 | B.PT_TREE_DEVICE, buf.ctypes.data, need - 1) == -1  # PT_E_INVALID
    assert L.pt_debug_export_tree(ctx._h, 9 | B.PT_TREE_DEVICE, None, 0) == -1
    assert L.pt_debug_export_tree(ctx._h, 4 | B.PT_TREE_DEVICE, None, 0) == 64  # PT_TREE_INFO: the host's either way
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. frames
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_moved(orc):
    """Context A: upload + update with movement 1.  Context B: a fresh upload of the moved scene.  The oracle's scene of the moved meshes."""
    scene = RC.make_scene("cornell")
    materials = RC.cornell_materials()
    mats = [m for _, m, _ in materials]
    mv = RC.moved(scene, 1)
    env = B.make_env(**RC.CORNELL_ENV)
    a = _ctx(scene, materials=mats, env=env)
    first, _ = a.render(RC.cornell_camera(W_, H_, B.to_camera_data), W_, H_, SPP, DEPTH)
    a.update_vertices(mv)
    b = _ctx(scene, dynamic=0, meshes=mv, materials=mats, env=env)
    S = orc.Scene(scene_io.flatten_scene(RC.as_entities(scene, mv), materials))
    yield dict(scene=scene, mats=mats, mv=mv, a=a, b=b, S=S, first=first, cam=RC.cornell_camera(W_, H_, B.to_camera_data), ocam=RC.cornell_camera(W_, H_, orc.to_camera_data), want={})
    a.close()
    b.close()


def _oracle_frame(orc, cm, watertight):
    if watertight not in cm["want"]:
        cm["S"].set_watertight(bool(watertight))
        cm["want"][watertight] = cm["S"].render(cm["ocam"], orc.make_env(**RC.CORNELL_ENV), W_, H_, SPP, DEPTH, want_rgba8=True, want_counters=True)
    return cm["want"][watertight]


PATHS = [("default path", {}, {}), ("group walk always", {"groups": 2}, {"groups": 1}), ("fallback instance", {"fallback": 1}, {"fallback": 0}),
         ("subtracting slab form", {"box_exact": 1}, {"box_exact": -1}), ("lane per pixel", {"kernel": 1}, {"kernel": 2}), ("watertight", {"watertight": 1}, {"watertight": 0})]


@pytest.mark.parametrize("label,opts,reset", PATHS, ids=[p[0].replace(" ", "_") for p in PATHS])
def test_frame_after_update_is_the_fresh_uploads_and_the_oracles(orc, cornell_moved, label, opts, reset):
    cm = cornell_moved
    want, want8, cnt = _oracle_frame(orc, cm, opts.get("watertight", 0))
    assert np.isfinite(want).all() and want.std() > 0.01
    assert (_bits(want) != _bits(cm["first"])).any(), "the moved scene gives another frame"
    got = {}
    for who in ("a", "b"):
        ctx = cm[who]
        try:
            for k, v in opts.items():
                ctx.set_option(k, v)
            rgb, rgba8 = ctx.render(cm["cam"], W_, H_, SPP, DEPTH, want_rgba8=True)
            st = ctx.stats()
            ctx.set_option("count", 1)  # the instrumented instance (it has no fallback form: a counted render never runs variant 3)
            counted, counted8 = ctx.render(cm["cam"], W_, H_, SPP, DEPTH, want_rgba8=True)
            cst = ctx.stats()
        finally:
            ctx.set_option("count", 0)
            for k, v in reset.items():
                ctx.set_option(k, v)
        if "fallback" in opts:
            assert st["kernel_variant"] == 3
        if "kernel" in opts:
            assert st["kernel_variant"] == 1
        _same_frame(counted, rgb, "%s, context %s: instrumented instance == product instance" % (label, who))
        np.testing.assert_array_equal(counted8, rgba8)
        got[who] = (rgb, rgba8, {k: int(cst[k]) for k in COUNTERS})
    for who, what in (("a", "update + render"), ("b", "fresh upload + render")):
        _same_frame(got[who][0], want, "%s, %s == the oracle" % (label, what))
        np.testing.assert_array_equal(got[who][1], want8)
        assert got[who][2] == {k: int(cnt[k]) for k in COUNTERS}, (label, what)
    _same_frame(got["a"][0], got["b"][0], label + ": update == fresh upload")


def test_batch_after_an_update_is_the_loop_of_single_renders(cornell_moved):
    cm = cornell_moved
    c = scene_io.load_scene_dir(RC.ASSETS, "cornell-box")["camera"]
    lf = np.asarray(c["look_from"], np.float64)
    cams = [cm["cam"], B.to_camera_data(list(lf + [0.3, 0.2, -0.1]), c["look_at"], c["look_up"], c["vertical_fov"] * 0.8, W_, H_)]
    rgb, rgba8 = cm["a"].render_batch([(cam, None) for cam in cams], W_, H_, SPP, DEPTH, want_rgba8=True, n_materials=len(cm["mats"]))
    for i, cam in enumerate(cams):
        one, one8 = cm["a"].render(cam, W_, H_, SPP, DEPTH, want_rgba8=True)
        _same_frame(rgb[i], one, "frame %d of the batch" % i)
        np.testing.assert_array_equal(rgba8[i], one8)
    assert (_bits(rgb[0]) != _bits(rgb[1])).any()


def test_four_updates_and_back(cornell_moved):
    """On a context of its own (the fixture's stays at movement 1)."""
    cm = cornell_moved
    scene = cm["scene"]
    ctx = _ctx(scene, materials=cm["mats"], env=B.make_env(**RC.CORNELL_ENV))
    uploaded = ctx.export_trees()
    first, first8 = ctx.render(cm["cam"], W_, H_, SPP, DEPTH, want_rgba8=True)
    _same_frame(first, cm["first"], "two contexts, one scene")
    for k in (1, 2, 3, 4):
        ctx.update_vertices(RC.moved(scene, k, amp=0.02 * k))
    other, _ = ctx.render(cm["cam"], W_, H_, SPP, DEPTH)
    assert (_bits(other) != _bits(first)).any()
    ctx.update_vertices(RC.moved(scene, 0))
    back, back8 = ctx.render(cm["cam"], W_, H_, SPP, DEPTH, want_rgba8=True)
    _same_frame(back, first, "four updates and back")
    np.testing.assert_array_equal(back8, first8)
    RC.same_arrays(uploaded, ctx.export_trees(device=True), "four updates and back: HBM against the uploaded arrays")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. normals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("new_normals", [True, False], ids=["normals_passed", "normals_null"])
def test_normals_follow_or_stay(orc, new_normals):
    from test_gpu_watertight import _scene_icospheres

    sc = _scene_icospheres()
    scene = (sc["ents"], len(sc["mats"]), 2)  # the movement shifts the small emitter away (three extents); the environment map still lights the two spheres
    W, H, spp, depth = sc["size"]
    up = dict(materials=sc["mats"], textures=sc["textures"], mesh_textures=sc["mesh_textures"])
    mv = RC.moved(scene, 1, amp=0.02, with_normals=new_normals)
    ctx = _ctx(scene, env=B.make_env(**sc["env"]), **up)
    ctx.update_vertices(mv if new_normals else [dict(vertices=m["vertices"]) for m in mv])
    fresh = _ctx(scene, dynamic=0, meshes=mv, env=B.make_env(**sc["env"]), **up)  # (without new normals, mv carries the old ones)
    names = [("glass", sc["mats"][0], ""), ("metal", sc["mats"][1], ""), ("glow", sc["mats"][2], "")]
    S = orc.Scene(scene_io.flatten_scene(RC.as_entities(scene, mv), names, {0: sc["textures"][0], 1: sc["textures"][0]}))
    stale = orc.Scene(scene_io.flatten_scene(RC.as_entities(scene, RC.moved(scene, 1, amp=0.02, with_normals=not new_normals)), names, {0: sc["textures"][0], 1: sc["textures"][0]}))
    for i, (frm, at, upv, fov) in enumerate(sc["cameras"]):
        ocam = orc.to_camera_data(tuple(frm), tuple(at), tuple(upv), fov, W, H)
        want, want8, _ = S.render(ocam, orc.make_env(**sc["env"]), W, H, spp, depth, want_rgba8=True)
        other, _, _ = stale.render(ocam, orc.make_env(**sc["env"]), W, H, spp, depth)
        assert (_bits(want) != _bits(other)).any(), "camera %d: the normals reach the shading (the other set of normals gives another frame)" % i
        cam = B.to_camera_data(frm, at, upv, fov, W, H)
        got, got8 = ctx.render(cam, W, H, spp, depth, want_rgba8=True)
        ref, ref8 = fresh.render(cam, W, H, spp, depth, want_rgba8=True)
        _same_frame(got, ref, "camera %d: update == fresh upload" % i)
        _same_frame(got, want, "camera %d: update == the oracle" % i)
        np.testing.assert_array_equal(got8, want8)
        np.testing.assert_array_equal(ref8, want8)
    ctx.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. ray probes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rects", "soup2"])
def test_probes_after_an_update_equal_the_oracles_brute_force(orc, name):
    scene = RC.make_scene(name)
    mv = RC.moved(scene, 1)
    tris = RC.soup_of(RC.as_entities(scene, mv))
    S = rb.oracle_scene(orc, tris)
    rays, cls = rb.make_rays(tris, np.random.default_rng(4242), 200, hit_fn=lambda r: S.intersect_n(r, use_bvh=True)[:2])
    held = rb.bands(rays, rb.scene_measure(tris), cls)[0]
    assert held.sum() > 0.7 * held.size
    truth = S.intersect_n(rays, use_bvh=False)
    assert 0.02 < truth[0][held].mean() < 0.999
    for leaf in (1, 4):
        ctx = _ctx(scene, leaf_size=leaf)
        ctx.update_vertices(mv)
        for op in B.PROBE_OPS:
            out = ctx.debug_eval(op, rays, 6)
            got = (out[:, 0] != 0, out[:, 1], out[:, 2], out[:, 3], np.ascontiguousarray(out[:, 4]).view(np.int32))
            bad = (got[0] != truth[0]) | (got[4] != truth[4])
            for k in ((2, 3) if op.startswith("group") else (1, 2, 3)):  # (the group walk carries no t)
                bad |= truth[0] & (np.ascontiguousarray(got[k]).view(np.uint32) != truth[k].view(np.uint32))
            bad = np.nonzero(bad & held)[0]
            assert bad.size == 0, "%s on %s after an update, leaf %d: %d of %d rays inside the domain differ from brute force; first: class %d %r" % (
                op, name, leaf, bad.size, held.sum(), cls[bad[0]], rays[bad[0]].tolist())
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. group
# ---------------------------------------------------------------------------------------------------------------------
def test_group_update(cornell_moved, tmp_path):
    cm = cornell_moved
    out = str(tmp_path / "got")
    rc, so, se = rccl_stub.run_child([sys.executable, os.path.join(ROOT, "tests", "refit_group_child.py"), out, "0,0", "1", str(W_), str(H_), str(SPP), str(DEPTH)],
                                     rccl_stub.stub_env(), 300)
    assert rc == 0, "child exited with %s\n%s\n%s" % (rc, so[-2000:], se[-4000:])
    info = json.load(open(os.path.join(out, "info.json")))
    assert info["size"] == 2
    want, want8 = cm["a"].render(cm["cam"], W_, H_, SPP, DEPTH, want_rgba8=True)
    _same_frame(np.load(os.path.join(out, "before_rgb.npy")), cm["first"], "group of 2 before the update")
    _same_frame(np.load(os.path.join(out, "after_rgb.npy")), want, "group of 2 after pt_group_update_vertices")
    np.testing.assert_array_equal(np.load(os.path.join(out, "after_rgba8.npy")), want8)
    single = cm["a"].update_info()
    for r in info["ranks"]:  # every device refitted its own replica
        assert r["levels"] == single["levels"] > 0 and r["slivers"] == single["slivers"] and np.float32(r["pad"]) == single["pad"] and r["h2d_bytes"] == single["h2d_bytes"] and r["device_ms"] > 0
