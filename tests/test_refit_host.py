"""pt_update_vertices on host-only contexts: the host twin of the refit (pt_bvh_refit + the gather of pt_scene.cpp).  No GPU.

Everything is compared on raw bits.  The scenes, the movement and the numpy definition of a box are in tests/refit_common.py: one
triangle (the root is a leaf code, no node), two triangles (one node), four meshes with different vertex bases - one of them without
triangles, unreferenced vertices that are huge or not finite, triangles on both sides of the sliver threshold and with NaN / infinite
corners -, the battery's rectangles, and the Cornell box (17 974 triangles).

1. identity: update with the uploaded arrays -> the five exported arrays unchanged; leaf sizes 1 / 4 / 7, wide_leaves 0 / 1, and the
   leaf_align / node_pairs layouts.
2. moved scene: references and the order of triangle ids unchanged; every box of the binary, quad and oct arrays equals the numpy
   recomputation from the definition; the structure checks of tests/ray_battery.py and pt_debug_quad_info / _oct_info pass.
3. PT_TREE_TRIS sorted by id equals that of a fresh upload of the moved scene; the sliver count of pt_debug_update_info is the number of
   point triangles there; the movement drives triangles across the threshold in both directions.
4. pt_debug_closest_hit_host_n after the update == after a fresh upload of the moved scene, on every battery ray inside the 10-extent
   domain, watertight 0 and 1: hit, id, t, u, v.
5. four updates and back: the arrays of the upload, byte for byte (the refit carries no state).
6. refusals leave the scene as it was; "dynamic" = 0 uploads the same arrays; the ABI version is 5.
7. this file once more against the ASan + UBSan build of the library.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_battery as rb
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(1, 1), (4, 1), (7, 1), (1, 0), (4, 0), (7, 0)]  # (leaf_size, wide_leaves)
LAYOUTS = [dict(leaf_align=4), dict(node_pairs=1), dict(leaf_align=3, node_pairs=1)]
IN_ASAN_CHILD = os.environ.get("PT_REFIT_ASAN_CHILD") == "1"
SCENES = ["one_tri", "two_tris", "meshes", "rects"] + ([] if IN_ASAN_CHILD else ["cornell"])  # (the sanitized run: the small scenes)
_scenes = {}


def _scene(name):
    if name not in _scenes:
        _scenes[name] = RC.make_scene(name)
    return _scenes[name]


def _ctx(scene, leaf=4, wide=1, dynamic=1, meshes=None, **opts):
    ctx = B.Context(-1)
    ctx.set_option("leaf_size", leaf)
    ctx.set_option("wide_leaves", wide)
    ctx.set_option("dynamic", dynamic)
    for k, v in opts.items():
        ctx.set_option(k, v)
    RC.upload(ctx, scene, meshes)
    return ctx


def _collapsed(ex):
    t = RC.tris_by_id(ex)
    return np.stack([t["p0"], t["p1"], t["p2"]], 1)


@pytest.mark.parametrize("name", SCENES)
def test_identity(name):
    scene = _scene(name)
    for kw in [dict(leaf=l, wide=w) for l, w in CONFIGS] + LAYOUTS:
        ctx = _ctx(scene, **kw)
        before = ctx.export_trees()
        ctx.update_vertices(RC.moved(scene, 0))
        RC.same_arrays(before, ctx.export_trees(), "%s %r: update with the uploaded arrays" % (name, kw))
        assert before["pad"].view(np.uint32) == ctx.export_trees()["pad"].view(np.uint32)
        ctx.close()


@pytest.mark.parametrize("name", SCENES)
def test_moved_scene_boxes_are_the_definition(name):
    scene = _scene(name)
    mv = RC.moved(scene, 1)
    for kw in [dict(leaf=l, wide=w) for l, w in CONFIGS] + LAYOUTS:
        ctx = _ctx(scene, **kw)
        before = ctx.export_trees()
        ctx.update_vertices(mv)
        ex = ctx.export_trees()
        what = "%s %r" % (name, kw)
        # the topology is the upload's
        assert np.array_equal(before["nodes"]["left"], ex["nodes"]["left"]) and np.array_equal(before["nodes"]["right"], ex["nodes"]["right"]), what
        assert np.array_equal(before["nodes4"]["child"], ex["nodes4"]["child"]) and np.array_equal(before["nodes8"]["c"]["ref"], ex["nodes8"]["c"]["ref"]), what
        assert np.array_equal(before["tris"]["id"], ex["tris"]["id"]) and np.array_equal(before["tris"]["material"], ex["tris"]["material"]), what
        assert all(before[k] == ex[k] for k in ("root", "root4", "root8", "depth", "depth4", "depth8", "max_leaf")), what
        # the boxes are the definition's, from the triangle records of a FRESH upload of the moved scene
        fresh = _ctx(scene, dynamic=0, meshes=mv, **kw)
        V = _collapsed(fresh.export_trees())
        fresh.close()
        RC.assert_boxes(ex, V, what)
        if name in ("meshes", "rects", "cornell"):
            assert ex["pad"] != before["pad"], "the shift of one mesh by three extents changes the pad"
        if "node_pairs" not in kw:  # (check_structure wants every node referenced: the sibling-pair layout has holes)
            rb.check_structure(ex, kw.get("wide", 1))
        ctx.quad_info()
        ctx.oct_info()
        ctx.close()


@pytest.mark.parametrize("name", SCENES)
def test_triangle_records_and_sliver_count(name):
    scene = _scene(name)
    ctx = _ctx(scene)
    points = []
    for k in (0, 1, 2):
        mv = RC.moved(scene, k)
        ctx.update_vertices(mv)
        fresh = _ctx(scene, dynamic=0, meshes=mv)
        want = RC.tris_by_id(fresh.export_trees())
        got = RC.tris_by_id(ctx.export_trees())
        assert got.tobytes() == want.tobytes(), "%s, update %d: triangle records differ from a fresh upload's" % (name, k)
        n_points = RC.point_triangles(fresh.export_trees())
        assert ctx.update_info()["slivers"] == n_points, (name, k)
        assert ctx.update_info()["pad"].view(np.uint32) == fresh.export_trees()["pad"].view(np.uint32)
        assert np.isfinite(np.stack([want["p0"], want["p1"], want["p2"]])).all(), "collapsed records are finite"
        points.append(((want["p0"] == want["p1"]) & (want["p0"] == want["p2"])).all(1))
        fresh.close()
    ctx.close()
    if name in ("meshes", "rects", "cornell"):
        assert points[0].any() and not points[0].all()
        for a, b in ((points[0], points[1]), (points[1], points[2])):
            assert (a & ~b).any() and (~a & b).any(), "the movement drives triangles across the sliver threshold in both directions"


@pytest.mark.parametrize("name", ["rects", "soup2"] + ([] if IN_ASAN_CHILD else ["cornell"]))
def test_host_closest_hit_equals_a_fresh_upload(name):
    scene = _scene(name)
    mv = RC.moved(scene, 1)
    fresh = _ctx(scene, dynamic=0, meshes=mv)
    V = _collapsed(fresh.export_trees())  # finite: what the battery aims at
    rays, cls = rb.make_rays(V, np.random.default_rng(4242), 150 if name == "cornell" else 400)
    held = rb.bands(rays, rb.scene_measure(V), cls)[0]
    assert held.sum() > 0.7 * held.size
    ctx = _ctx(scene)
    ctx.update_vertices(mv)
    for wt in (0, 1):
        ctx.set_option("watertight", wt)
        fresh.set_option("watertight", wt)
        got, want = ctx.closest_hit_host_n(rays), fresh.closest_hit_host_n(rays)
        assert 0.02 < want[0][held].mean() < 0.999
        bad = (got[0] != want[0]) | (got[4] != want[4])
        for k in (1, 2, 3):
            bad |= got[k].view(np.uint32) != want[k].view(np.uint32)
        bad = np.nonzero(bad & held)[0]
        assert bad.size == 0, "%s, watertight %d: %d of %d rays inside the domain differ; first: class %d %r" % (name, wt, bad.size, held.sum(), cls[bad[0]], rays[bad[0]].tolist())
    ctx.close()
    fresh.close()


@pytest.mark.parametrize("name", SCENES)
def test_four_updates_and_back(name):
    scene = _scene(name)
    for kw in (dict(leaf=4, wide=1), dict(leaf=1, wide=0), dict(leaf_align=4)):
        ctx = _ctx(scene, **kw)
        first = ctx.export_trees()
        for k in (1, 2, 3, 4):
            ctx.update_vertices(RC.moved(scene, k, amp=0.02 * k))
        assert ctx.export_trees()["tris"].tobytes() != first["tris"].tobytes()
        ctx.update_vertices(RC.moved(scene, 0))
        RC.same_arrays(first, ctx.export_trees(), "%s %r: four updates and back" % (name, kw))
        ctx.close()


def test_only_the_named_arrays_are_read_and_null_means_unchanged():
    """vertices = NULL leaves a mesh where it is, normals = NULL keeps the normals; indices and the other fields are not looked at."""
    scene = _scene("meshes")
    mv = RC.moved(scene, 1)
    ctx = _ctx(scene)
    ctx.update_vertices([mv[0], None, None, None])  # only mesh 0 moves
    part = [mv[0]] + [m for m, _ in scene[0]][1:]
    fresh = _ctx(scene, dynamic=0, meshes=part)
    assert RC.tris_by_id(ctx.export_trees()).tobytes() == RC.tris_by_id(fresh.export_trees()).tobytes()
    RC.assert_boxes(ctx.export_trees(), _collapsed(fresh.export_trees()), "one mesh of four moved")
    fresh.close()
    ctx.close()


def test_refusals_leave_the_scene_as_it_was():
    scene = _scene("meshes")
    meshes = RC.moved(scene, 1)
    L = B.lib()
    assert L.pt_abi_version() == 5
    empty = B.Context(-1)
    with pytest.raises(B.PtError, match=r"\(-4\)"):  # PT_E_NO_SCENE
        empty.update_vertices(meshes)
    static = _ctx(scene, dynamic=0)
    dynamic = _ctx(scene, dynamic=1)
    a, b = static.export_trees(), dynamic.export_trees()
    RC.same_arrays(a, b, "dynamic = 0 and dynamic = 1 upload the same arrays")
    assert a["pad"].view(np.uint32) == b["pad"].view(np.uint32)
    with pytest.raises(B.PtError, match=r"\(-1\).*dynamic"):  # PT_E_INVALID, and the message says why
        static.update_vertices(meshes)
    RC.same_arrays(a, static.export_trees(), "after the refusal on a static scene")
    refused = [
        ("a mesh short", meshes[:-1]),
        ("a mesh more", meshes + [meshes[0]]),
        ("a vertex count that differs", [dict(meshes[0], n_vertices=meshes[0]["vertices"].shape[0] - 1)] + meshes[1:]),
        ("a normal count that differs", meshes[:2] + [dict(meshes[2], n_normals=1)] + meshes[3:]),
        ("a count that differs on a mesh passed as unchanged", [meshes[0], dict(n_vertices=2, n_normals=3)] + meshes[2:]),
    ]
    for what, arg in refused:
        with pytest.raises(B.PtError, match=r"\(-1\)"):
            dynamic.update_vertices(arg)
        RC.same_arrays(b, dynamic.export_trees(), "after the refused call with " + what)
    assert L.pt_update_vertices(dynamic._h, None, len(meshes)) == -1  # a NULL mesh array with a non-zero count
    assert L.pt_update_vertices(None, None, 0) == -1
    RC.same_arrays(b, dynamic.export_trees(), "after the refused call with a NULL mesh array")
    assert dynamic.update_info()["levels"] == 0, "no update has run yet"
    with pytest.raises(B.PtError, match=r"\(-1\)"):
        dynamic.set_option("dynamic", 2)
    with pytest.raises(B.PtError, match=r"\(-1\).*host-only"):  # PT_TREE_DEVICE needs a device
        dynamic._export(0 | B.PT_TREE_DEVICE, B.NODE_DTYPE)
    dynamic.update_vertices(meshes)  # and the context still takes a good call
    assert dynamic.update_info()["levels"] == b["depth"] > 0
    assert dynamic.export_trees()["nodes"].tobytes() != b["nodes"].tobytes()
    # a later upload with dynamic = 0 drops what the updates needed
    dynamic.set_option("dynamic", 0)
    RC.upload(dynamic, scene)
    with pytest.raises(B.PtError, match=r"\(-1\).*dynamic"):
        dynamic.update_vertices(meshes)
    for c in (empty, static, dynamic):
        c.close()


def test_clone_takes_the_moved_scene_and_can_be_updated():
    """pt_debug_clone_scene (the replicas of a group) after an update: the clone holds the moved scene and what further updates need."""
    scene = _scene("rects")
    src, dst = _ctx(scene), B.Context(-1)
    src.update_vertices(RC.moved(scene, 1))
    dst.clone_scene_from(src)
    RC.same_arrays(src.export_trees(), dst.export_trees(), "clone after an update")
    dst.update_vertices(RC.moved(scene, 2), counts=src._counts)
    src.update_vertices(RC.moved(scene, 2))
    RC.same_arrays(src.export_trees(), dst.export_trees(), "clone and source after the same further update")
    src.close()
    dst.close()


@pytest.mark.skipif(IN_ASAN_CHILD, reason="this is the sanitized run")
def test_this_file_against_the_sanitized_library():
    """As tests/test_sanitizers.py runs test_abi_host.py: the host twin, the retained arrays and the refusals under ASan + UBSan."""
    pkg = os.path.join(ROOT, "owl-path-tracer_amd")
    try:
        subprocess.check_call(["make", "-C", os.path.join(pkg, "csrc"), "-s", "asan"], timeout=600)
    except (subprocess.CalledProcessError, OSError) as e:
        pytest.skip("sanitizer build unavailable: %s" % e)
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    libubsan = subprocess.check_output(["gcc", "-print-file-name=libubsan.so"], text=True).strip()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               PT_LIB_PATH=os.path.join(pkg, "libmi355pt_asan.so"), LD_PRELOAD=libasan + ":" + libubsan, PT_REFIT_ASAN_CHILD="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=1200, env=env,
                       cwd=ROOT, errors="replace")
    text = r.stdout + r.stderr
    assert "AddressSanitizer" not in text and "runtime error:" not in text, text[-4000:]
    assert r.returncode == 0, text[-4000:]
