"""The two device BVH builders of csrc/pt_lbvh.hip (bvh_builder 1: linear BVH after Karras, 2: PLOC + pt_bvh_from_hierarchy) against
the numpy references of tests/builder_ref.py, bit for bit, and the three ways in which build_bvh hands over to the host builder.

Equality means: the canonical form (pre-order; per node the raw bits of both child boxes, per leaf the ordered tuple of real triangle
ids), the pad bit for bit, depth and max_leaf.  tests/test_builder_ref_host.py holds the references to their definitions and asserts
what this file expects of every case (a device tree where the reference is shallow enough, a fallback where it is not).

1. equality with the reference on every case of builder_ref.CASE_NAMES at leaf sizes 1 / 4 / 7 (PLOC: also ploc_radius 1 and 64 at
   leaf size 4).  A combination with no more than leaf_size triangles (n = 2, 3 at leaf sizes 4 and 7) never reaches the device: it is
   compared with builder 0 byte for byte instead, as in test 5.  From 64 triangles on the form must differ from builder 0's, so a
   silent hand-over to the host builder cannot pass for a device tree.
2. the same upload twice on one context: byte-identical exports.
3. the Cornell box under max_bvh_depth = 14: both device trees are deeper (reference: 22 and 25 levels), the host builder takes over,
   nothing of the abandoned build shows in the export or in a frame, and the device tree is back with max_bvh_depth = 48.
4. the round budget of PLOC: an upload that would need more than 4096 rounds succeeds with the host builder's tree.  Before this
   test existed such an upload failed with PT_E_HIP ("device PLOC build failed: unknown error").
5. no more than leaf_size triangles: builder 0's tree, n = 1 included.

PT_WRITE_PROFILES=1 records reference figures, node counts and seconds in profiles/r12_device_builders.json, section "gpu".
"""
import os
import time

import numpy as np
import pytest

import builder_ref as br
import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

pytestmark = pytest.mark.gpu

W_, H_, SPP, DEPTH = 64, 48, 4, 16
_report = {"cases": {}, "seconds": {}}


@pytest.fixture(scope="module")
def ctxs():
    """One context per builder."""
    c = {b: B.Context(0) for b in (0, 1, 2)}
    for b, ctx in c.items():
        ctx.set_option("bvh_builder", b)
    yield c
    for ctx in c.values():
        ctx.close()


def build(ctx, tris, leaf=4, radius=br.DEFAULT_RADIUS, max_depth=br.DEFAULT_MAX_DEPTH):
    ctx.set_option("leaf_size", leaf)
    ctx.set_option("ploc_radius", radius)
    ctx.set_option("max_bvh_depth", max_depth)
    ctx.upload_scene([(rb.mesh_of(tris), 0)], [scene_io.MAT_DEFAULT], env=B.make_env(use_auto=True, intensity=1.0))
    return ctx.export_trees()


def assert_device_copy(ctx, ex):
    """The arrays in HBM are the host copies, byte for byte."""
    dev = ctx.export_trees(device=True)
    for k in ("nodes", "nodes4", "nodes8", "tris"):
        assert dev[k].tobytes() == ex[k].tobytes(), "%s in HBM differs from the host copy" % k


def frame(ctx, cam):
    rgb, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
    return rgb


def timed(name):
    class T:
        def __enter__(self):
            self.t0 = time.time()

        def __exit__(self, *a):
            _report["seconds"][name] = round(_report["seconds"].get(name, 0.0) + time.time() - self.t0, 3)

    return T()


# ---------------------------------------------------------------------------------------------------------------------
# 1. equality with the reference
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", br.CASE_NAMES)
@pytest.mark.parametrize("builder", (1, 2))
def test_equals_reference(ctxs, builder, name):
    compared = 0
    with timed("test_equals_reference[%d-%s]" % (builder, name)):
        for leaf, radius in br.combos(builder):
            tris = br.scene_cases(leaf)[name]
            what = "%s, builder %d, leaf_size %d, ploc_radius %d" % (name, builder, leaf, radius)
            ex = build(ctxs[builder], tris, leaf, radius)
            ex0 = build(ctxs[0], tris, leaf, radius)
            P = br.positions_of(ex)
            assert P.shape[0] == tris.shape[0]
            if tris.shape[0] <= leaf:  # never reaches the device: builder 0's tree
                assert br.export_bytes(ex) == br.export_bytes(ex0), what
            else:
                ref, h = br.reference(P, builder, leaf, radius)
                diff = br.same_tree(ex, ref)
                assert diff is None, "%s: %s" % (what, diff)
                if tris.shape[0] >= 64:
                    assert br.form_of_export(ex) != br.form_of_export(ex0), "%s: the tree is builder 0's" % what
                _report["cases"]["%s/builder%d/leaf%d/radius%d" % (name, builder, leaf, radius if builder == 2 else 0)] = dict(
                    triangles=int(P.shape[0]), reference_depth=ref.depth, reference_nodes=ref.n_nodes, nodes=int(ex["nodes"].size),
                    **({"rounds": h.rounds} if builder == 2 else {}))
            compared += 1
            rb.check_structure(ex)
            assert_device_copy(ctxs[builder], ex)
    assert compared == len(br.combos(builder))


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("soup2000", "cornell"))
@pytest.mark.parametrize("builder", (1, 2))
def test_same_upload_twice(ctxs, builder, name):
    """A k_fit that read a sibling's box before it was published, or PLOC node numbers (an atomicAdd) leaking into the layout, would
    differ between two builds."""
    tris = br.scene_cases(4)[name]
    ctx = ctxs[builder]
    with timed("test_same_upload_twice[%d-%s]" % (builder, name)):
        first = build(ctx, tris)
        first_dev = ctx.export_trees(device=True)
        second = build(ctx, tris)
        second_dev = ctx.export_trees(device=True)
    assert br.export_bytes(first) == br.export_bytes(second)
    assert br.export_bytes(first_dev) == br.export_bytes(second_dev)


# ---------------------------------------------------------------------------------------------------------------------
# 3. depth fallback
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_scene():
    sc = scene_io.load_scene_dir(rb.ASSETS, "cornell-box")
    c = sc["camera"]
    sc["cam"] = B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W_, H_)
    sc["mats"] = [m for _, m, _ in sc["materials"]]
    return sc


def upload_cornell(ctx, sc, max_depth):
    ctx.set_option("leaf_size", 4)
    ctx.set_option("ploc_radius", br.DEFAULT_RADIUS)
    ctx.set_option("max_bvh_depth", max_depth)
    ctx.upload_scene(sc["entities"], sc["mats"], env=B.make_env(color=(1, 1, 1), intensity=0.0))
    return ctx.export_trees()


@pytest.mark.parametrize("builder", (1, 2))
def test_depth_fallback(ctxs, cornell_scene, builder):
    ctx, sc = ctxs[builder], cornell_scene
    with timed("test_depth_fallback[%d]" % builder):
        # a device tree first, so that HBM and the host arrays hold something the abandoned build could leave behind
        ex = upload_cornell(ctx, sc, br.DEFAULT_MAX_DEPTH)
        P = br.positions_of(ex)
        ref, _ = br.reference(P, builder, 4)
        assert ref.too_deep(br.FALLBACK_DEPTH, builder)
        assert br.same_tree(ex, ref) is None
        ex = upload_cornell(ctx, sc, br.FALLBACK_DEPTH)  # succeeds
        ex0 = upload_cornell(ctxs[0], sc, br.FALLBACK_DEPTH)
        assert br.export_bytes(ex) == br.export_bytes(ex0), "the fallback tree is not builder 0's"
        assert 0 < ex["depth"] <= br.FALLBACK_DEPTH
        assert ctx.stats()["bvh_depth"] == ex["depth"] and ctx.stats()["bvh_nodes"] == ex["nodes"].size
        rb.check_structure(ex)
        assert_device_copy(ctx, ex)
        got, want = frame(ctx, sc["cam"]), frame(ctxs[0], sc["cam"])
        assert len(np.unique(want)) > 16, "the frame shows the scene"
        assert got.tobytes() == want.tobytes(), "a frame after the fallback differs from builder 0's"
        ex = upload_cornell(ctx, sc, br.DEFAULT_MAX_DEPTH)  # and back
        diff = br.same_tree(ex, ref)
        assert diff is None, diff
        assert_device_copy(ctx, ex)
        assert frame(ctx, sc["cam"]).tobytes() == want.tobytes()
    _report["cases"]["depth_fallback/builder%d" % builder] = dict(reference_depth=ref.depth, max_bvh_depth=br.FALLBACK_DEPTH, fallback_depth=int(ex0["depth"]))


# ---------------------------------------------------------------------------------------------------------------------
# 4. round cap
# ---------------------------------------------------------------------------------------------------------------------
def test_round_cap(ctxs):
    """ray_battery.strip_scene(9000): the reference needs 4 088 rounds and 22 levels, so the device tree stands, and it is the
    reference's (its digest is recorded in tests/golden/ploc_strip_rounds.json and recomputed by test_builder_ref_host.py: 6 s of numpy
    that this file leaves out).  Lengthening that strip does not reach the cap - float32 rounds its growing widths into a jitter from
    x ~ 2^16 on, many pairs are mutual at once and the count levels off: 4 091 rounds at 12 000 triangles, 4 095 at 20 000, the largest
    reference input allowed here.  builder_ref.level_strip(9000), equal widths, keeps one mutual pair per round: 4 515 rounds in the
    reference, beyond the cap.  That upload must succeed with builder 0's tree.
    Measured on an MI355X (profiles/r12_device_builders.json): 0.23 s for the upload with 4 088 rounds, 0.24 s for the one that gives
    up after 4 096 and builds on the host; the whole test 0.6 s."""
    gold = br.golden_rounds()
    ctx = ctxs[2]
    g = gold["strip_scene_%d" % br.STRIP_N]
    assert g["rounds"] <= br.PLOC_ROUND_CAP < gold["level_strip_%d" % br.STRIP_N]["rounds"]
    # the sliver strip: within the budget
    tris = rb.strip_scene(br.STRIP_N)
    t0 = time.time()
    ex = build(ctx, tris)  # succeeds
    _report["seconds"]["upload strip_scene(%d), %d rounds on the device" % (br.STRIP_N, g["rounds"])] = round(time.time() - t0, 3)
    ex0 = build(ctxs[0], tris)
    is_reference = br.form_digest(br.form_of_export(ex), ex["pad"], ex["depth"], ex["max_leaf"]) == g["digest"]
    assert is_reference or br.export_bytes(ex) == br.export_bytes(ex0), "the tree is neither the reference's nor builder 0's"
    assert is_reference, "the reference stays within the round budget and the depth limit: its tree is expected"
    rb.check_structure(ex)
    assert_device_copy(ctx, ex)
    cam = B.to_camera_data((0.004, 0.0005, 0.004), (0.004, 0.0005, 0.0), (0, 1, 0), 60.0, W_, H_)
    want = frame(ctxs[0], cam)
    assert len(np.unique(want)) > 16
    assert frame(ctx, cam).tobytes() == want.tobytes()
    # the level strip: beyond the budget
    tris = br.level_strip(br.STRIP_N)
    t0 = time.time()
    ex = build(ctx, tris)  # succeeds
    _report["seconds"]["upload level_strip(%d), %d rounds on the device, then the host builder" % (br.STRIP_N, br.PLOC_ROUND_CAP)] = round(time.time() - t0, 3)
    ex0 = build(ctxs[0], tris)
    assert br.export_bytes(ex) == br.export_bytes(ex0), "out of rounds: builder 0's tree is expected"
    rb.check_structure(ex)
    assert_device_copy(ctx, ex)
    cam = B.to_camera_data((4500.0, 0.5, 3.0), (4500.0, 0.5, 0.0), (0, 1, 0), 60.0, W_, H_)
    want = frame(ctxs[0], cam)
    assert len(np.unique(want)) > 16
    assert frame(ctx, cam).tobytes() == want.tobytes()
    _report["cases"]["round_cap"] = dict(strip_scene_rounds=g["rounds"], strip_scene_tree="reference", level_strip_reference_rounds=gold["level_strip_%d" % br.STRIP_N]["rounds"],
                                         level_strip_tree="builder 0")


# ---------------------------------------------------------------------------------------------------------------------
# 5. below the device threshold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", (1, 2))
def test_below_device_threshold(ctxs, builder):
    soup = br.scene_cases(4)["soup2000"]
    for leaf in br.LEAF_SIZES:
        for n in range(1, leaf + 1):
            ex, ex0 = build(ctxs[builder], soup[:n], leaf), build(ctxs[0], soup[:n], leaf)
            assert br.export_bytes(ex) == br.export_bytes(ex0), (leaf, n)
            assert ex["nodes"].size == 0 and ex["root"] < -1
            assert_device_copy(ctxs[builder], ex)


def test_zz_write_profile():
    """Last in the file: the figures gathered above, with PT_WRITE_PROFILES=1 (and the whole file run)."""
    if os.environ.get("PT_WRITE_PROFILES") != "1" or "round_cap" not in _report["cases"]:
        return
    br.write_profile("gpu", _report)
