"""Option "watertight" without a GPU: the option itself, the host walk against the bit-level reference, closed meshes, the exact referee,
and the resource report of the watertight translation unit.

* The key is accepted (it was an unknown option before), defaults to 0, takes 0 and 1 only, and what it selects shows in
  pt_debug_closest_hit_host_n: 1 gives the watertight answers, 0 again gives the answers from before, bit for bit.
* With watertight = 1 the host walk (the product's binary tree, leaf sizes 1 / 4 / 7) equals tests/watertight_ref.py - brute force in
  float32 numpy - on EVERY ray of the battery inside the 10-extent domain: hit and id equal, t, u, v bit for bit.  Classes 8 / 9 and
  origins beyond 10 extents are counted and recorded, as the probe tests do (the definition does not reach them: ray_battery.py).
* Closed meshes with shared float32 vertices, rays from strictly inside, random and aimed at shared edges / vertices, 2 000 per set:
  zero leaks with watertight = 1; with watertight = 0 on the same context afterwards the answers - leaks included - are a fresh
  context's: the switch leaves no state behind.
* tests/exact_hit.py, unmodified: R2 and R3 on every ray, and the reported id is never a certainly-missed triangle.  The t, u, v
  bounds of R1 were derived for tri_eval's operation sequence and do not apply to another one: the ratios are recorded, not asserted.
  The decided-ray shares the referee tests require are properties of the rays and are required here as well.
* The three wrong restatements of watertight_ref.py (float64 branch removed, u and v swapped, edge functions fused) are each told apart.
* `make asm-wt`: every instance of the watertight translation unit has 0 bytes of scratch, with the Makefile's flags.

PT_WRITE_PROFILES=1 records the figures in profiles/r09_watertight.json (section "cpu").
"""
import json
import os
import re

import numpy as np
import pytest

import ray_battery as rb
import watertight_ref as W
from owl_path_tracer_amd.pyhost import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r09_watertight.json")
SMALL_SCENES = ("rects", "one_leaf", "soup1", "soup2", "soup3", "soup_offset30", "strip")  # the battery's scenes below 10 000 triangles
N_PER_CLASS = 200
N_CLOSED = 2000
LEAVES = (1, 4, 7)
_report = {"rays_per_class": N_PER_CLASS, "scenes": {}, "closed_meshes": {}, "r1_bound_ratios_max": {}, "variants_told_apart_by": {}}
_ref_cache = {}


def write_profile(section, doc):
    if os.environ.get("PT_WRITE_PROFILES") != "1":
        return
    whole = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            whole = json.load(fh)
    whole[section] = doc
    with open(PROFILE, "w") as fh:
        json.dump(whole, fh, indent=1, sort_keys=True)


def battery(orc, name):
    """The referee's battery of the scene (seed 4242, its tables) and the watertight reference for its rays, once per process."""
    b = rb.referee_battery(orc, name, N_PER_CLASS)
    if name not in _ref_cache:
        _ref_cache[name] = W.brute_force(b["tris"], b["rays"])
    return b, _ref_cache[name][0], _ref_cache[name][1]


def host_ctx(tris, leaf=4, watertight=None):
    ctx = B.Context(-1)
    ctx.set_option("leaf_size", leaf)
    if watertight is not None:
        ctx.set_option("watertight", watertight)
    rb.upload(ctx, tris)
    return ctx


def same_answer(a, b):
    """hit, id and the bits of t, u, v on EVERY ray, misses included (two answers of the library)"""
    return all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == np.float32 else x, np.asarray(y).view(np.uint32) if np.asarray(y).dtype == np.float32 else y)
               for x, y in zip(a, b))


def test_option_is_accepted_defaults_to_zero_and_selects_the_test():
    tris, centre, half = rb.make_closed_mesh("ico320")
    rays = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(77), 400)["edges_and_vertices"]
    fresh = host_ctx(tris)
    before = fresh.closest_hit_host_n(rays)
    fresh.close()
    assert (~before[0]).any(), "Moeller-Trumbore leaks on rays aimed at shared edges and vertices: the two tests can be told apart here"
    ctx = host_ctx(tris)
    ctx.set_option("watertight", 0)  # the default, spelled out: nothing changes
    assert same_answer(before, ctx.closest_hit_host_n(rays))
    ctx.set_option("watertight", 1)  # refused as an unknown option before
    wt = ctx.closest_hit_host_n(rays)
    assert wt[0].all() and W.compare(W.brute_force(tris, rays)[0], wt).size == 0
    ctx.set_option("watertight", 0)
    assert same_answer(before, ctx.closest_hit_host_n(rays)), "back to 0: the answers from before, misses included, bit for bit"
    for bad in (2, -1, 7):
        with pytest.raises(B.PtError, match="watertight"):
            ctx.set_option("watertight", bad)
    # a single ray goes the same way
    ctx.set_option("watertight", 1)
    i = int(np.nonzero(~before[0])[0][0])
    h, t, u, v, p = ctx.closest_hit_host(rays[i, :3], rays[i, 3:])
    assert h and p == wt[4][i] and np.float32(t) == wt[1][i] and np.float32(u) == wt[2][i] and np.float32(v) == wt[3][i]
    ctx.close()


def test_lane_per_pixel_kernel_and_watertight_exclude_each_other():
    """kernel = 1 has no watertight form: whichever of the two options comes second is refused, by name, and the first one stays."""
    ctx = B.Context(-1)
    ctx.set_option("watertight", 1)
    with pytest.raises(B.PtError, match="watertight"):
        ctx.set_option("kernel", 1)
    ctx.set_option("kernel", 2)
    ctx.set_option("watertight", 0)
    ctx.set_option("kernel", 1)
    with pytest.raises(B.PtError, match="kernel"):
        ctx.set_option("watertight", 1)
    ctx.set_option("watertight", 0)
    ctx.close()


@pytest.mark.parametrize("name", SMALL_SCENES)
def test_host_walk_equals_the_reference_and_keeps_the_rules(orc, name):
    b, ref, n64 = battery(orc, name)
    tris, rays, cls, T = b["tris"], b["rays"], b["cls"], b["tables"]
    assert set(rb.CLASSES) <= set(np.unique(cls)), "every class of the battery is drawn"
    held, mid, far = rb.bands(rays, rb.scene_measure(tris), cls)
    outside = np.isin(cls, rb.OUTSIDE)
    # the decided shares are properties of the rays: the conditions of tests/test_exact_hit.py, unchanged
    dec = T.decided.astype(bool)
    class1, overall = float(dec[held & (cls == 1)].mean()), float(dec[held].mean())
    assert class1 >= 0.9 and overall >= 0.5, (name, class1, overall)
    rec = _report["scenes"][name] = dict(triangles=int(tris.shape[0]), rays=int(rays.shape[0]), rays_inside_the_domain=int(held.sum()),
                                         float64_branch_pairs=[int(n64), int(rays.shape[0]) * int(tris.shape[0])], mismatches_outside_the_domain={})
    answers = [("reference", ref)]
    for leaf in LEAVES:
        ctx = host_ctx(tris, leaf, watertight=1)
        got = ctx.closest_hit_host_n(rays)
        ctx.close()
        bad = W.compare(ref, got, held)
        assert bad.size == 0, "%s, leaf %d: the host walk differs from the reference on %d of %d rays inside the domain; first: class %d %r got %r want %r" % (
            name, leaf, bad.size, held.sum(), cls[bad[0]], rays[bad[0]].tolist(), [x[bad[0]].item() for x in got], [x[bad[0]].item() for x in ref])
        rec["mismatches_outside_the_domain"]["leaf %d" % leaf] = {k: [int(W.compare(ref, got, m).size), int(m.sum())] for k, m in (("10_to_42_extents", mid), ("beyond_42_extents", far), ("classes_8_9", outside))}
        answers.append(("closest_hit_host, leaf %d" % leaf, got))
    for who, ans in answers:
        res = T.check(ans)
        for rule, text in (("r2", "R2 (nothing certain was missed)"), ("r3", "R3 (decided rays have one answer)")):
            v = np.nonzero(res[rule])[0]
            assert v.size == 0, "%s on %s violates %s on %d rays; first: class %d, %s" % (who, name, text, v.size, cls[v[0]], T.describe(ans, v[0]))
        hit = np.asarray(ans[0], bool)
        missed = np.nonzero(hit & (T.lookup(np.where(hit, ans[4], -1)) < 0))[0]
        assert missed.size == 0, "%s on %s reports a certainly-missed triangle on %d of %d hits; first: class %d, %s" % (who, name, missed.size, hit.sum(), cls[missed[0]], T.describe(ans, missed[0]))
        for q in ("t", "u", "v"):  # recorded: how far the watertight t, u, v lie from exact, in units of the bound derived for tri_eval
            r = res["ratio_" + q][held & hit]
            k = "%s/%s" % (q, who.split(",")[0])
            _report["r1_bound_ratios_max"][k] = max(_report["r1_bound_ratios_max"].get(k, 0.0), float(r.max()) if r.size else 0.0)
    print(name, rec, {k: round(v, 2) for k, v in _report["r1_bound_ratios_max"].items()})


@pytest.mark.parametrize("name", rb.closed_mesh_names())
def test_closed_meshes_do_not_leak_and_the_switch_leaves_nothing_behind(name):
    tris, centre, half = rb.make_closed_mesh(name)
    sets = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(77), N_CLOSED)
    fresh = host_ctx(tris)
    before = {s: fresh.closest_hit_host_n(r) for s, r in sets.items()}
    fresh.close()
    ctx = host_ctx(tris)
    rec = _report["closed_meshes"][name] = dict(triangles=int(tris.shape[0]))
    for sname, rays in sets.items():
        ctx.set_option("watertight", 1)
        wt = ctx.closest_hit_host_n(rays)
        ref, n64 = W.brute_force(tris, rays)
        assert ref[0].all(), "the reference leaks on %d rays of %s / %s" % ((~ref[0]).sum(), name, sname)
        assert wt[0].all(), "%d of %d rays from inside %s (%s) leak with watertight = 1; first %r" % ((~wt[0]).sum(), rays.shape[0], name, sname, rays[~wt[0]][0].tolist())
        bad = W.compare(ref, wt)
        assert bad.size == 0, "%s / %s: %d rays differ from the reference; first %r" % (name, sname, bad.size, rays[bad[0]].tolist())
        ctx.set_option("watertight", 0)
        assert same_answer(before[sname], ctx.closest_hit_host_n(rays)), "watertight = 0 after 1 is not what a fresh context answers"
        rec[sname] = dict(rays=int(rays.shape[0]), leaks_watertight_0=int((~before[sname][0]).sum()), leaks_watertight_1=int((~wt[0]).sum()),
                          float64_branch_pairs=[int(n64), int(rays.shape[0]) * int(tris.shape[0])])
        print(name, sname, rec[sname])
    ctx.close()
    assert rec["edges_and_vertices"]["leaks_watertight_0"] > 0, "the aimed set is where Moeller-Trumbore leaks: without leaks before, zero after shows nothing"


VARIANTS = {"no_f64": "float64 branch removed", "swap_uv": "u and v swapped", "fused": "edge functions fused"}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_wrong_restatement_is_told_apart(orc, variant):
    """What the mutation builds of the library do, restated: each must differ from the reference where the tests look - bits of u, v
    on the battery (swap, fusing), ids and bits on the aimed rays of a closed mesh (float64 branch), leaks there (fusing)."""
    found = []
    b, ref, _ = battery(orc, "rects")
    got, _ = W.brute_force(b["tris"], b["rays"], variant)
    held = rb.bands(b["rays"], rb.scene_measure(b["tris"]), b["cls"])[0]
    d = W.compare(ref, got, held)
    if d.size:
        found.append("rects: %d of %d rays inside the domain differ" % (d.size, held.sum()))
    tris, centre, half = rb.make_closed_mesh("ico320")
    rays = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(77), N_CLOSED)["edges_and_vertices"]
    got, _ = W.brute_force(tris, rays, variant)
    d = W.compare(W.brute_force(tris, rays)[0], got)
    if d.size:
        found.append("ico320, aimed: %d of %d rays differ" % (d.size, rays.shape[0]))
    if not got[0].all():
        found.append("ico320, aimed: %d of %d rays leak" % ((~got[0]).sum(), rays.shape[0]))
    print(variant, found)
    assert found, "the variant '%s' (%s) is indistinguishable from the reference on the rays the tests use" % (variant, VARIANTS[variant])
    if variant == "fused":  # (an exact zero left as it is makes both neighbours accept: another id or other bits, no leak)
        assert any("leak" in f for f in found), "fused edge functions are not antisymmetric: the aimed rays must leak"
    _report["variants_told_apart_by"][variant] = found


def test_watertight_instances_need_no_scratch():
    """hipcc's resource report for pt_kernel_wt.hip with the flags `make asm-wt` passes (the Makefile's CXXFLAGS): the five render
    instances the library can launch (product / fallback, fma and subtracting slab form each, + the instrumented one) and the five
    probe kernels all show ScratchSize 0.  (plan_frame refuses an instance with scratch; this finds it without a GPU.)"""
    import resource_report

    resource_report.assert_ships_with_makefile_flags("pt_kernel_wt")
    blocks = resource_report.report("asm-wt")[1]
    render = [b for b in blocks if "pt_render_wt_kernel" in b[0]]
    probes = [b for b in blocks if "pt_probe_quad_wt_kernel" in b[0] or "pt_probe_group_wt_kernel" in b[0]]
    assert len(render) == 5 and len(probes) == 5, blocks
    assert len(blocks) == 10, "the watertight translation unit holds these ten kernels and no other: %r" % (blocks,)
    assert all(int(sz) == 0 for _, _, sz in blocks), blocks
    _report["resource_report"] = {name: dict(vgprs=int(v), scratch=int(sz)) for name, v, sz in blocks}


def test_zz_write_profile():
    """Last in the file: the figures gathered above, with PT_WRITE_PROFILES=1 (and the whole file run)."""
    if len(_report["scenes"]) == len(SMALL_SCENES) and len(_report["closed_meshes"]) == len(rb.closed_mesh_names()):
        write_profile("cpu", _report)
