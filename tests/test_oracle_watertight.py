"""The oracle's watertight twin (orc_scene_set_watertight / Scene(..., watertight=True)) without a GPU.

oracle/pt_oracle.c restates the watertight triangle test of option "watertight" = 1 from the text of DESIGN.md 2.1: a third
implementation next to the library's (csrc/pt_bvh.cpp on the host, csrc/pt_trace.h on the device) and tests/watertight_ref.py.  It is the
only one of them that renders, so it is what the watertight frames of the GPU are held to bit for bit (tests/test_gpu_watertight.py,
tests/test_gpu_fuzz.py).  What that rests on is checked here:

* The oracle's brute force with the switch at 1 equals watertight_ref.brute_force on EVERY ray of the battery - hit, id, the bits of
  t, u, v; classes 8 / 9 and far origins included: both sides are the same definition over all triangles, so there is no domain mask -
  on the battery's seven small scenes at 200 rays per class and on the Cornell box at 60.
* Its BVH walk equals its brute force on every ray inside the 10-extent domain (ray_battery.bands, classes 8 / 9 excluded); outside,
  mismatches are counted and printed.
* The library's CPU twin, Context(-1).closest_hit_host_n with "watertight" = 1, equals the oracle inside the domain at leaf sizes 1 / 4 / 7.
* The three wrong restatements of watertight_ref.py (float64 branch removed, u and v swapped, edge functions fused) each differ from the
  oracle on at least one battery ray: the comparison has teeth in this direction too.
* Frames: 1 and back to 0 on one Scene gives the Moeller-Trumbore frame again; the closed-emitter frame is the constant 2.0; a Cornell
  frame is the same through the hierarchy and by brute force.
* The precondition of the GPU fuzz leg: for each of the 40 default seeds the watertight oracle frame through the hierarchy equals the
  frame by brute force - no case is left out - and at least half of them differ in bits from the switch-0 frame (the seeds are fixed, so
  the count is one number: 27 of 40).

PT_WRITE_PROFILES=1 records the figures in profiles/r09_watertight.json (section "oracle").
"""
import numpy as np
import pytest

import ray_battery as rb
import test_gpu_fuzz as F
import watertight_ref as WR
from owl_path_tracer_amd.pyhost import binding as B, scene_io
from test_gpu_watertight import CORNELL_ENV, DEPTH, H_, N_PER_CLASS, SMALL_SCENES, SPP, W_, _battery
from test_watertight_host import VARIANTS, host_ctx, write_profile

SCENES = SMALL_SCENES + ("cornell",)
N_CORNELL = 60  # rays per class on the Cornell box (17 974 triangles): ~12 M (ray, triangle) pairs, a second or two of numpy
LEAVES = (1, 4, 7)
FUZZ_SEEDS = [20260405 + i for i in range(40)]  # the defaults of tests/test_gpu_fuzz.py, whatever PT_FUZZ_SEED / PT_FUZZ_CASES say
_report = {"battery": {}, "variants_told_apart_by": {}, "fuzz": {}}
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_frame(a, b, what):
    bad = _bits(a) != _bits(b)
    assert not bad.any(), "%s: %d of %d floats differ" % (what, bad.sum(), bad.size)


def battery(orc, name):
    """Once per scene and process: the battery, the numpy reference, and the watertight oracle's brute force and walk."""
    if name not in _cache:
        tris, rays, cls, S = _battery(orc, name, N_CORNELL if name == "cornell" else N_PER_CLASS)
        ref, _ = WR.brute_force(tris, rays)
        S.set_watertight(True)
        _cache[name] = dict(tris=tris, rays=rays, cls=cls, ref=ref, brute=S.intersect_n(rays, use_bvh=False), walk=S.intersect_n(rays, use_bvh=True),
                            held=rb.bands(rays, rb.scene_measure(tris), cls)[0])
    return _cache[name]


def _first(b, bad, got, want):
    i = bad[0]
    return "class %d %r got %r want %r" % (b["cls"][i], b["rays"][i].tolist(), [x[i].item() for x in got], [x[i].item() for x in want])


@pytest.mark.parametrize("name", SCENES)
def test_oracle_brute_force_equals_the_numpy_reference(orc, name):
    b = battery(orc, name)
    assert set(rb.CLASSES) <= set(np.unique(b["cls"])), "every class of the battery is drawn"
    bad = WR.compare(b["ref"], b["brute"])
    assert bad.size == 0, "%s: the oracle's brute force differs from the reference on %d of %d rays; first: %s" % (name, bad.size, b["rays"].shape[0], _first(b, bad, b["brute"], b["ref"]))
    _report["battery"].setdefault(name, {}).update(triangles=int(b["tris"].shape[0]), rays_compared_with_the_reference=int(b["rays"].shape[0]), hits=int(b["ref"][0].sum()),
                                                 rays_of_classes_8_9_among_them=int(np.isin(b["cls"], rb.OUTSIDE).sum()))
    print(name, _report["battery"][name])


@pytest.mark.parametrize("name", SCENES)
def test_oracle_walk_equals_its_brute_force_inside_the_domain(orc, name):
    b = battery(orc, name)
    held = b["held"]
    bad = WR.compare(b["brute"], b["walk"], held)
    assert bad.size == 0, "%s: the oracle's walk differs from its brute force on %d of %d rays inside the domain; first: %s" % (name, bad.size, held.sum(), _first(b, bad, b["walk"], b["brute"]))
    outside = int(WR.compare(b["brute"], b["walk"], ~held).size)
    _report["battery"].setdefault(name, {}).update(rays_inside_the_domain=int(held.sum()), walk_mismatches_outside_the_domain=[outside, int((~held).sum())])
    print("%s: %d rays inside the domain, walk == brute force on all; outside it %d of %d differ (counted)" % (name, held.sum(), outside, (~held).sum()))


@pytest.mark.parametrize("name", SCENES)
def test_host_walk_of_the_library_equals_the_oracle(orc, name):
    b = battery(orc, name)
    for leaf in LEAVES:
        ctx = host_ctx(b["tris"], leaf, watertight=1)
        got = ctx.closest_hit_host_n(b["rays"])
        ctx.close()
        bad = WR.compare(b["brute"], got, b["held"])
        assert bad.size == 0, "%s, leaf %d: closest_hit_host_n differs from the oracle on %d of %d rays inside the domain; first: %s" % (name, leaf, bad.size, b["held"].sum(), _first(b, bad, got, b["brute"]))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_a_wrong_restatement_differs_from_the_oracle(orc, variant):
    """An oracle that had made one of these mistakes itself would equal the variant and not the reference: each must be told apart on
    the battery's own rays."""
    found = []
    for name in SMALL_SCENES:
        b = battery(orc, name)
        got, _ = WR.brute_force(b["tris"], b["rays"], variant)
        d = WR.compare(b["brute"], got)
        if d.size:
            found.append("%s: %d of %d rays differ" % (name, d.size, b["rays"].shape[0]))
    print(variant, found)
    assert found, "the variant '%s' (%s) equals the oracle on every ray of the battery" % (variant, VARIANTS[variant])
    _report["variants_told_apart_by"][variant] = found


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
def _cornell_cam(orc, cornell, W, H):
    c = cornell["camera"]
    return orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)


def test_switch_there_and_back_is_the_frame_of_before(orc, cornell):
    cam, env = _cornell_cam(orc, cornell, W_, H_), orc.make_env(**CORNELL_ENV)
    mt, mt8, mtc = orc.Scene(cornell["flat"]).render(cam, env, W_, H_, SPP, DEPTH, want_rgba8=True, want_counters=True)
    S = orc.Scene(cornell["flat"])
    S.set_watertight(True)
    wt, _, _ = S.render(cam, env, W_, H_, SPP, DEPTH)
    assert (_bits(wt) != _bits(mt)).any(), "the switch did not reach the render"
    S.set_watertight(False)
    back, back8, backc = S.render(cam, env, W_, H_, SPP, DEPTH, want_rgba8=True, want_counters=True)
    _same_frame(back, mt, "1 and back to 0 == a fresh scene")
    np.testing.assert_array_equal(back8, mt8)
    assert backc == mtc
    _same_frame(orc.Scene(cornell["flat"], watertight=True).render(cam, env, W_, H_, SPP, DEPTH)[0], wt, "the constructor's argument == set_watertight")


def test_closed_emitter_frame_is_the_constant(orc):
    """The scene of test_invariant_frame_inside_a_closed_emitter (tests/test_gpu_watertight.py): every path ends at its first hit."""
    tris = (rb.icosphere(3) * np.float32(rb.CLOSED_RADIUS)).astype(np.float32)
    mat = scene_io.MAT_DEFAULT.copy()
    mat[16] = 2.0
    look_from, look_at = [0.11, -0.07, 0.05], [float(x) for x in tris[0, 0]]
    W, H, spp = 48, 40, 16
    S = orc.Scene(scene_io.flatten_scene([(rb.mesh_of(tris), 0)], [("glow", mat, "")]), watertight=True)
    for use_bvh in (True, False):
        got, _, _ = S.render(orc.to_camera_data(look_from, look_at, [0, 1, 0], 70.0, W, H), orc.make_env(color=(0, 0, 0), intensity=0.0), W, H, spp, 8, use_bvh=use_bvh)
        assert (_bits(got) == _bits(np.float32(2.0))).all(), "%d of %d values are not 2.0 (use_bvh=%r)" % ((_bits(got) != _bits(np.float32(2.0))).sum(), got.size, use_bvh)


def test_cornell_frame_does_not_depend_on_the_hierarchy(orc, cornell):
    cam, env = _cornell_cam(orc, cornell, W_, H_), orc.make_env(**CORNELL_ENV)
    S = orc.Scene(cornell["flat"], watertight=True)
    a, a8, ac = S.render(cam, env, W_, H_, SPP, DEPTH, use_bvh=True, want_rgba8=True, want_counters=True)
    b, b8, bc = S.render(cam, env, W_, H_, SPP, DEPTH, use_bvh=False, want_rgba8=True, want_counters=True)
    _same_frame(a, b, "Cornell, watertight: hierarchy == brute force")
    np.testing.assert_array_equal(a8, b8)
    for k in ("samples", "rays", "scatters", "env_misses", "nan_retries"):
        assert ac[k] == bc[k], k


def test_fuzz_frames_do_not_depend_on_the_hierarchy(orc):
    """What test_random_scenes_bitwise_watertight needs before it can compare any frame with the oracle's: the oracle's watertight frame of
    every default case is ONE frame, whichever way the oracle finds its hits.  No case may be left out."""
    differ = []
    for seed in FUZZ_SEEDS:
        c = F.draw_case(seed)
        flat = scene_io.flatten_scene(c["ents"], [("m%d" % i, m, "") for i, m in enumerate(c["mats"])], c["tex_by_mat"])
        frm, at, up, fov = c["camera"]
        W, H, spp, depth = c["W"], c["H"], c["spp"], c["depth"]
        cam, env = orc.to_camera_data(tuple(frm), tuple(at), tuple(up), fov, W, H), orc.make_env(**c["env"])
        S = orc.Scene(flat)
        mt, _, _ = S.render(cam, env, W, H, spp, depth)
        S.set_watertight(True)
        a, a8, _ = S.render(cam, env, W, H, spp, depth, use_bvh=True, want_rgba8=True)
        b, b8, _ = S.render(cam, env, W, H, spp, depth, use_bvh=False, want_rgba8=True)
        same = (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), "fuzz case seed=%d, watertight oracle: %d of %d values differ between the hierarchy and brute force; first at %s" % (seed, (~same).sum(), same.size, np.argwhere(~same)[0])
        assert (a8 == b8).all(), seed
        if not ((_bits(a) == _bits(mt)) | (np.isnan(a) & np.isnan(mt))).all():
            differ.append(seed)
    print("watertight oracle frames of the %d default fuzz cases: all independent of the hierarchy, %d differ in bits from the switch-0 frame" % (len(FUZZ_SEEDS), len(differ)))
    _report["fuzz"] = dict(cases=len(FUZZ_SEEDS), cases_left_out=0, frames_that_differ_from_switch_0=len(differ), seeds_with_the_switch_0_frame=[s for s in FUZZ_SEEDS if s not in differ])
    assert 2 * len(differ) >= len(FUZZ_SEEDS), "the option changes fewer than half of the frames: the fuzz leg would mostly repeat the other one"


def test_zz_write_profile():
    """Last in the file: the figures gathered above, with PT_WRITE_PROFILES=1 (and the whole file run)."""
    if len(_report["battery"]) == len(SCENES) and _report["fuzz"] and all("rays_inside_the_domain" in r and "rays_compared_with_the_reference" in r for r in _report["battery"].values()):
        write_profile("oracle", _report)
