"""The guide pass on random scenes without a GPU: the cases of tests/guide_fuzz_common.py through the CPU twins and the numpy restatements.

* pt_debug_aov_follow_host == tests/aov_follow_ref.py and pt_debug_aov_host == tests/aov_ref.py on every pixel of every case, all 8
  floats as bits (a NaN equals only the same NaN), the frames of the case's batch included; pt_debug_aov_host == the follow twin at
  max_follow = 0.  No pixel is left out, no case is filtered: 64 cases by default (PT_GUIDE_FUZZ_CASES=N for more).
* The domain: on every ray of every round of every frame the oracle's walk equals its brute force in hit, t bits and id (the closest-hit
  domain of DESIGN.md 2.1).  A seed that breaks this is a finding and fails the test.
* The census, over the fixed default seed set whatever the environment says: each branch of the definition that the hand-built scenes
  never take (guide_fuzz_common.CENSUS_KEYS) occurs in at least 3 cases and 50 samples, at least a third of the cases follow something
  and some frame holds a non-finite value.  These are properties of the generator, read from the restatement's log alone.
* The strip frame of the GPU file's overflow test (guide_fuzz_common.strip_scene): twin == restatement with watertight 0 and 1, no ray
  outside the domain; the fixture is pinned: 26.6 % of the samples on the wall, 95 distinct albedos, 204 follow rays, depth4 = 9.
PT_WRITE_PROFILES=1 writes the counts to profiles/r17_guide_fuzz.json, section "host"."""
import time

import numpy as np

import guide_fuzz_common as G
from owl_path_tracer_amd.pyhost import binding as B

N_DEFAULT = 64
DEFAULT_SEEDS = [G.DEFAULT_SEED0 + i for i in range(N_DEFAULT)]


def test_twins_equal_the_restatements_on_every_pixel(orc):
    t0 = time.time()
    pixels = frames = 0
    seeds = G.seeds(N_DEFAULT)
    for seed in seeds:
        r, t = G.reference(orc, seed), G.twin(B, seed)
        c = r["case"]
        G.assert_same(t["follow"], r["follow"], c, "pt_debug_aov_follow_host vs aov_follow_ref")
        G.assert_same(t["first"], r["first"], c, "pt_debug_aov_host vs aov_ref")
        G.assert_same(t["follow0"], t["first"], c, "the follow twin at max_follow = 0 vs pt_debug_aov_host")
        n = 3
        for f, want in enumerate(r["batch"] or []):
            G.assert_same(t["batch"][f], want, c, "batch frame %d: pt_set_materials + pt_debug_aov_follow_host vs aov_follow_ref" % f)
            n += 1
        frames += n
        pixels += n * c["W"] * c["H"]
    print("guide fuzz, host: %d cases, %d frames, %d pixels compared bit for bit, none left out (%.1f s)" % (len(seeds), frames, pixels, time.time() - t0))
    G.write_profile("host", dict(twins_vs_restatements=dict(seed0=seeds[0], cases=len(seeds), frames_compared=frames, pixels_compared=pixels, pixels_left_out=0,
                                                            seconds=round(time.time() - t0, 1))))


def test_every_ray_is_inside_the_closest_hit_domain(orc):
    rays, bad, t0 = 0, [], time.time()
    for seed in G.seeds(N_DEFAULT):
        r = G.reference(orc, seed)
        rays += r["rays"]
        if r["outside"]:
            bad.append((G.describe(r["case"]), r["outside"]))
    print("guide fuzz, host: %d rays, the oracle's walk against its brute force: %d cases differ" % (rays, len(bad)))
    G.write_profile("host", dict(domain=dict(rays_checked_against_brute_force=rays, rays_outside_the_domain=sum(n for _, n in bad), seconds=round(time.time() - t0, 1))))
    assert not bad, "the oracle's walk and its brute force differ (case, rays): %r" % bad


def test_census_of_the_default_seed_set(orc):
    cases, samples = G.census_of(orc, DEFAULT_SEEDS)
    followed = non_finite = 0
    for seed in DEFAULT_SEEDS:
        r = G.reference(orc, seed)
        followed += r["followed"]
        non_finite += not (np.isfinite(r["follow"]).all() and all(np.isfinite(a).all() for a in r["batch"] or []))
    for k in G.CENSUS_KEYS:
        print("%-40s %3d cases %8d samples" % (k, cases[k], samples[k]))
    print("cases that follow something: %d of %d; cases with a non-finite value in a frame: %d" % (followed, N_DEFAULT, non_finite))
    G.write_profile("host", dict(census={k: dict(cases=cases[k], samples=samples[k]) for k in G.CENSUS_KEYS}, census_seeds=N_DEFAULT, cases_that_follow=followed,
                                 cases_with_non_finite_output=non_finite))
    short = [k for k in G.CENSUS_KEYS if cases[k] < G.MIN_CASES or samples[k] < G.MIN_SAMPLES]
    assert not short, "the default seed set does not take these branches often enough: %r" % {k: (cases[k], samples[k]) for k in short}
    assert 3 * followed >= N_DEFAULT, followed
    assert non_finite >= 1


def test_strip_frame_of_the_overflow_test(orc):
    for wt in (0, 1):
        r, t = G.strip_reference(orc, wt), G.strip_twin(B, wt)
        c = dict(seed=-1, W=G.STRIP_W, H=G.STRIP_H, n=G.STRIP_N, max_follow=G.STRIP_MAX_FOLLOW, roughness_max=G.STRIP_ROUGHNESS_MAX, wt=wt, option=("leaf_size", 1),
                 shard=None, ents=G.strip_scene()["ents"])
        G.assert_same(t["first"], r["first"], c, "strip: pt_debug_aov_host vs aov_ref")
        G.assert_same(t["follow"], r["follow"], c, "strip, the wall a mirror: pt_debug_aov_follow_host vs aov_follow_ref")
        for f, want in enumerate(r["batch"] or []):
            G.assert_same(t["batch"][f], want, c, "strip, batch frame %d" % f)
        assert r["outside"] == 0, "strip, watertight %d: %d of %d rays outside the domain" % (wt, r["outside"], r["rays"])
        print("strip, watertight %d: %.1f %% of the samples hit the wall, %d distinct albedos, %d follow rays, depth4 %d" % (
            wt, 100 * r["wall_share"], r["albedos"], r["followed"], t["depth4"]))
        # the scene is deterministic: 204 of the 768 samples hit the wall, and each of them goes on from the mirror
        assert round(r["wall_share"] * G.STRIP_W * G.STRIP_H * G.STRIP_N) == 204 and r["albedos"] == 95 and r["followed"] == 204, (r["wall_share"], r["albedos"], r["followed"])
        assert (G.bits(r["follow"]) != G.bits(r["first"])).any()
        assert t["depth4"] == 9 and 3 * t["depth4"] + 1 > B.PT_LDS_STACK
