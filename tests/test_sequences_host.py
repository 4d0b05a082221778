"""Random call sequences (tests/seq_common.py) on host-only contexts, and the generator's own conditions.  No GPU.

1. every default sequence on B.Context(-1): the state-changing and the refused steps as drawn; every observing step becomes what a
   host-only context can show - pt_debug_aov_host on all pixels against tests/aov_ref.py, pt_debug_closest_hit_host_n on the rays of
   ray_battery.make_rays(.., 200) inside the domain against the oracle's brute force over the model's meshes, the exported boxes against
   their definition (also after every update).  That holds the host twin's state machine: the lazy refit, the watertight switch, the
   current tables and environment, refused calls that leave everything as it was.  Builders 1 and 2 hand over to builder 0 there,
   which is asserted on every upload.
2. what the default sequences contain between them (seq_common.coverage): all three builders followed by an update, a batch followed by
   a single frame, the guide pass between two equal renders, growth and shrink by 4 x, a shard change, all three stream kinds, every
   kind of refused call, both sides of the sort threshold.
3. with the oracle alone: a change is VISIBLE if the oracle's output of the next observing step differs from what that step shows in
   the state before the change (the blocks of the generator put the observation right behind the change).  At
   least 9 in 10 changes are visible, every kind at least three times, and at most 1 in 10 observed frames is constant - an invisible
   change or a flat frame cannot expose stale state.  box_exact and the scheduler knobs cannot change an image and are not counted.
4. the draws of the twelve default seeds are pinned: their call lists equal tests/golden/sequence_call_lists.json, written before the
   second family was added to the generator.
5. the second family (seq_common.draw_guide_sequence: follow guides, batch guides, the denoiser) the same three ways: on a host-only
   context - pt_debug_aov_follow_host against tests/aov_follow_ref.py, pt_debug_denoise_host on the model's inputs against
   tests/denoise_ref.py, refused calls through the twins, PT_E_NO_DEVICE for valid calls of the batch forms and PT_E_INVALID for invalid
   ones; what its twelve default seeds contain; and that their changes show, the follow kernels have something to follow and the
   filters change their frames.
6. the third family (seq_common.draw_accum_sequence: one accumulation in the middle of a context's life; model and runner part in
   tests/accum_seq_common.py): on a host-only context every step of the model is held through the library's CPU twins applied to the
   model's arrays before the step; what its twelve default seeds contain (every entry point twice, all three streams, every kind of change
   followed by an add, a selecting add after a knob, reprojects with and without a cap and two in one accumulation, a blocking and an
   all-asynchronous chain, both sides of the sort threshold, every refusal, a begin over a live accumulation, growth and shrink); with the
   oracle alone, that at least 9 in 10 changes alter the sums of the next add, every kind at least twice, and that at most 1 in 10
   reprojects keeps all or none of its pixels; and the pinned call lists of the second and third family
   (tests/golden/guide_sequence_call_lists.json, accum_sequence_call_lists.json).
"""
import json
import os

import numpy as np
import pytest

import accum_seq_common as AQ
import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B

SEEDS = SC.default_seeds()
GUIDE_SEEDS = SC.default_guide_seeds()


@pytest.fixture(scope="module")
def model(orc):
    return SC.Model(orc)


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_on_a_host_only_context(model, seed):
    seq = SC.draw_sequence(seed, host_only=True)
    assert [SC.describe(s) for s in seq["steps"]] == [SC.describe(s) for s in SC.draw_sequence(seed)["steps"]], "host_only does not change a draw"
    ctx = B.Context(-1)
    try:
        SC.run(ctx, seq, model)
    finally:
        ctx.close()


def test_the_default_sequences_cover_what_they_are_for():
    seqs = [SC.draw_sequence(s) for s in SEEDS]
    for seq in seqs:
        n = sum(len(m["indices"]) for m, _ in seq["upload"]["ents"])
        assert 8 <= len(seq["steps"]) <= 12 and 80 <= n <= 400 and 2 <= len(seq["upload"]["ents"]) <= 4 and seq["upload"]["ents"][-1][0].get("sliver")
        c = SC.coverage([seq])
        assert c["growth"] >= 1 and c["shrink"] >= 1, "seed %d: every sequence has a growth and a shrink of 4 x in pixels" % seq["seed"]
        for a, b in zip(seq["steps"], seq["steps"][1:] + [None]):
            if a["op"] == "refused" or SC.kind_of(a):  # looked at before anything else changes; the watertight switch by a guide pass (its depth is the hit's t)
                assert b is not None and b["op"] in (SC.AOV_OPS if SC.kind_of(a) == "watertight" else SC.OBSERVING), (seq["seed"], SC.describe(a))
    c = SC.coverage(seqs)
    assert c["builder_then_update"] == {0, 1, 2}
    assert c["batch_then_single"] >= 1 and c["aov_between_equal_renders"] >= 1 and c["shard_change"] >= 1 and c["upload_mid"] >= 1
    assert c["streams"] == {None, 0, 1}
    assert c["refused"] == set(SC.REFUSED)
    assert c["null_mesh"] >= 1 and c["normals"] >= 1
    assert c["spp"] == set(SC.SPP), "both sides of the sort threshold (4 x prepass_spp = 32 or 64)"


def test_changes_are_visible_and_frames_are_not_flat(model):
    shown, hidden, frames, flat = {k: 0 for k in SC.CHANGES}, [], 0, []
    for seed in SEEDS:
        sh, hi, fr, fl = SC.visibility(SC.draw_sequence(seed), model)
        for k, v in sh.items():
            shown[k] += v
        hidden += [(seed,) + h for h in hi]
        frames += fr
        flat += [(seed, i) for i in fl]
    n = sum(shown.values()) + len(hidden)
    print("visible changes: %d of %d %r; hidden: %r; flat frames: %d of %d %r" % (sum(shown.values()), n, shown, hidden, len(flat), frames, flat))
    assert 10 * sum(shown.values()) >= 9 * n, hidden
    assert all(v >= 3 for v in shown.values()), shown
    assert 10 * len(flat) <= frames, flat


def test_the_default_draws_are_the_pinned_ones():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_call_lists.json")) as f:
        pinned = json.load(f)
    assert pinned["seed0"] == SC.SEED0 and sorted(pinned["call_lists"]) == sorted(str(s) for s in SEEDS)
    for seed in SEEDS:
        seq = SC.draw_sequence(seed)
        assert ["upload: " + SC.describe(seq["upload"])] + [SC.describe(s) for s in seq["steps"]] == pinned["call_lists"][str(seed)], seed


@pytest.mark.parametrize("seed", GUIDE_SEEDS)
def test_guide_sequence_on_a_host_only_context(model, seed):
    seq = SC.draw_guide_sequence(seed, host_only=True)
    assert [SC.describe(s) for s in seq["steps"]] == [SC.describe(s) for s in SC.draw_guide_sequence(seed)["steps"]], "host_only does not change a draw"
    ctx = B.Context(-1)
    try:
        SC.run(ctx, seq, model)
    finally:
        ctx.close()


def test_the_default_guide_sequences_cover_what_they_are_for():
    seqs = [SC.draw_guide_sequence(s) for s in GUIDE_SEEDS]
    assert len(seqs) == 12 and not set(GUIDE_SEEDS) & set(SEEDS)
    for seq in seqs:
        steps = seq["steps"]
        assert 8 <= len(steps) <= 14 and len(seq["upload"]["ents"]) >= 3, seq["seed"]
        wt = 0
        for i, (a, b) in enumerate(zip(steps, steps[1:] + [None])):
            assert a["op"] not in SC.OBSERVING or (a["W"] <= 72 and a["H"] <= 56 and a.get("K", len(a.get("frames", [0]))) <= 3), (seq["seed"], SC.describe(a))
            if a["op"] == "refused" or SC.kind_of(a) or (a["op"] == "set_option" and a["key"] == "batch_frames"):  # looked at before anything else changes
                assert b is not None and b["op"] in (SC.FOLLOW_OPS if SC.kind_of(a) == "watertight" else SC.OBSERVING), (seq["seed"], SC.describe(a))
            if a["op"] == "set_option" and a["key"] == "watertight":
                wt = a["value"]
            assert not (wt and a["op"] in SC.AOV_BATCH_OPS + ("render_batch", "render_batch_device")), (seq["seed"], "a batch is only drawn while watertight is 0")
            if a["op"] in SC.FILTER_OPS and a["chain"]:  # the whole block blocking or the whole block asynchronous, over the same view and size
                r, g = steps[i - 2], steps[i - 1]
                assert {(s["op"] in SC.ASYNC_OPS) for s in (r, g, a)} in ({True}, {False}) and (r["W"], r["H"]) == (g["W"], g["H"]) == (a["W"], a["H"])
                assert r.get("cam") == g.get("cam") and [c for c, _ in r.get("frames", [])] == [c for c, _ in g.get("frames", [])] and a["src"]["render"] is r and a["src"]["guides"] is g
    c = SC.guide_coverage(seqs)
    print(c)
    assert all(v >= 2 for v in c["ops"].values()), c["ops"]
    assert all(v == {None, 0, 1} for v in c["streams"].values()), c["streams"]
    assert c["async_chains_mixed"] >= 3 and c["async_batch_chains"] >= 2
    assert all(v >= 2 for v in c["in_place"].values()), c["in_place"]
    for seed, n_filters, growth, shrink in c["filters"]:
        assert n_filters < 3 or (growth >= 1 and shrink >= 1), "seed %d: %d filters without a growth and a shrink of 4 x in filtered pixels" % (seed, n_filters)
    assert c["growth_and_shrink"] >= 6
    assert {0, 8} <= c["max_follow"] <= set(SC.MAX_FOLLOW) and c["roughness_max"] == set(SC.ROUGHNESS_MAX)
    assert c["refused"] == set(SC.GUIDE_REFUSED)
    assert c["table_kept"] >= 3
    assert c["between"] == set(SC.BETWEEN)
    assert c["bf1_before_k3_chain"] >= 1
    assert all(c["followed"][k] >= 2 for k in SC.GUIDE_LOOKS_AT), c["followed"]
    assert c["upload_mid"] >= 1 and 3 * c["glass_or_metal"] >= 2 * len(seqs)
    assert c["inf_sigma"] >= 1 and c["iterations"] == {1, 2, 3, 4, 5} and c["demodulate"] == {0, 1} and c["null_table"] == sum(c["ops"][o] for o in SC.AOV_BATCH_OPS)


def test_guide_changes_are_visible_and_the_guides_have_something_to_follow(model):
    shown, hidden, frames, flat, follow, filters = {k: 0 for k in SC.CHANGES}, [], 0, [], [0, 0], []
    for seed in GUIDE_SEEDS:
        sh, hi, fr, fl, fo, fi = SC.guide_visibility(SC.draw_guide_sequence(seed), model)
        for k, v in sh.items():
            shown[k] += v
        hidden += [(seed,) + h for h in hi]
        frames += fr
        flat += [(seed, i) for i in fl]
        follow = [follow[0] + fo[0], follow[1] + fo[1]]
        filters += [(seed,) + f for f in fi]
    n = sum(shown.values()) + len(hidden)
    print("visible changes: %d of %d %r; hidden: %r; flat buffers: %d of %d %r; follow passes that differ from max_follow = 0: %d of %d; least share of pixels a filter changes: %r" % (
        sum(shown.values()), n, shown, hidden, len(flat), frames, flat, follow[1], follow[0], min(filters, key=lambda f: f[2])))
    assert 10 * sum(shown.values()) >= 9 * n, hidden
    assert 3 * follow[1] >= follow[0], follow
    assert all(share >= 0.5 for _, _, share in filters), [f for f in filters if f[2] < 0.5]
    assert 10 * len(flat) <= frames, flat


# ---- the third family: one accumulation in the middle of a context's life (seq_common.draw_accum_sequence, tests/accum_seq_common.py) ----
ACCUM_SEEDS = SC.default_accum_seeds()


def _pinned(name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("seed", ACCUM_SEEDS)
def test_accum_sequence_on_a_host_only_context(model, seed):
    """Every step of the model is held through the library's CPU twins applied to the model's arrays before the step (select, resolve,
    reproject, variance, denoise_var, upsample); valid pt_accum_begin and pt_accum_reproject calls answer PT_E_NO_DEVICE, and - no
    accumulation can exist there - an add answers PT_E_INVALID, as the header says of an add without a begin."""
    seq = SC.draw_accum_sequence(seed, host_only=True)
    assert [SC.describe(s) for s in seq["steps"]] == [SC.describe(s) for s in SC.draw_accum_sequence(seed)["steps"]], "host_only does not change a draw"
    ctx = B.Context(-1)
    try:
        SC.run(ctx, seq, model)
    finally:
        ctx.close()


def test_the_default_accum_sequences_cover_what_they_are_for():
    seqs = [SC.draw_accum_sequence(s) for s in ACCUM_SEEDS]
    assert len(seqs) == 12 and not set(ACCUM_SEEDS) & (set(SEEDS) | set(GUIDE_SEEDS))
    for seq in seqs:
        assert 10 <= len(seq["steps"]) <= 16, seq["seed"]
        for s in seq["steps"]:
            if s["op"] == "accum_begin":
                assert 9 <= s["W"] <= 40 and 6 <= s["H"] <= 30, SC.describe(s)
            if s["op"] in ("accum_add", "accum_add_device"):
                assert s["n"] in SC.ACCUM_SPP and s["W"] * s["H"] * s["n"] <= max(SC.ACCUM_BUDGET, s["W"] * s["H"]), SC.describe(s)
    c = AQ.coverage(seqs)
    print(c)
    assert all(v >= 2 for v in c["ops"].values()), c["ops"]
    assert c["streams"] == {None, 0, 1}
    assert all(v >= 2 for v in c["change_then_add"].values()), c["change_then_add"]
    assert c["knob_then_selecting_add"] >= 2 and c["selecting"] >= 4
    assert 0 in c["caps"] and any(cap >= 2 for cap in c["caps"])
    assert c["reprojects_in_one"] >= 2
    assert c["async_chains"] >= 1 and c["blocking_chains"] >= 1
    assert {5, 8, 16} & c["add_sizes"] and {40, 64} <= c["add_sizes"], "both sides of the sort threshold (4 x prepass_spp = 32 or 64)"
    assert c["refused"] == set(SC.ACCUM_REFUSED)
    assert c["begin_over_live"] >= len(seqs)
    assert c["growth_and_shrink"] == len(seqs), "every sequence has a growth and a shrink of 4 x in the accumulation's pixels"
    assert c["between"] >= 2, "calls of the other families between two adds"


def test_accum_changes_are_visible_and_reprojects_keep_a_part(model):
    shown, hidden, shares = {k: 0 for k in SC.ACCUM_CHANGES}, [], []
    for seed in ACCUM_SEEDS:
        sh, hi, sr = AQ.visibility(SC.draw_accum_sequence(seed), model)
        for k, v in sh.items():
            shown[k] += v
        hidden += [(seed,) + h for h in hi]
        shares += [(seed,) + s for s in sr]
    n = sum(shown.values()) + len(hidden)
    print("visible changes: %d of %d %r; hidden: %r; history kept by the reprojects: %r" % (sum(shown.values()), n, shown, hidden, [(s, i, round(v, 3)) for s, i, v in shares]))
    assert 10 * sum(shown.values()) >= 9 * n, hidden
    assert all(v >= 2 for v in shown.values()), shown
    trivial = [s for s in shares if s[2] in (0.0, 1.0)]
    assert len(shares) >= 6 and 10 * len(trivial) <= len(shares), trivial


def test_the_accum_and_guide_draws_are_the_pinned_ones():
    for name, seed0, seeds, draw in (("accum_sequence_call_lists.json", SC.ASEED0, ACCUM_SEEDS, SC.draw_accum_sequence), ("guide_sequence_call_lists.json", SC.GSEED0, GUIDE_SEEDS, SC.draw_guide_sequence)):
        pinned = _pinned(name)
        assert pinned["seed0"] == seed0 and sorted(pinned["call_lists"]) == sorted(str(s) for s in seeds)
        for seed in seeds:
            seq = draw(seed)
            assert ["upload: " + SC.describe(seq["upload"])] + [SC.describe(s) for s in seq["steps"]] == pinned["call_lists"][str(seed)], (name, seed)
