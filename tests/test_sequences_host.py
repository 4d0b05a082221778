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
"""
import numpy as np
import pytest

import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B

SEEDS = SC.default_seeds()


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
