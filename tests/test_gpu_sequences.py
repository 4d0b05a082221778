"""Random call sequences on one context against the oracle, call by call (generator, model and runner: tests/seq_common.py).

One test per seed: a fresh context lives through an upload with option "dynamic" = 1 and a drawn builder and leaf size, then 8 to 12
calls - update_vertices, new tables, environments, shards, the watertight switch, scheduler knobs, a second upload; single frames,
batches and guide passes, blocking and asynchronous on the context's stream or on one of two caller streams; refused calls - and every
frame and guide buffer is the oracle's for the state the model says the context is in, bit for bit.  An asynchronous call is followed
by the next call at once; one pt_synchronize after the last step precedes the read-back.  After every update the arrays in HBM are held
to the box definition, on whatever tree builder 0, 1 or 2 made.  tests/test_sequences_host.py asserts what the default seeds contain
and that their changes show.

test_guide_sequence is the same for the second family (seq_common.draw_guide_sequence, 8 to 14 calls): pt_render_aov_follow,
pt_render_aov_batch, pt_denoise and pt_denoise_batch, blocking and asynchronous, in the middle of a context's life - render, guides and
filter chained over caller buffers on three streams with nothing in between, the filter's records growing and shrinking, per-frame
tables in front of the context's, the batch cut changed, refused calls that must leave the caller's buffers alone - against
tests/aov_follow_ref.py and tests/denoise_ref.py on the oracle's frames, bit for bit, and pt_get_stats' launches after every blocking call.

test_accum_sequence is the third family (seq_common.draw_accum_sequence, 10 to 16 calls; model: tests/accum_seq_common.py): three
accumulations of growing and shrinking size in the middle of a context's life - adds after scene changes and scheduler knobs, selecting
adds, reprojects, the filter and the upsampling chained on one stream, pt_denoise_var and pt_upsample of the model's own inputs, calls of the
other families in between, refused calls - every blocking step compared at once with state, read-back and info, the asynchronous ones and
the final state after the one pt_synchronize.  PT_WRITE_PROFILES=1 records its call lists and seconds in profiles/r20_accum_sequences.json.

12 seeds by default per family; PT_SEQ_CASES=N for more, PT_SEQ_ONLY=seed for one of any family (tools/seq_replay.py prints and replays
a seed).  One more test runs sequences over pt_group_* (two contexts on one card, the stub collective, a child process) with option
"watertight" = 1 and compares the group's frames and guide buffers with a single context's, which run() holds to the oracle: two of the
first family, and one of the second, whose follow passes are the group's and whose filter runs on rank 0's context.
PT_WRITE_PROFILES=1 records the call lists, the builder and the seconds per seed in profiles/r14_sequences.json, and those of the second
family beside the first family's seconds of the same run in profiles/r18_guide_sequences.json.

MEASURED: profiles/r18_guide_sequences.json has the seconds per seed of both families from one run (library, oracle, test).  The oracle's
side dominates; seq_common.SAMPLE_BUDGET, GUIDE_BUDGET and FILTER_BUDGET bound it per call.
"""
import json
import os
import sys
import time

import numpy as np
import pytest

import async_common as A
import rccl_stub
import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONLY = os.environ.get("PT_SEQ_ONLY")
N_CASES = int(os.environ.get("PT_SEQ_CASES", str(SC.N_DEFAULT)))
SEEDS = [s for s in [int(ONLY)] if s < SC.GSEED0] if ONLY else SC.default_seeds(N_CASES)
GUIDE_SEEDS = [s for s in [int(ONLY)] if SC.GSEED0 <= s < SC.ASEED0] if ONLY else SC.default_guide_seeds(N_CASES)
ACCUM_SEEDS = [s for s in [int(ONLY)] if s >= SC.ASEED0] if ONLY else SC.default_accum_seeds(N_CASES)
_report, _guide_report, _accum_report = {}, {}, {}


@pytest.fixture(scope="module")
def model(orc):
    m = SC.Model(orc)
    yield m
    if os.environ.get("PT_WRITE_PROFILES") == "1" and _report:
        path = os.path.join(ROOT, "profiles", "r14_sequences.json")
        with open(path, "w") as f:
            json.dump(dict(seed0=SC.SEED0, sequences=_report), f, indent=1, sort_keys=True)
    if os.environ.get("PT_WRITE_PROFILES") == "1" and _guide_report:
        first = {k: {t: v[t] for t in ("seconds_library", "seconds_oracle", "seconds_test")} for k, v in _report.items()}
        with open(os.path.join(ROOT, "profiles", "r18_guide_sequences.json"), "w") as f:
            json.dump(dict(seed0=SC.GSEED0, sequences=_guide_report, first_family_seconds_of_this_run=first, slowest_first_family_test=max([v["seconds_test"] for v in first.values()] or [0]),
                           slowest_guide_test=max(v["seconds_test"] for v in _guide_report.values())), f, indent=1, sort_keys=True)


    if os.environ.get("PT_WRITE_PROFILES") == "1" and _accum_report:
        with open(os.path.join(ROOT, "profiles", "r20_accum_sequences.json"), "w") as f:
            json.dump(dict(seed0=SC.ASEED0, accum_budget=SC.ACCUM_BUDGET, sequences=_accum_report, slowest_accum_test=max(v["seconds_test"] for v in _accum_report.values())), f, indent=1, sort_keys=True)


def _only_with(seeds):
    """PT_SEQ_ONLY names a seed of ONE family: the other family's test is not collected then (an empty parameter set would show as a skip)."""
    return (lambda f: pytest.mark.parametrize("seed", seeds)(f)) if seeds else (lambda f: None)


@_only_with(SEEDS)
def test_sequence(model, seed):
    seq = SC.draw_sequence(seed)
    ctx = B.Context(0)
    t0, o0 = time.time(), model.seconds
    try:
        SC.run(ctx, seq, model, A=A)
    finally:
        try:
            ctx.close()
        finally:
            A.destroy_streams()
    _report[str(seed)] = dict(calls=["upload: " + SC.describe(seq["upload"])] + [SC.describe(s) for s in seq["steps"]], builder=seq["upload"]["builder"],
                              seconds_library=round(SC.run.seconds, 3), seconds_oracle=round(model.seconds - o0, 3), seconds_test=round(time.time() - t0, 3))
    if os.environ.get("PT_WRITE_PROFILES") == "1":  # (the visible share costs the oracle one more frame per change: only for the record)
        shown, hidden, frames, flat = SC.visibility(seq, model)
        _report[str(seed)].update(changes=sum(shown.values()) + len(hidden), visible_changes=sum(shown.values()), observing_steps=frames, flat_frames=len(flat))
    print("seed %d: %d steps, %.2f s in the library, %.2f s in the oracle" % (seed, len(seq["steps"]), SC.run.seconds, model.seconds - o0))


@_only_with(GUIDE_SEEDS)
def test_guide_sequence(model, seed):
    seq = SC.draw_guide_sequence(seed)
    ctx = B.Context(0)
    t0, o0 = time.time(), model.seconds
    try:
        SC.run(ctx, seq, model, A=A)
    finally:
        try:
            ctx.close()
        finally:
            A.destroy_streams()
    _guide_report[str(seed)] = dict(calls=["upload: " + SC.describe(seq["upload"])] + [SC.describe(s) for s in seq["steps"]], builder=seq["upload"]["builder"],
                                    seconds_library=round(SC.run.seconds, 3), seconds_oracle=round(model.seconds - o0, 3), seconds_test=round(time.time() - t0, 3))
    print("guide seed %d: %d steps, %.2f s in the library, %.2f s in the oracle" % (seed, len(seq["steps"]), SC.run.seconds, model.seconds - o0))


@_only_with(ACCUM_SEEDS)
def test_accum_sequence(model, seed):
    import accum_seq_common as AQ

    seq = SC.draw_accum_sequence(seed)
    ctx = B.Context(0)
    t0, o0 = time.time(), model.seconds + AQ.oracle_seconds[0]
    try:
        SC.run(ctx, seq, model, A=A)
    finally:
        try:
            ctx.close()
        finally:
            A.destroy_streams()
    oracle = model.seconds + AQ.oracle_seconds[0] - o0
    _accum_report[str(seed)] = dict(calls=["upload: " + SC.describe(seq["upload"])] + [SC.describe(s) for s in seq["steps"]], builder=seq["upload"]["builder"],
                                    seconds_library=round(SC.run.seconds, 3), seconds_oracle=round(oracle, 3), seconds_test=round(time.time() - t0, 3))
    print("accum seed %d: %d steps, %.2f s in the library, %.2f s in the oracle" % (seed, len(seq["steps"]), SC.run.seconds, oracle))


def _group_seeds():
    """The first two default seeds whose group projection shows a frame AND a guide buffer after an update_vertices."""
    out = []
    for seed in SC.default_seeds():
        ops = [s["op"] for s in SC.group_projection(SC.draw_sequence(seed))["steps"]]
        if "update_vertices" in ops:
            rest = ops[ops.index("update_vertices"):]
            if "render" in rest and "render_aov" in rest:
                out.append(seed)
    return out[:2]


def _guide_group_seed():
    """The first seed of the second family whose group projection has a follow pass AND a filter on rank 0's context after an update_vertices."""
    for seed in SC.default_guide_seeds(64):
        ops = [s["op"] for s in SC.group_projection(SC.draw_guide_sequence(seed))["steps"]]
        if "update_vertices" in ops:
            rest = ops[ops.index("update_vertices"):]
            if "render_aov_follow" in rest and "denoise" in rest:
                return seed
    return None


def test_sequences_over_a_group(model, tmp_path):
    seeds = _group_seeds()
    assert len(seeds) == 2, seeds
    guide = _guide_group_seed()
    assert guide is not None
    seeds.append(guide)
    out = str(tmp_path / "got")
    rc, so, se = rccl_stub.run_child([sys.executable, os.path.join(ROOT, "tests", "seq_group_child.py"), out, "0,0"] + [str(s) for s in seeds], rccl_stub.stub_env(), 300)
    assert rc == 0, "child exited with %s\n%s\n%s" % (rc, so[-2000:], se[-4000:])
    done = json.load(open(os.path.join(out, "done.json")))
    for seed in seeds:
        seq = SC.group_projection(SC.draw_guide_sequence(seed) if seed == guide else SC.draw_sequence(seed))
        ctx = B.Context(0)
        try:
            single = SC.run(ctx, seq, model, A=A)  # the single context, held to the watertight oracle on the way
        finally:
            ctx.close()
        assert done[str(seed)]["size"] == 2 and done[str(seed)]["steps"] == [g[0] for g in single]
        kinds = set()
        for i, f, f8 in single:
            what = "group of 2, sequence seed=%d, step %d (%s)" % (seed, i, SC.describe(seq["steps"][i]))
            bad = SC.same(np.load(os.path.join(out, "%d_%d_rgb.npy" % (seed, i))), f)
            assert not bad.any(), "%s: %d of %d floats differ from the single context's" % (what, bad.sum(), bad.size)
            if f8 is not None:
                np.testing.assert_array_equal(np.load(os.path.join(out, "%d_%d_rgba8.npy" % (seed, i))), f8, err_msg=what)
            kinds.add(seq["steps"][i]["op"])
        assert kinds == ({"render", "render_aov_follow", "denoise"} if seed == guide else {"render", "render_aov"})
