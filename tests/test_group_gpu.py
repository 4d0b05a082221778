"""The one-process / N-context driver of csrc/pt_comm.cpp (pt_group_*: what `pt_main --gpus N` runs) with N > 1.

Every scenario runs in a CHILD process (tests/group_child.py; pt_comm.cpp resolves PT_RCCL_PATH once per process) with N contexts on
device 0 and the stub collective of tests/stub/fake_rccl.cpp - which is not RCCL and proves nothing about RCCL: what it exercises
is our side (ncclCommInitAll, clone_scene on ranks 1..N-1, the option / material fan-out, N asynchronous renders on N streams, the
grouped reduce, the RGBA8 pack of the reduced frame, the drain, buffer regrowth, the failure branches).  Where the box has the GPUs
the same scenarios also run on real devices through the real RCCL (test_real_devices).

The expected frame always comes from a plain single B.Context in this process - which the rest of the suite ties to the oracle -
never from the group.  All comparisons are exact (float frames as uint32 bit patterns): every pixel has exactly one non-zero
contributor and x + 0.0f == x.  The one exception, -0.0f + 0.0f == +0.0f, and NaNs (whose payload a sum need not keep) are ruled out
by asserting that the expected frames contain neither."""
import json
import os
import sys

import numpy as np
import pytest

import group_child as GC
import rccl_stub
from conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = os.path.join(ROOT, "tests", "group_child.py")
CHILD_LIMIT = 300  # seconds per child: start-up + a handful of frames of a few ms each take < 10 s; the rest is slack for a loaded box
CORNELL = ["render", "cornell", 320, 200, 48, 16, 1]  # scenario a's frame: + tag

_expected = {}


def _B():
    return GC.pkg()[0]


def _device_count():
    import torch

    return torch.cuda.device_count()


def _want(steps, tmp_path):
    """The same steps on ONE plain context in this process (cached: they do not depend on the group size)."""
    key = json.dumps(steps)
    if key not in _expected:
        d = str(tmp_path / "want")
        ctx = _B().Context(0)
        info = GC.run_steps(ctx, steps, d)
        ctx.close()
        frames = {}
        for st in steps:
            if st[0] == "render":
                rgb = np.load(os.path.join(d, st[7] + "_rgb.npy"))
                assert not np.isnan(rgb).any() and not (rgb.view(np.uint32) == 0x80000000).any(), "an exact comparison of sums needs frames without NaN and -0.0f"
                assert rgb.std() > 0.01, "a frame that shows nothing proves nothing"
                frames[st[7]] = (rgb, np.load(os.path.join(d, st[7] + "_rgba8.npy")) if st[6] else None)
        _expected[key] = (frames, info)
    return _expected[key]


def _child(tmp_path, argv, env, name="got"):
    out = str(tmp_path / name)
    rc, so, se = rccl_stub.run_child([sys.executable, CHILD, argv[0], out] + argv[1:], env, CHILD_LIMIT)
    assert rc == 0, "child %s exited with %s\n%s\n%s" % (argv[0], rc, so[-2000:], se[-4000:])
    return out, json.load(open(os.path.join(out, "info.json")))


def _group(tmp_path, devices, steps, env=None):
    sf = tmp_path / "steps.json"
    sf.write_text(json.dumps(steps))
    out, info = _child(tmp_path, ["steps", ",".join(str(d) for d in devices), str(sf)], env or rccl_stub.stub_env())
    assert info["size"] == len(devices)
    return out, info


def _same(out, tag, want, what):
    rgb, rgba8 = want
    got = np.load(os.path.join(out, tag + "_rgb.npy"))
    bad = got.view(np.uint32) != rgb.view(np.uint32)
    assert not bad.any(), "%s '%s': %d of %d floats differ from the single-context frame (%d NaN)" % (what, tag, bad.sum(), bad.size, np.isnan(got).sum())
    if rgba8 is not None:
        np.testing.assert_array_equal(np.load(os.path.join(out, tag + "_rgba8.npy")), rgba8, err_msg="%s '%s' RGBA8" % (what, tag))


def _check(tmp_path, devices, steps, single_steps=None, env=None):
    """Group over `devices` runs `steps`; every rendered frame must equal the one a single context gets from `single_steps` (default:
    the same steps)."""
    want, want_info = _want(single_steps or steps, tmp_path)
    out, info = _group(tmp_path, devices, steps, env)
    for st in steps:
        if st[0] == "render":
            _same(out, st[7], want[st[7]], "group of %d" % len(devices))
    return out, info, want, want_info


SIZES = [2, 3, 4]  # 3: ranks with different tile counts


def steps_parity():
    return [["upload", "cornell"], CORNELL + ["first"], CORNELL + ["second"]]


@pytest.mark.parametrize("n", SIZES)
def test_frame_parity(tmp_path, n):
    """a. Cornell box 320x200, 48 spp, depth 16, RGBA8 requested, twice on the same group (communicator and buffers reused)."""
    _check(tmp_path, [0] * n, steps_parity())


def steps_regrowth():
    return [["upload", "cornell"], ["render", "cornell", 64, 48, 16, 16, 1, "small"], ["render", "cornell", 320, 200, 16, 16, 1, "grown"],
            ["render", "cornell", 100, 37, 16, 16, 1, "odd"], ["render", "cornell", 100, 37, 16, 16, 0, "odd_no_rgba8"]]


@pytest.mark.parametrize("n", SIZES)
def test_buffer_regrowth_and_shrink(tmp_path, n):
    """b. One group: 64x48, then 320x200 (buffers regrow), then 100x37 (not a multiple of the tile, smaller than the allocation),
    then without the RGBA8 image."""
    _check(tmp_path, [0] * n, steps_regrowth())


def steps_empty_ranks():
    return [["upload", "cornell"], ["render", "cornell", 16, 16, 32, 16, 1, "one_tile"], ["render", "cornell", 40, 24, 32, 16, 1, "six_tiles"]]


def test_ranks_without_a_tile(tmp_path):
    """c. 16x16 at N = 4 is one tile: three ranks take the n_pixels == 0 branch of pt_render_device inside a grouped reduce; 40x24
    has six tiles."""
    B = _B()
    assert [len(B.shard_pixels(16, 16, 16, r, 4)) for r in range(4)] == [256, 0, 0, 0]
    assert sum(len(B.shard_pixels(40, 24, 16, r, 4)) > 0 for r in range(4)) >= 2
    _check(tmp_path, [0] * 4, steps_empty_ranks())


def steps_clone():
    cube = lambda name, tag: [["upload", name], ["info", tag], ["render", name, 160, 96, 16, 6, 1, tag]]
    s = cube("cube_map", "map") + cube("cube_auto", "auto")
    for builder in (1, 2):
        s += [["option", "bvh_builder", builder]] + cube("cube_map", "builder%d" % builder)
    s += [["option", "bvh_builder", 3]]
    for leaf in (1, 7):
        s += [["option", "leaf_size", leaf]] + cube("cube_auto", "leaf%d" % leaf)
    s += [["option", "leaf_size", 4], ["upload", "cornell"], ["info", "cornell"], ["render", "cornell", 160, 96, 16, 16, 1, "cornell"]]  # another scene on the live group
    return s


@pytest.mark.parametrize("n", SIZES)
def test_clone_under_real_use(tmp_path, n):
    """d. Texture + environment map / automatic sky through clone_scene; the tree of every builder and of leaf sizes 1 and 7 built on
    rank 0 and cloned; every rank reports the tree rank 0 has, which is the tree a single context builds; a second upload on the live
    group."""
    steps = steps_clone()
    _, info, _, want_info = _check(tmp_path, [0] * n, steps)
    for tag in [st[1] for st in steps if st[0] == "info"]:
        assert len(info[tag]) == n
        for i in range(n):
            for k in ("quad", "oct", "bvh_nodes"):
                assert info[tag][i][k] == info[tag][0][k], "%s: rank %d's %s differs from rank 0's" % (tag, i, k)
        for k in ("quad", "oct", "bvh_nodes"):
            assert info[tag][0][k] == want_info[tag][0][k], (tag, k)
        assert info[tag][0]["bvh_nodes"] > 0


def steps_materials():
    return [["upload", "cornell"], CORNELL + ["before"], ["materials", "cornell", 3, 1, 0.1], CORNELL + ["after"]]


@pytest.mark.parametrize("n", SIZES)
def test_material_hot_swap(tmp_path, n):
    """e. One changed material (the left wall's green 0.89 -> 0.1: the wall itself and everything it lights) through
    Group.set_materials: a rank that kept the old array would leave its tiles as they were, and the comparison with the single context's
    frame after the same set_materials would fail there - given that every rank owns pixels the swap changes, which is asserted."""
    out, _, want, _ = _check(tmp_path, [0] * n, steps_materials())
    a, b = want["before"][0], want["after"][0]
    changed = (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)
    W, H = 320, 200
    for r in range(n):  # the swap is visible in every rank's share of the frame, so every rank is under test
        ids = _B().shard_pixels(W, H, 16, r, n)
        assert changed.reshape(-1)[ids].any(), "rank %d of %d owns no pixel that the swap changes" % (r, n)


OPTIONS = [[("groups", 2)], [("whole", 1)], [("schedule", 0), ("chunk_spp", 3)], [("kernel", 1)], [("fallback", 1)], [("box_exact", 1)]]
DEFAULTS = dict(groups=1, whole=-1, schedule=1, chunk_spp=64, kernel=2, fallback=0, box_exact=-1)  # csrc/pt_internal.h


def steps_options():
    s = [["upload", "cornell"]]
    for opts in OPTIONS:
        s += [["option", k, v] for k, v in opts]
        s += [CORNELL + ["_".join("%s%d" % kv for kv in opts)]]
        s += [["option", k, DEFAULTS[k]] for k, _ in opts]
    return s + [["option", "count", 1], CORNELL + ["count"], ["info", "count"]]


@pytest.mark.parametrize("n", SIZES)
def test_option_fan_out_and_load_split(tmp_path, n):
    """f. Options through Group.set_option leave the frame as the single context with default options renders it.  With count = 1
    every rank reports exactly the samples of ITS tiles: frame equality cannot see the split (any partition of the pixels sums to the
    right frame, including rank 0 rendering everything while the others idle)."""
    steps = steps_options()
    single = [["upload", "cornell"]] + [CORNELL + [st[7]] for st in steps if st[0] == "render"]
    _, info, _, _ = _check(tmp_path, [0] * n, steps, single_steps=single)
    W, H, spp = CORNELL[2], CORNELL[3], CORNELL[4]
    samples = [r["samples"] for r in info["count"]]
    assert samples == [len(_B().shard_pixels(W, H, 16, r, n)) * spp for r in range(n)]
    assert sum(samples) == W * H * spp


def _small_want(tmp_path):
    return _want([["upload", "cornell"], GC.SMALL], tmp_path)[0]["after"]


def test_failure_init_all(tmp_path):
    """g. ncclCommInitAll returns an error (injected on the host): no group, a message that names the call, and the device is fine -
    a plain context in the same process renders the cube."""
    out, info = _child(tmp_path, ["fail_initall"], rccl_stub.stub_env(FAKE_RCCL_FAIL="initall"))
    assert info["group_is_null"] and "ncclCommInitAll" in info["error"], info
    want = _want([["upload", "cube_auto"], ["render", "cube_auto", 64, 48, 8, 4, 1, "after"]], tmp_path)[0]["after"]
    _same(out, "after", want, "plain context after the failed create")


def test_failure_reduce_on_one_rank(tmp_path):
    """g. ncclReduce of rank 1 of 3 returns an error: PT_E_HIP, the group's message names the device and says to destroy the group,
    pt_group_destroy returns, a fresh group in the same process renders correctly."""
    out, info = _child(tmp_path, ["fail_render", "0,0,0"], rccl_stub.stub_env(FAKE_RCCL_FAIL="reduce:1"))
    assert info["rc"] == GC.PT_E_HIP and info["destroyed"], info
    assert "ncclReduce failed on device 0" in info["error"] and "destroy the group" in info["error"], info
    assert info["rank_errors"][1] == info["error"], info  # the failing rank's context carries it too
    _same(out, "after", _small_want(tmp_path), "fresh group after the failed reduce")


def test_failure_group_end(tmp_path):
    """g. ncclGroupEnd returns an error: PT_E_HIP through fail_all, which drains every stream (the call returns); destroy returns."""
    out, info = _child(tmp_path, ["fail_render", "0,0"], rccl_stub.stub_env(FAKE_RCCL_FAIL="groupend"))
    assert info["rc"] == GC.PT_E_HIP and info["destroyed"] and "ncclGroupEnd failed" in info["error"], info
    _same(out, "after", _small_want(tmp_path), "fresh group after the failed group end")


def test_argument_errors(tmp_path):
    """g. What the group entry points refuse - a group whose second context cannot be created is taken apart half-made - and that a
    group still renders correctly after refusing."""
    out, info = _child(tmp_path, ["arg_errors"], rccl_stub.stub_env())
    for n in (0, 65):
        assert info["create_%d" % n]["is_null"] and "%d devices" % n in info["create_%d" % n]["error"], info
    assert info["create_half"]["is_null"] and "no usable HIP device" in info["create_half"]["error"], info
    assert info["no_scene"]["rc"] == GC.PT_E_NO_SCENE and "pt_upload_scene not called" in info["no_scene"]["error"], info
    assert info["null_cam"] == info["null_rgb"] == info["zero_width"] == GC.PT_E_INVALID, info
    assert info["ctx_out_of_range"] == [True, True]
    ng = info["null_group"]
    assert ng["upload"] == ng["materials"] == ng["option"] == ng["render"] == GC.PT_E_INVALID and ng["size"] == 0 and ng["ctx_is_null"], info
    _same(out, "after", _small_want(tmp_path), "group after the refused calls")


def test_stub_self_checks(tmp_path):
    """h. So that a green run means something: the stub alone, through ctypes - a grouped reduce of three device buffers gives the
    rank-ordered host sum on the root and quiet NaNs on the others; a missing rank, a rank twice, mismatched counts and an ungrouped
    reduce are ncclInvalidUsage and touch no buffer; nesting; the injected return codes."""
    _, info = _child(tmp_path, ["stub_selfcheck", rccl_stub.stub_path()], dict(os.environ))
    assert info["checks"] == ["grouped_sum_and_nans", "missing_rank", "mismatched_counts", "rank_twice", "ungrouped", "nesting_and_recovery", "injection",
                              "world_one_null_devices"]


@pytest.mark.parametrize("which", ["two", "all"])
@pytest.mark.parametrize("scenario", ["parity", "empty_ranks", "materials"])
def test_real_devices(tmp_path, scenario, which):
    """i. Scenarios a, c and e on devices 0..N-1 through the real RCCL (no stub), N = 2 and N = all devices."""
    nd = _device_count()
    if nd < 2:
        pytest.skip("needs 2 GPUs")
    n = 2 if which == "two" else nd
    if which == "all" and nd == 2:
        pytest.skip("2 devices: covered by 'two'")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("PT_RCCL_PATH", None)
    _check(tmp_path, list(range(n)), dict(parity=steps_parity, empty_ranks=steps_empty_ranks, materials=steps_materials)[scenario](), env=env)
