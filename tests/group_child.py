"""What the children of tests/test_group_gpu.py run (`python tests/group_child.py MODE OUT_DIR ...`), and the step interpreter the
parent uses too: run_steps() drives a B.Group (child) or a plain B.Context (parent, the expected frames) through the same list of
steps, because both have upload_scene / set_materials / set_option / render.  Results go to OUT_DIR as .npy files and info.json.

Steps: ["option", key, value], ["upload", scene], ["materials", scene, material index, float index, value],
["render", scene (camera), W, H, spp, depth, want_rgba8, tag], ["info", tag] (per rank: quad_info, oct_info, bvh_nodes, samples)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_E_INVALID, PT_E_HIP, PT_E_NO_SCENE = -1, -3, -4


def pkg():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B, scene_io

    return B, scene_io


def scene(name):
    """cornell: the cornell box, no environment light; cube_map / cube_auto: the textured cube (checker stand-in) under an
    environment map / the automatic sky."""
    B, scene_io = pkg()
    assets = os.path.join(ROOT, "assets")
    if name == "cornell":
        sc = scene_io.load_scene_dir(assets, "cornell-box")
        textures, mesh_textures, env = None, None, dict(color=(1, 1, 1), intensity=0.0)
    elif name in ("cube_map", "cube_auto"):
        sc = scene_io.load_scene_dir(assets, "cube")
        textures, mesh_textures = [scene_io.checker_texture()], [0] * len(sc["entities"])
        if name == "cube_auto":
            env = dict(use_auto=True, intensity=1.0)
        else:
            yy, xx = np.mgrid[0:16, 0:32]
            env = dict(use_map=True, intensity=1.0, env_map=((xx * 8) | ((yy * 16) << 8) | (((xx + yy) * 5) << 16) | (0xFF << 24)).astype(np.uint32))
    else:
        raise ValueError(name)
    return dict(entities=sc["entities"], materials=np.stack([m for _, m, _ in sc["materials"]]).astype(np.float32), textures=textures,
                mesh_textures=mesh_textures, env=env, camera=sc["camera"])


def camera(name, W, H):
    B, _ = pkg()
    c = scene(name)["camera"]
    return B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)


def upload(obj, name):
    B, _ = pkg()
    s = scene(name)
    obj.upload_scene(s["entities"], s["materials"], textures=s["textures"], mesh_textures=s["mesh_textures"], env=B.make_env(**s["env"]))


def run_steps(obj, steps, out_dir):
    B, _ = pkg()
    os.makedirs(out_dir, exist_ok=True)
    info = {}
    for st in steps:
        op = st[0]
        if op == "option":
            obj.set_option(st[1], st[2])
        elif op == "upload":
            upload(obj, st[1])
        elif op == "materials":
            mats = scene(st[1])["materials"].copy()
            mats[st[2], st[3]] = st[4]
            obj.set_materials(mats)
        elif op == "render":
            _, name, W, H, spp, depth, want8, tag = st
            rgb, rgba8 = obj.render(camera(name, W, H), W, H, spp, depth, want_rgba8=bool(want8))
            np.save(os.path.join(out_dir, tag + "_rgb.npy"), rgb)
            if want8:
                np.save(os.path.join(out_dir, tag + "_rgba8.npy"), rgba8)
        elif op == "info":
            ranks = [obj.ctx(i) for i in range(obj.size)] if isinstance(obj, B.Group) else [obj]
            info[st[1]] = [dict(quad=c.quad_info(), oct=c.oct_info(), bvh_nodes=int(c.stats()["bvh_nodes"]), samples=int(c.stats()["samples"])) for c in ranks]
        else:
            raise ValueError(op)
    return info


def finish(out_dir, info):
    with open(os.path.join(out_dir, "info.json.tmp"), "w") as f:
        json.dump(info, f)
    os.replace(os.path.join(out_dir, "info.json.tmp"), os.path.join(out_dir, "info.json"))


def mode_steps(out_dir, devices, steps_file):
    B, _ = pkg()
    g = B.Group([int(d) for d in devices.split(",")])
    info = run_steps(g, json.load(open(steps_file)), out_dir)
    info["size"] = g.size
    g.close()
    finish(out_dir, info)


SMALL = ["render", "cornell", 64, 48, 8, 16, 1, "after"]


def _raw_render(B, g, name, W, H, cam=True, rgb=True):
    out = np.zeros((H if H > 0 else 1, W if W > 0 else 1, 3), np.float32)
    return B.lib().pt_group_render(g._g, C.byref(camera(name, max(W, 1), max(H, 1))) if cam else None, W, H, 8, 16,
                                   out.ctypes.data_as(C.POINTER(C.c_float)) if rgb else None, None)


def mode_fail_initall(out_dir):
    """FAKE_RCCL_FAIL=initall is set: pt_group_create must fail cleanly, a plain context must work afterwards."""
    B, _ = pkg()
    L = B.lib()
    g = L.pt_group_create((C.c_int32 * 2)(0, 0), 2)
    info = dict(group_is_null=not g, error=L.pt_last_error(None).decode())
    ctx = B.Context(0)
    run_steps(ctx, [["upload", "cube_auto"], ["render", "cube_auto", 64, 48, 8, 4, 1, "after"]], out_dir)
    ctx.close()
    finish(out_dir, info)


def mode_fail_render(out_dir, devices):
    """FAKE_RCCL_FAIL names a reduce or the group end: pt_group_render must fail with PT_E_HIP and return, pt_group_destroy must
    return, and with the injection cleared a fresh group in the same process must render correctly."""
    B, _ = pkg()
    devs = [int(d) for d in devices.split(",")]
    g = B.Group(devs)
    upload(g, "cornell")
    rc = _raw_render(B, g, "cornell", 64, 48)
    info = dict(rc=rc, error=g.last_error(), rank_errors=[B.lib().pt_last_error(g.ctx(i)._h).decode() for i in range(g.size)])
    g.close()
    info["destroyed"] = True
    del os.environ["FAKE_RCCL_FAIL"]  # (unsetenv: the stub reads the variable at call time)
    g = B.Group(devs)
    upload(g, "cornell")
    run_steps(g, [SMALL], out_dir)
    g.close()
    finish(out_dir, info)


def mode_arg_errors(out_dir):
    B, _ = pkg()
    L = B.lib()
    info = {}
    for n in (0, 65):
        g = L.pt_group_create((C.c_int32 * 65)(), n)
        info["create_%d" % n] = dict(is_null=not g, error=L.pt_last_error(None).decode())
    g = L.pt_group_create((C.c_int32 * 2)(0, 1 << 20), 2)  # the second pt_create fails: destroy of a half-made group (no buffers, no communicator)
    info["create_half"] = dict(is_null=not g, error=L.pt_last_error(None).decode())
    g = B.Group([0, 0])
    info["no_scene"] = dict(rc=_raw_render(B, g, "cornell", 64, 48), error=g.last_error())
    upload(g, "cornell")
    info["null_cam"] = _raw_render(B, g, "cornell", 64, 48, cam=False)
    info["null_rgb"] = _raw_render(B, g, "cornell", 64, 48, rgb=False)
    info["zero_width"] = _raw_render(B, g, "cornell", 0, 48)
    info["ctx_out_of_range"] = [L.pt_group_ctx(g._g, i) is None for i in (-1, 2)]
    mats = scene("cornell")["materials"]
    fp = mats.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros((48, 64, 3), np.float32)
    info["null_group"] = dict(upload=L.pt_group_upload_scene(None, None, 0, fp, mats.shape[0], None, 0, None, None),
                              materials=L.pt_group_set_materials(None, fp, mats.shape[0]), option=L.pt_group_set_option(None, b"count", 1),
                              render=L.pt_group_render(None, C.byref(camera("cornell", 64, 48)), 64, 48, 8, 16, out.ctypes.data_as(C.POINTER(C.c_float)), None),
                              size=L.pt_group_size(None), ctx_is_null=L.pt_group_ctx(None, 0) is None)
    L.pt_group_destroy(None)
    run_steps(g, [SMALL], out_dir)  # the group is still good after every refused call
    g.close()
    finish(out_dir, info)


def mode_stub_selfcheck(out_dir, stub):
    """The stub alone through ctypes (no libmi355pt): what a green group test rests on."""
    S = C.CDLL(stub)
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    S.ncclCommInitAll.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int)]
    S.ncclReduce.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    S.ncclCommDestroy.argtypes = [C.c_void_p]
    F32, SUM, OK, INTERNAL, USAGE = 7, 0, 0, 3, 5
    N = 1000
    rng = np.random.default_rng(11)
    src = [(rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N)).astype(np.float32) for _ in range(3)]
    QNAN = np.uint32(0x7FC00000)

    def dev(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), a.nbytes) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return p

    def host(p, n=N):
        a = np.empty(n, np.float32)
        assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, a.nbytes, 2) == 0
        return a

    comms = (C.c_void_p * 3)()
    assert S.ncclCommInitAll(comms, 3, (C.c_int * 3)(0, 0, 0)) == OK  # the same device three times
    checks = []
    marker = np.full(N, 7.0, np.float32)

    def reduce_all(root, ranks=(0, 1, 2), counts=(N, N, N), depth=1, in_place=False):
        send = [dev(a) for a in src]
        recv = send if in_place else [dev(marker) for _ in src]
        for _ in range(depth):
            assert S.ncclGroupStart() == OK
        rcs = [S.ncclReduce(send[r], recv[r], counts[r], F32, SUM, root, comms[r], None) for r in ranks]
        inner = [S.ncclGroupEnd() for _ in range(depth - 1)]
        after_inner = [host(p) for p in recv]
        end = S.ncclGroupEnd()
        got = [host(p) for p in recv]
        for p in set(x.value for x in send + recv):
            assert hip.hipFree(p) == 0
        return rcs, inner, after_inner, end, got

    def expect_sum(got, root):
        want = src[root].copy()
        for r in range(3):
            if r != root:
                want = want + src[r]  # float32, rank order after the root: the order of the process mode
        np.testing.assert_array_equal(got[root].view(np.uint32), want.view(np.uint32))
        for r in range(3):
            if r != root:
                assert (got[r].view(np.uint32) == QNAN).all(), "non-root receive buffer must be all quiet NaNs"

    for root in (0, 1):
        for in_place in (False, True):
            rcs, _, _, end, got = reduce_all(root, in_place=in_place)
            assert rcs == [OK] * 3 and end == OK
            expect_sum(got, root)
    checks.append("grouped_sum_and_nans")

    def untouched(got):
        for a in got:
            np.testing.assert_array_equal(a, marker)

    rcs, _, _, end, got = reduce_all(0, ranks=(0, 2))
    assert rcs == [OK] * 2 and end == USAGE
    untouched(got)
    checks.append("missing_rank")
    rcs, _, _, end, got = reduce_all(0, counts=(N, N - 1, N))
    assert end == USAGE
    untouched(got)
    checks.append("mismatched_counts")
    rcs, _, _, end, got = reduce_all(0, ranks=(0, 1, 1, 2))
    assert end == USAGE
    untouched(got)
    checks.append("rank_twice")
    a, b = dev(src[0]), dev(marker)
    assert S.ncclReduce(a, b, N, F32, SUM, 0, comms[0], None) == USAGE
    np.testing.assert_array_equal(host(b), marker)
    assert S.ncclGroupEnd() == USAGE  # no group open
    checks.append("ungrouped")
    rcs, inner, after_inner, end, got = reduce_all(0, depth=2)
    assert inner == [OK] and end == OK
    untouched(after_inner)  # the inner end executes nothing
    expect_sum(got, 0)
    checks.append("nesting_and_recovery")  # (also: the refused groups above left nothing behind)

    os.environ["FAKE_RCCL_FAIL"] = "groupend"
    rcs, _, _, end, got = reduce_all(0)
    assert rcs == [OK] * 3 and end == INTERNAL
    untouched(got)
    os.environ["FAKE_RCCL_FAIL"] = "reduce:2"
    rcs, _, _, end, got = reduce_all(0)
    assert rcs == [OK, OK, INTERNAL] and end == USAGE
    untouched(got)
    os.environ["FAKE_RCCL_FAIL"] = "initall"
    assert S.ncclCommInitAll((C.c_void_p * 2)(), 2, None) == INTERNAL
    del os.environ["FAKE_RCCL_FAIL"]
    rcs, _, _, end, got = reduce_all(0)
    assert end == OK
    expect_sum(got, 0)
    checks.append("injection")
    one = (C.c_void_p * 1)()
    assert S.ncclCommInitAll(one, 1, None) == OK  # devices NULL: 0..n-1
    assert S.ncclGroupStart() == OK and S.ncclReduce(a, b, N, F32, SUM, 0, one[0], None) == OK and S.ncclGroupEnd() == OK
    np.testing.assert_array_equal(host(b).view(np.uint32), src[0].view(np.uint32))
    checks.append("world_one_null_devices")
    hip.hipFree(a), hip.hipFree(b)
    for c in list(comms) + list(one):
        assert S.ncclCommDestroy(c) == OK
    finish(out_dir, dict(checks=checks))


if __name__ == "__main__":
    mode, out = sys.argv[1], sys.argv[2]
    os.makedirs(out, exist_ok=True)
    {"steps": mode_steps, "fail_initall": mode_fail_initall, "fail_render": mode_fail_render, "arg_errors": mode_arg_errors,
     "stub_selfcheck": mode_stub_selfcheck}[mode](out, *sys.argv[3:])
