"""The guide pass (pt_render_aov: first-hit albedo, normal, depth, coverage) without a GPU.

* The four exports exist and the ABI version is still 5.
* Argument errors of pt_debug_aov_host and pt_render_aov on a host-only context: checked before anything is touched.
* aov_ref.fma32 (float64 product and sum, exact decision on float32 ties) against pure Fraction arithmetic: random operands and
  constructed cases in which the float64 sum IS a float32 tie and the exact sum is not.
* The numpy restatement tests/aov_ref.py tied to the oracle: for every pixel of every test frame, sample 0's ray and hit equal row 0 of
  Scene.trace_sample(sample = 0) bit for bit (org, dir, hit flag, t, u, v, prim), and where the log has a row 1 its origin equals the
  restatement's interp3 of the hit triangle's positions (which pins fma32 and the barycentric order).  On every ray of the cases the
  oracle's walk and its brute force agree (the closest-hit domain of DESIGN.md 2.1).
* pt_debug_aov_host == aov_ref, all 8 channels of every pixel, on the cases of aov_common.py with watertight 0 and 1.
* A host-only context after pt_update_vertices equals a fresh upload of the moved meshes.
* The guide kernels need no scratch: the resource report of `make asm-aov`."""
import ctypes as C
import re
from fractions import Fraction

import numpy as np
import pytest

import aov_common as AC
import aov_ref
import refit_common as RC
import resource_report
from owl_path_tracer_amd.pyhost import binding as B

ROOT = AC.ROOT
F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
FRAMES = sorted({(name, W, H) for name, W, H, _ in AC.CASES})


def test_exports_and_abi():
    L = B.lib()
    for name in ("pt_render_aov", "pt_render_aov_device", "pt_group_render_aov", "pt_debug_aov_host"):
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\(" % name, open(B.HEADER_PATH).read()), name
    assert L.pt_abi_version() == 5


def test_argument_errors_on_a_host_only_context():
    L = B.lib()
    sc = AC.scene("cube")
    cam = AC.camera(sc, 8, 8, B.to_camera_data)
    ids = np.arange(64, dtype=np.uint32)
    out = np.full((64, 8), 7.0, F32)
    idp, outp = ids.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_float))
    ctx = B.Context(-1)
    try:
        assert L.pt_debug_aov_host(ctx._h, C.byref(cam), 8, 8, 1, idp, 64, outp) == PT_E_NO_SCENE
        assert L.pt_render_aov(ctx._h, C.byref(cam), 8, 8, 1, outp) == PT_E_NO_DEVICE  # no CPU fallback of the render entry point
        AC.upload(ctx, sc, B)
        assert L.pt_render_aov(ctx._h, C.byref(cam), 8, 8, 1, outp) == PT_E_NO_DEVICE
        assert L.pt_render_aov_device(ctx._h, C.byref(cam), 8, 8, 1, C.c_void_p(16), None) == PT_E_NO_DEVICE
        assert L.pt_group_render_aov(None, C.byref(cam), 8, 8, 1, outp) == PT_E_INVALID
        for args in [(None, C.byref(cam), 8, 8, 1, idp, 64, outp), (ctx._h, None, 8, 8, 1, idp, 64, outp), (ctx._h, C.byref(cam), 8, 8, 1, idp, 64, None),
                     (ctx._h, C.byref(cam), 8, 8, 1, None, 64, outp), (ctx._h, C.byref(cam), 8, 8, 1, idp, -1, outp), (ctx._h, C.byref(cam), 8, 8, 0, idp, 64, outp),
                     (ctx._h, C.byref(cam), 8, 8, -3, idp, 64, outp), (ctx._h, C.byref(cam), 0, 8, 1, idp, 64, outp), (ctx._h, C.byref(cam), 8, -1, 1, idp, 64, outp),
                     (ctx._h, C.byref(cam), 65536, 8, 1, idp, 64, outp), (ctx._h, C.byref(cam), 8, 7, 1, idp, 64, outp)]:  # 8 x 7: ids 56..63 lie outside the frame
            assert L.pt_debug_aov_host(*args) == PT_E_INVALID, args[2:7]
        assert (out == 7.0).all(), "a refused call wrote to the output"
        assert L.pt_debug_aov_host(ctx._h, C.byref(cam), 8, 8, 1, idp, 0, outp) == 0
        assert L.pt_debug_aov_host(ctx._h, C.byref(cam), 8, 8, 2, idp, 64, outp) == 64
        assert np.isfinite(out).all() and (out != 7.0).any()
    finally:
        ctx.close()


def _naive_fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def test_fma32_against_fractions():
    rng = np.random.default_rng(7)
    n = 4000
    a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    c = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(F32)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3].astype(np.float64))).astype(F32)  # cancellation: the sum is the product's rounding error
    # constructed: 3 * (1 + k 2^-23) with k odd is a float32 midpoint (1.5 k ulps of 2^-22); a tiny c of either sign puts the exact sum
    # beside it, and the float64 sum drops c - a float32 tie that the exact value is not
    k = rng.integers(0, 1 << 20, 600) * 2 + 1  # (the product stays below 4: one binade, ulp 2^-22)
    ta = np.full(k.size, 3.0, F32)
    tb = (1.0 + k.astype(np.float64) * 2.0 ** -23).astype(F32)
    assert (tb.astype(np.float64) == 1.0 + k * 2.0 ** -23).all()
    tc = (np.where(rng.integers(0, 2, k.size) == 1, 1.0, -1.0) * 2.0 ** rng.choice([-80, -60, -100], k.size)).astype(F32)
    exact_ties = (ta.copy(), tb.copy(), np.zeros(k.size, F32))  # c = 0: true ties, ties-to-even
    for name, (x, y, z) in (("random", (a, b, c)), ("beside a tie", (ta, tb, tc)), ("true ties", exact_ties)):
        got = aov_ref.fma32(x, y, z)
        want = np.array([aov_ref.round_fraction_to_f32(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))) for p, q, r in zip(x, y, z)], F32)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), name
    wrong = _naive_fma(ta, tb, tc).view(np.uint32) != aov_ref.fma32(ta, tb, tc).view(np.uint32)
    assert wrong.mean() > 0.3, "the constructed cases must be ones the two roundings of float64 get wrong"
    # the referee itself, on values whose rounding is known
    assert aov_ref.round_fraction_to_f32(Fraction(1) + Fraction(1, 1 << 24)) == F32(1.0)                      # tie -> even
    assert aov_ref.round_fraction_to_f32(Fraction(1) + Fraction(3, 1 << 24)) == F32(1.0 + 2.0 ** -22)          # tie -> even (up)
    assert aov_ref.round_fraction_to_f32(Fraction(1) + Fraction(1, 1 << 24) + Fraction(1, 1 << 90)) == F32(1.0 + 2.0 ** -23)


def _u32(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("name,W,H", FRAMES)
def test_restatement_is_tied_to_the_oracle(orc, name, W, H, wt):
    sc = AC.scene(name)
    flat = sc["flat"]
    S = orc.Scene(flat, watertight=bool(wt))
    ocam = AC.camera(sc, W, H, orc.to_camera_data)
    env = orc.make_env(**sc["env"])
    n = max(k for nm, w, h, k in AC.CASES if (nm, w, h) == (name, W, H))
    r = aov_ref.samples(S, flat, sc["env"], ocam.as_array(), W, H, n, np.arange(W * H))
    # the domain: the oracle's walk and its brute force agree on every ray of the case
    walk = S.intersect_n(r["rays"].reshape(-1, 6), use_bvh=True)
    for a, b in zip(walk, (r["hit"], r["t"], r["u"], r["v"], r["prim"])):
        assert (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b.reshape(-1)).view(np.uint8)).all()
    pos = np.asarray(flat["positions"], F32).reshape(-1, 3, 3)
    rows1 = 0
    for pid in range(W * H):
        log = S.trace_sample(ocam, env, W, H, pid % W, pid // W, 0, 4)
        assert log.shape[0] >= 1
        row = log[0]
        assert (_u32(row[0:6]) == _u32(r["rays"][pid, 0])).all(), (pid, row[0:6], r["rays"][pid, 0])
        hit = bool(r["hit"][pid, 0])
        assert (row[6] != 0) == hit, pid
        if hit:
            assert (_u32(row[7:10]) == _u32([r["t"][pid, 0], r["u"][pid, 0], r["v"][pid, 0]])).all(), pid
            assert int(_u32(row[10:11]).view(np.int32)[0]) == int(r["prim"][pid, 0]), pid
        if log.shape[0] > 1:  # the path went on from the hit point: interp3 of the positions, (1 - u - v, u, v) in this order
            assert hit
            u, v = r["u"][pid, 0:1], r["v"][pid, 0:1]
            tri = pos[int(r["prim"][pid, 0])]
            vp = aov_ref.interp3(F32(1.0) - u - v, u, v, tri[None, 0], tri[None, 1], tri[None, 2])[0]
            assert (_u32(log[1][0:3]) == _u32(vp)).all(), (pid, log[1][0:3], vp)
            rows1 += 1
    assert rows1 > W * H // 20, "too few second rows to pin interp3 (%d)" % rows1


@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("name,W,H,n", AC.CASES)
def test_host_twin_equals_the_restatement(orc, name, W, H, n, wt):
    sc = AC.scene(name)
    want = AC.reference(orc, name, W, H, n, wt)
    assert np.isfinite(want).all()
    alpha = want[..., 3]
    assert 0.05 < alpha.mean() < 0.95 and want[..., 7].max() > 0, "the frame must show hits and misses"
    ctx = B.Context(-1)
    try:
        AC.upload(ctx, sc, B)
        ctx.set_option("watertight", wt)
        cam = AC.camera(sc, W, H, B.to_camera_data)
        AC.assert_same(ctx.aov_host(cam, W, H, n), want, "%s %dx%d n=%d wt=%d: host twin vs aov_ref" % (name, W, H, n, wt))
        ids = np.array([W * H - 1, 0, W + 1, 0], np.uint32)  # list order, any ids, repeats
        part = ctx.aov_host(cam, W, H, n, pixel_ids=ids)
        AC.assert_same(part, want[::-1].reshape(-1, 8)[ids], "listed pixels")
    finally:
        ctx.close()


def test_normals_and_albedo_say_what_the_header_says(orc):
    """Spot checks of the definition on the reference itself: emitter albedo = emission, default material for index -1, normals of unit
    length and not flipped (some face away from the camera), miss = environment."""
    name, W, H, n = "ico_colour", 24, 16, 1
    sc = AC.scene(name)
    S = orc.Scene(sc["flat"])
    r = aov_ref.samples(S, sc["flat"], sc["env"], AC.camera(sc, W, H, orc.to_camera_data).as_array(), W, H, n, np.arange(W * H))
    c, hit, prim = r["contrib"][:, 0], r["hit"][:, 0], r["prim"][:, 0]
    mi = np.asarray(sc["flat"]["material_index"])[np.maximum(prim, 0)]
    assert (c[~hit][:, :3] == (np.array([0.25, 0.5, 1.0], F32) * F32(2.0))).all() and (c[~hit][:, 3:] == 0).all()
    assert (hit & (mi == 2)).any() and (c[hit & (mi == 2)][:, :3] == F32(9.0)).all()
    assert (hit & (mi == -1)).any() and (c[hit & (mi == -1)][:, :3] == F32(0.8)).all()
    ln = np.linalg.norm(c[hit][:, 4:7].astype(np.float64), axis=1)
    assert np.abs(ln - 1).max() < 1e-6
    assert (c[hit][:, 3] == 1).all() and (c[hit][:, 7] == r["t"][:, 0][hit]).all()


@pytest.mark.parametrize("scene_name,frm,at", [("rects", [0.4, 0.6, 3.0], [0.5, 0.5, 0.0]), ("cornell", [3.0, 1.0, 0.0], [0.0, 1.0, 0.0])])
def test_host_only_context_after_update_vertices(scene_name, frm, at):
    scene = RC.make_scene(scene_name)
    W, H, n = 24, 16, 2
    cam = B.to_camera_data(frm, at, [0, 1, 0], 50.0, W, H)
    env = B.make_env(color=(0.5, 0.25, 1.0), intensity=1.0)
    dyn = B.Context(-1)
    try:
        dyn.set_option("dynamic", 1)
        RC.upload(dyn, scene, env=env)
        before = dyn.aov_host(cam, W, H, n)
        for k, with_normals in ((1, False), (2, True)):
            meshes = RC.moved(scene, k, with_normals=with_normals)
            dyn.update_vertices(meshes)
            fresh = B.Context(-1)
            try:
                RC.upload(fresh, scene, meshes, env=env)
                want = fresh.aov_host(cam, W, H, n)
            finally:
                fresh.close()
            got = dyn.aov_host(cam, W, H, n)
            AC.assert_same(got, want, "%s, update %d" % (scene_name, k))
            assert (AC.bits(got) != AC.bits(before)).any(), "the movement must show in the buffers"
    finally:
        dyn.close()


def test_guide_kernels_need_no_scratch():
    """From the Makefile's own target (the flags that ship): every instance of the guide kernel, both builds, reports ScratchSize 0."""
    blocks = resource_report.report("asm-aov")[1]
    names = [b[0] for b in blocks]
    assert all("pt_aov_" in nm for nm in names), "the guide translation units hold the guide kernels and no other: %r" % (names,)
    assert len(blocks) == 5 and len(set(names)) == 5, names  # binary walk + two slab forms of the quad walk; the watertight build: the two quad forms
    assert sum("pt_aov_wt_kernel" in nm for nm in names) == 2, names
    assert all(int(sz) == 0 for _, _, sz in blocks), blocks
    assert all(int(v) <= 128 for _, v, _ in blocks), blocks  # the budget of four waves per SIMD the kernel is launched with
