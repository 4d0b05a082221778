"""The guide pass over a ray image (pt_render_aov_rays; include/mi355pt.h "ray images") without a GPU.

* The three exports exist, are in B.EXPORTS and in the header, the ABI version is still 5 and the _device form is in both lists of the
  streams contract.
* Every refusal of the header on a host-only context, by code and by message; a refused call writes nothing.  (A communicator needs a
  device: that refusal is tests/test_gpu_aov_rays.py's.)
* pt_debug_aov_rays_host == tests/aov_rays_ref.py, all 8 channels of every pixel, over the cases of tests/aov_rays_common.py: Cornell,
  the textured cube, mirror_wall and tir; the pixel-centre rays at 20 x 13 and 64 x 48 and 24 x 16 probe rays from inside and up to 5
  extents outside the scene; n_samples 1 and 3; max_follow 0 and 4.  And on the closed icosphere (tir) under Scene(..., watertight=True).
  The same over JITTER_CASES: the scrambled and equirect tables of tests/ray_tables.py, whose jitter differs from record to record, at
  1 x 1 to 64 x 48, n_samples 1, 3 and 16, under both triangle tests, each case first shown to meet the precondition of
  tests/ray_tables.py in guide buffers (RC.precondition); a restatement with the neighbouring record's jitter, the draws swapped or dv added first is
  told apart from the twin on them.
* Consequence (a): a zero-jitter record is pt_debug_aov_follow_host's pixel under its degenerate camera, one call per listed ray.
* Consequence (b): eight jittered 1 x 1 images at n_samples = 16 from the origin are pt_debug_aov_follow_host's under {0, dir, du, dv}.
* Consequence (c): where a pixel's coverage at n = 1 says hit, its depth at max_follow = 0 is t of pt_debug_trace_rays_host on sample 0's
  ray - on a pinhole table and on a scrambled one.
* `make asm-aov-rays`: exactly the four instances, no scratch, at most 128 VGPRs, no static LDS - the stack and the parked words are
  the launch's dynamic (PT_LDS_STACK + PT_AOV_PARK) * 64 * 4 bytes, which tests/test_gpu_aov_rays.py reads back from pt_get_stats - and
  the other guide and render targets report what they reported before."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import aov_rays_common as RC
import aov_rays_ref
import ray_image_ref as RR
import ray_tables as RT
import resource_report
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import ray_image as RI
from owl_path_tracer_amd.pyhost import scene_io

ROOT = RC.ROOT
F32, U32 = np.float32, np.uint32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_render_aov_rays", "pt_render_aov_rays_device", "pt_debug_aov_rays_host")


def test_exports_abi_and_streams_contract():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    assert "pt_render_aov_rays_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_render_aov_rays_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)
    assert re.search(r"pt_render_rays and pt_render_aov_rays run on the context's stream", header)
    assert RC.record_dtype() == B.RAY_GEN_DTYPE
    for name in ("render_aov_rays", "render_aov_rays_device", "aov_rays_host"):
        assert callable(getattr(B.Context, name))


def test_refusals_and_error_codes():
    L = B.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    W, H = 5, 3
    rays = RI.fixed((0.0, 1.0, 3.0), (0.0, 0.0, -1.0), W, H)
    aov = np.full((H, W, 8), 7.0, F32)
    ids = np.arange(W * H, dtype=U32)
    r, o, idp = rays.ctypes.data_as(vp), aov.ctypes.data_as(fp), ids.ctypes.data_as(C.POINTER(C.c_uint32))
    v16 = vp(16)
    ok = B.aov_default_params()
    ctx = B.Context(-1)
    hd = ctx._h

    def msg():
        return L.pt_last_error(hd).decode()

    def blocking(rr=r, w=W, h=H, p=ok, out=o):
        return L.pt_render_aov_rays(hd, rr, w, h, C.byref(p) if p is not None else None, out)

    def device(rr=v16, w=W, h=H, p=ok, out=v16):
        return L.pt_render_aov_rays_device(hd, rr, w, h, C.byref(p) if p is not None else None, out, None)

    def twin(rr=r, w=W, h=H, p=ok, out=o, n=W * H, pid=idp):
        return L.pt_debug_aov_rays_host(hd, rr, w, h, C.byref(p) if p is not None else None, pid, n, out)

    forms = ((blocking, "pt_render_aov_rays", "rays", "out_aov"), (device, "pt_render_aov_rays_device", "d_rays", "d_out_aov"), (twin, "pt_debug_aov_rays_host", "rays", "out"))
    try:
        # without a scene
        for fn, who, _, _ in forms:
            assert fn() == PT_E_NO_SCENE and who + ":" in msg() and "pt_upload_scene not called" in msg(), who
        RC.upload(ctx, RC.scene("cornell"), B)
        assert L.pt_render_aov_rays(None, r, W, H, None, o) == PT_E_INVALID
        assert L.pt_render_aov_rays_device(None, v16, W, H, None, v16, None) == PT_E_INVALID
        assert L.pt_debug_aov_rays_host(None, r, W, H, None, idp, W * H, o) == PT_E_INVALID
        bad_params = (dict(n_samples=0), dict(n_samples=-2), dict(max_follow=-1), dict(max_follow=9), dict(roughness_max=-0.01), dict(roughness_max=1.01),
                      dict(roughness_max=float("nan")), dict(roughness_max=float("inf")), dict(reserved=1), dict(reserved=-1))
        for fn, who, rname, oname in forms:
            assert fn(rr=None) == PT_E_INVALID and "%s: NULL %s" % (who, rname) in msg()
            assert fn(out=None) == PT_E_INVALID and "%s: NULL %s" % (who, oname) in msg()
            # the sizes pt_render_aov refuses
            for kw in (dict(w=0), dict(h=0), dict(w=-1), dict(w=65536), dict(h=65536)):
                assert fn(**kw) == PT_E_INVALID and "bad guide pass size" in msg(), (who, kw)
            # what pt_render_aov_follow refuses in p
            for bad in bad_params:
                assert fn(p=B.aov_default_params(**bad)) == PT_E_INVALID and who + ":" in msg(), (who, bad, msg())
        for fn, who, _, _ in forms[:2]:
            # a scene without quad nodes: option quad = 0 (there are no binary-walk instances)
            ctx.set_option("quad", 0)
            try:
                assert fn() == PT_E_INVALID and who + ":" in msg() and "quad nodes (option quad = 0)" in msg(), msg()
                assert fn(rr=None) == PT_E_INVALID and "NULL" in msg()  # invalid arguments first
            finally:
                ctx.set_option("quad", 1)
            assert fn() == PT_E_NO_DEVICE  # valid arguments: no CPU fallback behind the entry point
            assert fn(p=None) == PT_E_NO_DEVICE  # NULL = the defaults
            ctx.set_option("watertight", 1)  # the guide pass has watertight instances
            try:
                assert fn() == PT_E_NO_DEVICE
            finally:
                ctx.set_option("watertight", 0)
        for bad in (vp(24), vp(4), vp(17), vp(72)):
            assert device(rr=bad) == PT_E_INVALID and "pt_render_aov_rays_device: d_rays is not 16-byte aligned" in msg()
            assert device(out=bad) == PT_E_INVALID and "pt_render_aov_rays_device: d_out_aov is not 16-byte aligned" in msg()
        # the twin's own arguments
        assert twin(n=-1) == PT_E_INVALID and twin(pid=None) == PT_E_INVALID
        assert twin(w=W, h=H - 1) == PT_E_INVALID and "outside the 5x2 frame" in msg()  # ids 10..14 lie outside
        # the records, which the blocking form and the twin read: not finite, or no direction
        for fn, who in ((blocking, "pt_render_aov_rays"), (twin, "pt_debug_aov_rays_host")):
            for field in ("org", "dir", "du", "dv"):
                for bad in (np.nan, np.inf, -np.inf):
                    for i, comp in ((0, 0), (7, 1), (W * H - 1, 2)):
                        t = rays.copy()
                        t[field][i, comp] = bad
                        assert fn(rr=t.ctypes.data_as(vp)) == PT_E_INVALID
                        assert "%s: record %d (pixel %d, %d): %s is not finite" % (who, i, i % W, i // W, field) in msg(), msg()
            t = rays.copy()
            t["dir"][9] = (0.0, -0.0, 0.0)
            assert fn(rr=t.ctypes.data_as(vp)) == PT_E_INVALID and "%s: record 9 (pixel 4, 1): dir is 0" % who in msg()
        assert (aov == 7.0).all(), "a refused call wrote to its output"
        t = rays.copy()  # the reserved floats are not read: anything may stand there; a zero jitter and a tiny direction are rays
        for k in range(4):
            t["reserved%d" % k] = np.nan
        t["dir"][3] = (0.0, 1e-15, 0.0)
        assert blocking(rr=t.ctypes.data_as(vp)) == PT_E_NO_DEVICE
        assert (aov == 7.0).all()
        assert twin(rr=t.ctypes.data_as(vp)) == W * H and np.isfinite(aov).all() and (aov != 7.0).any()
        assert twin(n=0) == 0
        # the twin walks the host's binary tree: it works whatever "quad" says
        ctx.set_option("quad", 0)
        try:
            RC.assert_same(ctx.aov_rays_host(t, W, H, ok, pixel_ids=ids), aov.reshape(-1, 8), "the twin with option quad = 0")
        finally:
            ctx.set_option("quad", 1)
        RC.assert_same(ctx.aov_rays_host(t, W, H, pixel_ids=ids), aov.reshape(-1, 8), "NULL parameters are the defaults")
        with pytest.raises(B.PtError, match="records for a 5x3 ray image"):
            ctx.render_aov_rays(rays[:-1], W, H)
        with pytest.raises(B.PtError, match="records for a 5x3 ray image"):
            ctx.aov_rays_host(rays[:-1], W, H)
        with pytest.raises(B.PtError, match="no CPU fallback"):
            ctx.render_aov_rays(rays, W, H)
    finally:
        ctx.close()


def _host(name, wt=0):
    ctx = B.Context(-1)
    RC.upload(ctx, RC.scene(name), B)
    ctx.set_option("watertight", wt)
    return ctx


@pytest.mark.parametrize("name,kind,W,H,n,k", RC.CASES, ids=lambda v: str(v))
def test_host_twin_equals_the_restatement(orc, name, kind, W, H, n, k):
    what = "%s %s %dx%d n=%d max_follow=%d" % (name, kind, W, H, n, k)
    want, smp = RC.reference(orc, name, kind, W, H, n, k, 0, want_samples=True)
    assert np.isfinite(want).all()
    table = RC.table(name, kind, W, H, B.to_camera_data)
    assert table.tobytes() == RC.table(name, kind, W, H, orc.to_camera_data).tobytes()
    ctx = _host(name)
    try:
        got = ctx.aov_rays_host(table, W, H, RC.params(B, n, k, RC.ROUGHNESS_MAX))
        RC.assert_same(got, want, what + ": host twin vs aov_rays_ref")
        ids = np.array([W * H - 1, 0, W + 1, 0], U32)  # list order, any ids, repeats
        part = ctx.aov_rays_host(table, W, H, RC.params(B, n, k, RC.ROUGHNESS_MAX), pixel_ids=ids)
        RC.assert_same(part, want[::-1].reshape(-1, 8)[ids], what + ": listed pixels")
    finally:
        ctx.close()
    hit = smp["hit0"]
    if kind == "probes":
        assert hit.any(), what
    if k == 4 and name in ("mirror_wall", "tir"):
        first = RC.reference(orc, name, kind, W, H, n, 0, 0)
        assert (RC.bits(want) != RC.bits(first)).any(), what + ": the case must follow something"


@pytest.mark.parametrize("name,kind,W,H,n,k", RC.JITTER_CASES, ids=lambda v: str(v))
def test_host_twin_equals_the_restatement_on_jittered_tables(orc, name, kind, W, H, n, k):
    what = "%s %s %dx%d n=%d max_follow=%d" % (name, kind, W, H, n, k)
    want, smp = RC.reference(orc, name, kind, W, H, n, k, 0, want_samples=True)
    assert np.isfinite(want).all()
    table = RC.table(name, kind, W, H, B.to_camera_data)
    assert table.dtype == B.RAY_GEN_DTYPE
    shares = RC.precondition(orc, name, kind, W, H, n, k)  # the case can tell records apart, or it is no case
    print(what + ": pixels that differ: " + ", ".join("%s %.1f %%" % (v, 100 * x) for v, x in shares.items()))
    ctx = _host(name)
    try:
        got = ctx.aov_rays_host(table, W, H, RC.params(B, n, k, RC.ROUGHNESS_MAX))
        RC.assert_same(got, want, what + ": host twin vs aov_rays_ref")
        ctx.set_option("watertight", 1)
        RC.assert_same(ctx.aov_rays_host(table, W, H, RC.params(B, n, k, RC.ROUGHNESS_MAX)), RC.reference(orc, name, kind, W, H, n, k, 1), what + ", watertight")
    finally:
        ctx.close()
    if W * H > 1:
        assert smp["hit0"].any(), what


@pytest.mark.parametrize("name", ["mirror_wall", "tir"])
def test_a_wrong_generator_differs_from_the_twin(name):
    """At n_samples = 1 the guide buffers of a table under a generator of some form (RR.FORMS) are those of the zero-jitter table that holds
    that form's sum of sample 0 (RR.one_sample_table): the right form gives the twin's buffers of the jittered table bit for bit, every
    wrong form gives others - a kernel with that mistake would fail tests/test_gpu_aov_rays.py, which compares every pixel."""
    import oracle as orc

    W, H = 20, 13
    t = RT.scrambled(name, W, H)
    rx, ry = RR.draws(orc, W, H, 1)
    prm = RC.params(B, 1, 4, RC.ROUGHNESS_MAX)
    ctx = _host(name)
    try:
        want = ctx.aov_rays_host(t, W, H, prm)
        shares = {}
        for form in RR.FORMS:
            got = ctx.aov_rays_host(RR.one_sample_table(t, rx[:, 0], ry[:, 0], form), W, H, prm)
            shares[form] = float((RC.bits(got) != RC.bits(want)).any(-1).mean())
    finally:
        ctx.close()
    print(name, shares)
    assert shares["right"] == 0.0
    for form in RR.FORMS:
        if form != "right":
            assert shares[form] > 0.0, "the form '%s' (%s) gives the twin's buffers" % (form, RR.FORMS[form])


@pytest.mark.parametrize("kind,W,H", [("centres", 20, 13), ("probes",) + RC.PROBE_SIZE])
def test_watertight_on_the_closed_icosphere(orc, kind, W, H):
    name, n, k = "tir", 3, 4
    want = RC.reference(orc, name, kind, W, H, n, k, 1)
    ctx = _host(name, wt=1)
    try:
        RC.assert_same(ctx.aov_rays_host(RC.table(name, kind, W, H, B.to_camera_data), W, H, RC.params(B, n, k, RC.ROUGHNESS_MAX)), want, "tir %s, watertight" % kind)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", RC.SCENES)
def test_consequence_a_zero_jitter_is_the_degenerate_camera(name):
    """One call of the existing follow twin per listed ray, through the camera {org, L, 0, 0}; the tests choose org and L, never dir."""
    rng = np.random.default_rng(7)
    for kind, W, H in (("centres", 20, 13), ("probes",) + RC.PROBE_SIZE):
        orgs, targets = RC.rays_of(name, kind, W, H, B.to_camera_data)
        table = RC.fixed_table(orgs, targets)
        ids = np.sort(rng.choice(W * H, 24, replace=False)).astype(U32)
        ctx = _host(name)
        try:
            for n, k in ((1, 0), (3, 4)):
                prm = RC.params(B, n, k, RC.ROUGHNESS_MAX)
                got = ctx.aov_rays_host(table, W, H, prm, pixel_ids=ids)
                for j, i in enumerate(ids):
                    c12, d = RR.degenerate_camera(orgs[i], targets[i])
                    assert (d == table["dir"][i]).all()
                    want = ctx.aov_follow_host(RC.camera_of(B, c12), W, H, prm, pixel_ids=[i])
                    RC.assert_same(got[j:j + 1], want, "%s %s ray %d n=%d max_follow=%d" % (name, kind, i, n, k))
        finally:
            ctx.close()


def _centred_cornell():
    """Cornell translated so that the origin lies inside the box (tests/test_gpu_ray_image.py, leg C)."""
    sc = scene_io.load_scene_dir(os.path.join(ROOT, "assets"), "cornell-box")
    P = np.concatenate([m["vertices"] for m, _ in sc["entities"]]).astype(np.float64)
    centre = (0.5 * (P.min(0) + P.max(0))).astype(F32)
    ents = [(dict(m, vertices=(m["vertices"] - centre).astype(F32)), mid) for m, mid in sc["entities"]]
    flat = scene_io.flatten_scene(ents, sc["materials"])
    lo, hi = flat["positions"].reshape(-1, 3).min(0), flat["positions"].reshape(-1, 3).max(0)
    assert (lo < 0).all() and (hi > 0).all(), "the origin lies inside the translated box"
    return ents, sc["materials"], flat


def test_consequence_b_one_pixel_images_are_the_camera_they_name(orc):
    ents, materials, flat = _centred_cornell()
    mats = [m.copy() for _, m, _ in materials]
    mats[1][4], mats[1][7] = 1.0, 0.0  # one material becomes a mirror: some of the samples are followed
    envk = dict(color=(0.3, 0.6, 0.2), intensity=0.75)
    S = orc.Scene(flat)
    ctx = B.Context(-1)
    try:
        ctx.upload_scene(ents, mats, env=B.make_env(**envk))
        seen = set()
        followed = 0
        for k, t in enumerate(RC.jitter_records(B.RAY_GEN_DTYPE)):
            prm = B.aov_default_params(n_samples=16)
            got = ctx.aov_rays_host(t, 1, 1, prm)
            cam = RC.camera_of(B, np.concatenate([np.zeros(3, F32), t["dir"][0], t["du"][0], t["dv"][0]]))
            RC.assert_same(got, ctx.aov_follow_host(cam, 1, 1, prm), "1 x 1 image %d" % k)
            RC.assert_same(got, aov_rays_ref.aov(S, flat, envk, t, 1, 1, 16, 4, 0.3, materials=np.array(mats, F32)), "1 x 1 image %d vs aov_rays_ref" % k)
            followed += int((RC.bits(got) != RC.bits(ctx.aov_rays_host(t, 1, 1, B.aov_default_params(n_samples=16, max_follow=0)))).any())
            seen.add(got.tobytes())
        assert len(seen) == 8 and followed >= 1
    finally:
        ctx.close()


def _consequence_c(name, table, W, H):
    rays0 = aov_rays_ref.table_rays(table, W, H, 1, np.arange(W * H))[:, 0]
    ctx = _host(name)
    try:
        got = ctx.aov_rays_host(table, W, H, B.aov_default_params(n_samples=1, max_follow=0), pixel_ids=np.arange(W * H))
        hits = ctx.trace_rays_host(rays0)
    finally:
        ctx.close()
    covered = got[:, 3] == 1
    assert covered.sum() > W * H // 4 and ((got[:, 3] == 0) | covered).all()
    assert (covered == (hits["prim"] >= 0)).all()
    assert (got[covered, 7].view(U32) == hits["t"][covered].view(U32)).all()
    assert (got[~covered, 7] == 0).all()


@pytest.mark.parametrize("name", ["cornell", "mirror_wall"])
def test_consequence_c_sample_0_is_the_first_camera_ray(orc, name):
    """A jittered table (pinhole of the scene's camera): sample 0's ray is aov_rays_ref.table_rays' - the ray pt_render_rays starts the
    pixel's first path on - and where coverage says hit, the first-hit depth is the ray query's t on it."""
    W, H = 20, 13
    _consequence_c(name, RI.pinhole(RC.camera(RC.scene(name), W, H, B.to_camera_data), W, H), W, H)


@pytest.mark.parametrize("name", ["cornell", "mirror_wall", "tir"])
def test_consequence_c_on_a_scrambled_table(orc, name):
    """The same where every record has its own origin, direction and jitter."""
    _consequence_c(name, RT.scrambled(name, 20, 13), 20, 13)


# ---- resource reports ---------------------------------------------------------------------------------------------------
def test_ray_image_guide_kernels_need_no_scratch_and_fit_128_vgprs():
    """From the Makefile's own target (the flags that ship): the four ray-image instances and no other - both slab forms of the quad walk
    under both triangle tests - ScratchSize 0, at most 128 VGPRs (the four waves per SIMD the kernel is launched with), no static LDS:
    what the kernel uses is the launch's dynamic allocation, (PT_LDS_STACK + PT_AOV_PARK) * 64 * 4 bytes of a CU's 160 KB."""
    rep = resource_report.resources("asm-aov-rays")
    names = sorted(rep)
    assert len(rep) == 4, names
    assert sum("pt_aov_rays_wt_kernel" in nm for nm in names) == 2 and sum("pt_aov_rays_kernel" in nm for nm in names) == 2, names
    # template arguments <BINARY, EXACT> as the Itanium mangling spells them: quad walk only
    assert sorted(re.search(r"kernel(I\w+?EE)v", nm).group(1) for nm in names) == ["ILb0ELb0EE", "ILb0ELb0EE", "ILb0ELb1EE", "ILb0ELb1EE"], names
    for nm, v in rep.items():
        assert v["scratch"] == 0 and 0 < v["vgprs"] <= 128 and v["agprs"] == 0 and v["occupancy"] >= 4 and v["lds"] == 0, (nm, v)
    assert RC.lds_bytes_of_the_guide_kernels() == (12 + 15) * 64 * 4 and 16 * RC.lds_bytes_of_the_guide_kernels() <= 160 * 1024  # 16 waves per CU


def test_the_other_guide_targets_list_their_kernels():
    for target, count, word, wt in (("asm-aov-follow", 5, "pt_aov_follow_", 2), ("asm-aov", 5, "pt_aov_", 2), ("asm-aov-follow-batch", 3, "pt_aov_follow_batch_kernel", 0)):
        rep = resource_report.resources(target)
        names = sorted(rep)
        assert len(rep) == count and all(word in nm for nm in names) and not any("rays" in nm for nm in names), (target, names)
        assert sum("_wt_kernel" in nm for nm in names) == wt, (target, names)
        if target == "asm-aov":
            assert not any("follow" in nm for nm in names), names
        assert all(v["scratch"] == 0 and v["vgprs"] <= 128 for v in rep.values()), (target, rep)


@pytest.mark.parametrize("target", ["asm", "asm-wt", "asm-batch"])
def test_render_kernels_are_the_parents(target):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "render_kernel_resources.json")))["targets"][target]
    got = resource_report.resources(target)
    assert sorted(got) == sorted(want)
    for nm in want:
        assert got[nm] == want[nm], (nm, got[nm], want[nm])
