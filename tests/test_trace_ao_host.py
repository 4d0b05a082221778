"""pt_trace_ao - fused ambient occlusion over the caller's rays (include/mi355pt.h "ray queries: ambient occlusion") - without a GPU: the
CPU twin pt_debug_trace_ao_host against tests/ao_ref.py, bit for bit on the 32 bytes of every compared record.

* The exports are in the header, in B.EXPORTS and in the library; the record is 32 bytes and the parameters 16 with their fields where
  the header puts them; the ABI version is still 5; pt_trace_ao_device is in both lists of the streams contract.
* Twin against the restatement on the six cases of tests/ao_common.py (the 64 x 48 centre tables of the cube, Cornell, mirror_wall and
  tir; the closed icosphere from outside and from inside) at n_rays 1, 4 and 16, both flag values, a radius of a quarter of the scene's
  extent and +inf, two seeds.
* The five mutations of the restatement each change a compared record on some case.
* The twin's occlusion rays, fed to pt_debug_trace_rays_host(occluded = 1), give clear for every record, compared or not; the first 16
  bytes are the closest-hit twin's on every ray; a miss and a zero normal give ao = 1, n = 0; pt_update_vertices equals a fresh upload;
  "watertight" = 1 on the icosphere.
* Every refusal, by name, on a host-only context.
* `make asm-rays-ao`: 2 + 2 kernels, no scratch, at most 128 VGPRs.

RECORDS LEFT OUT of the bit-for-bit comparison by the rule of tests/ao_ref.py (a primary or occlusion ray that grazes its closest hit
below 1e-2 rad; cap: 1 % of a case's records, 0 on the cube), observed over all settings, as the largest share of one setting (always
at K = 16; K = 1 leaves out none anywhere):
  cube 0 of 3072; cornell 5 (0.16 %); mirror_wall 1 (0.03 %); tir 7 (0.23 %); ico_out 6 of 1000 (0.60 %); ico_in 9 of 1000 (0.90 %).
The icosphere's shares are under the shading-normal flag: its vertex normals are all (0, 1, 0), so hemispheres near its equator lie
along the surface.  (test_twin_against_restatement prints the share of every setting.)"""
import ctypes as C
import re

import numpy as np
import pytest

import ao_common as AC
import ao_ref
import ray_battery as rb
import resource_report
import surface_common as SC
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_ao_default_params", "pt_trace_ao", "pt_trace_ao_device", "pt_debug_trace_ao_host")
OFFSETS = dict(t=0, u=4, v=8, prim=12, n=16, ao=28)


def _host(c, **opts):
    ctx = B.Context(-1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    c["upload"](ctx)
    return ctx


def _host_soup(tris, **opts):
    ctx = B.Context(-1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    rb.upload(ctx, tris)
    return ctx


def test_exports_abi_and_records():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    assert re.search(r"#define PT_AO_SHADING_NORMAL 1\b", header) and B.PT_AO_SHADING_NORMAL == 1 and ao_ref.SHADING_NORMAL == 1
    for dt in (B.AO_DTYPE, ao_ref.DTYPE):
        assert dt.itemsize == 32
        assert {k: dt.fields[k][1] for k in dt.names} == OFFSETS
        assert dt.fields["prim"][0] == np.int32
    assert C.sizeof(B.AoParams) == 16 and [f for f, _ in B.AoParams._fields_] == ["n_rays", "flags", "radius", "seed"]
    for struct, want in (("pt_ao_hit", ["t", "u", "v", "prim", "n[3]", "ao"]), ("pt_ao_params", ["n_rays", "flags", "radius", "seed"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
        fields = re.findall(r"(float|int32_t|uint32_t)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert [n.strip() for _, decl in fields for n in decl.split(",")] == want
    d = B.ao_default_params()
    assert (d.n_rays, d.flags, d.radius, d.seed) == (16, 0, float("inf"), 0)
    assert "pt_trace_ao_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_trace_ao_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)
    assert re.search(r"pt_trace_surface, pt_trace_ao, pt_render_rays and pt_render_aov_rays run on the context's stream", header), "the blocking list"


@pytest.mark.parametrize("seed", AC.SEEDS)
@pytest.mark.parametrize("flags", AC.FLAGS)
@pytest.mark.parametrize("name", AC.CASES)
def test_twin_against_restatement(orc, name, flags, seed):
    c = AC.case(orc, name)
    hit = c["truth"][0]
    assert hit.any()
    ctx = _host(c)
    for K in AC.KS:
        m = AC.mask(c, K, flags, seed)
        print("%s flags=%d seed=%d K=%d: %d rays, %d hit, %d left out (%.2f %%)" % (name, flags, seed, K, hit.size, hit.sum(), (~m).sum(), 100.0 * (~m).mean()))
        for which in AC.RADII:
            got = ctx.trace_ao_host(c["rec"], AC.params(c, K, flags, which, seed))
            AC.assert_same(got, AC.want(c, K, flags, which, seed), m, "%s K=%d flags=%d radius=%s seed=%d: twin vs restatement" % (name, K, flags, which, seed))
    ctx.close()


def test_the_settings_matter(orc):
    """The two radii, the two seeds and the three K give different records somewhere: the comparison above is not of constants."""
    c = AC.case(orc, "cornell")
    a = AC.want(c, 16, 0, "inf", AC.SEEDS[0])
    assert ao_ref.differ(a, AC.want(c, 16, 0, "quarter", AC.SEEDS[0])).any()
    assert ao_ref.differ(a, AC.want(c, 16, 0, "inf", AC.SEEDS[1])).any()
    assert ao_ref.differ(a, AC.want(c, 4, 0, "inf", AC.SEEDS[0])).any()
    assert len(np.unique(a["ao"])) > 4
    m = AC.case(orc, "mirror_wall")
    assert ao_ref.differ(AC.want(m, 16, 0, "inf", AC.SEEDS[0]), AC.want(m, 16, 1, "inf", AC.SEEDS[0])).any(), "the flag: ns is not ng on some mesh"


@pytest.mark.parametrize("mutation", ao_ref.MUTATIONS)
def test_the_comparison_tells_each_mutation(orc, mutation):
    """Each wrong reading changes a compared record: the facing flip seen from inside the icosphere, whose normals point outwards;
    the rest on Cornell.  The twin agrees with the right reading and not with the wrong one."""
    name = "ico_in" if mutation == "no_facing_flip" else "cornell"
    K, flags, which, seed = 4, 0, "quarter", AC.SEEDS[1]
    c = AC.case(orc, name)
    right, m = AC.want(c, K, flags, which, seed), AC.mask(c, K, flags, seed)
    wrong = ao_ref.ao(c["S"], c["flat"], c["rays"], c["truth"], K, flags, AC.radius_of(c, which), seed, mutation=mutation)
    changed = ao_ref.differ(right, wrong) & m
    print("%s on %s: %d of %d compared records change" % (mutation, name, changed.sum(), m.sum()))
    assert changed.any(), "the case is too weak for " + mutation
    ctx = _host(c)
    got = ctx.trace_ao_host(c["rec"], AC.params(c, K, flags, which, seed))
    AC.assert_same(got, right, m, "%s: twin vs the right reading" % name)
    assert (ao_ref.differ(got, wrong) & m).any()
    ctx.close()


@pytest.mark.parametrize("name", ("cornell", "tir", "ico_in"))
def test_occlusion_rays_give_clear_through_the_occlusion_twin(orc, name):
    c = AC.case(orc, name)
    ctx = _host(c)
    for K, flags, which in ((1, 0, "inf"), (5, 1, "quarter"), (16, 0, "quarter")):
        prm = AC.params(c, K, flags, which, 7)
        got, ao_rays = ctx.trace_ao_host(c["rec"], prm, return_rays=True)
        assert ao_rays.shape == (got.shape[0], K) and ao_rays.dtype == B.RAY_DTYPE
        occ = ctx.trace_rays_host(ao_rays.reshape(-1), occluded=True).reshape(-1, K)
        assert ((occ == 0).sum(1) == AC.clear_of(got, K)).all(), "every record, compared or not"
        traced = (got["prim"] >= 0) & (got["n"] != 0).any(1)
        assert (ao_rays["tmax"][traced] == AC.radius_of(c, which) if which != "inf" else ao_rays["tmax"][traced] == F32(1e10)).all()
        assert (ao_rays["tmax"][~traced] == 0).all() and (got["ao"][~traced] == 1).all()
        assert ao_ref.differ(got, ctx.trace_ao_host(c["rec"], prm)).sum() == 0, "the rays are an extra output"
    ctx.close()


@pytest.mark.parametrize("name", AC.CASES)
def test_first_16_bytes_are_the_closest_hit_twins(orc, name):
    c = AC.case(orc, name)
    ctx = _host(c)
    want = ctx.trace_rays_host(c["rec"])
    for K, flags in ((1, 0), (4, 1)):
        got = ctx.trace_ao_host(c["rec"], B.ao_default_params(n_rays=K, flags=flags, seed=3))
        assert TC.same(AC.first16(got), want).all(), "%s: every ray" % name
    ctx.close()
    if name == "cornell":  # the ray's own bound: pt_trace_closest's thi
        bt = TC.battery(orc, "cornell")
        ctx = _host_soup(bt["tris"])
        for label, rec, _, _, _ in TC.tmax_cases(orc, "cornell"):
            got = ctx.trace_ao_host(rec, B.ao_default_params(n_rays=1))
            assert TC.same(AC.first16(got), ctx.trace_rays_host(rec)).all(), label
        ctx.close()


def test_a_miss_and_a_zero_normal(orc):
    tris = rb.make_scene("one_leaf")
    mesh = rb.mesh_of(tris)
    mesh["normals"] = np.zeros_like(mesh["normals"])
    ctx = B.Context(-1)
    ctx.upload_scene([(mesh, 0)], [scene_io.MAT_DEFAULT])
    rays = np.float32([[0.1, 0.1, 0.25, 0, 0, -1], [0.1, 0.1, 0.25, 0, 0, 1], [5, 5, 5, 0, 0, 1]])  # down onto triangle 0, up onto triangle 1, a miss
    rec = B.make_rays(rays)
    out = np.full(3 * 32 + 32, 0xA5, np.uint8)
    prm = B.ao_default_params(n_rays=8, flags=B.PT_AO_SHADING_NORMAL)
    assert B.lib().pt_debug_trace_ao_host(ctx._h, rec.ctypes.data_as(C.c_void_p), 3, C.byref(prm), out.ctypes.data_as(C.c_void_p), None) == 3
    got = out[:-32].view(B.AO_DTYPE)
    assert (out[-32:] == 0xA5).all(), "bytes past n * 32 are not the call's"
    assert got["prim"].tolist() == [0, 1, -1]
    assert (got.view(np.uint32).reshape(3, 8)[:, 4:7] == 0).all(), "n = +0: nothing to face"
    assert (got["ao"] == 1).all()
    assert (got[2:].view(np.uint32) == np.uint32([0, 0, 0, 0xFFFFFFFF, 0, 0, 0, 0x3F800000])).all(), "a miss: {+0, +0, +0, -1}, {+0, +0, +0, 1.0f}"
    assert TC.same(AC.first16(got), ctx.trace_rays_host(rec)).all()
    # about the geometric normal the same rays see each other's triangle: ray 0 looks down from between the two and its hemisphere
    # looks up at triangle 1
    geo = ctx.trace_ao_host(rec, B.ao_default_params(n_rays=64))
    assert geo["n"][0].tolist() == [0, 0, 1] and geo["n"][1].tolist() == [0, 0, -1] and geo["ao"][0] < 1 and geo["ao"][1] < 1 and geo["ao"][2] == 1
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    rays = TC.battery(orc, "soup1")["rays"][:1500]
    prm = B.ao_default_params(n_rays=4, seed=11)
    ctx = _host_soup(tris, dynamic=1)
    before = ctx.trace_ao_host(rays, prm)
    ctx.update_vertices([rb.mesh_of(moved)])
    fresh = _host_soup(moved)
    want = fresh.trace_ao_host(rays, prm)
    assert ao_ref.differ(want, before).any(), "the deformation changes records"
    AC.assert_same(ctx.trace_ao_host(rays, prm), want, None, "twin after pt_update_vertices vs a fresh upload")
    ctx.close()
    fresh.close()


def test_watertight_on_the_icosphere(orc):
    for name in AC.ICO:
        c = AC.case(orc, name, watertight=True)
        if name == "ico_in":
            assert c["truth"][0].all(), "no miss from inside a closed mesh under the watertight test"
        ctx = _host(c, watertight=1)
        for K, flags, which in ((4, 0, "inf"), (4, 1, "quarter")):
            got = ctx.trace_ao_host(c["rec"], AC.params(c, K, flags, which, 5))
            w = ao_ref.ao(c["S"], c["flat"], c["rays"], c["truth"], K, flags, AC.radius_of(c, which), 5)
            m = ao_ref.compared(c["S"], c["flat"], c["rays"], c["truth"], ao_ref.prepare(c["S"], c["flat"], c["rays"], c["truth"], flags, 5, K), K)
            assert (~m).sum() <= AC.MAX_LEFT_OUT * m.size
            AC.assert_same(got, w, m, "%s, watertight, K=%d flags=%d radius=%s" % (name, K, flags, which))
        ctx.close()


def test_refusals_and_error_codes():
    L = B.lib()
    vp = C.c_void_p
    rays = B.make_rays(np.float32([[0.1, 0.1, 3.0, 0, 0, -1]] * 4))
    out = np.full(4 * 8, 7, np.int32).view(B.AO_DTYPE)
    r, o = rays.ctypes.data_as(vp), out.ctypes.data_as(vp)
    v16 = vp(16)
    ctx = B.Context(-1)
    hd = ctx._h
    blocking, device, twin = L.pt_trace_ao, L.pt_trace_ao_device, L.pt_debug_trace_ao_host
    ok = B.ao_default_params(n_rays=2)

    def msg():
        return L.pt_last_error(hd).decode()

    # without a scene
    assert blocking(hd, r, 4, None, o) == PT_E_NO_SCENE and "pt_trace_ao" in msg()
    assert device(hd, v16, 4, None, v16, None) == PT_E_NO_SCENE and "pt_trace_ao_device" in msg()
    assert twin(hd, r, 4, None, o, None) == PT_E_NO_SCENE and "pt_debug_trace_ao_host" in msg()
    rb.upload(ctx, rb.make_scene("rects"))
    # pt_trace_closest's refusals, by name, before anything is touched
    assert blocking(None, r, 4, None, o) == PT_E_INVALID
    assert blocking(hd, None, 4, None, o) == PT_E_INVALID and "pt_trace_ao: NULL rays" in msg()
    assert blocking(hd, r, 4, None, None) == PT_E_INVALID and "pt_trace_ao: NULL out" in msg()
    for n in (-1, 2 ** 31, 2 ** 40):
        assert blocking(hd, r, n, None, o) == PT_E_INVALID and "pt_trace_ao: n = %d" % n in msg()
    assert blocking(hd, r, 4, None, o) == PT_E_NO_DEVICE  # valid arguments, NULL parameters: no CPU fallback behind the entry point
    assert blocking(hd, r, 4, C.byref(ok), o) == PT_E_NO_DEVICE
    assert blocking(hd, None, 0, None, None) == PT_E_NO_DEVICE  # n = 0 asks for no array, and is still a device call
    assert device(None, v16, 4, None, v16, None) == PT_E_INVALID
    assert device(hd, None, 4, None, v16, None) == PT_E_INVALID and "pt_trace_ao_device: NULL d_rays" in msg()
    assert device(hd, v16, 4, None, None, None) == PT_E_INVALID and "pt_trace_ao_device: NULL d_out" in msg()
    for n in (-1, 2 ** 31):
        assert device(hd, v16, n, None, v16, None) == PT_E_INVALID and "pt_trace_ao_device: n = %d" % n in msg()
    for bad in (vp(24), vp(4), vp(17)):
        assert device(hd, bad, 4, None, v16, None) == PT_E_INVALID and "pt_trace_ao_device: d_rays is not 16-byte aligned" in msg()
        assert device(hd, v16, 4, None, bad, None) == PT_E_INVALID and "pt_trace_ao_device: d_out is not 16-byte aligned" in msg()
    assert device(hd, v16, 4, None, vp(32), None) == PT_E_NO_DEVICE  # the second record of an aligned array is aligned
    assert device(hd, v16, 4, C.byref(ok), v16, None) == PT_E_NO_DEVICE
    assert device(hd, None, 0, None, None, None) == PT_E_NO_DEVICE
    # the parameters, by name, for the three forms alike
    bad_params = [(dict(n_rays=0), "n_rays 0 outside 1..4096"), (dict(n_rays=-3), "n_rays -3"), (dict(n_rays=4097), "n_rays 4097"), (dict(flags=2), "unknown flags 0x2"),
                  (dict(flags=-2147483648), "unknown flags"), (dict(flags=3), "unknown flags 0x3"), (dict(radius=0.0), "radius 0 must be > 0"),
                  (dict(radius=-1.0), "radius -1"), (dict(radius=float("nan")), "radius nan"), (dict(radius=float("-inf")), "radius -inf")]
    for changes, text in bad_params:
        p = B.ao_default_params(**changes)
        assert blocking(hd, r, 4, C.byref(p), o) == PT_E_INVALID and "pt_trace_ao: " + text in msg(), (changes, msg())
        assert device(hd, v16, 4, C.byref(p), v16, None) == PT_E_INVALID and "pt_trace_ao_device: " + text in msg(), (changes, msg())
        assert twin(hd, r, 4, C.byref(p), o, None) == PT_E_INVALID and "pt_debug_trace_ao_host: " + text in msg(), (changes, msg())
    for good in (dict(n_rays=1), dict(n_rays=4096), dict(flags=1), dict(radius=1e-30), dict(radius=float("inf")), dict(seed=0xFFFFFFFF)):
        assert blocking(hd, r, 4, C.byref(B.ao_default_params(**good)), o) == PT_E_NO_DEVICE, good
    # the twin: the same argument refusals, and it works here
    assert twin(None, r, 4, None, o, None) == PT_E_INVALID
    assert twin(hd, None, 4, None, o, None) == PT_E_INVALID and "pt_debug_trace_ao_host: NULL rays" in msg()
    assert twin(hd, r, 4, None, None, None) == PT_E_INVALID and "pt_debug_trace_ao_host: NULL out" in msg()
    assert twin(hd, r, -1, None, o, None) == PT_E_INVALID and twin(hd, r, 2 ** 31, None, o, None) == PT_E_INVALID
    assert (out.view(np.int32) == 7).all(), "a refused call wrote to the output"
    # without quad nodes: PT_E_INVALID by name, invalid arguments first; the twin walks the binary tree and goes on working
    ctx.set_option("quad", 0)
    assert blocking(hd, r, 4, None, o) == PT_E_INVALID and "pt_trace_ao" in msg() and "quad" in msg()
    assert blocking(hd, None, 4, None, o) == PT_E_INVALID and "NULL rays" in msg()
    assert device(hd, v16, 4, None, v16, None) == PT_E_INVALID and "pt_trace_ao_device" in msg() and "quad" in msg()
    assert (out.view(np.int32) == 7).all()
    assert twin(hd, r, 4, C.byref(ok), o, None) == 4 and twin(hd, None, 0, None, None, None) == 0
    assert (out["prim"] >= 0).all()
    ctx.close()


def test_ao_kernels_resources():
    """From the Makefile's own target (the flags that ship): the two EXACT instances of each unit and nothing else, no scratch, at most
    128 VGPRs (four waves per SIMD); the ray units hold what they held."""
    blocks = resource_report.report("asm-rays-ao")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 4 and len(set(names)) == 4, names
    assert sum("pt_rays_ao_wt_kernel" in nm for nm in names) == 2 and sum("pt_rays_ao_kernel" in nm for nm in names) == 2, names
    for nm, vgprs, scratch in blocks:
        assert int(scratch) == 0 and 0 < int(vgprs) <= 128, (nm, vgprs, scratch)
    rays = [b[0] for b in resource_report.report("asm-rays")[1]]
    assert len(rays) == 8 and not any("_ao" in nm for nm in rays), rays
    surf = [b[0] for b in resource_report.report("asm-rays-surface")[1]]
    assert len(surf) == 4 and not any("_ao" in nm for nm in surf), surf
