"""pt_trace_surface - closest hit with the surface record at the hit (include/mi355pt.h "ray queries: the surface at the hit") - without
a GPU: the CPU twin pt_debug_trace_surface_host against tests/surface_ref.py, bit for bit on the 80 bytes of every compared record.

* The three exports are in the header, in B.EXPORTS and in the library; the record is 80 bytes with its fields where the header puts
  them; the ABI version is still 5; pt_trace_surface_device is in both lists of the streams contract.
* Twin against the restatement: the zero-jitter tables of tests/surface_common.py (Cornell, the textured cube, mirror_wall, tir; centre
  rays at 20 x 13 and 64 x 48, the 24 x 16 probes) and every scene of the ray battery.
* Four mutations of the restatement (bx / by swapped, ng from the reversed cross product, the texture looked up only without emission,
  p = org + t * dir) each change a compared record on the cube or on mirror_wall - so the comparison above can tell them.
* The first 16 bytes are pt_debug_trace_rays_host's record on all rays, the per-ray tmax cases included; a miss is the 80 bytes of the
  definition in a buffer prefilled with 0xA5; pt_set_materials moves base and emission and nothing else; a mesh with a negative material
  index takes the defaults; "watertight" on the closed icosphere; pt_update_vertices equals a fresh upload.
* Every refusal of pt_trace_closest on a host-only context, plus a misaligned d_out.
* `make asm-rays-surface`: exactly 2 + 2 kernels named pt_rays_surface, 0 scratch, at most 128 VGPRs; `make asm-rays` still lists its
  4 + 4 and none named surface."""
import ctypes as C
import re

import numpy as np
import pytest

import ray_battery as rb
import resource_report
import surface_common as SC
import surface_ref
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_trace_surface", "pt_trace_surface_device", "pt_debug_trace_surface_host")
OFFSETS = dict(t=0, u=4, v=8, prim=12, p=16, material=28, ng=32, tu=44, ns=48, tv=60, base=64, emission=76)


def _host_scene(name, **opts):
    ctx = B.Context(-1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    SC.upload(ctx, SC.scene(name), B)
    return ctx


def _host_soup(tris, **opts):
    ctx = B.Context(-1)
    for k, v in opts.items():
        ctx.set_option(k, v)
    rb.upload(ctx, tris)
    return ctx


def test_exports_abi_and_record():
    L = B.lib()
    header = open(B.HEADER_PATH).read()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in B.EXPORTS
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert L.pt_abi_version() == 5 and re.search(r"#define PT_ABI_VERSION 5\b", header)
    for dt in (B.SURFACE_DTYPE, surface_ref.DTYPE):
        assert dt.itemsize == 80
        assert {k: dt.fields[k][1] for k in dt.names} == OFFSETS
        assert dt.fields["prim"][0] == np.int32 and dt.fields["material"][0] == np.int32
    struct = re.search(r"typedef struct pt_surface \{(.*?)\} pt_surface;", header, flags=re.S).group(1)
    fields = re.findall(r"(float|int32_t)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", struct, flags=re.S))
    names = [n.strip() for _, decl in fields for n in decl.split(",")]
    assert names == ["t", "u", "v", "prim", "p[3]", "material", "ng[3]", "tu", "ns[3]", "tv", "base[3]", "emission"], names
    assert "pt_trace_surface_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_trace_surface_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)


@pytest.mark.parametrize("name,kind,W,H", SC.TABLES)
def test_twin_against_restatement_on_tables(orc, name, kind, W, H):
    case = SC.table_case(orc, name, kind, W, H)
    hit = case["truth"][0]
    print("%s %s %dx%d: %d rays, %d hit" % (name, kind, W, H, hit.size, hit.sum()))
    assert hit.any() and (kind != "probes" or not hit.all()), "the table has hits, and the probes miss too"
    ctx = _host_scene(name)
    SC.assert_same(ctx.trace_surface_host(case["rec"]), case["want"], None, "%s %s %dx%d: twin vs restatement" % (name, kind, W, H))
    ctx.close()


@pytest.mark.parametrize("name", rb.scene_names())
def test_twin_against_restatement_on_battery(orc, name):
    case = SC.battery_case(orc, name)
    ctx = _host_soup(case["tris"])
    got = ctx.trace_surface_host(case["rec"])
    SC.assert_same(got, case["want"], case["mask"], "%s: twin vs restatement" % name)
    h = got["prim"] >= 0
    assert (got["material"][h] == 0).all() and (got["base"][h] == F32(0.8)).all() and (got["emission"][h] == 0).all() and (got["tu"] == 0).all() and (got["tv"] == 0).all()
    ctx.close()


@pytest.mark.parametrize("mutation", surface_ref.MUTATIONS)
def test_the_comparison_tells_each_mutation(orc, mutation):
    """Each wrong reading changes a compared record - on the cube, and for the texture rule on mirror_wall with its textured wall
    emitting (pt_set_materials), the one place where an emitter has a texture.  The twin agrees with the right reading there too."""
    name, kind, W, H = ("mirror_wall" if mutation == "texture_unless_emitting" else "cube"), "centres", 64, 48
    case = SC.table_case(orc, name, kind, W, H)
    mats = SC.emitting_wall() if name == "mirror_wall" else None
    right = surface_ref.surface(case["flat"], case["truth"], case["rays"], materials=mats)
    wrong = surface_ref.surface(case["flat"], case["truth"], case["rays"], materials=mats, mutation=mutation)
    changed = surface_ref.differ(right, wrong)
    print("%s on %s: %d of %d records change" % (mutation, name, changed.sum(), changed.size))
    assert changed.any(), "the case is too weak for " + mutation
    ctx = _host_scene(name)
    if mats is not None:
        ctx.set_materials(mats)
    got = ctx.trace_surface_host(case["rec"])
    SC.assert_same(got, right, None, "%s: twin vs the right reading" % name)
    assert surface_ref.differ(got, wrong).any()
    ctx.close()


def test_first_16_bytes_are_the_closest_hit_twins(orc):
    for name in TC.TMAX_SCENES:
        bt = TC.battery(orc, name)
        ctx = _host_soup(bt["tris"])
        for label, rec, want_hits, _, mask in [("tmax +inf", B.make_rays(bt["rays"]), bt["hits"], None, bt["mask"])] + TC.tmax_cases(orc, name):
            got = ctx.trace_surface_host(rec)
            assert TC.same(SC.first16(got), ctx.trace_rays_host(rec)).all(), "%s, %s: every ray, compared or not" % (name, label)
            TC.assert_same(SC.first16(got), want_hits, mask, "%s, %s: against the oracle" % (name, label))
        ctx.close()
    for name, kind, W, H in SC.TABLES[:3]:
        case = SC.table_case(orc, name, kind, W, H)
        ctx = _host_scene(name)
        assert TC.same(SC.first16(ctx.trace_surface_host(case["rec"])), ctx.trace_rays_host(case["rec"])).all()
        ctx.close()


def test_a_miss_is_all_80_bytes(orc):
    case = SC.table_case(orc, "mirror_wall", "probes", *SC.AR.PROBE_SIZE)
    ctx = _host_scene("mirror_wall")
    rec = case["rec"]
    out = np.full(rec.shape[0] * 80 + 80, 0xA5, np.uint8)
    assert B.lib().pt_debug_trace_surface_host(ctx._h, rec.ctypes.data_as(C.c_void_p), rec.shape[0], out.ctypes.data_as(C.c_void_p)) == rec.shape[0]
    got = out[:-80].view(B.SURFACE_DTYPE)
    miss = ~case["truth"][0]
    assert miss.any() and (got["prim"][miss] == -1).all()
    assert (got[miss].view(np.uint8).reshape(-1, 80) == SC.miss_bytes()).all(), "a miss: {+0, +0, +0, -1}, p = +0, material = -1, the rest +0"
    assert (out[-80:] == 0xA5).all(), "bytes past n * 80 are not the call's"
    SC.assert_same(got, case["want"], None, "mirror_wall probes in a prefilled buffer")
    ctx.close()


def test_set_materials_moves_base_and_emission_only(orc):
    case = SC.table_case(orc, "mirror_wall", "centres", 64, 48)
    ctx = _host_scene("mirror_wall")
    before = ctx.trace_surface_host(case["rec"])
    mats = SC.emitting_wall()
    mats[1, :3] = F32([0.125, 0.25, 0.5])  # the mirror's colour: no texture there, so base follows the row
    ctx.set_materials(mats)
    after = ctx.trace_surface_host(case["rec"])
    SC.assert_same(after, surface_ref.surface(case["flat"], case["truth"], materials=mats), None, "after pt_set_materials")
    wall, mirror = after["material"] == 0, after["material"] == 1
    assert wall.any() and mirror.any()
    assert (after["emission"][wall] == F32(SC.EMISSION)).all() and (before["emission"][wall] == 0).all()
    assert (after["base"][mirror] == F32([0.125, 0.25, 0.5])).all() and not (before["base"][mirror] == F32([0.125, 0.25, 0.5])).all()
    assert (after["base"][wall].view(np.uint32) == before["base"][wall].view(np.uint32)).all(), "the wall's base is its texel, emitting or not"
    b, a = before.copy(), after.copy()
    for r in (a, b):
        r["base"], r["emission"] = 0, 0
    assert not surface_ref.differ(a, b).any(), "everything but base and emission is unchanged"
    ctx.close()


def test_negative_material_index_gives_the_defaults(orc):
    tris = rb.make_scene("one_leaf")
    red = scene_io.material(base_color=(1.0, 0.0, 0.0), emission=3.0)
    ents = [(rb.mesh_of(tris[:1]), -1), (rb.mesh_of(tris[1:]), 0)]
    flat = scene_io.flatten_scene(ents, [("red", red, "")])
    rays = np.float32([[0.1, 0.1, 0.25, 0, 0, -1], [0.1, 0.1, 0.25, 0, 0, 1], [5, 5, 5, 0, 0, 1]])  # down onto triangle 0, up onto triangle 1, a miss
    truth = orc.Scene(flat).intersect_n(rays, use_bvh=False)
    assert truth[0].tolist() == [True, True, False] and truth[4][:2].tolist() == [0, 1]
    ctx = B.Context(-1)
    ctx.upload_scene(ents, [red])
    got = ctx.trace_surface_host(rays)
    SC.assert_same(got, surface_ref.surface(flat, truth), None, "a mesh with material_index -1")
    assert got["material"].tolist() == [-1, 0, -1] and got["emission"].tolist() == [0.0, 3.0, 0.0]
    assert (got["base"][0] == F32(0.8)).all() and got["base"][1].tolist() == [1.0, 0.0, 0.0]
    assert got["ng"][0].tolist() == [0.0, 0.0, 1.0] and got["ns"][0].tolist() == [0.0, 1.0, 0.0], "ng follows the index order, ns the vertex normals; neither is flipped towards the ray"
    ctx.close()


def test_watertight_on_the_closed_mesh(orc):
    tris, rays, mt, wt = TC.closed_case(orc)
    assert wt[0].all()
    flat = SC.battery_flat(tris)
    ctx = _host_soup(tris, watertight=1)
    got = ctx.trace_surface_host(rays)
    assert (got["prim"] >= 0).all(), "no miss from inside a closed mesh under the watertight test"
    SC.assert_same(got, surface_ref.surface(flat, wt), None, "closed mesh, watertight")
    ctx.set_option("watertight", 0)
    SC.assert_same(ctx.trace_surface_host(rays), surface_ref.surface(flat, mt), None, "closed mesh, Moeller-Trumbore")
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    rays = TC.battery(orc, "soup1")["rays"]
    ctx = _host_soup(tris, dynamic=1)
    before = ctx.trace_surface_host(rays)
    ctx.update_vertices([rb.mesh_of(moved)])
    fresh = _host_soup(moved)
    want = fresh.trace_surface_host(rays)
    assert surface_ref.differ(want, before).any(), "the deformation changes records"
    SC.assert_same(ctx.trace_surface_host(rays), want, None, "twin after pt_update_vertices vs a fresh upload")
    mask = TC.compared(moved, rays, TC.battery(orc, "soup1")["cls"])
    truth = rb.oracle_scene(orc, moved).intersect_n(rays, use_bvh=False)
    SC.assert_same(want, surface_ref.surface(SC.battery_flat(moved), truth), mask, "the moved scene vs restatement")
    ctx.close()
    fresh.close()


def test_refusals_and_error_codes():
    L = B.lib()
    vp = C.c_void_p
    rays = B.make_rays(np.float32([[0.1, 0.1, 3.0, 0, 0, -1]] * 4))
    out = np.full(4 * 20, 7, np.int32).view(B.SURFACE_DTYPE)
    r, o = rays.ctypes.data_as(vp), out.ctypes.data_as(vp)
    v16 = vp(16)
    ctx = B.Context(-1)
    hd = ctx._h
    blocking, device, twin = L.pt_trace_surface, L.pt_trace_surface_device, L.pt_debug_trace_surface_host

    def msg():
        return L.pt_last_error(hd).decode()

    # without a scene
    assert blocking(hd, r, 4, o) == PT_E_NO_SCENE and "pt_trace_surface" in msg()
    assert device(hd, v16, 4, v16, None) == PT_E_NO_SCENE and "pt_trace_surface_device" in msg()
    assert twin(hd, r, 4, o) == PT_E_NO_SCENE and "pt_debug_trace_surface_host" in msg()
    rb.upload(ctx, rb.make_scene("rects"))
    # refused by name, before anything is touched
    assert blocking(None, r, 4, o) == PT_E_INVALID
    assert blocking(hd, None, 4, o) == PT_E_INVALID and "pt_trace_surface: NULL rays" in msg()
    assert blocking(hd, r, 4, None) == PT_E_INVALID and "pt_trace_surface: NULL out" in msg()
    for n in (-1, 2 ** 31, 2 ** 40):
        assert blocking(hd, r, n, o) == PT_E_INVALID and "pt_trace_surface: n = %d" % n in msg()
    assert blocking(hd, r, 4, o) == PT_E_NO_DEVICE  # valid arguments: no CPU fallback behind the entry point
    assert blocking(hd, None, 0, None) == PT_E_NO_DEVICE  # n = 0 asks for no array, and is still a device call
    assert device(None, v16, 4, v16, None) == PT_E_INVALID
    assert device(hd, None, 4, v16, None) == PT_E_INVALID and "pt_trace_surface_device: NULL d_rays" in msg()
    assert device(hd, v16, 4, None, None) == PT_E_INVALID and "pt_trace_surface_device: NULL d_out" in msg()
    for n in (-1, 2 ** 31):
        assert device(hd, v16, n, v16, None) == PT_E_INVALID and "pt_trace_surface_device: n = %d" % n in msg()
    for bad in (vp(24), vp(4), vp(17)):
        assert device(hd, bad, 4, v16, None) == PT_E_INVALID and "pt_trace_surface_device: d_rays is not 16-byte aligned" in msg()
        assert device(hd, v16, 4, bad, None) == PT_E_INVALID and "pt_trace_surface_device: d_out is not 16-byte aligned" in msg()
    assert device(hd, v16, 4, vp(80), None) == PT_E_NO_DEVICE  # the second record of an aligned array is aligned
    assert device(hd, v16, 4, v16, None) == PT_E_NO_DEVICE
    assert device(hd, None, 0, None, None) == PT_E_NO_DEVICE
    # the twin: the same argument refusals, and it works here
    assert twin(None, r, 4, o) == PT_E_INVALID
    assert twin(hd, None, 4, o) == PT_E_INVALID and "pt_debug_trace_surface_host: NULL rays" in msg()
    assert twin(hd, r, 4, None) == PT_E_INVALID and "pt_debug_trace_surface_host: NULL out" in msg()
    assert twin(hd, r, -1, o) == PT_E_INVALID and twin(hd, r, 2 ** 31, o) == PT_E_INVALID
    assert (out.view(np.int32) == 7).all(), "a refused call wrote to the output"
    # without quad nodes: PT_E_INVALID by name, invalid arguments first; the twin walks the binary tree and goes on working
    ctx.set_option("quad", 0)
    assert blocking(hd, r, 4, o) == PT_E_INVALID and "pt_trace_surface" in msg() and "quad" in msg()
    assert blocking(hd, None, 4, o) == PT_E_INVALID and "NULL rays" in msg()
    assert device(hd, v16, 4, v16, None) == PT_E_INVALID and "pt_trace_surface_device" in msg() and "quad" in msg()
    assert (out.view(np.int32) == 7).all()
    assert twin(hd, r, 4, o) == 4 and twin(hd, None, 0, None) == 0
    assert (out["prim"] >= 0).all()
    ctx.close()


def test_surface_kernels_resources():
    """From the Makefile's own targets (the flags that ship): the two EXACT instances of each surface unit and nothing else, no scratch,
    at most 128 VGPRs (four waves per SIMD); the ray units hold what they held."""
    blocks = resource_report.report("asm-rays-surface")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 4 and len(set(names)) == 4, names
    assert all("pt_rays_surface" in nm for nm in names), names
    assert sum("pt_rays_surface_wt_kernel" in nm for nm in names) == 2 and sum("pt_rays_surface_kernel" in nm for nm in names) == 2, names
    for nm, vgprs, scratch in blocks:
        assert int(scratch) == 0 and 0 < int(vgprs) <= 128, (nm, vgprs, scratch)
    rays = [b[0] for b in resource_report.report("asm-rays")[1]]
    assert len(rays) == 8 and len(set(rays)) == 8 and not any("surface" in nm for nm in rays), rays
    assert sum("pt_rays_wt_kernel" in nm for nm in rays) == 4 and sum("pt_rays_kernel" in nm for nm in rays) == 4, rays
