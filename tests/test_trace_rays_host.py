"""Ray queries on the caller's rays (pt_trace_closest, pt_trace_occluded; include/mi355pt.h "ray queries") without a GPU.

* The six exports exist, are in B.EXPORTS and in the header, the two records are 32 and 16 bytes, the ABI version is still 5, the _device
  forms are in both lists of the streams contract and option "rays_refill" takes 0..63.
* The CPU twin pt_debug_trace_rays_host against the oracle's brute force on every scene of tests/ray_battery.py with make_rays(n = 2000):
  t, u, v bits and the id, the occlusion byte against `hit`.  Compared: classes 1-6 and class 7 up to DOMAIN_EXTENTS; left out are the
  OUTSIDE classes 8 and 9 (asserted here to be under 15 % of every battery) and the farther origins of class 7.
* Per-ray tmax: +inf, NaN, 1e10, -1, 1e-3, half the ray's oracle t, exactly its oracle t (the same hit comes back) and nextafter(t, 0)
  (that hit is gone); expectations from Scene.intersect_n / intersect(tmin = 1e-3, tmax = thi, use_bvh = False), grouped by bound.
* The watertight twin against Scene(..., watertight = True); a closed icosphere with rays aimed at its edges and vertices: occluded for
  every one under "watertight" = 1, whatever the oracle says under 0.
* After pt_update_vertices on a "dynamic" upload the twin equals a fresh upload; pt_prim_to_mesh on a two-mesh scene; every refusal and
  error code of the header on a host-only context; n = 0; `make asm-rays`: exactly the eight instances, 0 scratch, at most 128 VGPRs."""
import ctypes as C
import re

import numpy as np
import pytest

import ray_battery as rb
import resource_report
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

ROOT = rb.ROOT
F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_trace_closest", "pt_trace_closest_device", "pt_trace_occluded", "pt_trace_occluded_device", "pt_debug_trace_rays_host", "pt_prim_to_mesh")
WT_SCENES = ("cornell", "rects", "soup1", "strip")


def _host(tris, **opts):
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
    assert B.RAY_DTYPE.itemsize == 32 and B.HIT_DTYPE.itemsize == 16
    assert [B.RAY_DTYPE.fields[k][1] for k in ("org", "tmax", "dir", "unused")] == [0, 12, 16, 28]
    for name in ("pt_trace_closest_device", "pt_trace_occluded_device"):
        assert name in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
        assert name in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)
    assert '"rays_refill"' in header
    ctx = B.Context(-1)
    for v in (0, 16, 63, 32):
        ctx.set_option("rays_refill", v)
    for v in (-1, 64):
        with pytest.raises(B.PtError, match="rays_refill"):
            ctx.set_option("rays_refill", v)
    assert '"rays_grid"' in header
    for v in (5, 0):
        ctx.set_option("rays_grid", v)
    ctx.close()


@pytest.mark.parametrize("name", rb.scene_names())
def test_twin_against_brute_force(orc, name):
    bt = TC.battery(orc, name)
    rays, cls, mask = bt["rays"], bt["cls"], bt["mask"]
    outside = np.isin(cls, rb.OUTSIDE)
    print("%s: %d rays, %d compared, %d in the OUTSIDE classes (%.1f %%)" % (name, rays.shape[0], mask.sum(), outside.sum(), 100.0 * outside.mean()))
    assert outside.mean() < 0.15, "the OUTSIDE classes 8 and 9 are the only rays left out beside far origins: under 15 % of the battery"
    assert not (mask & outside).any() and set(rb.CLASSES) <= set(np.unique(cls[mask]))
    ctx = _host(bt["tris"])
    got = ctx.trace_rays_host(rays)  # tmax = +inf
    TC.assert_same(got, bt["hits"], mask, "%s: twin vs brute force" % name, rays, cls)
    occ = ctx.trace_rays_host(rays, occluded=True)
    TC.assert_same(occ, bt["occ"], mask, "%s: occluded twin vs the oracle's hit flag" % name, rays, cls)
    miss = got["prim"] < 0
    assert miss.any() and (got[miss].view(np.uint32).reshape(-1, 4)[:, :3] == 0).all(), "a miss is {+0, +0, +0, -1}"
    # the float the library does not read, and a direction that is not normalised: t is in units of |dir|
    r2 = B.make_rays(rays)
    r2["unused"] = F32(-7.0)
    assert TC.same(ctx.trace_rays_host(r2), got).all()
    ctx.close()


@pytest.mark.parametrize("name", TC.TMAX_SCENES)
def test_per_ray_tmax(orc, name):
    bt = TC.battery(orc, name)
    ctx = _host(bt["tris"])
    for label, rec, want_hits, want_occ, mask in TC.tmax_cases(orc, name):
        TC.assert_same(ctx.trace_rays_host(rec), want_hits, mask, "%s: %s" % (name, label))
        TC.assert_same(ctx.trace_rays_host(rec, occluded=True), want_occ, mask, "%s: occluded, %s" % (name, label))
    ctx.close()


@pytest.mark.parametrize("name", WT_SCENES)
def test_watertight_twin(orc, name):
    bt = TC.battery(orc, name, watertight=True)
    ctx = _host(bt["tris"], watertight=1)
    TC.assert_same(ctx.trace_rays_host(bt["rays"]), bt["hits"], bt["mask"], "%s: watertight twin vs Scene(watertight = True)" % name, bt["rays"], bt["cls"])
    TC.assert_same(ctx.trace_rays_host(bt["rays"], occluded=True), bt["occ"], bt["mask"], "%s: watertight occluded twin" % name, bt["rays"], bt["cls"])
    ctx.set_option("watertight", 0)  # switchable between calls, no new upload
    mt = TC.battery(orc, name)
    TC.assert_same(ctx.trace_rays_host(bt["rays"]), mt["hits"], mt["mask"], "%s: back to Moeller-Trumbore" % name)
    ctx.close()


def test_closed_mesh(orc):
    tris, rays, mt, wt = TC.closed_case(orc)
    assert wt[0].all(), "exact geometry: every ray from inside a closed mesh hits, and the watertight oracle agrees"
    print("Moeller-Trumbore lets %d of %d aimed rays through" % ((~mt[0]).sum(), rays.shape[0]))
    ctx = _host(tris, watertight=1)
    assert (ctx.trace_rays_host(rays, occluded=True) == 1).all()
    TC.assert_same(ctx.trace_rays_host(rays), TC.hits_of(wt), None, "closed mesh, watertight", rays)
    ctx.set_option("watertight", 0)
    TC.assert_same(ctx.trace_rays_host(rays, occluded=True), mt[0].astype(np.uint8), None, "closed mesh, Moeller-Trumbore: whatever the oracle says", rays)
    TC.assert_same(ctx.trace_rays_host(rays), TC.hits_of(mt), None, "closed mesh, Moeller-Trumbore", rays)
    ctx.close()


def test_after_update_vertices(orc):
    tris, moved = TC.moved_scene()
    rays = TC.battery(orc, "soup1")["rays"]
    ctx = _host(tris, dynamic=1)
    before = ctx.trace_rays_host(rays)
    ctx.update_vertices([rb.mesh_of(moved)])
    fresh = _host(moved)
    want = fresh.trace_rays_host(rays)
    assert not TC.same(want, before).all(), "the deformation changes hits"
    TC.assert_same(ctx.trace_rays_host(rays), want, None, "twin after pt_update_vertices vs a fresh upload", rays)
    TC.assert_same(ctx.trace_rays_host(rays, occluded=True), fresh.trace_rays_host(rays, occluded=True), None, "occluded twin after pt_update_vertices")
    ctx.close()
    fresh.close()


def test_prim_to_mesh():
    L = B.lib()
    a = rb.make_scene("one_leaf")  # triangles in the planes z = 0 and z = 0.5 over (0.1, 0.1), a third one aside
    b = np.concatenate([a + F32([0, 0, 2]), a[:2] + F32([0, 0, 4])]).astype(F32)  # the same at z = 2 / 2.5 and at z = 4 / 4.5
    na, nb = a.shape[0], b.shape[0]
    ctx = B.Context(-1)
    m, t = C.c_int32(-5), C.c_int32(-5)
    assert L.pt_prim_to_mesh(ctx._h, 0, C.byref(m), C.byref(t)) == PT_E_NO_SCENE and "pt_prim_to_mesh" in L.pt_last_error(ctx._h).decode()
    ctx.upload_scene([(rb.mesh_of(a), 0), (rb.mesh_of(b), 0)], [scene_io.MAT_DEFAULT])
    assert ctx.stats()["n_triangles"] == na + nb
    for prim, want in ((0, (0, 0)), (1, (0, 1)), (na - 1, (0, na - 1)), (na, (1, 0)), (na + 1, (1, 1)), (na + nb - 1, (1, nb - 1))):
        assert ctx.prim_to_mesh(prim) == want, prim
    for prim in (-1, na + nb, 2 ** 31 - 1, -2 ** 31):
        assert L.pt_prim_to_mesh(ctx._h, prim, C.byref(m), C.byref(t)) == PT_E_INVALID, prim
        assert "pt_prim_to_mesh" in L.pt_last_error(ctx._h).decode()
    assert (m.value, t.value) == (-5, -5), "a refused call wrote its outputs"
    assert L.pt_prim_to_mesh(ctx._h, na, None, None) == 0  # either output is optional
    assert L.pt_prim_to_mesh(None, 0, C.byref(m), C.byref(t)) == PT_E_INVALID
    # the ids the twin reports are these ids: from (0.1, 0.1, 3) down onto mesh 1's triangle 1 (z = 2.5), up onto its triangle 3 (z = 4),
    # and from z = 1 down onto mesh 0's triangle 1 (z = 0.5)
    hits = ctx.trace_rays_host(np.float32([[0.1, 0.1, 3.0, 0, 0, -1], [0.1, 0.1, 3.0, 0, 0, 1], [0.1, 0.1, 1.0, 0, 0, -1]]))
    assert [ctx.prim_to_mesh(p) for p in hits["prim"]] == [(1, 1), (1, 3), (0, 1)], hits
    assert np.allclose(hits["t"], [0.5, 1.0, 0.5], rtol=1e-6)
    ctx.close()


def test_refusals_and_error_codes():
    L = B.lib()
    vp = C.c_void_p
    rays = B.make_rays(np.float32([[0.1, 0.1, 3.0, 0, 0, -1]] * 4))
    hits = np.full(4, 7, np.int32).repeat(4).view(B.HIT_DTYPE)
    occ = np.full(4, 7, np.uint8)
    r, oh, oo = rays.ctypes.data_as(vp), hits.ctypes.data_as(vp), occ.ctypes.data_as(vp)
    v16, v24 = vp(16), vp(24)
    ctx = B.Context(-1)
    hd = ctx._h
    blocking = ((L.pt_trace_closest, "pt_trace_closest", oh), (L.pt_trace_occluded, "pt_trace_occluded", oo))
    device = ((L.pt_trace_closest_device, "pt_trace_closest_device"), (L.pt_trace_occluded_device, "pt_trace_occluded_device"))
    twin = lambda rr, n, occl, out: L.pt_debug_trace_rays_host(hd, rr, n, occl, out)

    def msg():
        return L.pt_last_error(hd).decode()

    # without a scene
    for fn, who, out in blocking:
        assert fn(hd, r, 4, out) == PT_E_NO_SCENE and who in msg()
    for fn, who in device:
        assert fn(hd, v16, 4, v16, None) == PT_E_NO_SCENE and who in msg()
    assert twin(r, 4, 0, oh) == PT_E_NO_SCENE and "pt_debug_trace_rays_host" in msg()
    rb.upload(ctx, rb.make_scene("rects"))
    # refused by name, before anything is touched
    for fn, who, out in blocking:
        assert fn(None, r, 4, out) == PT_E_INVALID
        assert fn(hd, None, 4, out) == PT_E_INVALID and who + ": NULL rays" in msg()
        assert fn(hd, r, 4, None) == PT_E_INVALID and who + ": NULL out" in msg()
        for n in (-1, 2 ** 31, 2 ** 40):
            assert fn(hd, r, n, out) == PT_E_INVALID and who + ": n = %d" % n in msg()
        assert fn(hd, r, 4, out) == PT_E_NO_DEVICE  # valid arguments: no CPU fallback behind the entry point
        assert fn(hd, None, 0, None) == PT_E_NO_DEVICE  # n = 0 asks for no array, and is still a device call
    for fn, who in device:
        assert fn(None, v16, 4, v16, None) == PT_E_INVALID
        assert fn(hd, None, 4, v16, None) == PT_E_INVALID and who + ": NULL d_rays" in msg()
        assert fn(hd, v16, 4, None, None) == PT_E_INVALID and who + ": NULL d_out" in msg()
        for n in (-1, 2 ** 31):
            assert fn(hd, v16, n, v16, None) == PT_E_INVALID and who + ": n = %d" % n in msg()
        for bad in (vp(24), vp(4), vp(17)):
            assert fn(hd, bad, 4, v16, None) == PT_E_INVALID and who + ": d_rays is not 16-byte aligned" in msg()
        assert fn(hd, v16, 4, v16, None) == PT_E_NO_DEVICE
    assert L.pt_trace_closest_device(hd, v16, 4, v24, None) == PT_E_INVALID and "pt_trace_closest_device: d_out is not 16-byte aligned" in msg()
    assert L.pt_trace_occluded_device(hd, v16, 4, vp(17), None) == PT_E_NO_DEVICE  # a byte per ray: any address
    # the twin: the same argument refusals, and it works here
    assert twin(None, 4, 0, oh) == PT_E_INVALID and "pt_debug_trace_rays_host: NULL rays" in msg()
    assert twin(r, 4, 1, None) == PT_E_INVALID and "pt_debug_trace_rays_host: NULL out" in msg()
    assert twin(r, -1, 0, oh) == PT_E_INVALID and twin(r, 2 ** 31, 0, oh) == PT_E_INVALID
    assert (hits.view(np.int32) == 7).all() and (occ == 7).all(), "a refused call wrote to the output"
    # without quad nodes: PT_E_INVALID by name, invalid arguments first; the twin walks the binary tree and goes on working.  (Option
    # "quad" = 0 stands for both causes: no scene the host builder makes here is deep enough - 3 * depth4 + 1 > 64 - to lose its quad nodes.)
    ctx.set_option("quad", 0)
    for fn, who, out in blocking:
        assert fn(hd, r, 4, out) == PT_E_INVALID and who in msg() and "quad" in msg()
        assert fn(hd, None, 4, out) == PT_E_INVALID and "NULL rays" in msg()
    for fn, who in device:
        assert fn(hd, v16, 4, v16, None) == PT_E_INVALID and who in msg() and "quad" in msg()
    assert (hits.view(np.int32) == 7).all() and (occ == 7).all()
    assert twin(r, 4, 0, oh) == 4 and twin(r, 4, 1, oo) == 4
    assert (hits["prim"] >= 0).all() and (occ == 1).all()
    ctx.close()


def test_n_zero(orc):
    ctx = _host(rb.make_scene("one_leaf"))
    none = np.zeros(0, B.RAY_DTYPE)
    assert ctx.trace_rays_host(none).shape == (0,) and ctx.trace_rays_host(none, occluded=True).shape == (0,)
    assert B.lib().pt_debug_trace_rays_host(ctx._h, None, 0, 0, None) == 0
    ctx.close()


def test_ray_kernels_resources():
    """From the Makefile's own target (the flags that ship): the four <OCCLUDED, EXACT> instances of each translation unit and nothing
    else, no scratch, at most 128 VGPRs (four waves per SIMD)."""
    blocks = resource_report.report("asm-rays")[1]
    names = [b[0] for b in blocks]
    assert len(blocks) == 8 and len(set(names)) == 8, names
    assert all("pt_rays_" in nm for nm in names), "the ray translation units hold the ray kernels and no other: %r" % (names,)
    assert sum("pt_rays_wt_kernel" in nm for nm in names) == 4 and sum("pt_rays_kernel" in nm for nm in names) == 4, names
    for nm, vgprs, scratch in blocks:
        assert int(scratch) == 0 and 0 < int(vgprs) <= 128, (nm, vgprs, scratch)
