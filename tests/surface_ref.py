"""The surface record of pt_trace_surface (include/mi355pt.h "ray queries: the surface at the hit") restated in numpy from the ORIGINAL
flat scene (scene_io.flatten_scene: positions, normals, texcoords, material and texture indices, material table, textures) and the
oracle's brute-force closest hit (hit, t, u, v, prim).  It builds on tests/aov_ref.py's fma32, interp3 and normalize3 and on
orc.tex_nearest; cross is restated from csrc/pt_device.h.  Nothing here reads the library under test.

MUTATIONS are the wrong readings of the definition that tests/test_trace_surface_host.py shows to change a compared record."""
import numpy as np

import aov_ref
import oracle as orc

F32 = np.float32
fma32, interp3, normalize3 = aov_ref.fma32, aov_ref.interp3, aov_ref.normalize3
MUTATIONS = ("swap_bx_by", "ng_reversed", "texture_unless_emitting", "p_from_ray")
DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("p", "<f4", (3,)), ("material", "<i4"), ("ng", "<f4", (3,)), ("tu", "<f4"),
                  ("ns", "<f4", (3,)), ("tv", "<f4"), ("base", "<f4", (3,)), ("emission", "<f4")])
assert DTYPE.itemsize == 80


def cross3(a, b):
    """pt_device.h cross: (fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)))"""
    return np.stack([fma32(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), fma32(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])),
                     fma32(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], -1).astype(F32)


def unit3(a):
    """normalize, or (0, 0, 0) where a component of that is not finite"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = normalize3(np.asarray(a, F32))
    return np.where(np.isfinite(n).all(-1, keepdims=True), n, F32(0.0)).astype(F32)


def surface(flat, truth, rays=None, materials=None, mutation=None):
    """truth: (hit, t, u, v, prim) of oracle.Scene.intersect_n(..., use_bvh=False) -> (n,) DTYPE records.  materials: the current table if
    not flat's (pt_set_materials); rays: (n, 6) origins and directions, needed by the mutation p_from_ray only."""
    assert mutation is None or mutation in MUTATIONS
    hit, t, u, v, prim = (np.asarray(a) for a in truth)
    out = np.zeros(hit.shape[0], DTYPE)  # a miss: {+0, +0, +0, -1}, p = +0, material = -1, every remaining word +0
    out["prim"], out["material"] = -1, -1
    if not hit.any():
        return out
    p = prim[hit]
    hu, hv = u[hit].astype(F32), v[hit].astype(F32)
    bx, by = (hv, hu) if mutation == "swap_bx_by" else (hu, hv)
    bw = F32(1.0) - bx - by
    pos = np.asarray(flat["positions"], F32).reshape(-1, 3, 3)[p]
    nrm = np.asarray(flat["normals"], F32).reshape(-1, 3, 3)[p]
    tc = np.zeros((p.size, 3, 2), F32) if flat["texcoords"] is None else np.asarray(flat["texcoords"], F32).reshape(-1, 3, 2)[p]
    h = np.zeros(p.size, DTYPE)
    h["t"], h["u"], h["v"], h["prim"] = t[hit], hu, hv, p
    h["p"] = interp3(bw, bx, by, pos[:, 0], pos[:, 1], pos[:, 2])
    if mutation == "p_from_ray":
        r = np.asarray(rays, F32)[hit]
        h["p"] = r[:, :3] + t[hit].astype(F32)[:, None] * r[:, 3:]
    h["ns"] = unit3(interp3(bw, bx, by, nrm[:, 0], nrm[:, 1], nrm[:, 2]))
    e1, e2 = pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]
    h["ng"] = unit3(cross3(e2, e1) if mutation == "ng_reversed" else cross3(e1, e2))
    h["tu"] = fma32(by, tc[:, 2, 0], fma32(bx, tc[:, 1, 0], bw * tc[:, 0, 0]))
    h["tv"] = fma32(by, tc[:, 2, 1], fma32(bx, tc[:, 1, 1], bw * tc[:, 0, 1]))
    mats = np.asarray(flat["materials"] if materials is None else materials, F32).reshape(-1, orc.MAT_FLOATS)
    mi = np.asarray(flat["material_index"], np.int32)[p]
    h["material"] = mi
    m = np.where((mi >= 0)[:, None], mats[np.maximum(mi, 0)], aov_ref.MAT_DEFAULT[None, :]).astype(F32)
    base = m[:, :3].copy()
    ti = np.where(mi >= 0, np.asarray(flat["texture_index"], np.int32)[p], -1)
    look = ti >= 0
    if mutation == "texture_unless_emitting":
        look = look & ~(m[:, 16] > 0)
    for i in np.nonzero(look)[0]:
        base[i] = orc.tex_nearest(flat["textures"][int(ti[i])], float(h["tu"][i]), float(h["tv"][i]))
    h["base"], h["emission"] = base, m[:, 16]
    out[hit] = h
    return out


def differ(a, b):
    """Per record: any of the 80 bytes differs."""
    return (a.view(np.uint8).reshape(a.shape[0], -1) != b.view(np.uint8).reshape(b.shape[0], -1)).any(1)
