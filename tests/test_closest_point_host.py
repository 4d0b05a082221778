"""pt_closest_point (include/mi355pt.h "point queries: the nearest surface") without a GPU.

* The three exports exist, are in B.EXPORTS and in the header; the records are 16 and 32 bytes with the header's offsets; the ABI version
  is still 5; pt_closest_point_device is in both lists of the streams contract.
* The restatement (tests/closest_point_ref.py): its vectorised form against its plain per-point, per-triangle loop; each of its five
  named wrong variants changes a record on a case made for it.
* The CPU twin pt_debug_closest_point_host against the restatement, bit for bit on all 32 bytes of EVERY record, on Cornell, the
  textured cube, the closed icosphere from outside and inside and every scene of tests/ray_battery.py (none is left out: all satisfy
  the premise), with the point sets of tests/closest_point_common.py; a mesh uploaded twice (every record a tie: the lower id wins); a
  scene of needles (slivers are never reported); radii +inf, NaN, negative, exactly the distance and one float below it, too small.
* THE PREMISE of the pruning argument, for the winner of every point and for every triangle on a subsample, also out to 10 extents.
* AN OUTSIDE WITNESS in float64 (test_float64_witness: the bound is derived there).
* After pt_update_vertices the twin equals a fresh upload's; every refusal and error code on a host-only context; n = 0; `make
  asm-points`: one kernel, 0 scratch, at most 128 VGPRs."""
import ctypes as C
import re

import numpy as np
import pytest

import closest_point_common as PC
import closest_point_ref as R
import ray_battery as rb
import resource_report
from owl_path_tracer_amd.pyhost import binding as B

F32 = np.float32
PT_E_INVALID, PT_E_NO_DEVICE, PT_E_NO_SCENE = -1, -2, -4
NAMES = ("pt_closest_point", "pt_closest_point_device", "pt_debug_closest_point_host")
U = 2.0 ** -24  # unit roundoff of float32


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
    assert B.POINT_DTYPE.itemsize == 16 and B.POINT_HIT_DTYPE.itemsize == 32
    assert B.POINT_DTYPE == R.POINT_DTYPE and B.POINT_HIT_DTYPE == R.POINT_HIT_DTYPE
    assert [B.POINT_DTYPE.fields[k][1] for k in ("p", "radius")] == [0, 12]
    assert [B.POINT_HIT_DTYPE.fields[k][1] for k in ("dist", "u", "v", "prim", "q", "feature")] == [0, 4, 8, 12, 16, 28]
    assert re.search(r"typedef struct pt_point\s*\{ float p\[3\]; float radius; \} pt_point;", header)
    assert re.search(r"typedef struct pt_point_hit \{ float dist, u, v; int32_t prim; float q\[3\]; int32_t feature; \} pt_point_hit;", header)
    assert "pt_closest_point_device" in re.search(r"The asynchronous calls \(([^)]*)\)", header).group(1)
    assert "pt_closest_point_device" in re.search(r"Waits on the host for the context's last asynchronous call - (.*?) - and for the context's own stream", header, flags=re.S).group(1)
    for word in ("a sign (inside or outside)", "the k nearest triangles", "PREMISE"):
        assert word in header


# ---------------------------------------------------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------------------------------------------------
def test_vectorised_restatement_equals_the_plain_loop():
    for name, n in (("one_leaf", 60), ("cube", 40), ("soup1", 60), ("soup3", 12)):
        c = PC.case(name)
        pts = c["ref"][:: max(1, c["ref"].shape[0] // n)][:n]
        PC.assert_same(R.closest(c["T"], pts), R.closest_loop(c["T"], pts), name + ": vectorised vs loop")
    tris, pts = _radius_case()
    PC.assert_same(R.closest(tris, pts), R.closest_loop(tris, pts), "radii: vectorised vs loop")


def _variant_cases():
    """{variant: (triangles, points)} on which the variant changes a record."""
    tri = F32([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]])
    twice = np.concatenate([tri, tri])
    above = B.make_points(F32([[0.25, 0.25, 0.5]]), 0.5)  # dd = 0.25 = r2 exactly
    # a thin triangle (height 2.9e-5 over an edge of 2: no sliver) and a point 3.3e-5 above its apex p2: d2 and d4 lose the apex's height
    # to rounding, vc <= 0 comes out, and step 3 (edge p0p1) holds as well as step 4 (vertex p2) - found by a seeded search
    thin = F32([[[0, 0, 0], [2, 0, 0], [0.41901076, 2.9193341e-05, 0]]])
    return {"ties_to_higher_id": (twice, B.make_points(F32([[0.25, 0.25, 0.5]]))), "le_without_id": (twice, B.make_points(F32([[2.0, -1.0, 0.3]]))),
            "step4_before_step3": (thin, B.make_points(F32([[0.41901076, 6.265153e-05, 0]]))), "uv_exchanged": (tri, B.make_points(F32([[0.6, 0.1, 0.5], [0.7, -1.0, 0.0]]))),
            "r2_strict": (tri, above)}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_wrong_variant_changes_a_record(variant):
    tris, pts = _variant_cases()[variant]
    T = R.triangles(tris)
    assert not R.collapsed(T).any()
    right = R.closest(T, pts)
    assert (right["prim"] >= 0).all()
    for form in (R.closest, R.closest_loop):
        wrong = form(T, pts, variant=variant)
        assert R.differ(wrong, right).any(), "%s (%s) changes nothing" % (variant, form.__name__)
    # ... and the twin sides with the definition
    ctx = _host(tris)
    PC.assert_same(ctx.closest_point_host(pts), right, variant + ": the twin on the variant's case")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the twin against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.SCENES)
def test_twin_against_the_restatement_and_the_premise(name):
    c = PC.case(name)
    ctx = _host(c["tris"])
    got = ctx.closest_point_host(c["ref"])
    PC.assert_same(got, PC.want(name), name + ": twin vs restatement")
    assert (got["prim"] >= 0).all(), "radius = +inf: every point finds a triangle"
    feats = np.bincount(got["feature"], minlength=7)
    print("%s: %d triangles, %d points, features face/p0/p1/p2/e01/e12/e02 = %s" % (name, c["T"].shape[0], got.shape[0], feats))
    assert name in ("ico_in",) or (feats[1:4].sum() > 0 and feats[4:].sum() > 0), "vertex and edge winners occur"
    assert not R.collapsed(c["T"])[got["prim"]].any(), "a collapsed triangle is never reported"
    pairs, real = PC.premise(ctx, c, c["ref"], got)
    # the same out to 10 extents, the edge of the stated domain
    P = c["tris"].reshape(-1, 3).astype(np.float64)
    far = B.make_points((P.min(0) - 10.0 * c["extent"] + np.random.default_rng(3).random((64, 3)) * (np.ptp(P, axis=0) + 20.0 * c["extent"])).astype(F32))
    far_pairs, _ = PC.premise(ctx, c, far, ctx.closest_point_host(far), n_all=8)
    print("%s: premise held on %d pairs (%s)" % (name, pairs + far_pairs, "quad tree" if real else "the root is a leaf: no box is tested"))
    assert real == (name not in ("one_leaf", "soup1"))
    ctx.close()


def test_closed_mesh_vertex_regions_are_exact_ties():
    """A vertex of the icosphere pushed outwards: every incident triangle reports the vertex itself, the same q and the same dd, and the
    lowest id among them wins."""
    c = PC.case("ico_out")
    T = c["T"]
    k = np.random.default_rng(5).integers(0, T.shape[0], 200)
    v = T[k, 0]
    x = (v.astype(np.float64) * 1.5).astype(F32)  # the sphere is centred on the origin
    ctx = _host(c["tris"])
    got = ctx.closest_point_host(B.make_points(x))
    PC.assert_same(got, R.closest(T, B.make_points(x)), "vertex regions: twin vs restatement")
    assert (got["feature"] >= 1).all() and (got["feature"] <= 3).all() and (got["q"] == v).all()
    incident = (T[None, :, :, :] == v[:, None, None, :]).all(3).any(2)  # (points, triangles)
    assert (incident.sum(1) >= 5).all()
    assert (got["prim"] == incident.argmax(1)).all(), "ties go to the lowest id among the incident triangles"
    ctx.close()


def test_mesh_uploaded_twice_the_lower_id_wins():
    tris = rb.make_closed_mesh("ico320")[0]
    n = tris.shape[0]
    ctx = B.Context(-1)
    from owl_path_tracer_amd.pyhost import scene_io

    ctx.upload_scene([(rb.mesh_of(tris), 0), (rb.mesh_of(tris), 0)], [scene_io.MAT_DEFAULT])
    pts = B.make_points(PC.points_of("twice", tris, 500, 11))
    got = ctx.closest_point_host(pts)
    PC.assert_same(got, R.closest(R.triangles(np.concatenate([tris, tris])), pts), "uploaded twice: twin vs restatement")
    assert (got["prim"] >= 0).all() and (got["prim"] < n).all(), "every record is a tie between id and id + n: the lower one wins"
    one = _host(tris)
    PC.assert_same(got, one.closest_point_host(pts), "uploaded twice vs once")
    one.close()
    ctx.close()


def test_slivers_are_never_reported():
    tris, x = PC.needle_scene()
    T = R.triangles(tris)
    assert R.collapsed(T).sum() == 50
    pts = B.make_points(x[:400])
    ctx = _host(tris)
    got = ctx.closest_point_host(pts)
    PC.assert_same(got, R.closest(T, pts), "needles: twin vs restatement")
    assert (got["prim"] >= 50).all() and (got["dist"] >= 3.0).all(), "the quad below is the nearest surface: the needles are not there"
    assert PC.premise(ctx, dict(name="needles", T=T), pts, got)[1]
    ctx.close()
    only = _host(tris[:50])  # nothing but slivers: nothing is found
    got = only.closest_point_host(pts)
    assert (got["prim"] == -1).all() and not got.view(np.uint32).reshape(-1, 8)[:, [0, 1, 2, 4, 5, 6, 7]].any()
    only.close()


def _radius_case():
    """The plane z = 0 (one large triangle) and points at distance exactly 0.5 above it, with every kind of radius."""
    tris = F32([[[-4, -4, 0], [4, -4, 0], [0, 6, 0]]])
    half, below = F32(0.5), np.nextafter(F32(0.5), F32(0))
    radii = F32([np.inf, np.nan, 1e10, 3e38, 0.5, below, -1.0, -np.inf, -0.0, 0.0, 1e-3, 0.49, 0.51])
    x = np.tile(F32([0.25, 0.5, 0.5]), (radii.size, 1))
    return tris, B.make_points(x, radii)


def test_radii():
    tris, pts = _radius_case()
    ctx = _host(tris)
    got = ctx.closest_point_host(pts)
    PC.assert_same(got, R.closest(R.triangles(tris), pts), "radii: twin vs restatement")
    found = got["prim"] == 0
    assert found.tolist() == [True, True, True, True, True, False, False, False, False, False, False, False, True], got
    assert (got["dist"][found] == F32(0.5)).all() and (got["feature"][found] == 0).all()
    assert not got[~found].view(np.uint32).reshape(-1, 8)[:, [0, 1, 2, 4, 5, 6, 7]].any(), "nothing found: prim = -1 and every other word +0"
    # radius 0 finds a point ON the surface (dd = 0 = r2), and -0.0 is not negative
    on = B.make_points(F32([[0.25, 0.5, 0.0]] * 2), F32([0.0, -0.0]))
    got = ctx.closest_point_host(on)
    assert (got["prim"] == 0).all() and (got["dist"] == 0).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the float64 witness
# ---------------------------------------------------------------------------------------------------------------------
def _closest64(T, x):
    """Float64 closest points of every triangle (n_t, 3, 3) to every point (n_p, 3): (squared distance (n_p, n_t))."""
    p0, p1, p2 = (T[None, :, k, :].astype(np.float64) for k in range(3))
    x = x[:, None, :].astype(np.float64)
    dot = lambda a, b: (a * b).sum(-1)
    ab, ac, ap, bp, cp = p1 - p0, p2 - p0, x - p0, x - p1, x - p2
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        s3, s5, s6 = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        k = 1.0 / (va + vb + vc)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        shape = np.broadcast_shapes(ap.shape)
        q = np.select([c[..., None] for c in conds], [np.broadcast_to(p0, shape), np.broadcast_to(p1, shape), p0 + ab * s3[..., None], np.broadcast_to(p2, shape), p0 + ac * s5[..., None],
                                                     p1 + (p2 - p1) * s6[..., None]], p0 + ab * (vb * k)[..., None] + ac * (vc * k)[..., None])
    return dot(x - q, x - q)


@pytest.mark.parametrize("name", ("cornell", "cube", "ico_out", "ico_in", "rects", "soup2", "strip", "dragon"))
def test_float64_witness(name):
    """The reported dist against the float64 minimum distance d* over all triangles, per point x with nearest triangle T*.
    THE BOUND, with u = 2^-24, E = the scene's measure, X = the largest |coordinate| of x, L / l / A the longest edge, shortest edge and
    area of T*, D = d* + L (no vertex of T* is farther from x):
      rounding  q has at most 4 roundings of coordinates <= E per component, e = x - q one of a value <= X + E, so |e| is off by at
                most sqrt(3) u (X + 5 E); dot(e, e) has 3 roundings and sqrt_ one, each relative u on the distance:
                    a = u (sqrt(3) (X + 5 E) + 4 dist).
      placement q is a point ON the triangle (a vertex, p + e s with 0 <= s <= 1, or a convex combination), so it cannot be nearer than
                d* by more than the rounding above; it can be farther by its displacement along the triangle.  Each d_k is a dot
                product of 3 roundings with |d_k| <= L D: off by 3 u L D.  An edge parameter s = d / (d - d') has the exact divisor
                |edge|^2 >= l^2: off by (3 + 6 + 1) u L D / l^2 + u, a displacement of at most b_edge = 10 u L D / l + u L.  A face
                weight is a difference of two products of two d's, off by 2 (3 + 3 + 1) u + 2 u = 16 u (L D)^2, over the sum S = 4 A^2
                of three of them, off by 3 * 16 u + 2 * 6 u = 60 u (L D)^2; v and w are each off by (16 + 60) u (L D)^2 / S + 2 u, a
                displacement of at most b_face = 152 u L^3 D^2 / (4 A^2) + 4 u L.  A step chosen wrongly under rounding is chosen
                within these errors of the boundary between two regions, where the two formulas agree to the same order:
                    b = b_edge + b_face.
    ASSERTED: d* - a <= dist <= d* + a + b for every point (so no triangle is closer than dist - a); dist >= the float64 distance from
    x to the REPORTED q - a.  The largest error seen and the largest error / bound are printed; b is loose for far points and small
    triangles (it grows with D^2 / A) and a alone is what the near points are held to."""
    c = PC.case(name)
    T = c["T"][~R.collapsed(c["T"])]
    ctx = _host(c["tris"])
    pts = c["ref"]
    got = ctx.closest_point_host(pts)
    ctx.close()
    x = pts["p"].astype(np.float64)
    worst = worst_ratio = 0.0
    step = max(1, (1 << 20) // T.shape[0])
    for lo in range(0, x.shape[0], step):
        sl = slice(lo, lo + step)
        dd = _closest64(T, pts["p"][sl])
        star = dd.argmin(1)
        d_star = np.sqrt(dd[np.arange(star.size), star])
        t = T[star].astype(np.float64)
        edges = np.stack([np.linalg.norm(t[:, 1] - t[:, 0], axis=1), np.linalg.norm(t[:, 2] - t[:, 1], axis=1), np.linalg.norm(t[:, 0] - t[:, 2], axis=1)], 1)
        Lmax, lmin = edges.max(1), edges.min(1)
        A2 = 0.25 * (np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) ** 2).sum(1)
        D = d_star + Lmax
        dist = got["dist"][sl].astype(np.float64)
        a = U * (np.sqrt(3.0) * (np.abs(x[sl]).max(1) + 5.0 * c["E"]) + 4.0 * dist)
        b = (10.0 * U * Lmax * D / lmin + U * Lmax) + (152.0 * U * Lmax ** 3 * D ** 2 / (4.0 * A2) + 4.0 * U * Lmax)
        err = dist - d_star
        assert (err >= -a).all(), "%s: a reported distance is below the float64 minimum by more than the rounding bound" % name
        assert (err <= a + b).all(), "%s: a reported distance exceeds the float64 minimum by more than the bound" % name
        to_q = np.linalg.norm(x[sl] - got["q"][sl].astype(np.float64), axis=1)
        assert (np.abs(dist - to_q) <= a).all(), "%s: dist is not the distance to the reported q" % name
        worst = max(worst, float(np.abs(err).max() / c["E"]))
        worst_ratio = max(worst_ratio, float((np.abs(err) / (a + np.where(err > 0, b, 0.0))).max()))
    print("%s: largest |dist - d*| = %.3g E; largest error / bound = %.3g" % (name, worst, worst_ratio))


# ---------------------------------------------------------------------------------------------------------------------
# scene changes, refusals, resources
# ---------------------------------------------------------------------------------------------------------------------
def test_after_update_vertices():
    tris = rb.make_scene("soup2")
    ext = float(np.ptp(tris.reshape(-1, 3), axis=0).max())
    P = tris.astype(np.float64)
    moved = (P + 0.03 * ext * np.sin(3.0 * P[..., [1, 2, 0]] / ext + 0.5)).astype(F32)
    pts = PC.case("soup2")["ref"]
    ctx = _host(tris, dynamic=1)
    before = ctx.closest_point_host(pts)
    ctx.update_vertices([rb.mesh_of(moved)])
    fresh = _host(moved)
    want = fresh.closest_point_host(pts)
    assert R.differ(want, before).any(), "the deformation changes records"
    PC.assert_same(ctx.closest_point_host(pts), want, "twin after pt_update_vertices vs a fresh upload")
    PC.assert_same(want, R.closest(R.triangles(moved), pts), "the fresh upload vs the restatement")
    ctx.close()
    fresh.close()


def test_refusals_and_error_codes():
    L = B.lib()
    vp = C.c_void_p
    pts = B.make_points(F32([[0.1, 0.1, 3.0]] * 4))
    out = np.full(4 * 8, 7, np.int32).view(B.POINT_HIT_DTYPE)
    p, o = pts.ctypes.data_as(vp), out.ctypes.data_as(vp)
    v16 = vp(16)
    ctx = B.Context(-1)
    hd = ctx._h
    msg = lambda: L.pt_last_error(hd).decode()
    blocking, device, twin = L.pt_closest_point, L.pt_closest_point_device, L.pt_debug_closest_point_host
    # without a scene
    assert blocking(hd, p, 4, o) == PT_E_NO_SCENE and "pt_closest_point" in msg()
    assert device(hd, v16, 4, v16, None) == PT_E_NO_SCENE and "pt_closest_point_device" in msg()
    assert twin(hd, p, 4, o) == PT_E_NO_SCENE and "pt_debug_closest_point_host" in msg()
    rb.upload(ctx, rb.make_scene("rects"))
    # refused by name, before anything is touched
    assert blocking(None, p, 4, o) == PT_E_INVALID and device(None, v16, 4, v16, None) == PT_E_INVALID and twin(None, p, 4, o) == PT_E_INVALID
    assert blocking(hd, None, 4, o) == PT_E_INVALID and "pt_closest_point: NULL pts" in msg()
    assert blocking(hd, p, 4, None) == PT_E_INVALID and "pt_closest_point: NULL out" in msg()
    for n in (-1, 2 ** 31, 2 ** 40):
        assert blocking(hd, p, n, o) == PT_E_INVALID and "pt_closest_point: n = %d" % n in msg()
        assert twin(hd, p, n, o) == PT_E_INVALID and "pt_debug_closest_point_host: n = %d" % n in msg()
    assert blocking(hd, p, 4, o) == PT_E_NO_DEVICE  # valid arguments: no CPU fallback behind the entry point
    assert blocking(hd, None, 0, None) == PT_E_NO_DEVICE  # n = 0 asks for no array, and is still a device call
    assert device(hd, None, 4, v16, None) == PT_E_INVALID and "pt_closest_point_device: NULL d_pts" in msg()
    assert device(hd, v16, 4, None, None) == PT_E_INVALID and "pt_closest_point_device: NULL d_out" in msg()
    for n in (-1, 2 ** 31):
        assert device(hd, v16, n, v16, None) == PT_E_INVALID and "pt_closest_point_device: n = %d" % n in msg()
    for bad in (vp(24), vp(4), vp(17)):
        assert device(hd, bad, 4, v16, None) == PT_E_INVALID and "pt_closest_point_device: d_pts is not 16-byte aligned" in msg()
        assert device(hd, v16, 4, bad, None) == PT_E_INVALID and "pt_closest_point_device: d_out is not 16-byte aligned" in msg()
    for stream in (None, vp(0x1000)):
        assert device(hd, v16, 4, v16, stream) == PT_E_NO_DEVICE
        assert L.pt_synchronize(hd) == 0
    assert twin(hd, None, 4, o) == PT_E_INVALID and "pt_debug_closest_point_host: NULL pts" in msg()
    assert twin(hd, p, 4, None) == PT_E_INVALID and "pt_debug_closest_point_host: NULL out" in msg()
    assert (out.view(np.int32) == 7).all(), "a refused call wrote to the output"
    # without quad nodes: PT_E_INVALID by name, invalid arguments first; the twin needs no hierarchy and goes on working
    ctx.set_option("quad", 0)
    assert blocking(hd, p, 4, o) == PT_E_INVALID and "pt_closest_point" in msg() and "quad" in msg()
    assert blocking(hd, None, 4, o) == PT_E_INVALID and "NULL pts" in msg()
    assert device(hd, v16, 4, v16, None) == PT_E_INVALID and "pt_closest_point_device" in msg() and "quad" in msg()
    assert (out.view(np.int32) == 7).all()
    assert twin(hd, p, 4, o) == 4 and (out["prim"] >= 0).all()
    # n = 0
    assert twin(hd, None, 0, None) == 0 and ctx.closest_point_host(np.zeros(0, B.POINT_DTYPE)).shape == (0,)
    ctx.close()


def test_point_kernel_resources():
    """From the Makefile's own target (the flags that ship): the one kernel of the unit, no scratch, at most 128 VGPRs at the launch
    bounds of the ray kernels (four waves per SIMD)."""
    res = resource_report.resources("asm-points")
    assert len(res) == 1 and "pt_points_kernel" in next(iter(res)), list(res)
    r = next(iter(res.values()))
    print("asm-points:", r)
    assert r["scratch"] == 0 and 0 < r["vgprs"] <= 128 and r["agprs"] == 0 and r["occupancy"] >= 4
    resource_report.assert_ships_with_makefile_flags("pt_kernel_points")
