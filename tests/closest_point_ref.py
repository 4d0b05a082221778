"""pt_closest_point (include/mi355pt.h "point queries: the nearest surface") restated in numpy from the flat scene arrays: float32, one IEEE
operation per numpy operation, nothing contracted, an fma only inside dot (fma32 below).  Nothing here imports the library under test,
and nothing comes from oracle/.

* triangles(flat): the scene's triangles in global id order after the sliver rule of the header (float64, the upload's expressions).
* closest(tris, pts): the vectorised form - every triangle against every point, the steps of the definition selected in their order.
* closest_loop(tris, pts): the plain form - a loop over the points, inside it a loop over the triangles in id order, the seven steps as
  an if / elif chain on numpy float32 scalars and the winner rule as the header writes it.  The vectorised form is held to it
  (tests/test_closest_point_host.py).
* VARIANTS: named wrong readings of the definition, each taken by both forms through `variant=`; the host test shows for each a case
  on which it changes a record.

Python 3.10 has no math.fma: fma32(a, b, c) forms the product in float64 (exact: 24 + 24 bits), adds in float64 and rounds to float32;
the double rounding can only go wrong where the float64 sum sits exactly on a float32 rounding tie, and there the error term of the
float64 addition decides (the construction of tests/aov_ref.py, which imports the oracle and is therefore not imported here)."""
import numpy as np

F32 = np.float32
NO_ID = 0x7fffffff
R_MAX = F32(1e10)
POINT_DTYPE = np.dtype([("p", "<f4", (3,)), ("radius", "<f4")])
POINT_HIT_DTYPE = np.dtype([("dist", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("q", "<f4", (3,)), ("feature", "<i4")])
VARIANTS = ("ties_to_higher_id", "le_without_id", "step4_before_step3", "uv_exchanged", "r2_strict")
PAIRS_PER_CHUNK = 1 << 21


def fma32(a, b, c):
    """round32(a * b + c) with ONE rounding, elementwise on float32 arrays (finite operands, results in the normal range)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)  # exact
    c64 = c.astype(np.float64)
    s = p + c64                                      # one float64 rounding
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(F32)                            # a second rounding: wrong only if s is a float32 tie that the exact sum is not
        d = s - r.astype(np.float64)                 # exact
        nb = np.nextafter(r, np.where(d > 0, F32(np.inf), F32(-np.inf)).astype(F32))
        tie = (d != 0) & np.isfinite(s) & (2.0 * d == (nb.astype(np.float64) - r.astype(np.float64)))
        if tie.any():
            t = s - p
            e = (p - (s - t)) + (c64 - t)            # TwoSum: p + c = s + e exactly
            lo, hi = np.minimum(r, nb), np.maximum(r, nb)
            r = np.where(tie & (e < 0), lo, np.where(tie & (e > 0), hi, r)).astype(F32)
    return r


def dot3(a, b):
    """pt_device.h dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))"""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def triangles(flat_or_tris):
    """(n, 3, 3) float32: the triangles in global id order with the sliver rule applied - a triangle whose height over its longest edge
    is at most 1e-5 of that edge (|e1 x e2|^2 <= 1e-10 max|e|^4 in float64, NaN included) becomes its first finite corner, three
    times.  Takes a flat scene (tests: scene_io.flatten_scene) or an (n, 3, 3) array."""
    pos = flat_or_tris["positions"] if isinstance(flat_or_tris, dict) else flat_or_tris
    t = np.array(pos, F32).reshape(-1, 3, 3)
    p = t.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2, e3 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 2] - p[:, 1]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        sq = lambda v: (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        n2, L2 = sq(n), np.maximum(np.maximum(sq(e1), sq(e2)), sq(e3))
        keep = n2 > 1e-10 * L2 * L2
    fin = np.isfinite(t).all(2)  # (n, 3): corner is finite
    first = np.where(fin.any(1), fin.argmax(1), 0)
    point = np.where(fin.any(1)[:, None], t[np.arange(t.shape[0]), first], F32(0))
    return np.where(keep[:, None, None], t, point[:, None, :]).astype(F32)


def collapsed(tris):
    return ((tris[:, 0] == tris[:, 1]) & (tris[:, 0] == tris[:, 2])).all(1)


def bound(radius):
    """(rmax, r2, searches): rmax = radius < 1e10f ? radius : 1e10f; r2 = rmax * rmax; a negative rmax finds nothing."""
    radius = np.asarray(radius, F32)
    with np.errstate(invalid="ignore"):
        rmax = np.where(radius < R_MAX, radius, R_MAX).astype(F32)
    with np.errstate(over="ignore"):
        r2 = (rmax * rmax).astype(F32)
    return rmax, r2, ~(rmax < 0)


# ---------------------------------------------------------------------------------------------------------------------
# the plain form
# ---------------------------------------------------------------------------------------------------------------------
def _tri_scalar(p0, p1, p2, x, variant):
    """(q, u, v, feature, dd) of one triangle and one point: steps 1 to 7 in their order."""
    zero, one = F32(0), F32(1)
    ab = p1 - p0
    ac = p2 - p0
    ap = x - p0
    d1 = dot3(ab, ap)
    d2 = dot3(ac, ap)
    bp = x - p1
    d3 = dot3(ab, bp)
    d4 = dot3(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = x - p2
    d5 = dot3(ab, cp)
    d6 = dot3(ac, cp)
    step3 = vc <= 0 and d1 >= 0 and d3 <= 0
    step4 = d6 >= 0 and d5 <= d6
    if variant == "step4_before_step3" and step4:
        step3 = False
    with np.errstate(all="ignore"):
        if d1 <= 0 and d2 <= 0:
            q, u, v, feature = p0, zero, zero, 1
        elif d3 >= 0 and d4 <= d3:
            q, u, v, feature = p1, one, zero, 2
        elif step3:
            s = d1 / (d1 - d3)
            q, u, v, feature = p0 + ab * s, s, zero, 4
        elif step4:
            q, u, v, feature = p2, zero, one, 3
        else:
            vb = d5 * d2 - d1 * d6
            va = d3 * d6 - d5 * d4
            e = d4 - d3
            f = d5 - d6
            if vb <= 0 and d2 >= 0 and d6 <= 0:
                s = d2 / (d2 - d6)
                q, u, v, feature = p0 + ac * s, zero, s, 6
            elif va <= 0 and e >= 0 and f >= 0:
                s = e / (e + f)
                q, u, v, feature = p1 + (p2 - p1) * s, one - s, s, 5
            else:
                k = one / ((va + vb) + vc)
                fv = vb * k
                fw = vc * k
                q, u, v, feature = (p0 + ab * fv) + ac * fw, fv, fw, 0
        e3 = x - q
        dd = dot3(e3, e3)
    if variant == "uv_exchanged":
        u, v = v, u
    return q.astype(F32), F32(u), F32(v), feature, F32(dd)


def closest_loop(tris, pts, variant=None):
    assert variant is None or variant in VARIANTS
    tris = np.asarray(tris, F32)
    pts = np.asarray(pts)
    out = np.zeros(pts.shape[0], POINT_HIT_DTYPE)
    out["prim"] = -1
    gone = collapsed(tris)
    for i in range(pts.shape[0]):
        x = pts["p"][i].astype(F32)
        rmax, r2, searches = bound(pts["radius"][i])
        best, best_id, rec = F32(r2), NO_ID, None
        if not searches:
            continue
        for t in range(tris.shape[0]):
            if gone[t]:
                continue
            q, u, v, feature, dd = _tri_scalar(tris[t, 0], tris[t, 1], tris[t, 2], x, variant)
            if variant == "ties_to_higher_id":
                take = dd < best or (dd == best and (best_id == NO_ID or t > best_id))
            elif variant == "le_without_id":
                take = dd <= best
            elif variant == "r2_strict":
                take = dd < best or (dd == best and best_id != NO_ID and t < best_id)  # nothing found yet: dd == r2 is not taken
            else:
                take = dd < best or (dd == best and t < best_id)
            if take:
                best, best_id, rec = dd, t, (q, u, v, feature)
        if rec is not None:
            out["dist"][i] = np.sqrt(best, dtype=F32)
            out["u"][i], out["v"][i], out["prim"][i], out["q"][i], out["feature"][i] = rec[1], rec[2], best_id, rec[0], rec[3]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the vectorised form
# ---------------------------------------------------------------------------------------------------------------------
def tri_all(tris, x, variant=None):
    """Every triangle (T, 3, 3) against every point (N, 3): dict of (N, T) arrays q (N, T, 3), u, v, feature, dd."""
    p0, p1, p2 = (tris[None, :, k, :] for k in range(3))
    x = x[:, None, :]
    with np.errstate(all="ignore"):
        ab = p1 - p0
        ac = p2 - p0
        ap = x - p0
        d1 = dot3(ab, ap)
        d2 = dot3(ac, ap)
        bp = x - p1
        d3 = dot3(ab, bp)
        d4 = dot3(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = x - p2
        d5 = dot3(ab, cp)
        d6 = dot3(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e = d4 - d3
        f = d5 - d6
        c1 = (d1 <= 0) & (d2 <= 0)
        c2 = (d3 >= 0) & (d4 <= d3)
        c3 = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        c4 = (d6 >= 0) & (d5 <= d6)
        c5 = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        c6 = (va <= 0) & (e >= 0) & (f >= 0)
        if variant == "step4_before_step3":
            c3 = c3 & ~c4
        s3 = d1 / (d1 - d3)
        s5 = d2 / (d2 - d6)
        s6 = e / (e + f)
        k = F32(1) / ((va + vb) + vc)
        fv = vb * k
        fw = vc * k
        conds = [c1, c2, c3, c4, c5, c6]
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        u = np.select(conds, [zero, one, s3, zero, zero, one - s6], fv).astype(F32)
        v = np.select(conds, [zero, zero, zero, one, s5, s6], fw).astype(F32)
        feature = np.select(conds, [1, 2, 4, 3, 6, 5], 0).astype(np.int32)
        q3, q5, q6, q7 = p0 + ab * s3[..., None], p0 + ac * s5[..., None], p1 + (p2 - p1) * s6[..., None], (p0 + ab * fv[..., None]) + ac * fw[..., None]
        shape = q7.shape
        q = np.select([c[..., None] for c in conds], [np.broadcast_to(p0, shape), np.broadcast_to(p1, shape), q3, np.broadcast_to(p2, shape), q5, q6], q7).astype(F32)
        e3 = x - q
        dd = dot3(e3, e3)
    if variant == "uv_exchanged":
        u, v = v, u
    return dict(q=q, u=u, v=v, feature=feature, dd=dd)


def closest(tris, pts, variant=None):
    """POINT_HIT_DTYPE records of the points (POINT_DTYPE) over the triangles (n, 3, 3) in global id order."""
    assert variant is None or variant in VARIANTS
    tris = np.asarray(tris, F32)
    pts = np.asarray(pts)
    n, T = pts.shape[0], tris.shape[0]
    out = np.zeros(n, POINT_HIT_DTYPE)
    out["prim"] = -1
    gone = collapsed(tris)
    step = max(1, PAIRS_PER_CHUNK // max(T, 1))
    for lo in range(0, n, step):
        sl = slice(lo, min(n, lo + step))
        r = tri_all(tris, pts["p"][sl].astype(F32), variant)
        _, r2, searches = bound(pts["radius"][sl])
        dd = r["dd"]
        with np.errstate(invalid="ignore"):
            cand = (dd < r2[:, None]) if variant == "r2_strict" else (dd <= r2[:, None])  # a NaN dd is no candidate
        cand &= ~gone[None, :] & searches[:, None]
        key = np.where(cand, dd, F32(np.inf))
        low = key.min(1)
        is_low = cand & (key == low[:, None])
        if variant in ("ties_to_higher_id", "le_without_id"):  # in id order `dd <= best` ends on the last of the tied triangles
            win = T - 1 - is_low[:, ::-1].argmax(1)
        else:
            win = is_low.argmax(1)
        found = is_low.any(1)
        rows = np.arange(dd.shape[0])
        rec = out[sl]
        rec["dist"] = np.where(found, np.sqrt(dd[rows, win], dtype=F32), F32(0))
        rec["u"] = np.where(found, r["u"][rows, win], F32(0))
        rec["v"] = np.where(found, r["v"][rows, win], F32(0))
        rec["prim"] = np.where(found, win, -1)
        rec["q"] = np.where(found[:, None], r["q"][rows, win], F32(0))
        rec["feature"] = np.where(found, r["feature"][rows, win], 0)
        out[sl] = rec
    return out


def differ(a, b):
    """Per record: any of the 32 bytes differs."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype.itemsize == 32 and b.dtype.itemsize == 32 and a.shape == b.shape
    return (a.view(np.uint8).reshape(-1, 32) != b.view(np.uint8).reshape(-1, 32)).any(1)
