"""A referee for closest-hit answers that knows geometry and nothing else: plain numpy / Python, no GPU, no product code, no oracle code.

For float32 rays and float32 triangles, per (ray, triangle) pair:

* t*, u*, v*: where the ray's line meets the triangle's plane, and the barycentrics of that point (Moeller-Trumbore's quantities),
  evaluated in float64 from the float32 inputs.
* Et, Eu, Ev: a bound on |float32 result - exact value| for tri_eval as csrc/pt_trace.h writes it - e1, e2, tv by one subtraction each,
  cross and dot as in pt_device.h, the correctly rounded 1 / det, three products - by propagating an absolute error through that
  sequence.  Every float32 rounding contributes at most 2^-24 |result| + 2^-149 (gradual underflow: denormals are kept), a product of
  two inexact factors |a| Eb + |b| Ea + Ea Eb, the reciprocal Edet / (|det| (|det| - Edet)), unbounded where |det| <= Edet.  A fused
  multiply-add is bounded like the unfused pair (an upper bound, and independent of where the product fuses).  A result that may
  leave float32's range has no bound (infinite).  The float64 evaluation's own error runs through the same propagation at 2^-52
  relative to each computed value (float64 never underflows on these operands: every intermediate lies within 2^+-700) and is added
  to the bound, so the bound holds between the float32 result and the float64 value that is stored.  The bound arithmetic is itself
  float64: fewer than 2^10 operations on non-negative terms, so a final factor 1 + 2^-40 covers its own rounding.  No constant here is
  tuned.
* det* = 0 (the ray is parallel to the plane, or the triangle has no area) is an exact miss.  Where float64 cannot tell det* from 0
  the sign is decided in exact rational arithmetic (float32 values are dyadic rationals).
* The sliver rule in the words of include/mi355pt.h: a triangle whose height over its longest edge is below 1e-5 of that edge is
  never hit; within a relative 1e-6 of that threshold either answer is accepted.

Per pair that makes a triangle CERTAINLY HIT (u* - Eu > 0, v* - Ev > 0, (u* + v*) + Es <= 1 with Es the bound of the float32 sum,
t* - Et > kTMin, no sliver), CERTAINLY NOT HIT (one of the four fails by more than its bound, exact miss, sliver) or OPEN.

Three rules for an answer (hit, t, u, v, id) of any walk:

R1  the reported hit is real: id is a triangle of the scene that is not certainly not hit, and t, u, v lie within Et, Eu, Ev of it.
R2  nothing certain was missed: no certainly-hit triangle with t* + Et below the reported triangle's t* - Et; none at all on a miss.
R3  decided rays have one answer: where exactly one triangle is certainly hit and every other is certainly not hit or certainly
    farther (or all are certainly not hit), hit and id are the referee's.  Where all that remain are bit-identical copies of one
    certainly-hit triangle, the lowest id wins (equal float32 t: the tie rule).
"""
import os
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

U32 = 2.0 ** -24
TINY32 = 2.0 ** -149
U64 = 2.0 ** -52
MAX32 = 2.0 ** 127  # a float32 result that may reach this has no bound here
SELF = 1.0 + 2.0 ** -40  # the bound arithmetic's own rounding
K_TMIN = float(np.float32(1e-3))
SLIVER = 1e-5
SLIVER_BAND = 1e-6


class Q:
    """v: float64 evaluation; a: bound on |v - exact|; e: bound on |float32 result - exact|."""
    __slots__ = ("v", "a", "e")

    def __init__(self, v, a, e):
        self.v, self.a, self.e = v, a, e

    def mag(self):
        return np.abs(self.v) + self.a  # >= |exact|


def _exact_input(x):
    z = np.zeros_like(x)
    return Q(x, z, z)


def _rounded32(mag, e):
    """Bound after one float32 rounding of a result whose unrounded value is within e of an exact value of magnitude <= mag."""
    out = e + U32 * (mag + e) + TINY32
    return np.where(mag + out < MAX32, out, np.inf)


def _sub(a, b):
    v = a.v - b.v
    acc = a.a + b.a + U64 * np.abs(v)
    return Q(v, acc, _rounded32(np.abs(v) + acc, a.e + b.e))


def _add(a, b):
    v = a.v + b.v
    acc = a.a + b.a + U64 * np.abs(v)
    return Q(v, acc, _rounded32(np.abs(v) + acc, a.e + b.e))


def _mul(a, b):
    v = a.v * b.v
    ma, mb = a.mag(), b.mag()
    acc = ma * b.a + mb * a.a + a.a * b.a + U64 * np.abs(v)
    return Q(v, acc, _rounded32(np.abs(v) + acc, ma * b.e + mb * a.e + a.e * b.e))


def _cross(a, b):
    return [_sub(_mul(a[(i + 1) % 3], b[(i + 2) % 3]), _mul(a[(i + 2) % 3], b[(i + 1) % 3])) for i in range(3)]


def _dot(a, b):
    return _add(_mul(a[2], b[2]), _add(_mul(a[1], b[1]), _mul(a[0], b[0])))


def _recip(d):
    v = 1.0 / d.v
    lo = np.abs(d.v) - d.a  # <= |exact det|
    acc = np.where(lo > 0, d.a / (np.abs(d.v) * lo), np.inf) + U64 * np.abs(v)
    room = lo - d.e
    pert = np.where(room > 0, d.e / (lo * room), np.inf)
    return Q(v, acc, _rounded32(1.0 / np.where(lo > 0, lo, np.nan), pert))


def triangle_edges(tris):
    """p0, e1 = p1 - p0, e2 = p2 - p0 as Q over (1, triangles): the part of tri_eval that does not depend on the ray."""
    T = np.asarray(tris, np.float32).astype(np.float64)
    p0, p1, p2 = ([_exact_input(T[None, :, k, i]) for i in range(3)] for k in range(3))
    with np.errstate(all="ignore"):
        return p0, [_sub(p1[i], p0[i]) for i in range(3)], [_sub(p2[i], p0[i]) for i in range(3)]


def pair_values(tris, rays, edges=None):
    """t, u, v, s = u + v, det as Q over (rays, triangles), in tri_eval's operation order."""
    p0, e1, e2 = edges or triangle_edges(tris)
    R = np.asarray(rays, np.float32).astype(np.float64)
    o = [_exact_input(R[:, None, i]) for i in range(3)]
    d = [_exact_input(R[:, None, 3 + i]) for i in range(3)]
    with np.errstate(all="ignore"):
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        inv = _recip(det)
        tv = [_sub(o[i], p0[i]) for i in range(3)]
        u = _mul(_dot(tv, pv), inv)
        qv = _cross(tv, e1)
        v = _mul(_dot(d, qv), inv)
        t = _mul(_dot(e2, qv), inv)
        s = _add(u, v)
    return t, u, v, s, det


def _frac_det(tri, ray):
    f = [[Fraction(float(x)) for x in p] for p in tri]
    d = [Fraction(float(x)) for x in ray[3:6]]
    e1 = [f[1][i] - f[0][i] for i in range(3)]
    e2 = [f[2][i] - f[0][i] for i in range(3)]
    pv = [d[(i + 1) % 3] * e2[(i + 2) % 3] - d[(i + 2) % 3] * e2[(i + 1) % 3] for i in range(3)]
    return sum(e1[i] * pv[i] for i in range(3))


def sliver_classes(tris):
    """(never hit, either way): height over the longest edge below 1e-5 of that edge, within a relative 1e-6 of that threshold.
    height / longest edge = |e1 x e2| / L^2, in float64 from the float32 vertices (relative error some 1e-15: far inside the band)."""
    T = np.asarray(tris, np.float32).astype(np.float64)
    e = [T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], T[:, 2] - T[:, 1]]
    L2 = np.max([(x * x).sum(1) for x in e], axis=0)
    area2 = np.sqrt((np.cross(e[0], e[1]) ** 2).sum(1))
    with np.errstate(all="ignore"):
        ratio = np.where(L2 > 0, area2 / L2, 0.0)
    ratio = np.where(np.isfinite(ratio), ratio, 0.0)  # non-finite vertices: no geometry
    return ratio < SLIVER * (1 - SLIVER_BAND), (ratio >= SLIVER * (1 - SLIVER_BAND)) & (ratio <= SLIVER * (1 + SLIVER_BAND))


class Tables:
    """What the referee knows about a set of rays on a scene, kept sparse: per ray the triangles that are not certainly not hit."""

    def __init__(self, tris, rays, threads=None, pairs_per_chunk=250000):
        self.tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
        self.rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        self.n_tris, n = self.tris.shape[0], self.rays.shape[0]
        self.sliver, self.sliver_band = sliver_classes(self.tris)
        # bit-identical copies: the lowest id of each set
        _, first, inverse = np.unique(self.tris.reshape(-1, 9).view(np.uint32), axis=0, return_index=True, return_inverse=True)
        lowest = np.full(first.size, self.n_tris, np.int64)
        np.minimum.at(lowest, inverse.reshape(-1), np.arange(self.n_tris))
        self.canon = lowest[inverse.reshape(-1)]
        self.exact_fallbacks = 0
        self.edges = triangle_edges(self.tris)
        chunk = max(4, -(-pairs_per_chunk // max(1, self.n_tris)))  # arrays of a quarter million: below ~100 000 elements the allocator dominates
        starts = list(range(0, n, chunk))
        threads = threads or min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4)
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(lambda lo: self._chunk(lo, min(n, lo + chunk)), starts))
        counts = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, np.int64)
        self.ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        names = ("tri", "t", "u", "v", "et", "eu", "ev", "cert")
        for k, name in enumerate(names):
            setattr(self, name, np.concatenate([p[1][k] for p in parts]) if parts else np.zeros(0))
        self.ray_of = np.repeat(np.arange(n), counts)
        for k, name in enumerate(("cert_hi", "decided", "want_hit", "want_id", "tie", "n_cert")):
            setattr(self, name, np.concatenate([p[2][k] for p in parts]) if parts else np.zeros(0))
        self.exact_fallbacks = sum(p[3] for p in parts)

    def _chunk(self, lo, hi):
        t, u, v, s, det = pair_values(self.tris, self.rays[lo:hi], self.edges)
        m = hi - lo
        with np.errstate(all="ignore"):
            Et, Eu, Ev, Es = ((x.e + x.a) * SELF for x in (t, u, v, s))
            # exact miss: det* = 0.  float64 says so itself where its own error is 0; where it cannot tell, rationals decide
            miss = (det.v == 0) & (det.a == 0)
            unsure = ~miss & ~(np.abs(det.v) > det.a)
            unsure &= ~self.sliver[None, :]
            fallbacks = 0
            for r, k in zip(*np.nonzero(unsure)):
                fallbacks += 1
                if _frac_det(self.tris[k], self.rays[lo + r]) == 0:
                    miss[r, k] = True
            cert = (u.v - Eu > 0) & (v.v - Ev > 0) & (s.v + Es <= 1.0) & (t.v - Et > K_TMIN) & ~miss
            cert &= ~(self.sliver | self.sliver_band)[None, :]
            notc = (u.v + Eu < 0) | (v.v + Ev < 0) | (s.v - Es > 1.0) | (t.v + Et < K_TMIN) | miss | self.sliver[None, :]
            poss = ~notc
            hi_t = np.where(cert, t.v + Et, np.inf)
            cert_hi = hi_t.min(1) if self.n_tris else np.full(m, np.inf)
            # R3: competitors = possible and not certainly farther than the nearest certain hit
            comp = poss & ~(t.v - Et > cert_hi[:, None])
            n_comp = comp.sum(1)
            first = comp.argmax(1) if self.n_tris else np.zeros(m, np.int64)
            rows = np.arange(m)
            first_cert = cert[rows, first] if self.n_tris else np.zeros(m, bool)
            d_hit = (n_comp == 1) & first_cert
            d_miss = poss.sum(1) == 0
            canon_first = self.canon[first] if self.n_tris else first
            same = (comp & (self.canon[None, :] != canon_first[:, None])).sum(1) == 0
            tie = (n_comp > 1) & same & first_cert  # identical copies have identical values: all certain together
        rr, kk = np.nonzero(poss)
        per_pair = (kk.astype(np.int64), t.v[rr, kk], u.v[rr, kk], v.v[rr, kk], Et[rr, kk], Eu[rr, kk], Ev[rr, kk], cert[rr, kk])
        per_ray = (cert_hi, d_hit | d_miss, d_hit | tie, np.where(d_hit | tie, canon_first, -1).astype(np.int64), tie, cert.sum(1))
        return np.bincount(rr, minlength=m).astype(np.int64), per_pair, per_ray, fallbacks

    # -----------------------------------------------------------------------------------------------------------------
    def lookup(self, ids):
        """Index into the per-pair arrays of (ray r, triangle ids[r]); -1 where that triangle is certainly not hit (or no triangle)."""
        ids = np.asarray(ids, np.int64)
        n = self.rays.shape[0]
        key = self.ray_of * (self.n_tris + 1) + self.tri  # sorted: rays ascending, triangles ascending within a ray
        want = np.arange(n) * (self.n_tris + 1) + np.clip(ids, 0, self.n_tris)
        pos = np.searchsorted(key, want)
        ok = (ids >= 0) & (ids < self.n_tris) & (pos < key.size)
        ok &= key[np.minimum(pos, max(key.size - 1, 0))] == want if key.size else False
        return np.where(ok, pos, -1)

    def check(self, answer, with_t=True, rays_mask=None):
        """answer = (hit bool, t, u, v float32, id int32) per ray.  Returns a dict: r1, r2, r3 (bool per ray: the rule is violated),
        ratio_t / ratio_u / ratio_v (|float32 - exact| / bound of the reported hit; 0 where there is none or it is unbounded)."""
        hit, t, u, v, ids = answer
        hit = np.asarray(hit, bool)
        n = self.rays.shape[0]
        ids = np.asarray(ids).astype(np.int64)
        pos = self.lookup(np.where(hit, ids, -1))
        found = pos >= 0
        p = np.maximum(pos, 0)
        r1 = hit & ~found
        out = {}
        if self.tri.size == 0:
            z = np.zeros(n)
            out.update(ratio_t=z, ratio_u=z.copy(), ratio_v=z.copy())
            rep_lo = np.full(n, np.inf)
        else:
            for name, got, val, err in (("t", t, self.t, self.et), ("u", u, self.u, self.eu), ("v", v, self.v, self.ev)):
                if name == "t" and not with_t:
                    out["ratio_t"] = np.zeros(n)
                    continue
                g = np.asarray(got, np.float32).astype(np.float64)
                E = err[p]
                with np.errstate(all="ignore"):
                    dist = np.abs(g - val[p])
                    bounded = hit & found & np.isfinite(E)
                    r1 |= bounded & ~(dist <= E)  # a NaN answer against a finite bound fails too
                    out["ratio_" + name] = np.where(bounded & (E > 0), np.nan_to_num(dist / E, nan=np.inf), 0.0)
            with np.errstate(all="ignore"):
                rep_lo = np.where(hit & found, self.t[p] - self.et[p], np.inf)
                rep_lo = np.where(np.isnan(rep_lo), -np.inf, rep_lo)
        r2 = np.where(hit, self.cert_hi < rep_lo, np.isfinite(self.cert_hi)) & ~(hit & ~found)
        want_hit = self.want_hit.astype(bool)
        r3 = (self.decided.astype(bool) | self.tie.astype(bool)) & ((hit != want_hit) | (want_hit & (ids != self.want_id)))
        if rays_mask is not None:
            r1, r2, r3 = r1 & rays_mask, r2 & rays_mask, r3 & rays_mask
        out.update(r1=r1, r2=r2, r3=r3)
        return out

    def describe(self, answer, i):
        hit, t, u, v, ids = answer
        sl = slice(self.ptr[i], self.ptr[i + 1])
        poss = [(int(k), "certain" if c else "open", float(a), float(b)) for k, c, a, b in zip(self.tri[sl][:6], self.cert[sl], self.t[sl], self.et[sl])]
        return "ray %d %r: answered hit %r id %d t %r u %r v %r; referee: decided %r tie %r expects hit %r id %d, nearest certain t + Et %r, possible triangles (id, state, t*, Et) %r" % (
            i, self.rays[i].tolist(), bool(hit[i]), int(ids[i]), float(t[i]), float(u[i]), float(v[i]), bool(self.decided[i]), bool(self.tie[i]), bool(self.want_hit[i]),
            int(self.want_id[i]), float(self.cert_hi[i]), poss)


def assert_rules(tables, answer, who, with_t=True, rays_mask=None, cls=None):
    """R1-R3 on every ray (of rays_mask); the message names the rule and the first offending ray.  Returns check()'s dict."""
    res = tables.check(answer, with_t, rays_mask)
    for rule, text in (("r1", "R1 (the reported hit is real)"), ("r2", "R2 (nothing certain was missed)"), ("r3", "R3 (decided rays have one answer)")):
        bad = np.nonzero(res[rule])[0]
        if bad.size:
            raise AssertionError("%s violates %s on %d of %d rays; first: %s%s" % (
                who, text, bad.size, tables.rays.shape[0], "class %d, " % cls[bad[0]] if cls is not None else "", tables.describe(answer, bad[0])))
    return res


def answer_of_probe(out):
    """(hit, t, u, v, id) from a pt_debug_eval closest-hit / probe row (hit, t, u, v, id bits, ...)."""
    out = np.asarray(out, np.float32)
    return out[:, 0] != 0, out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy(), np.ascontiguousarray(out[:, 4]).view(np.int32)


def check_triangle_records(tris, records):
    """The product's application of the sliver rule, on the records read back with pt_debug_export_tree(PT_TREE_TRIS): every record is
    its input triangle, or that triangle collapsed to one point, the latter exactly where the restated rule says so (band excepted)."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    real = records["id"] != 0x7fffffff
    rec = records[real]
    order = np.argsort(rec["id"])
    rec = rec[order]
    assert np.array_equal(rec["id"], np.arange(tris.shape[0])), "every input triangle has one record"
    V = np.stack([rec["p0"], rec["p1"], rec["p2"]], 1)
    same = (V.view(np.uint32) == tris.view(np.uint32)).all((1, 2))
    point = (V[:, 0] == V[:, 1]).all(1) & (V[:, 0] == V[:, 2]).all(1)
    never, band = sliver_classes(tris)
    assert (same | point).all(), "a triangle record is neither its input nor a point: ids %r" % np.nonzero(~(same | point))[0][:8].tolist()
    collapsed = point & ~same
    kept = same & ~point
    wrong = (collapsed & ~never & ~band) | (kept & never)
    assert not wrong.any(), "sliver rule applied differently from its statement on ids %r" % np.nonzero(wrong)[0][:8].tolist()
    return dict(collapsed=int(collapsed.sum()), in_band=int(band.sum()))


class OnDemand:
    """Tables for the rays somebody asks about, built when first asked: for the few rays on which two walks differ."""

    def __init__(self, tris, rays):
        self.tris, self.rays, self.parts = tris, rays, []

    def inadmissible(self, idx, answer, with_t=True):
        """Of the rays idx, those on which `answer` (over all rays) violates R1 or R2."""
        idx = np.asarray(idx, np.int64)
        covered = np.concatenate([p[0] for p in self.parts]) if self.parts else np.zeros(0, np.int64)
        new = np.setdiff1d(idx, covered)
        if new.size:
            self.parts.append((new, Tables(self.tris, self.rays[new])))
        bad = []
        for ids, T in self.parts:
            m = np.isin(ids, idx)
            if m.any():
                res = T.check(tuple(np.asarray(a)[ids] for a in answer), with_t, rays_mask=m)
                bad.append(ids[res["r1"] | res["r2"]])
        return np.concatenate(bad) if bad else np.zeros(0, np.int64)
