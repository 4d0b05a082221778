"""The watertight triangle test of option "watertight" = 1, restated in float32 numpy as brute force over all triangles: the bit-level
reference of tests/test_watertight_host.py (the library's host walk), tests/test_gpu_watertight.py (the device's ray probes) and
tests/test_oracle_watertight.py (the oracle's watertight twin, which in turn is the reference of the watertight FRAMES: numpy brute
force does not render).  No GPU, no product code, no oracle code.

The test of Woop, Benthin and Wald ("Watertight Ray/Triangle Intersection", JCGT 2013) in the operation sequence DESIGN.md 2.1 fixes.
numpy's float32 `*`, `-`, `+`, `/` are correctly rounded and never fused, so every intermediate here is what an IEEE implementation
of that sequence must produce.

Per ray:  kz = index of the largest |d| component (the first on a tie), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky swapped
if d[kz] < 0;  Sx = d[kx] / d[kz], Sy = d[ky] / d[kz], Sz = 1 / d[kz].
Per triangle:  A = p0 - o, B = p1 - o, C = p2 - o;  Ax = A[kx] - Sx A[kz], Ay = A[ky] - Sy A[kz] (B, C alike);
U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax; if one of them is exactly 0 all three again from float64 products and a
float64 difference, rounded to float32;  rejected if one is < 0 and another > 0;  det = (U + V) + W, rejected if 0;
T = (U (Sz A[kz]) + V (Sz B[kz])) + W (Sz C[kz]);  inv = 1 / det, t = T inv, u = V inv (weight of p1), v = W inv (weight of p2).
Closest hit: two-sided, t > kTMin, the minimum t over all triangles, ties to the lower id; slivers (exact_hit.sliver_classes) never hit.

`variant` restates one deliberately wrong form each (the tests show that they are told apart): "no_f64" leaves the exact zeros as
they are, "swap_uv" exchanges u and v, "fused" evaluates every edge function as fma(a, b, -(c d)) - the product c d rounded, the
rest exact - which is what a contracting compiler makes of it.
"""
import numpy as np

import exact_hit

F32 = np.float32
K_TMIN = F32(1e-3)


def _fused_edge(a, b, c, d):
    """fma(a, b, -(c * d)) in float32: c * d rounded to float32, a * b exact in float64, the sum rounded once to float64 and then to
    float32 (the float64 sum of a 48-bit product and a 24-bit addend is exact unless their exponents lie > 29 bits apart: then the
    second rounding can differ from a true fma in a halfway case; this variant only has to differ from the unfused form)."""
    cd = (c * d).astype(F32).astype(np.float64)
    return (a.astype(np.float64) * b.astype(np.float64) - cd).astype(F32)


def ray_constants(rays):
    """kx, ky, kz (int, per ray) and Sx, Sy, Sz (float32)."""
    d = np.asarray(rays, F32)[:, 3:6]
    n = d.shape[0]
    rows = np.arange(n)
    kz = np.argmax(np.abs(d), axis=1)  # the first maximum
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = d[rows, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        dz = d[rows, kz]
        sx, sy, sz = d[rows, kx] / dz, d[rows, ky] / dz, F32(1.0) / dz
    assert sx.dtype == F32 and sz.dtype == F32
    return kx, ky, kz, sx, sy, sz


def pair_values(tris, rays, variant=None):
    """(accepted before t is looked at, t, u, v, took the float64 branch) over (rays, triangles), float32."""
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    rays = np.asarray(rays, F32).reshape(-1, 6)
    n = rays.shape[0]
    rows = np.arange(n)
    kx, ky, kz, sx, sy, sz = ray_constants(rays)
    o = rays[:, :3]
    with np.errstate(all="ignore"):
        P = [tris[None, :, k, :] - o[:, None, :] for k in range(3)]  # A, B, C: (rays, triangles, 3)
        z = [p[rows, :, kz] for p in P]
        x = [p[rows, :, kx] - sx[:, None] * zz for p, zz in zip(P, z)]
        y = [p[rows, :, ky] - sy[:, None] * zz for p, zz in zip(P, z)]
        (Ax, Bx, Cx), (Ay, By, Cy), (Az, Bz, Cz) = x, y, z
        if variant == "fused":
            U, V, W = _fused_edge(Cx, By, Cy, Bx), _fused_edge(Ax, Cy, Ay, Cx), _fused_edge(Bx, Ay, By, Ax)
        else:
            U, V, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        assert U.dtype == F32
        zero = (U == 0) | (V == 0) | (W == 0)
        if variant == "no_f64":
            zero = np.zeros_like(zero)
        if zero.any():
            def e64(a, b, c, d):
                a, b, c, d = (q[zero].astype(np.float64) for q in (a, b, c, d))
                return (a * b - c * d).astype(F32)

            u64, v64, w64 = e64(Cx, By, Cy, Bx), e64(Ax, Cy, Ay, Cx), e64(Bx, Ay, By, Ax)
            U, V, W = U.copy(), V.copy(), W.copy()
            U[zero], V[zero], W[zero] = u64, v64, w64
        mixed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        szc = sz[:, None]
        T = (U * (szc * Az) + V * (szc * Bz)) + W * (szc * Cz)
        inv = F32(1.0) / det
        t, u, v = T * inv, V * inv, W * inv
        assert t.dtype == F32 and u.dtype == F32
        ok = ~mixed & (det != 0)
    return ok, t, u, v, zero


def brute_force(tris, rays, variant=None, pairs_per_chunk=400000):
    """(hit bool, t, u, v float32, id int32; -1 and zeros on a miss) per ray, and the number of pairs that took the float64 branch."""
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    rays = np.asarray(rays, F32).reshape(-1, 6)
    never = exact_hit.sliver_classes(tris)[0]
    n, nt = rays.shape[0], tris.shape[0]
    hit, ids = np.zeros(n, bool), np.full(n, -1, np.int32)
    t_o, u_o, v_o = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, F32)
    step = max(1, pairs_per_chunk // max(1, nt))
    n64 = 0
    for lo in range(0, n, step):
        ok, t, u, v, zero = pair_values(tris, rays[lo:lo + step], variant)
        n64 += int(zero[:, ~never].sum())
        with np.errstate(all="ignore"):
            ok = ok & (t > K_TMIN) & ~never[None, :]
        tt = np.where(ok, t, F32(np.inf))
        k = tt.argmin(1)  # the first minimum: ties go to the lower id
        rows = np.arange(t.shape[0])
        h = ok[rows, k]
        hit[lo:lo + step], ids[lo:lo + step] = h, np.where(h, k, -1)
        t_o[lo:lo + step], u_o[lo:lo + step], v_o[lo:lo + step] = (np.where(h, q[rows, k], F32(0)) for q in (t, u, v))
    if variant == "swap_uv":
        u_o, v_o = v_o, u_o
    return (hit, t_o, u_o, v_o, ids), n64


def moeller_trumbore_leaks(tris, rays):
    """How many of `rays` unfused float32 Moeller-Trumbore (tests/test_exact_hit.py, restated_brute_force) reports as misses."""
    from test_exact_hit import restated_brute_force

    return int((~restated_brute_force(tris, rays)[0]).sum())


def same_bits(a, b):
    return np.asarray(a, F32).view(np.uint32) == np.asarray(b, F32).view(np.uint32)


def compare(ref, got, mask=None, with_t=True):
    """Indices (within mask) where `got` differs from `ref`: hit, id, and the bits of t (with_t), u, v on hits."""
    rh, rt, ru, rv, ri = ref
    gh, gt, gu, gv, gi = got
    rh, gh = np.asarray(rh, bool), np.asarray(gh, bool)
    bad = (rh != gh) | (np.asarray(ri, np.int64) != np.asarray(gi, np.int64))
    both = rh & gh
    bad |= both & ~(same_bits(ru, gu) & same_bits(rv, gv))
    if with_t:
        bad |= both & ~same_bits(rt, gt)
    if mask is not None:
        bad &= mask
    return np.nonzero(bad)[0]
