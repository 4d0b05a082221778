// pt_trace.h -- device code shared by every kernel family that walks the tree (pt_kernel.hip: the wavefront-scheduled product kernel;
// pt_kernel_aux.hip: the lane-per-pixel variant and the validation kernel; pt_probes.h, pt_aov_first.h, pt_aov_follow.h,
// pt_rays_kernels.h, pt_ao.h): closest-hit building blocks (slab test, Moeller-Trumbore, binary node step, quad-node step, and
// quad_walk_step: the one bounded step of the quad walk that every family outside the wavefront kernel calls), the reference's
// path loop body after owl::traceRay (shade_hit: device.cu:136-214), camera rays (device.cu:231-241) and the work counters.
// Everything is in an anonymous namespace: each translation unit gets its own inlined copy.
#pragma once
#include <cstdlib>

#include "pt_device.h"
#include "pt_types.h"

using namespace ptd;

#define PT_BLOCK 256 // threads per workgroup of the lane-per-pixel and validation kernels
#define PT_DONE (-1) // ~0: a leaf reference with count 0 never occurs
#define PT_WAVE 64

namespace {

#ifndef PT_WATERTIGHT
#define PT_WATERTIGHT 0 // 1: pt_kernel_wt.hip, the watertight triangle test (below, "WATERTIGHT BUILD")
#endif

struct Hit {
    float t, u, v;
    int slot; // leaf-order index of the triangle
    int id;   // global triangle id (tie-break + shading record)
};
// No hit yet, and none accepted at or beyond t (a hit at exactly t is taken: every real id is below this one).
__device__ __forceinline__ void hit_reset(Hit& h, float t) { h.t = t; h.u = 0.0f; h.v = 0.0f; h.id = 0x7fffffff; h.slot = -1; }
// What the leaf code and quad_walk_step ask of the sink H that takes accepted triangles - a Hit here, the best one so far; a HitList in
// pt_hits.h - beside its member t, the cull bound: is (t, id) in front of what it holds, take this triangle, does it hold one.
__device__ __forceinline__ bool hit_admits(const Hit& h, float t, int id) { return t < h.t || (t == h.t && id < h.id); }
__device__ __forceinline__ void hit_take(Hit& h, float t, float u, float v, int id, int slot) { h.t = t; h.u = u; h.v = v; h.id = id; h.slot = slot; }
__device__ __forceinline__ bool hit_found(const Hit& h) { return h.slot >= 0; }

struct Counters {
    uint32_t rays = 0, nodes = 0, tris = 0, scat = 0, env = 0, samples = 0, retry = 0;
    unsigned long long cyc[8] = {}; // COUNT build: shader-clock cycles per phase {node steps, tri steps, retire, hit pass, miss pass, park/resume, sleep, total}
    uint32_t sched[32] = {}; // wave-uniform scheduler census (wavefront kernel)
    uint32_t depth[4] = {};  // per lane: pushes, pushes at stack depth >= 8 / 12 / 16
    uint32_t grp[6] = {};    // wave-uniform census of the group walk: phases, iterations, busy groups, node groups, leaf groups, rays
    unsigned long long grp_cyc = 0;
    uint32_t lobe[16] = {};  // wave-uniform census of the hit passes by sampled lobe (PtCounters::lobes)
    uint32_t cull_nohit = 0, cull_beyond = 0, leaf_noimp = 0; // per lane: quad steps that enter no child; of those: node beyond the best hit; leaf steps that do not improve the hit
#if PT_WATERTIGHT
    uint32_t wt64 = 0; // per lane: (ray, triangle) pairs whose edge functions were recomputed from float64 products (pt_stats.trav[2])
#endif
};

// Pointers read out of the parameter block are generic; every buffer is hipMalloc memory, so all accesses below go through
// address_space(1) pointers: global_load/global_store (vmcnt only) instead of flat_* (vmcnt + lgkmcnt, aperture check).
#define PT_AS1 __attribute__((address_space(1)))
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <class T>
__device__ __forceinline__ T PT_AS1* gp(T* p) { return (T PT_AS1*)p; }
__device__ __forceinline__ f32x4 ldg4(const void* base, size_t byte_off) { return *(const f32x4 PT_AS1*)((const char PT_AS1*)base + byte_off); }
// the same at a 32-bit per-lane offset from a wave-uniform base (the buffer is < 4 GiB): global_load_dwordx4 v, v_off, s[base] offset:imm,
// no 64-bit address arithmetic per lane; imm is added outside the 32-bit sum so that it folds into the instruction
__device__ __forceinline__ f32x4 ldg4u(const void* base, uint32_t byte_off, int imm) { return *(const f32x4 PT_AS1*)((const char PT_AS1*)base + (size_t)byte_off + imm); }
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 ldg2u(const void* base, uint32_t byte_off, int imm) { return *(const f32x2 PT_AS1*)((const char PT_AS1*)base + (size_t)byte_off + imm); }
__device__ __forceinline__ float fmin_hw(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ float fmax_hw(float a, float b) { return __builtin_fmaxf(a, b); }

// Slab test.  (bound - o) * inv keeps the error relative (2 roundings), the 1.0000004 factor covers it and
// the host builder pads every box (pt_bvh.cpp), so the test is conservative w.r.t. every hit tri_test can
// report: the closest hit does not depend on BVH topology or traversal order.  NaNs (0 * inf) are ignored
// by min/max exactly as in the oracle; signed zeros cannot change the comparison.
__device__ __forceinline__ bool box_test(float bminx, float bminy, float bminz, float bmaxx, float bmaxy, float bmaxz, v3 o, v3 inv,
                                         float tbest, float& tnear)
{
    float t0x = (bminx - o.x) * inv.x, t1x = (bmaxx - o.x) * inv.x;
    float t0y = (bminy - o.y) * inv.y, t1y = (bmaxy - o.y) * inv.y;
    float t0z = (bminz - o.z) * inv.z, t1z = (bmaxz - o.z) * inv.z;
    float tn = fmax_hw(fmax_hw(fmin_hw(t0x, t1x), fmin_hw(t0y, t1y)), fmax_hw(fmin_hw(t0z, t1z), kTMin));
    float tf = fmin_hw(fmin_hw(fmax_hw(t0x, t1x), fmax_hw(t0y, t1y)), fmin_hw(fmax_hw(t0z, t1z), tbest));
    tnear = tn;
    return tn <= tf * 1.0000004f;
}

// The same test with the slab distances as fma(bound, inv, -(o * inv)): see node4_step (below) for the error bound and when the
// host asks for the subtracting form instead.
__device__ __forceinline__ bool box_test_fma(float bminx, float bminy, float bminz, float bmaxx, float bmaxy, float bmaxz, v3 o, v3 inv, float tbest, float& tnear)
{
    const float nx = -(o.x * inv.x), ny = -(o.y * inv.y), nz = -(o.z * inv.z);
    float t0x = fma_(bminx, inv.x, nx), t1x = fma_(bmaxx, inv.x, nx);
    float t0y = fma_(bminy, inv.y, ny), t1y = fma_(bmaxy, inv.y, ny);
    float t0z = fma_(bminz, inv.z, nz), t1z = fma_(bmaxz, inv.z, nz);
    float tn = fmax_hw(fmax_hw(fmin_hw(t0x, t1x), fmin_hw(t0y, t1y)), fmax_hw(fmin_hw(t0z, t1z), kTMin));
    float tf = fmin_hw(fmin_hw(fmax_hw(t0x, t1x), fmax_hw(t0y, t1y)), fmin_hw(fmax_hw(t0z, t1z), tbest));
    tnear = tn;
    return tn <= tf * 1.0000004f;
}

// Reciprocal direction of a ray FOR THE SLAB TESTS of the wavefront kernel: v_rcp_f32 (1 ulp) instead of the correctly rounded division
// (ten instructions each, three per ray, in the refill step every lane runs through).  A slab distance is then off by a relative
// 2^-23 at most, i.e. a plane seems displaced by < 1.2e-7 x its distance from the ray origin - every box is padded by 1e-5 x the scene
// extent (pt_bvh.cpp), eighty times that - so the test stays conservative with respect to every hit the triangle test can report,
// and the triangle test itself (which decides t, u, v and the image) does not use it.
// The reciprocal is CLAMPED to +-PT_INV_MAX: a direction component of exactly 0 (a horizontal camera's middle row: the jitter is absorbed
// when `lower_left + v * vertical - origin` is formed, ~3e-5 of that row's samples; mirror bounces keep it) must not become inf in the
// fma form of the slab test - fma(plane, inf, -(o * inf)) is NaN only where plane and o have the same sign and -inf otherwise, which
// culled every box that straddles 0 on that axis, the root included (3 pixels of C2's 262 144 differed from the oracle at 256 spp:
// profiles/r04_notes.md 7; found by the whole-frame comparison at full spp).  With a finite reciprocal both forms give
// (plane - o) * 1e18 up to rounding: no constraint from a slab the origin is inside of, a cull for one it is outside of, and a ray that
// runs within 1e-8 of a box face - which is padded, so >= 1e-5 extents away from every triangle of the box - may be culled either way.
#ifndef PT_FAST_RAY_INV
#define PT_FAST_RAY_INV 1
#endif
#ifndef PT_INV_MAX
#define PT_INV_MAX 1e18f // (tests build a variant with infinity here to see the regression tests fail)
#endif
__device__ __forceinline__ v3 ray_inv(v3 d)
{
#if PT_FAST_RAY_INV
    const float x = __builtin_amdgcn_rcpf(d.x), y = __builtin_amdgcn_rcpf(d.y), z = __builtin_amdgcn_rcpf(d.z);
#else
    const float x = 1.0f / d.x, y = 1.0f / d.y, z = 1.0f / d.z;
#endif
    return V(__builtin_amdgcn_fmed3f(x, -PT_INV_MAX, PT_INV_MAX), __builtin_amdgcn_fmed3f(y, -PT_INV_MAX, PT_INV_MAX), __builtin_amdgcn_fmed3f(z, -PT_INV_MAX, PT_INV_MAX));
}

// Moeller-Trumbore, two-sided, kTMin < t; ties in t go to the lower global id (order independent result).
// tri_eval works on a record that is already in registers, so that a leaf step can issue the loads of all its triangles
// before the first test (one memory round trip per leaf instead of one per triangle).
template <class H> __device__ __forceinline__ void tri_eval(const f32x4 a, const f32x4 b, const f32x4 c, int slot, v3 o, v3 d, H& h)
{
    v3 p0 = V(a.x, a.y, a.z), p1 = V(a.w, b.x, b.y), p2 = V(b.z, b.w, c.x);
    int id = __float_as_int(c.y);
    v3 e1 = p1 - p0, e2 = p2 - p0;
    v3 pv = cross(d, e2);
    float det = dot(e1, pv);
    float inv = 1.0f / det;
    v3 tv = o - p0;
    float u = dot(tv, pv) * inv;
    v3 qv = cross(tv, e1);
    float v = dot(d, qv) * inv;
    float t = dot(e2, qv) * inv;
    if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > kTMin && hit_admits(h, t, id)) hit_take(h, t, u, v, id, slot);
}
template <class H> __device__ __forceinline__ void tri_test(const PtTri* __restrict__ tris, int slot, v3 o, v3 d, H& h)
{
    const size_t tb = (size_t)(uint32_t)slot * sizeof(PtTri);
    const f32x4 a = ldg4(tris, tb), b = ldg4(tris, tb + 16), c = ldg4(tris, tb + 32);
    tri_eval(a, b, c, slot, o, d, h);
}
// tri_eval's acceptance of one triangle, with u + v already formed
template <class H> __device__ __forceinline__ void tri_take(float t, float u, float v, float uv, int id, int slot, H& h)
{
    if (u >= 0.0f && v >= 0.0f && uv <= 1.0f && t > kTMin && hit_admits(h, t, id)) hit_take(h, t, u, v, id, slot);
}
__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
// Two triangles at once, {first, second} in the two halves of packed-f32 registers (v_pk_mul / v_pk_add / v_pk_fma_f32): each half does
// exactly tri_eval's operations in tri_eval's order - dot and cross as in pt_device.h, an fma only where they have one, the correctly
// rounded 1/det per triangle - so t, u and v are tri_eval's bit for bit.  The hits are merged in (t, id) order, first then second (take1:
// the second is a triangle of the leaf).
template <class H> __device__ __forceinline__ void tri_eval2(const f32x4 a0, const f32x4 b0, const f32x2 c0, const f32x4 a1, const f32x4 b1, const f32x2 c1, int slot0, bool take1,
                                          const f32x2 ox, const f32x2 oy, const f32x2 oz, const f32x2 dx, const f32x2 dy, const f32x2 dz, H& h)
{
    const f32x2 p0x = {a0.x, a1.x}, p0y = {a0.y, a1.y}, p0z = {a0.z, a1.z};
    const f32x2 p1x = {a0.w, a1.w}, p1y = {b0.x, b1.x}, p1z = {b0.y, b1.y};
    const f32x2 p2x = {b0.z, b1.z}, p2y = {b0.w, b1.w}, p2z = {c0.x, c1.x};
    const f32x2 e1x = p1x - p0x, e1y = p1y - p0y, e1z = p1z - p0z;
    const f32x2 e2x = p2x - p0x, e2y = p2y - p0y, e2z = p2z - p0z;
    const f32x2 pvx = fma2(dy, e2z, -(dz * e2y)), pvy = fma2(dz, e2x, -(dx * e2z)), pvz = fma2(dx, e2y, -(dy * e2x)); // cross(d, e2)
    const f32x2 det = fma2(e1z, pvz, fma2(e1y, pvy, e1x * pvx));                                                      // dot(e1, pv)
    const f32x2 inv = {1.0f / det.x, 1.0f / det.y};
    const f32x2 tvx = ox - p0x, tvy = oy - p0y, tvz = oz - p0z;
    const f32x2 u = fma2(tvz, pvz, fma2(tvy, pvy, tvx * pvx)) * inv;                                                   // dot(tv, pv) * inv
    const f32x2 qvx = fma2(tvy, e1z, -(tvz * e1y)), qvy = fma2(tvz, e1x, -(tvx * e1z)), qvz = fma2(tvx, e1y, -(tvy * e1x)); // cross(tv, e1)
    const f32x2 v = fma2(dz, qvz, fma2(dy, qvy, dx * qvx)) * inv;                                                      // dot(d, qv) * inv
    const f32x2 t = fma2(e2z, qvz, fma2(e2y, qvy, e2x * qvx)) * inv;                                                   // dot(e2, qv) * inv
    const f32x2 uv = u + v;
    tri_take(t.x, u.x, v.x, uv.x, __float_as_int(c0.y), slot0, h);
    if (take1) tri_take(t.y, u.y, v.y, uv.y, __float_as_int(c1.y), slot0 + 1, h);
}
#if PT_WATERTIGHT
// WATERTIGHT BUILD (the *_wt.hip units include their family's code with PT_WATERTIGHT = 1; option "watertight").  The triangle test of Woop,
// Benthin and Wald ("Watertight Ray/Triangle Intersection", JCGT 2013) in the fixed float32 sequence of DESIGN.md 2.1: the ray's dominant
// axis becomes z, the vertices are sheared into the ray's frame and the three 2-D edge functions U, V, W decide the hit.  An edge
// function is a difference of two products of the SAME four float32 values for the two triangles that share the edge, with the roles
// exchanged: as long as nothing is fused, the two are exact negatives of each other, so a ray can never be outside both.  Hence: no fma
// anywhere in here (plain * and -, and the translation unit is compiled with -ffp-contract=off; the pragma below keeps that true under
// any flags), and where an edge function is exactly 0 all three are recomputed with float64 products (exact for float32 factors) and a
// float64 difference, rounded to float32, which keeps the sign of the exact value.
// kz = index of the largest |d| component (first wins), kx = (kz + 1) % 3, ky = (kx + 1) % 3, kx and ky exchanged for d[kz] < 0 (the
// definition keeps the winding; with a two-sided test the exchange only shows in the signs of zeros - u = +0 or -0 on an edge - and
// the bits are part of the contract: pt_bvh.cpp and tests/watertight_ref.py index, this code selects, and the tests compare bit for bit).
// The axes are chosen with compare-and-select, never by indexing a register array: each of the three picks is "first flag ? x :
// (second flag ? y : z)" with six per-ray flags, two v_cndmask per component whatever the permutation.
struct WtRay {
    bool x0, x1, y0, y1, z0, z1; // kx == 0, kx == 1, ky == 0, ky == 1, kz == 0, kz == 1
    float sx, sy, sz;            // d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]: correctly rounded divisions
};
// (handed on as scalars: the struct as a reference parameter stayed in memory across the leaf loop - 16 bytes of scratch per lane)
#define PT_WT_PASS(r) (r).x0, (r).x1, (r).y0, (r).y1, (r).z0, (r).z1, (r).sx, (r).sy, (r).sz
#define PT_WT_PARAMS const bool rx0, const bool rx1, const bool ry0, const bool ry1, const bool rz0, const bool rz1, const float rsx, const float rsy, const float rsz
#define PT_WT_FROM_PARAMS {rx0, rx1, ry0, ry1, rz0, rz1, rsx, rsy, rsz}
__device__ __forceinline__ float wt_pick(const bool f0, const bool f1, float x, float y, float z) { return f0 ? x : (f1 ? y : z); }
__device__ __forceinline__ f32x2 wt_pick(const bool f0, const bool f1, f32x2 x, f32x2 y, f32x2 z) { return f0 ? x : (f1 ? y : z); }
__device__ __forceinline__ WtRay wt_ray(v3 dir)
{
    const float dx = dir.x, dy = dir.y, dz0 = dir.z;
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz0);
    WtRay r;
    r.z0 = ax >= ay && ax >= az;
    r.z1 = !r.z0 && ay >= az;
    const bool z2 = !r.z0 && !r.z1;
    const float dz = wt_pick(r.z0, r.z1, dx, dy, dz0);
    const bool sw = dz < 0.0f;
    r.x0 = sw ? r.z1 : z2;   // kx: kz + 1, or kz + 2 after the exchange
    r.x1 = sw ? z2 : r.z0;
    r.y0 = sw ? z2 : r.z1;   // ky: kz + 2, or kz + 1
    r.y1 = sw ? r.z0 : z2;
    r.sx = wt_pick(r.x0, r.x1, dx, dy, dz0) / dz;
    r.sy = wt_pick(r.y0, r.y1, dx, dy, dz0) / dz;
    r.sz = 1.0f / dz;
    return r;
}
// one edge function from float64 products: the products are exact, the difference is rounded to float64 and then to float32
__device__ __forceinline__ float wt_edge64(float a, float b, float c, float d)
{
#pragma clang fp contract(off)
    return (float)((double)a * (double)b - (double)c * (double)d);
}
// acceptance: the edge functions do not disagree in sign, det != 0, then tri_take's rule for t and the tie-break (u, v are not tested
// again: V / det may round to 1 + 2^-23 on an edge, and rejecting that would open the seam the test exists to close)
template <class H> __device__ __forceinline__ void wt_take(float U, float V, float W, float det, float t, float u, float v, int id, int slot, H& h)
{
    const bool neg = U < 0.0f || V < 0.0f || W < 0.0f, pos = U > 0.0f || V > 0.0f || W > 0.0f;
    if (!(neg && pos) && det != 0.0f && t > kTMin && hit_admits(h, t, id)) hit_take(h, t, u, v, id, slot);
}
// One triangle (the group walk's lane-per-triangle leaf, triangles beyond the fourth of a leaf).  n64: instrumented instance, counts the
// pairs that took the float64 branch.
template <class H> __device__ __forceinline__ void tri_eval_wt(const f32x4 a, const f32x4 b, const f32x4 c, int slot, v3 o, PT_WT_PARAMS, H& h, uint32_t* n64 = nullptr)
{
#pragma clang fp contract(off)
    const WtRay r = PT_WT_FROM_PARAMS;
    const float a0 = a.x - o.x, a1 = a.y - o.y, a2 = a.z - o.z; // A = p0 - o
    const float b0 = a.w - o.x, b1 = b.x - o.y, b2 = b.y - o.z; // B = p1 - o
    const float c0 = b.z - o.x, c1 = b.w - o.y, c2 = c.x - o.z; // C = p2 - o
    const float Az = wt_pick(r.z0, r.z1, a0, a1, a2), Bz = wt_pick(r.z0, r.z1, b0, b1, b2), Cz = wt_pick(r.z0, r.z1, c0, c1, c2);
    const float Ax = wt_pick(r.x0, r.x1, a0, a1, a2) - r.sx * Az, Ay = wt_pick(r.y0, r.y1, a0, a1, a2) - r.sy * Az;
    const float Bx = wt_pick(r.x0, r.x1, b0, b1, b2) - r.sx * Bz, By = wt_pick(r.y0, r.y1, b0, b1, b2) - r.sy * Bz;
    const float Cx = wt_pick(r.x0, r.x1, c0, c1, c2) - r.sx * Cz, Cy = wt_pick(r.y0, r.y1, c0, c1, c2) - r.sy * Cz;
    float U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const bool zero = U == 0.0f || V == 0.0f || W == 0.0f;
    if (__ballot(zero) != 0ull) { // wave-uniform: rare for ordinary rays, the rule for rays aimed at a vertex or an edge
        const float U64 = wt_edge64(Cx, By, Cy, Bx), V64 = wt_edge64(Ax, Cy, Ay, Cx), W64 = wt_edge64(Bx, Ay, By, Ax);
        U = zero ? U64 : U; V = zero ? V64 : V; W = zero ? W64 : W;
        if (n64) *n64 += zero ? 1u : 0u;
    }
    const float det = (U + V) + W;
    const float T = (U * (r.sz * Az) + V * (r.sz * Bz)) + W * (r.sz * Cz);
    const float inv = 1.0f / det;
    wt_take(U, V, W, det, T * inv, V * inv, W * inv, __float_as_int(c.y), slot, h);
}
// Two triangles at once in packed-f32 registers, as tri_eval2: each half does exactly tri_eval_wt's operations in its order
// (v_pk_mul_f32 / v_pk_add_f32 round like their scalar forms), the reciprocal of det per triangle.
template <class H> __device__ __forceinline__ void tri_eval_wt2(const f32x4 a0, const f32x4 b0, const f32x2 c0, const f32x4 a1, const f32x4 b1, const f32x2 c1, int slot0, bool take1, const f32x2 ox,
                                             const f32x2 oy, const f32x2 oz, PT_WT_PARAMS, H& h, uint32_t* n64 = nullptr)
{
#pragma clang fp contract(off)
    const WtRay r = PT_WT_FROM_PARAMS;
    const f32x2 A0 = (f32x2){a0.x, a1.x} - ox, A1 = (f32x2){a0.y, a1.y} - oy, A2 = (f32x2){a0.z, a1.z} - oz;
    const f32x2 B0 = (f32x2){a0.w, a1.w} - ox, B1 = (f32x2){b0.x, b1.x} - oy, B2 = (f32x2){b0.y, b1.y} - oz;
    const f32x2 C0 = (f32x2){b0.z, b1.z} - ox, C1 = (f32x2){b0.w, b1.w} - oy, C2 = (f32x2){c0.x, c1.x} - oz;
    const f32x2 sx = {r.sx, r.sx}, sy = {r.sy, r.sy}, sz = {r.sz, r.sz};
    const f32x2 Az = wt_pick(r.z0, r.z1, A0, A1, A2), Bz = wt_pick(r.z0, r.z1, B0, B1, B2), Cz = wt_pick(r.z0, r.z1, C0, C1, C2);
    const f32x2 Ax = wt_pick(r.x0, r.x1, A0, A1, A2) - sx * Az, Ay = wt_pick(r.y0, r.y1, A0, A1, A2) - sy * Az;
    const f32x2 Bx = wt_pick(r.x0, r.x1, B0, B1, B2) - sx * Bz, By = wt_pick(r.y0, r.y1, B0, B1, B2) - sy * Bz;
    const f32x2 Cx = wt_pick(r.x0, r.x1, C0, C1, C2) - sx * Cz, Cy = wt_pick(r.y0, r.y1, C0, C1, C2) - sy * Cz;
    f32x2 U = Cx * By - Cy * Bx, V = Ax * Cy - Ay * Cx, W = Bx * Ay - By * Ax;
    const bool zero0 = U.x == 0.0f || V.x == 0.0f || W.x == 0.0f, zero1 = U.y == 0.0f || V.y == 0.0f || W.y == 0.0f;
    if (__ballot(zero0 || zero1) != 0ull) {
        const f32x2 U64 = {wt_edge64(Cx.x, By.x, Cy.x, Bx.x), wt_edge64(Cx.y, By.y, Cy.y, Bx.y)};
        const f32x2 V64 = {wt_edge64(Ax.x, Cy.x, Ay.x, Cx.x), wt_edge64(Ax.y, Cy.y, Ay.y, Cx.y)};
        const f32x2 W64 = {wt_edge64(Bx.x, Ay.x, By.x, Ax.x), wt_edge64(Bx.y, Ay.y, By.y, Ax.y)};
        U.x = zero0 ? U64.x : U.x; V.x = zero0 ? V64.x : V.x; W.x = zero0 ? W64.x : W.x;
        U.y = zero1 ? U64.y : U.y; V.y = zero1 ? V64.y : V.y; W.y = zero1 ? W64.y : W.y;
        if (n64) *n64 += (zero0 ? 1u : 0u) + ((zero1 && take1) ? 1u : 0u);
    }
    const f32x2 det = (U + V) + W;
    const f32x2 T = (U * (sz * Az) + V * (sz * Bz)) + W * (sz * Cz);
    const f32x2 inv = {1.0f / det.x, 1.0f / det.y};
    const f32x2 t = T * inv, u = V * inv, v = W * inv;
    wt_take(U.x, V.x, W.x, det.x, t.x, u.x, v.x, __float_as_int(c0.y), slot0, h);
    if (take1) wt_take(U.y, V.y, W.y, det.y, t.y, u.y, v.y, __float_as_int(c1.y), slot0 + 1, h);
}
#endif // PT_WATERTIGHT
// All triangles of one leaf: the records of the first PT_LEAF_PREFETCH triangles are requested together, the tests follow.
// The wavefront kernel's leaf step; tris is below 4 GiB there (pt_render.cpp, plan_frame): 32-bit offsets from the wave-uniform base.
#ifndef PT_LEAF_PREFETCH
#define PT_LEAF_PREFETCH 4
#endif
#if PT_WATERTIGHT
// The watertight leaf step: the same loads and the same pairing; the ray's axes and shear are formed here, once per leaf step, from d
// alone (carrying them with the ray would cost five registers in the walk and a wider park area; the arithmetic gives the same bits).
template <class H> __device__ __forceinline__ void leaf_test(const PtTri* __restrict__ tris, int first, int count, v3 o, v3 d, H& h, uint32_t* n64 = nullptr)
{
    static_assert(PT_LEAF_PREFETCH == 4, "the leaf step tests the triangles of a leaf in two pairs");
    f32x4 ra[4], rb[4];
    f32x2 rc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kk = k < count ? k : count - 1;
        const uint32_t tb = (uint32_t)(first + kk) * (uint32_t)sizeof(PtTri);
        ra[k] = ldg4u(tris, tb, 0); rb[k] = ldg4u(tris, tb, 16); rc[k] = ldg2u(tris, tb, 32);
    }
    const WtRay r = wt_ray(d);
    const f32x2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z};
    tri_eval_wt2(ra[0], rb[0], rc[0], ra[1], rb[1], rc[1], first, count > 1, ox, oy, oz, PT_WT_PASS(r), h, n64);
    if (count > 2) tri_eval_wt2(ra[2], rb[2], rc[2], ra[3], rb[3], rc[3], first + 2, count > 3, ox, oy, oz, PT_WT_PASS(r), h, n64);
    for (int k = 4; k < count; ++k) { // leaf_size > 4 only
        const size_t tb = (size_t)(uint32_t)(first + k) * sizeof(PtTri);
        tri_eval_wt(ldg4(tris, tb), ldg4(tris, tb + 16), ldg4(tris, tb + 32), first + k, o, PT_WT_PASS(r), h, n64);
    }
}
#else
template <class H> __device__ __forceinline__ void leaf_test(const PtTri* __restrict__ tris, int first, int count, v3 o, v3 d, H& h)
{
#if PT_LEAF_PREFETCH == 0
    for (int k = 0; k < count; ++k) tri_test(tris, first + k, o, d, h);
#else
    static_assert(PT_LEAF_PREFETCH == 4, "the leaf step tests the triangles of a leaf in two pairs");
    f32x4 ra[4], rb[4];
    f32x2 rc[4]; // {p2.z, id}: the material index and the pad word are not needed here
    // unconditional loads (lanes with fewer triangles re-read their last one): one basic block, so all requests are in flight
    // before the first wait; with a per-triangle predicate the compiler waits inside each predicated block
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kk = k < count ? k : count - 1;
        const uint32_t tb = (uint32_t)(first + kk) * (uint32_t)sizeof(PtTri);
        ra[k] = ldg4u(tris, tb, 0); rb[k] = ldg4u(tris, tb, 16); rc[k] = ldg2u(tris, tb, 32);
    }
    const f32x2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z}, dx = {d.x, d.x}, dy = {d.y, d.y}, dz = {d.z, d.z};
    tri_eval2(ra[0], rb[0], rc[0], ra[1], rb[1], rc[1], first, count > 1, ox, oy, oz, dx, dy, dz, h);
    if (count > 2) tri_eval2(ra[2], rb[2], rc[2], ra[3], rb[3], rc[3], first + 2, count > 3, ox, oy, oz, dx, dy, dz, h);
    for (int k = 4; k < count; ++k) tri_test(tris, first + k, o, d, h); // leaf_size > 4 only
#endif
}
#endif // PT_WATERTIGHT

// One BVH-node step for a lane: test both children, descend into the nearer hit child, push the other.
// Stack entry i lives in LDS (stack[i * STRIDE]) for i < LDS_ENTRIES, else in the lane's HBM overflow column
// (ovf[(i - LDS_ENTRIES) * STRIDE]): on C4 0.006 % of the binary walk's pushes go deeper than 12 (census of the instrumented build: profiles/r01_summary.md), so a 12-entry LDS
// stack halves the LDS a wave needs for BVHs of any depth.  LDS_ENTRIES = 0x7fffffff: everything in LDS.
#ifndef PT_LDS_STACK
#define PT_LDS_STACK 12 // levels of a lane's stack that the one-wave kernels keep in LDS (wavefront kernel, probes, guide kernels, ray queries)
#endif
template <int STRIDE, int LDS_ENTRIES>
__device__ __forceinline__ void stack_push(uint32_t* stack, uint32_t PT_AS1* ovf, int sp, uint32_t v)
{
    if (LDS_ENTRIES == 0x7fffffff || sp < LDS_ENTRIES) stack[sp * STRIDE] = v;
    else ovf[(sp - LDS_ENTRIES) * STRIDE] = v;
}
template <int STRIDE, int LDS_ENTRIES>
__device__ __forceinline__ uint32_t stack_pop(uint32_t* stack, uint32_t PT_AS1* ovf, int sp)
{
    if (LDS_ENTRIES == 0x7fffffff || sp < LDS_ENTRIES) return stack[sp * STRIDE];
    return ovf[(sp - LDS_ENTRIES) * STRIDE];
}

template <int STRIDE, int LDS_ENTRIES>
__device__ __forceinline__ void node_step(const PtNode* __restrict__ nodes, uint32_t* stack, uint32_t PT_AS1* ovf, v3 o, v3 inv, float tbest, int& cur,
                                          int& sp, uint32_t* depth_census = nullptr)
{
    const size_t nb = (size_t)(uint32_t)cur * sizeof(PtNode);
    const f32x4 a = ldg4(nodes, nb), b = ldg4(nodes, nb + 16), c = ldg4(nodes, nb + 32), chf = ldg4(nodes, nb + 48);
    const int chl = __float_as_int(chf.x), chr = __float_as_int(chf.y);
    // slab test of both children at once, {left, right} in the two halves of packed-f32 registers.  Same IEEE operations as
    // box_test: (bound - o) * inv, min/max ignoring NaN, far side scaled by 1.0000004.
    const f32x2 lox = {a.x, a.y}, loy = {a.z, a.w}, loz = {b.x, b.y}, hix = {b.z, b.w}, hiy = {c.x, c.y}, hiz = {c.z, c.w};
    const f32x2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z}, ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
    const f32x2 t0x = (lox - ox) * ix, t1x = (hix - ox) * ix;
    const f32x2 t0y = (loy - oy) * iy, t1y = (hiy - oy) * iy;
    const f32x2 t0z = (loz - oz) * iz, t1z = (hiz - oz) * iz;
    const float tl = fmax_hw(fmax_hw(fmin_hw(t0x.x, t1x.x), fmin_hw(t0y.x, t1y.x)), fmax_hw(fmin_hw(t0z.x, t1z.x), kTMin));
    const float tr = fmax_hw(fmax_hw(fmin_hw(t0x.y, t1x.y), fmin_hw(t0y.y, t1y.y)), fmax_hw(fmin_hw(t0z.y, t1z.y), kTMin));
    f32x2 tf = {fmin_hw(fmin_hw(fmax_hw(t0x.x, t1x.x), fmax_hw(t0y.x, t1y.x)), fmin_hw(fmax_hw(t0z.x, t1z.x), tbest)),
                fmin_hw(fmin_hw(fmax_hw(t0x.y, t1x.y), fmax_hw(t0y.y, t1y.y)), fmin_hw(fmax_hw(t0z.y, t1z.y), tbest))};
    const f32x2 pad = {1.0000004f, 1.0000004f};
    tf = tf * pad;
    const bool hl = tl <= tf.x, hr = tr <= tf.y;
    // near child first; the far one is pushed only when both are hit
    const bool right_first = hr && (!hl || tr < tl);
    const int nearc = right_first ? chr : chl;
    const int farc = right_first ? chl : chr;
    if (hl && hr) {
        stack_push<STRIDE, LDS_ENTRIES>(stack, ovf, sp, (uint32_t)farc);
        if (depth_census) { depth_census[0] += 1; depth_census[1] += sp >= 8; depth_census[2] += sp >= 12; depth_census[3] += sp >= 16; }
        ++sp;
    }
    if (hl || hr) {
        cur = nearc;
    } else if (sp > 0) {
        --sp;
        cur = (int)stack_pop<STRIDE, LDS_ENTRIES>(stack, ovf, sp);
    } else {
        cur = PT_DONE;
    }
}

// Quad-node step (PtNode4, pt_types.h): the four grandchild boxes of a binary node in one 128-byte record - one cache line and
// one memory round trip per TWO levels of the binary tree.  Slab test as in node_step, two packed pairs; the lane continues with
// the nearest hit child and pushes the other hit children (in slot order; any visiting order gives the same closest hit).
// The lane reads its own record with 7 x global_load_dwordx4 = 7 vL1D accesses per lane and step, at 32-bit offsets from the wave-uniform
// base (the host keeps the quad nodes below 4 GiB: pt_render.cpp).  (Two validated experiments that did not pay - whole-line cooperative
// fetches through an LDS staging area, 64-byte records with 8-bit planes - live in variants/.)
template <int STRIDE, int LDS_ENTRIES, bool CENSUS = false>
__device__ __forceinline__ void node4_step(const PtNode4* __restrict__ nodes4, uint32_t* stack, uint32_t PT_AS1* ovf, v3 o, v3 inv, float tbest, int& cur, int& sp,
                                           const bool exact, uint32_t* n_nohit = nullptr, uint32_t* n_beyond = nullptr)
{
    bool crossed = false; // CENSUS: the ray crosses some slot's box when the bound of the best hit is ignored
    // Octant order: on each axis the ray enters a slab through the plane row that faces it - lo for inv > 0, hi for inv < 0 - and leaves
    // through the other one, so the step fetches the rows as (entry, exit) pairs and needs no per-axis min / max.  Both slab forms below are
    // monotone in the plane for a fixed inv (correctly rounded operations of a monotone function), so for lo <= hi the entry distance IS
    // the minimum of the two and the exit distance the maximum, bit for bit; every non-empty slot has finite lo <= hi (the host and device
    // builders pad finite boxes; pt_debug_quad_info checks it) and an empty slot {+inf, +inf} still misses (entry +inf or exit -inf).
    // The sign bit picks the row: ray_inv never returns 0, NaN or an infinity, and d = -0 gives -PT_INV_MAX, whose sign matches.
    const uint32_t ex = (uint32_t)(__float_as_int(inv.x) >> 31) & 48u; // 0 or 48: byte offset of the entry row from the lo row
    const uint32_t ey = (uint32_t)(__float_as_int(inv.y) >> 31) & 48u;
    const uint32_t ez = (uint32_t)(__float_as_int(inv.z) >> 31) & 48u;
    const uint32_t rec = (uint32_t)cur * (uint32_t)sizeof(PtNode4);
    const f32x4 nx4 = ldg4u(nodes4, rec + ex, 0), ny4 = ldg4u(nodes4, rec + ey, 16), nz4 = ldg4u(nodes4, rec + ez, 32);
    const f32x4 fx4 = ldg4u(nodes4, rec + (ex ^ 48u), 0), fy4 = ldg4u(nodes4, rec + (ey ^ 48u), 16), fz4 = ldg4u(nodes4, rec + (ez ^ 48u), 32);
    const f32x4 cf = ldg4u(nodes4, rec, 96);
    // Slab distances (round 4): fma(plane, 1/d, -(o/d)) - one packed fma per pair of planes instead of a subtraction and a multiplication
    // (24 of the step's ~150 VALU operations; C4 492 -> 484-486 ms, C3 149 -> 146).  Against (plane - o) * (1/d) the distance is off by
    // |o/d| 2^-24, i.e. the plane seems displaced by |o| 2^-24 in space: rays start on surfaces or at the camera, the boxes are padded by
    // 1e-5 x the scene extent, and the host launches the instances with the subtracting form (`exact`) for a camera farther than 42
    // extents from the origin (pt_render.cpp) - the test stays conservative with respect to every hit the triangle test can report, and
    // the triangle test decides the image.  The reciprocals are finite (ray_inv clamps them: a direction component of exactly 0 would
    // otherwise give -inf or NaN here depending on the signs of plane and origin, and cull boxes the ray runs through).
    // (Both forms behind a run-time switch in ONE instance cost 4 %: C4 486 -> 508 ms, profiles/r04_notes.md.)
    const f32x2 ox = {o.x, o.x}, oy = {o.y, o.y}, oz = {o.z, o.z}, ix = {inv.x, inv.x}, iy = {inv.y, inv.y}, iz = {inv.z, inv.z};
    const float nx = -(o.x * inv.x), ny = -(o.y * inv.y), nz = -(o.z * inv.z);
    const f32x2 nox = {nx, nx}, noy = {ny, ny}, noz = {nz, nz};
    const f32x2 pad = {1.0000004f, 1.0000004f};
    // Keys of the nearest-child choice: the entry distance's bits for a hit slot (a positive float: the bits order as unsigned integers),
    // all ones for a miss - integer min / max and compares instead of selects of booleans.
    const uint32_t kMiss = 0xffffffffu;
    uint32_t key[4];
#pragma unroll
    for (int p = 0; p < 2; ++p) { // slots {0, 1} and {2, 3}
        const f32x2 enx = p ? (f32x2){nx4.z, nx4.w} : (f32x2){nx4.x, nx4.y}, eny = p ? (f32x2){ny4.z, ny4.w} : (f32x2){ny4.x, ny4.y};
        const f32x2 enz = p ? (f32x2){nz4.z, nz4.w} : (f32x2){nz4.x, nz4.y}, exx = p ? (f32x2){fx4.z, fx4.w} : (f32x2){fx4.x, fx4.y};
        const f32x2 exy = p ? (f32x2){fy4.z, fy4.w} : (f32x2){fy4.x, fy4.y}, exz = p ? (f32x2){fz4.z, fz4.w} : (f32x2){fz4.x, fz4.y};
        f32x2 tnx, tfx, tny, tfy, tnz, tfz;
        if (exact) { // a compile-time constant in the product instances (see pt_render_wave_kernel: EXACT)
            tnx = (enx - ox) * ix; tfx = (exx - ox) * ix;
            tny = (eny - oy) * iy; tfy = (exy - oy) * iy;
            tnz = (enz - oz) * iz; tfz = (exz - oz) * iz;
        } else {
            tnx = __builtin_elementwise_fma(enx, ix, nox); tfx = __builtin_elementwise_fma(exx, ix, nox);
            tny = __builtin_elementwise_fma(eny, iy, noy); tfy = __builtin_elementwise_fma(exy, iy, noy);
            tnz = __builtin_elementwise_fma(enz, iz, noz); tfz = __builtin_elementwise_fma(exz, iz, noz);
        }
        const float ta = fmax_hw(fmax_hw(tnx.x, tny.x), fmax_hw(tnz.x, kTMin));
        const float tb = fmax_hw(fmax_hw(tnx.y, tny.y), fmax_hw(tnz.y, kTMin));
        f32x2 tf = {fmin_hw(fmin_hw(tfx.x, tfy.x), fmin_hw(tfz.x, tbest)), fmin_hw(fmin_hw(tfx.y, tfy.y), fmin_hw(tfz.y, tbest))};
        tf = tf * pad;
        key[2 * p] = ta <= tf.x ? __float_as_uint(ta) : kMiss;
        key[2 * p + 1] = tb <= tf.y ? __float_as_uint(tb) : kMiss;
        if (CENSUS) { // instrumented instance: would the slot be hit without the bound of the best hit so far?
            const float fa = fmin_hw(fmin_hw(tfx.x, tfy.x), tfz.x) * 1.0000004f;
            const float fb = fmin_hw(fmin_hw(tfx.y, tfy.y), tfz.y) * 1.0000004f;
            crossed = crossed || ta <= fa || tb <= fb;
        }
    }
    const int r0 = __float_as_int(cf.x), r1 = __float_as_int(cf.y), r2 = __float_as_int(cf.z), r3 = __float_as_int(cf.w);
    const bool b01 = key[1] < key[0], b23 = key[3] < key[2]; // the pair's second slot is the nearer one
    const uint32_t m01 = b01 ? key[1] : key[0], M01 = b01 ? key[0] : key[1], m23 = b23 ? key[3] : key[2], M23 = b23 ? key[2] : key[3];
    const int n01 = b01 ? r1 : r0, f01 = b01 ? r0 : r1, n23 = b23 ? r3 : r2, f23 = b23 ? r2 : r3; // nearer / farther child of each pair
    const bool in_b = m23 < m01; // the nearest hit is in slot pair {2, 3}
    const int nearc = in_b ? n23 : n01;
    const bool any = (in_b ? m23 : m01) != kMiss;
    if (CENSUS) { // steps that enter nothing, and of those the ones where the ray does cross a box: the node lies beyond the best hit
        *n_nohit += any ? 0u : 1u;
        *n_beyond += (!any && crossed) ? 1u : 0u;
    }
    // push order: the two slots of the OTHER pair first, the farther one first, then the nearest's sibling (popped first): siblings share a
    // parent box, so the sibling is usually the next nearest.  Three pushes at most; a pushed key is a hit.
    const int x1 = in_b ? f01 : f23, x2 = in_b ? n01 : n23, x3 = in_b ? f23 : f01;
    const bool h1 = (in_b ? M01 : M23) != kMiss, h2 = (in_b ? m01 : m23) != kMiss, h3 = (in_b ? M23 : M01) != kMiss;
    // (strictly by entry distance - the partner inserted where its distance puts it - costs 12 more instructions per step and saves
    // 0.1 % of the triangle tests: C4 497 -> 515 ms, C5 3 211 -> 3 353, profiles/r04_notes.md)
    if (LDS_ENTRIES == 0x7fffffff) {
        // common instance (the caller made sure sp + 3 stays inside the LDS part): store above the top whether or not the entry is
        // pushed - the slot is free either way - and advance sp by the predicate; no branches
        stack[sp * STRIDE] = (uint32_t)x1; sp += h1 ? 1 : 0;
        stack[sp * STRIDE] = (uint32_t)x2; sp += h2 ? 1 : 0;
        stack[sp * STRIDE] = (uint32_t)x3; sp += h3 ? 1 : 0;
    } else {
        if (h1) { stack_push<STRIDE, LDS_ENTRIES>(stack, ovf, sp, (uint32_t)x1); ++sp; }
        if (h2) { stack_push<STRIDE, LDS_ENTRIES>(stack, ovf, sp, (uint32_t)x2); ++sp; }
        if (h3) { stack_push<STRIDE, LDS_ENTRIES>(stack, ovf, sp, (uint32_t)x3); ++sp; }
    }
    if (any) {
        cur = nearc;
    } else if (sp > 0) {
        --sp;
        cur = (int)stack_pop<STRIDE, LDS_ENTRIES>(stack, ovf, sp);
    } else {
        cur = PT_DONE;
    }
}

// ONE BOUNDED STEP of a lane's quad walk, for every one-wave kernel outside the wavefront kernel (quad probe, guide kernels, ray
// queries, ambient occlusion): the node step at a node, the leaf test at a leaf, and after a leaf the next entry of the stack - or
// PT_DONE where the stack is empty, or at once where any_hit is set and the lane holds a hit (an occlusion walk: tbest never shrinks
// below the ray's bound there, so ordering the children buys nothing and node4_step is left as it is).  The caller starts a walk with
// cur = P.root, sp = 0, steps = 0, hit_reset(h, bound) and steps while cur != PT_DONE.
// BOUNDS AND TERMINATION: a walk is over after at most 2^20 + 1 calls (`steps`: a ray needs a few thousand), and the three pushes of a
// node step stay below `cap`, which the host derives from the tree (3 * depth4 + 1, + 3 for the stores above the top).  A walk that runs
// out of either is an OVERRUN: error_flag is set, cur = PT_DONE, and the function returns false; it returns true after every step it took.
// What an overrun does to the result is the caller's:
//     quad probe, first-hit and follow guide kernels    leave the walk with the best hit so far
//     ray kernels (closest, occluded, surface)          retire the ray as a miss (h.slot = -1); first-K hits (pt_hits.h): as K misses
//     ambient occlusion                                 k = AO_OVERRUN: the ray retires as a miss with ao = 1
template <int LDS_ENTRIES, class H>
__device__ __forceinline__ bool quad_walk_step(const PtKernelParams& P, const PtNode4* __restrict__ nodes4, const PtTri* __restrict__ tris, uint32_t* stack, uint32_t PT_AS1* ovf,
                                               const int cap, v3 o, v3 d, v3 inv, H& h, int& cur, int& sp, int& steps, const bool exact, const bool any_hit)
{
    if (++steps > (1 << 20) || sp + 3 > cap) {
        gp(P.error_flag)[0] = 1u;
        cur = PT_DONE;
        return false;
    }
    if (cur >= 0) {
        node4_step<PT_WAVE, LDS_ENTRIES>(nodes4, stack, ovf, o, inv, h.t, cur, sp, exact);
    } else {
        const uint32_t code = ~(uint32_t)cur;
        leaf_test(tris, (int)(code >> 3), (int)(code & 7u), o, d, h);
        if ((any_hit && hit_found(h)) || sp == 0) {
            cur = PT_DONE;
        } else {
            --sp;
            cur = (int)stack_pop<PT_WAVE, LDS_ENTRIES>(stack, ovf, sp);
        }
    }
    return true;
}

// STRIDE: words between two levels of a lane's stack = threads of the workgroup (the guide kernels of pt_aov_first.h / pt_aov_follow.h run it with one wave)
template <bool COUNT, int STRIDE = PT_BLOCK>
__device__ __forceinline__ void closest_hit(const PtKernelParams& P, uint32_t* stack, v3 o, v3 d, Hit& h, Counters& cn)
{
    h.t = kTMax; h.u = 0.0f; h.v = 0.0f; h.id = 0x7fffffff; h.slot = -1;
    const v3 inv = V(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    int sp = 0;
    int cur = P.root;
    const PtNode* __restrict__ nodes = P.nodes;
    const PtTri* __restrict__ tris = P.tris;
    for (;;) {
        while (cur >= 0) { // internal nodes: runs until every lane of the wave is at a leaf or finished
            if (COUNT) ++cn.nodes;
            node_step<STRIDE, 0x7fffffff>(nodes, stack, nullptr, o, inv, h.t, cur, sp);
        }
        if (cur == PT_DONE) break;
        uint32_t code = ~(uint32_t)cur;
        int first = (int)(code >> 3), count = (int)(code & 7u);
        for (int i = 0; i < count; ++i) {
            if (COUNT) ++cn.tris;
            tri_test(tris, first + i, o, d, h);
        }
        if (sp == 0) break;
        --sp;
        cur = (int)stack[sp * STRIDE];
    }
}

// interp3(bw, bx, by, a, b, c), the interpolation of a vertex attribute at a hit:
//     (1-u-v)*a + u*b + v*c  (device.cu:59,72,86-89), evaluated as an fma chain,
// is pt_device.h's ("the surface at a hit"), so that the CPU twins run the copy the kernels compile.
// (This note takes the lines the function took: the resource reports name kernels by source line, and the headers that hold kernels include this one.)

struct PathState {
    uint32_t rng;
    v3 org, dir, throughput;
    int depth, lobe, retries;
};

enum { SR_CONTINUE = 0, SR_END = 1, SR_RETRY = 2 };

// One iteration of the reference's path loop after owl::traceRay returned (device.cu:136-214).
// tslot < 0 = miss.  Returns SR_CONTINUE (ps.org/dir/throughput/depth updated, trace again), SR_END (radiance set; the
// sample contributes radiance * throughput, device.cu:217) or SR_RETRY (NaN/Inf f: shade the same hit again, :196-201).
template <bool COUNT>
__device__ __forceinline__ int shade_hit(const PtKernelParams& P, const float* mats, int tslot, float hu, float hv, PathState& ps, v3& radiance,
                                         Counters& cn)
{
    radiance = vs(0.0f);
    if (tslot < 0) { // miss: device.cu:136-148
        if (P.env_use_map && P.env_map.width > 0) {
            float tu, tv;
            uv_on_sphere(ps.dir, tu, tv);
            radiance = radiance + tex_nearest(gp(P.env_map.texels), P.env_map.width, P.env_map.height, tu, tv);
            if (COUNT) ++cn.env;
        } else if (P.env_use_auto) {
            radiance = radiance + lerp3(vs(1.0f), V(0.5f, 0.7f, 1.0f), 0.5f * (ps.dir.y + 1.0f));
        } else {
            radiance = radiance + V(P.env_color[0], P.env_color[1], P.env_color[2]);
        }
        radiance = radiance * P.env_intensity;
        return SR_END;
    }
    const size_t tb = (size_t)(uint32_t)tslot * sizeof(PtTri);
    // triangle and shading record share the leaf-order index, and the triangle record repeats the material index: two dependent
    // round trips (records, then material) instead of three
    const f32x4 a = ldg4(P.tris, tb), b = ldg4(P.tris, tb + 16), c = ldg4(P.tris, tb + 32);
    const size_t sb = (size_t)(uint32_t)tslot * sizeof(PtShade);
    const f32x4 s0 = ldg4(P.shade, sb), s1 = ldg4(P.shade, sb + 16), s2 = ldg4(P.shade, sb + 32), s3 = ldg4(P.shade, sb + 48);
    int mi = __float_as_int(c.z);
    Material mat = material_default(); // device.cu:150-154
    int tex_slot = -1;
    if (mi >= 0) {
        const float PT_AS1* mp = gp(mats) + mi * PT_MAT_STRIDE;
        mat = material_load(mp);
        tex_slot = __float_as_int(mp[17]);
    }
    if (mat.emission > 0.0f) { // device.cu:157-161: assignment, white, two-sided
        radiance = vs(mat.emission);
        return SR_END;
    }
    // attribute fetch: device.cu:164-173
    float bx = hu, by = hv;
    float bw = 1.0f - bx - by;
    v3 v_p = interp3(bw, bx, by, V(a.x, a.y, a.z), V(a.w, b.x, b.y), V(b.z, b.w, c.x));
    v3 v_n = normalize(interp3(bw, bx, by, V(s0.x, s0.y, s0.z), V(s0.w, s1.x, s1.y), V(s1.z, s1.w, s2.x)));
    if (tex_slot >= 0) { // device.cu:75-94
        float tu = fma_(by, s3.z, fma_(bx, s3.x, bw * s2.z));
        float tv = fma_(by, s3.w, fma_(bx, s3.y, bw * s2.w));
        const PtTexDesc PT_AS1* tdp = gp(P.textures) + tex_slot;
        mat.base_color = tex_nearest(gp(tdp->texels), tdp->width, tdp->height, tu, tv);
    }
    if (COUNT) ++cn.scat;

    // device.cu:176-190 (wo = -normalize(ray direction), device.cu:267-268)
    v3 wo = -normalize(ps.dir);
    v3 T, B;
    onb(v_n, T, B);
    v3 local_wo = to_local(T, B, v_n, wo);
    v3 local_wi = vs(0.0f);
    float pdf = 0.0f;
    v3 f = sample_disney(mat, local_wo, ps.rng, local_wi, pdf, ps.lobe);
    v3 wi = to_world(T, B, v_n, local_wi);

    if (pdf < 1e-5f) return SR_END; // device.cu:193
    if (isinf_(f.x) || isinf_(f.y) || isinf_(f.z) || isnan_(f.x) || isnan_(f.y) || isnan_(f.z)) {
        // device.cu:196-201: "--depth; continue" -> same ray again with fresh draws
        if (COUNT) ++cn.retry;
        // safety net (also in the oracle): a hit whose BSDF is NaN for every draw would spin forever
        if (++ps.retries > 64) return SR_END;
        return SR_RETRY;
    }
    ps.retries = 0;
    float aci = abs_(cos_theta(local_wi));
    ps.throughput = ps.throughput * ((f * aci) / pdf); // device.cu:204
    ps.org = v_p;                                      // device.cu:205 (no normal offset)
    ps.dir = wi;
    // device.cu:209-214: inverted, uncompensated Russian roulette
    float beta_max = max_(ps.throughput.x, max_(ps.throughput.y, ps.throughput.z));
    if (ps.lobe != kLobeGlass && ps.depth > 3) {
        float q = max_(0.05f, 1.0f - beta_max);
        if (rng_next(ps.rng) > q) return SR_END;
    }
    ++ps.depth;
    if (ps.depth >= P.max_depth) return SR_END; // loop bound, device.cu:130 (radiance stays 0)
    return SR_CONTINUE;
}

// Camera ray for the next sample of pixel (px, py): device.cu:231-241
__device__ __forceinline__ void gen_camera_ray(const PtKernelParams& P, int px, int py, PathState& ps)
{
    float rx = rng_next(ps.rng);
    float ry = rng_next(ps.rng);
    float su = ((float)px + rx) / (float)P.width;
    float sv = ((float)py + ry) / (float)P.height;
    const v3 cam_origin = V(P.cam[0], P.cam[1], P.cam[2]);
    const v3 cam_llc = V(P.cam[3], P.cam[4], P.cam[5]);
    const v3 cam_hor = V(P.cam[6], P.cam[7], P.cam[8]);
    const v3 cam_ver = V(P.cam[9], P.cam[10], P.cam[11]);
    ps.org = cam_origin;
    ps.dir = normalize(((cam_llc + cam_hor * su) + cam_ver * sv) - cam_origin);
    ps.throughput = vs(1.0f);
    ps.depth = 0;
    ps.lobe = kLobeNone;
    ps.retries = 0;
}

// The same ray from a camera record in HBM (12 floats: origin, llc, horizontal, vertical) and the row py INSIDE the pixel's frame: the
// batch instances (pt_kernel_batch.hip), where every lane may render a pixel of another frame.  Operation for operation gen_camera_ray.
__device__ __forceinline__ void gen_camera_ray_from(const PtKernelParams& P, const float PT_AS1* cam, int px, int py, PathState& ps)
{
    float rx = rng_next(ps.rng);
    float ry = rng_next(ps.rng);
    float su = ((float)px + rx) / (float)P.width;
    float sv = ((float)py + ry) / (float)P.height;
    const v3 cam_origin = V(cam[0], cam[1], cam[2]);
    const v3 cam_llc = V(cam[3], cam[4], cam[5]);
    const v3 cam_hor = V(cam[6], cam[7], cam[8]);
    const v3 cam_ver = V(cam[9], cam[10], cam[11]);
    ps.org = cam_origin;
    ps.dir = normalize(((cam_llc + cam_hor * su) + cam_ver * sv) - cam_origin);
    ps.throughput = vs(1.0f);
    ps.depth = 0;
    ps.lobe = kLobeNone;
    ps.retries = 0;
}

// The ray of the next sample of pixel (px, py) from the caller's ray image (pt_render_rays; include/mi355pt.h, pt_ray_gen): the record of
// the pixel at table + 16 * (px + W * py) floats as four 16-byte loads {org, -}, {dir, -}, {du, -}, {dv, -} (the fourth floats are loaded
// and not used), dir_s = normalize((dir + du * rx) + dv * ry).  The same two draws in the same order and the same resets as gen_camera_ray:
// only the ray itself differs.  The ray-image instances (pt_kernel_rayimage.hip) call it once per sample: the record is not kept.
__device__ __forceinline__ void gen_ray_from(const PtKernelParams& P, const float PT_AS1* table, int px, int py, PathState& ps)
{
    float rx = rng_next(ps.rng);
    float ry = rng_next(ps.rng);
    const size_t rb = ((size_t)(uint32_t)px + (size_t)(uint32_t)P.width * (size_t)(uint32_t)py) * 64; // < 2^31 pixels: below 2^37 bytes
    const f32x4 r0 = *(const f32x4 PT_AS1*)((const char PT_AS1*)table + rb);
    const f32x4 r1 = *(const f32x4 PT_AS1*)((const char PT_AS1*)table + rb + 16);
    const f32x4 r2 = *(const f32x4 PT_AS1*)((const char PT_AS1*)table + rb + 32);
    const f32x4 r3 = *(const f32x4 PT_AS1*)((const char PT_AS1*)table + rb + 48);
    ps.org = V(r0.x, r0.y, r0.z);
    ps.dir = normalize((V(r1.x, r1.y, r1.z) + V(r2.x, r2.y, r2.z) * rx) + V(r3.x, r3.y, r3.z) * ry);
    ps.throughput = vs(1.0f);
    ps.depth = 0;
    ps.lobe = kLobeNone;
    ps.retries = 0;
}

template <bool COUNT>
__device__ __forceinline__ void flush_counters(const PtKernelParams& P, const Counters& cn)
{
    if (!COUNT) return;
    unsigned long long v[7] = {cn.samples, cn.rays, cn.nodes, cn.tris, cn.scat, cn.env, cn.retry};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        unsigned long long x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        v[k] = x;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&P.counters->samples, v[0]);
        atomicAdd(&P.counters->rays, v[1]);
        atomicAdd(&P.counters->nodes, v[2]);
        atomicAdd(&P.counters->tris, v[3]);
        atomicAdd(&P.counters->scatters, v[4]);
        atomicAdd(&P.counters->env_misses, v[5]);
        atomicAdd(&P.counters->nan_retries, v[6]);
#pragma unroll
        for (int k = 0; k < 24; ++k) atomicAdd(&P.counters->sched[k], (unsigned long long)cn.sched[k]);
#pragma unroll
        for (int k = 0; k < 8; ++k) atomicAdd(&P.counters->sched[24 + k], cn.cyc[k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd(&P.counters->grp[k], (unsigned long long)cn.grp[k]);
        atomicAdd(&P.counters->grp[6], cn.grp_cyc);
#pragma unroll
        for (int k = 0; k < 16; ++k) atomicAdd(&P.counters->lobes[k], (unsigned long long)cn.lobe[k]);
    }
    {
        unsigned long long x0 = cn.cull_nohit, x1 = cn.cull_beyond, x3 = cn.leaf_noimp;
        for (int off = 32; off > 0; off >>= 1) { x0 += __shfl_down(x0, off, 64); x1 += __shfl_down(x1, off, 64); x3 += __shfl_down(x3, off, 64); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&P.counters->trav[0], x0); atomicAdd(&P.counters->trav[1], x1); atomicAdd(&P.counters->trav[3], x3); }
    }
#if PT_WATERTIGHT
    {
        unsigned long long x2 = cn.wt64;
        for (int off = 32; off > 0; off >>= 1) x2 += __shfl_down(x2, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&P.counters->trav[2], x2);
    }
#endif
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned long long x = cn.depth[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&P.counters->sched[19 + k], x);
    }
}

// 32-bit result in an SGPR: with __builtin_popcountll the compiler keeps wave-uniform counts as 64-bit values and compares them on the VALU
__device__ __forceinline__ int popc64(unsigned long long m)
{
    int r;
    asm("s_bcnt1_i32_b64 %0, %1" : "=s"(r) : "s"(m) : "scc");
    return r;
}
// number of set bits of m below this lane
__device__ __forceinline__ int rank_in(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

} // namespace
