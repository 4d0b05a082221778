// pt_hits.h -- the kernel of pt_trace_hits (include/mi355pt.h, "ray queries: the first K hits"): the first K triangles along each of the
// caller's rays, in (t, id) order.  Translation units of their own - pt_kernel_rays_hits.hip and, with PT_WATERTIGHT = 1,
// pt_kernel_rays_hits_wt.hip include this header - so that every other `make asm-*` target goes on listing the kernels it listed.  Two
// instances per unit (EXACT 0 / 1).
// The kernel is the persistent loop of pt_ray_range.h around quad_walk_step (pt_trace.h), as the ray kernels of pt_rays_kernels.h are,
// with ONE difference: what takes the triangles a leaf step accepts is not a Hit (the best one so far) but a HitList, the lane's
// sorted list of the first K so far.  The leaf code of pt_trace.h is a template on that sink: the arithmetic, its order, the packed
// pairs, the per-triangle reciprocal and the watertight float64 branch are the closest-hit kernels', so t, u and v of a triangle are
// bit for bit what pt_trace_closest would store for it; only hit_admits / hit_take / hit_found are overloaded here.
// THE LIST lives in LDS behind the lane's stack, lane-strided like it: word w of entry j of lane l is
//     lds[(PT_LDS_STACK + j * PT_HITS_WORDS + w) * 64 + l],
// so the 64 lanes of any access touch 64 consecutive words whatever their j - no bank conflict - and nothing is indexed at run time
// in registers (that would be scratch, and the geometry query refuses builds with scratch).  The launch sizes it by K (park_words of
// pt_wave_geometry): (12 + K * PT_HITS_WORDS) * 256 bytes per wave.
// AN ENTRY is the record the lane stores, {t, u, v, id} (PT_HITS_WORDS = 4): a lane retires by copying its entries out.  (A 3-word
// entry {t, id, slot} with u and v formed again at retirement measured 5 to 26 % slower for a quarter less LDS: README.md,
// profiles/r30_hits.json; it is not in the source any more.)
// THE BOUND of a lane, L.t / L.id: {thi, 0x7fffffff} until the list is full, then entry K-1.  A triangle enters iff the test accepts
// it and (t, id) < bound (hit_admits), which is tri_take's rule with the bound in place of the best hit: a hit at exactly thi is taken, and of two
// triangles with bit-equal t both enter, the lower id first.  L.t is also the cull bound node4_step gets (through quad_walk_step,
// unchanged): it keeps boxes with tnear <= bound * pad, so a triangle that ties with entry K-1 is still reached.
// AT MOST ONCE: a triangle is in one leaf, a walk visits a leaf once, and the leaf step offers a triangle to the sink only under its
// count guards (take1, count > 2; the records it re-reads as padding are never offered).  Those guards stand in leaf_test / tri_eval2 as they did; the insertion RELIES on them, where a merge would not.
// INSERTION shifts from the tail: at most K entry moves per accepted triangle, each PT_HITS_WORDS LDS reads and writes.
// A walk that runs out of its step or stack bound empties the list: the ray retires with K miss records, error_flag is set.
// TERMINATION: pt_ray_range.h's argument; the insertion loop runs j down from at most K - 1 to 0, the retirement loop over K entries.
#pragma once
#include "pt_instance.h"
#include "pt_ray_range.h"
#if PT_WATERTIGHT
#define PT_HITS_KERNEL pt_rays_hits_wt_kernel
#define PT_HITS_LAUNCH pt_launch_rays_hits_wt
#define PT_HITS_GEOMETRY pt_rays_hits_geometry_wt
#else
#define PT_HITS_KERNEL pt_rays_hits_kernel
#define PT_HITS_LAUNCH pt_launch_rays_hits
#define PT_HITS_GEOMETRY pt_rays_hits_geometry
#endif
#ifndef PT_HITS_WAVES_PER_EU
#define PT_HITS_WAVES_PER_EU 4 // 128 VGPRs, 16 waves per CU; the LDS (3 + K KB per wave of a CU's 160 KB) allows that many up to K = 4 and fewer from K = 8 on, where the measured grids shrink (README.md)
#endif
#define PT_HITS_WORDS 4 // words of an entry: {t, u, v, id}
#define PT_HITS_ID 3    // the word of an entry that holds the triangle id; word 0 is t

namespace {

struct HitList {
    uint32_t* e; // the lane's list: word w of entry j at e[(j * PT_HITS_WORDS + w) * PT_WAVE]
    int k, n;    // K, and the entries held (<= K)
    float t;     // the bound: no triangle at or beyond (t, id) enters.  The cull bound of the node step
    int id;
};
// An empty list of k entries for a ray whose bound is thi (a hit at exactly thi is taken: every real id is below this one).
__device__ __forceinline__ void hits_reset(HitList& L, int k, float thi) { L.k = k; L.n = 0; L.t = thi; L.id = 0x7fffffff; }
__device__ __forceinline__ bool hit_found(const HitList& L) { return L.n > 0; }

__device__ __forceinline__ bool hit_admits(const HitList& L, float t, int id) { return t < L.t || (t == L.t && id < L.id); }
// (t, id) is below the bound: it enters at its place, the entries behind it move one back, and the last of a full list leaves.
__device__ __forceinline__ void hit_take(HitList& L, float t, float u, float v, int id, int slot)
{
    uint32_t* const e = L.e;
    const bool full = L.n == L.k;
    int j = full ? L.k - 1 : L.n; // the place that opens: behind the tail, or the tail of a full list
    for (; j > 0; --j) {
        uint32_t* const p = e + (j - 1) * (PT_HITS_WORDS * PT_WAVE);
        const float tp = __uint_as_float(p[0]);
        const int ip = (int)p[PT_HITS_ID * PT_WAVE];
        if (tp < t || (tp == t && ip < id)) break; // entry j - 1 stays in front
#pragma unroll
        for (int w = 0; w < PT_HITS_WORDS; ++w) p[(PT_HITS_WORDS + w) * PT_WAVE] = p[w * PT_WAVE];
    }
    uint32_t* const q = e + j * (PT_HITS_WORDS * PT_WAVE);
    q[0] = __float_as_uint(t);
    q[1 * PT_WAVE] = __float_as_uint(u); q[2 * PT_WAVE] = __float_as_uint(v); q[PT_HITS_ID * PT_WAVE] = (uint32_t)id;
    L.n += full ? 0 : 1;
    if (L.n == L.k) { // full: the bound is the last entry from now on
        const uint32_t* const z = e + (L.k - 1) * (PT_HITS_WORDS * PT_WAVE);
        L.t = __uint_as_float(z[0]);
        L.id = (int)z[PT_HITS_ID * PT_WAVE];
    }
}

} // namespace

template <bool EXACT>
__global__ void __launch_bounds__(PT_WAVE, PT_HITS_WAVES_PER_EU) PT_HITS_KERNEL(const PtKernelParams P, const PtHitsArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    uint32_t* stack = lds + lane; // stack[level * 64 + lane]
    const int ovf_levels = A.r.cap > PT_LDS_STACK ? A.r.cap - PT_LDS_STACK : 0;
    uint32_t PT_AS1* ovf = gp(A.r.ovf) + (size_t)blockIdx.x * ((size_t)ovf_levels * PT_WAVE) + lane;
    const PtNode4* __restrict__ nodes4 = P.nodes4;
    const PtTri* __restrict__ tris = P.tris;
    RayRange R = ray_range(A.r);
    int ray = -1, cur = PT_DONE, sp = 0, steps = 0; // ray < 0: the lane is idle
    v3 o = vs(0.0f), d = vs(0.0f), inv = vs(0.0f);
    HitList L;
    L.e = lds + PT_LDS_STACK * PT_WAVE + lane;
    hits_reset(L, A.k, 0.0f);
    const auto start = [&](int i) {
        hits_reset(L, A.k, ray_load(A.r.rays, i, o, d, inv));
        cur = P.root; sp = 0; steps = 0;
        ray = i;
    };
    while (ray_range_refill(R, A.r.refill, ray < 0, start)) {
        if (ray >= 0) {
            if (cur != PT_DONE && !quad_walk_step<PT_LDS_STACK>(P, nodes4, tris, stack, ovf, A.r.cap, o, d, inv, L, cur, sp, steps, EXACT, false))
                L.n = 0; // the walk ran out of its bounds: retired with K misses
            if (cur == PT_DONE) { // the walk has ended: K records are stored now, the lane is idle from the next round on
                f32x4 PT_AS1* y = (f32x4 PT_AS1*)((char PT_AS1*)A.r.out + (size_t)(uint32_t)ray * ((size_t)A.k * 16));
                for (int j = 0; j < A.k; ++j) {
                    f32x4 rec = {0.0f, 0.0f, 0.0f, __int_as_float(-1)};
                    if (j < L.n) {
                        const uint32_t* const p = L.e + j * (PT_HITS_WORDS * PT_WAVE);
                        rec = (f32x4){__uint_as_float(p[0]), __uint_as_float(p[1 * PT_WAVE]), __uint_as_float(p[2 * PT_WAVE]), __uint_as_float(p[3 * PT_WAVE])};
                    }
                    y[j] = rec;
                }
                ray = -1;
            }
        }
    }
}

static const void* hits_instance(int exact) { return exact ? (const void*)PT_HITS_KERNEL<true> : (const void*)PT_HITS_KERNEL<false>; }

// k: the K of the launch (1..PT_HITS_K_MAX): the list's K * PT_HITS_WORDS words per lane follow the stack in LDS
extern "C" hipError_t PT_HITS_GEOMETRY(int exact, int k, PtGeometry* g)
{
    if (k < 1 || k > PT_HITS_K_MAX) return hipErrorInvalidValue;
    return pt_wave_geometry(g, PT_LDS_STACK, k * PT_HITS_WORDS, hits_instance(exact));
}

extern "C" hipError_t PT_HITS_LAUNCH(const PtKernelParams* p, const PtHitsArgs* a, int grid, size_t lds_bytes, hipStream_t stream)
{
    if (!pt_ray_ranges_ok(grid, a->r)) return hipErrorInvalidValue;
    if (a->k < 1 || a->k > PT_HITS_K_MAX || lds_bytes < (size_t)(PT_LDS_STACK + a->k * PT_HITS_WORDS) * PT_WAVE * 4) return hipErrorInvalidValue; // the list must fit behind the stack
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel(hits_instance(p->box_exact), dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
