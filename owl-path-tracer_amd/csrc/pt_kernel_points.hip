// pt_kernel_points.hip -- the kernel of pt_closest_point (include/mi355pt.h, "point queries: the nearest surface"): for each of the caller's
// points the nearest triangle of the scene within the point's radius.  A translation unit of its own, so that every other `make asm-*`
// target goes on listing the kernels it listed; no header of another family is touched.
// NOT the ray walk: a nearest-first, distance-pruned descent of the quad tree.  What it shares with the ray kernels is the shape of a
// wave - one wave per workgroup, the persistent lane-refill loop of pt_ray_range.h over the wave's range of the points, a lane's stack
// in LDS with the deeper levels in the wave's HBM column (stack_push / stack_pop, pt_trace.h), a step bound and a stack cap - and
// nothing of the arithmetic: the box distance and the closest point of a triangle are pt_points_math.h, which the CPU twin compiles too.
//   POINT I/O    a point is ONE 16-byte load {p, radius}, a result two 16-byte stores {dist, u, v, prim}, {q, feature}.
//   NODE STEP    the record's six plane rows and the child row: seven 16-byte loads, as node4_step.  Per slot dbox =
//                point_box_dist2(lo, hi, x); a slot is entered iff its child is not empty and !(dbox > best) - the empty slot is tested
//                by its reference: its dbox is +inf, but so may `best` compare (1e20f is finite; the test costs one compare).  The
//                lane descends into the entered slot with the smallest dbox and pushes the others, farthest first (a five-exchange
//                sorting network on (dbox bits, reference) keys: dbox >= +0, so its bits order as unsigned integers).  The order is
//                performance only: pruning is exact whatever it is (pt_points_math.h).
//   STALE ENTRIES  an entry is ONE word, the reference: pop and fetch.  An entry that the best distance has overtaken since it was pushed
//                costs a node step that enters nothing (seven loads of a record that is mostly in cache) or a leaf step that changes
//                nothing.  The other form - PT_POINTS_STACK_DIST = 1: two words, the reference and the bits of its dbox, stale
//                entries dropped at pop without a fetch - was built and measured against this one (tools/point_bench.py,
//                profiles/r28_points.json): it is slower on every scene and point set, 2 to 16 % at four ranges per wave (C4
//                stand-in, lattice points: 1 086 against 1 228 Mpoints/s), with 6 KB of LDS a wave or with 3.  It stays behind the macro.
//   LEAF STEP    point_tri over the leaf's `count` triangles; the first four records are requested together with the ray leaf's
//                48-byte loads (two 16-byte rows and {p2.z, id}), lanes with fewer triangles re-read their last one.
//   RETIREMENT   a lane whose walk ends stores its record and is idle from the next round on.  A walk that runs out of its step or
//                stack bound sets the bound flag and retires as not found.
// TERMINATION: pt_ray_range.h's argument; a walk is over after at most 2^20 + 1 steps, a point is one walk.
#include "pt_instance.h"
#include "pt_points_math.h"
#include "pt_ray_range.h"

#ifndef PT_POINTS_STACK_DIST
#define PT_POINTS_STACK_DIST 0
#endif
#ifndef PT_POINTS_WAVES_PER_EU
#define PT_POINTS_WAVES_PER_EU 4 // 128 VGPRs, the launch bounds of the ray kernels
#endif
#define PT_POINTS_ENTRY_WORDS (PT_POINTS_STACK_DIST ? 2 : 1)
// stack words of a lane kept in LDS: PT_LDS_STACK entries in either form (3 KB a wave, 6 KB with the distances)
#ifndef PT_POINTS_LDS_WORDS
#define PT_POINTS_LDS_WORDS (PT_LDS_STACK * PT_POINTS_ENTRY_WORDS)
#endif

namespace {

struct PointKey {
    uint32_t key; // bits of dbox for an entered slot, all ones for one that is not entered
    int ref;
};
__device__ __forceinline__ void key_sort2(PointKey& a, PointKey& b)
{
    const bool sw = b.key < a.key;
    const PointKey lo = sw ? b : a, hi = sw ? a : b;
    a = lo;
    b = hi;
}

__device__ __forceinline__ void point_push(uint32_t* stack, uint32_t PT_AS1* ovf, int& sp, const PointKey k)
{
    stack_push<PT_WAVE, PT_POINTS_LDS_WORDS>(stack, ovf, sp * PT_POINTS_ENTRY_WORDS, (uint32_t)k.ref);
    if (PT_POINTS_STACK_DIST) stack_push<PT_WAVE, PT_POINTS_LDS_WORDS>(stack, ovf, sp * PT_POINTS_ENTRY_WORDS + 1, k.key);
    ++sp;
}

// The next node or leaf of the lane's stack, PT_DONE where it is empty.  With the distance beside the reference, entries that the best
// distance has overtaken since they were pushed are dropped here.
__device__ __forceinline__ int point_pop(uint32_t* stack, uint32_t PT_AS1* ovf, int& sp, const float best)
{
    while (sp > 0) {
        --sp;
        const int ref = (int)stack_pop<PT_WAVE, PT_POINTS_LDS_WORDS>(stack, ovf, sp * PT_POINTS_ENTRY_WORDS);
        if (!PT_POINTS_STACK_DIST) return ref;
        const float dbox = __uint_as_float(stack_pop<PT_WAVE, PT_POINTS_LDS_WORDS>(stack, ovf, sp * PT_POINTS_ENTRY_WORDS + 1));
        if (!(dbox > best)) return ref;
    }
    return PT_DONE;
}

__device__ __forceinline__ void point_node_step(const PtNode4* __restrict__ nodes4, uint32_t* stack, uint32_t PT_AS1* ovf, const v3 x, const float best, int& cur, int& sp)
{
    const uint32_t rec = (uint32_t)cur * (uint32_t)sizeof(PtNode4);
    const f32x4 lx = ldg4u(nodes4, rec, 0), ly = ldg4u(nodes4, rec, 16), lz = ldg4u(nodes4, rec, 32);
    const f32x4 hx = ldg4u(nodes4, rec, 48), hy = ldg4u(nodes4, rec, 64), hz = ldg4u(nodes4, rec, 80);
    const f32x4 cf = ldg4u(nodes4, rec, 96);
    const uint32_t kMiss = 0xffffffffu;
    PointKey k[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float dbox = point_box_dist2(V(lx[s], ly[s], lz[s]), V(hx[s], hy[s], hz[s]), x);
        k[s].ref = __float_as_int(cf[s]);
        k[s].key = (k[s].ref != -1 && !(dbox > best)) ? __float_as_uint(dbox) : kMiss;
    }
    key_sort2(k[0], k[1]); key_sort2(k[2], k[3]); key_sort2(k[0], k[2]); key_sort2(k[1], k[3]); key_sort2(k[1], k[2]);
    // farthest first, so that the nearer of the others is popped first; an entered slot sorts before every slot that is not
    if (k[3].key != kMiss) point_push(stack, ovf, sp, k[3]);
    if (k[2].key != kMiss) point_push(stack, ovf, sp, k[2]);
    if (k[1].key != kMiss) point_push(stack, ovf, sp, k[1]);
    cur = k[0].key != kMiss ? k[0].ref : point_pop(stack, ovf, sp, best);
}

__device__ __forceinline__ void point_leaf_step(const PtTri* __restrict__ tris, const int first, const int count, const v3 x, PointBest& b)
{
    f32x4 ra[4], rb[4];
    f32x2 rc[4]; // {p2.z, id}
    // unconditional loads, as the ray leaf's: one basic block, all requests in flight before the first wait
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kk = k < count ? k : count - 1;
        const uint32_t tb = (uint32_t)(first + kk) * (uint32_t)sizeof(PtTri);
        ra[k] = ldg4u(tris, tb, 0); rb[k] = ldg4u(tris, tb, 16); rc[k] = ldg2u(tris, tb, 32);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < count) point_tri(V(ra[k].x, ra[k].y, ra[k].z), V(ra[k].w, rb[k].x, rb[k].y), V(rb[k].z, rb[k].w, rc[k].x), __float_as_int(rc[k].y), x, b);
    for (int k = 4; k < count; ++k) { // leaf_size > 4 only
        const uint32_t tb = (uint32_t)(first + k) * (uint32_t)sizeof(PtTri);
        const f32x4 a = ldg4u(tris, tb, 0), bb = ldg4u(tris, tb, 16);
        const f32x2 c = ldg2u(tris, tb, 32);
        point_tri(V(a.x, a.y, a.z), V(a.w, bb.x, bb.y), V(bb.z, bb.w, c.x), __float_as_int(c.y), x, b);
    }
}

} // namespace

__global__ void __launch_bounds__(PT_WAVE, PT_POINTS_WAVES_PER_EU) pt_points_kernel(const PtKernelParams P, const PtRaysArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    uint32_t* stack = lds + lane; // stack[word * 64 + lane]
    const int ovf_words = A.cap * PT_POINTS_ENTRY_WORDS > PT_POINTS_LDS_WORDS ? A.cap * PT_POINTS_ENTRY_WORDS - PT_POINTS_LDS_WORDS : 0;
    uint32_t PT_AS1* ovf = gp(A.ovf) + (size_t)blockIdx.x * ((size_t)ovf_words * PT_WAVE) + lane;
    const PtNode4* __restrict__ nodes4 = P.nodes4;
    const PtTri* __restrict__ tris = P.tris;
    RayRange R = ray_range(A);
    int pt = -1, cur = PT_DONE, sp = 0, steps = 0; // pt < 0: the lane is idle
    v3 x = vs(0.0f);
    PointBest b;
    point_reset(b, 0.0f);
    const auto start = [&](int i) {
        const f32x4 r = ldg4(A.rays, (size_t)(uint32_t)i * 16);
        x = V(r.x, r.y, r.z);
        const float rmax = point_rmax(r.w);
        point_reset(b, rmax * rmax);
        cur = point_searches(rmax) ? P.root : PT_DONE; // a negative radius: the walk has ended before it began
        sp = 0; steps = 0;
        pt = i;
    };
    while (ray_range_refill(R, A.refill, pt < 0, start)) {
        if (pt >= 0) {
            if (cur != PT_DONE) {
                if (++steps > (1 << 20) || sp + 3 > A.cap) { // the walk ran out of its bounds: retired as not found
                    gp(P.error_flag)[0] = 1u;
                    b.id = kPointNoId;
                    cur = PT_DONE;
                } else if (cur >= 0) {
                    point_node_step(nodes4, stack, ovf, x, b.dd, cur, sp);
                } else {
                    const uint32_t code = ~(uint32_t)cur;
                    point_leaf_step(tris, (int)(code >> 3), (int)(code & 7u), x, b);
                    cur = point_pop(stack, ovf, sp, b.dd);
                }
            }
            if (cur == PT_DONE) { // the walk has ended: the record is stored now, the lane is idle from the next round on
                const bool found = b.id != kPointNoId;
                f32x4 PT_AS1* y = (f32x4 PT_AS1*)((char PT_AS1*)A.out + (size_t)(uint32_t)pt * 32);
                y[0] = found ? (f32x4){sqrt_(b.dd), b.u, b.v, __int_as_float(b.id)} : (f32x4){0.0f, 0.0f, 0.0f, __int_as_float(-1)};
                y[1] = found ? (f32x4){b.q.x, b.q.y, b.q.z, __int_as_float(b.feature)} : (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                pt = -1;
            }
        }
    }
}

extern "C" int pt_points_entry_words(void) { return PT_POINTS_ENTRY_WORDS; }

extern "C" hipError_t pt_points_geometry(PtGeometry* g)
{
    return pt_wave_geometry(g, PT_POINTS_LDS_WORDS, 0, (const void*)pt_points_kernel);
}

// a->cap: the stack ENTRIES a lane may use (stack bound + the three pushes of a step); a->ovf: (cap * words per entry - LDS words) * 64
// words per workgroup
extern "C" hipError_t pt_launch_points(const PtKernelParams* p, const PtRaysArgs* a, int grid, size_t lds_bytes, hipStream_t stream)
{
    if (!pt_ray_ranges_ok(grid, *a) || a->cap < 3) return hipErrorInvalidValue;
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel((const void*)pt_points_kernel, dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
