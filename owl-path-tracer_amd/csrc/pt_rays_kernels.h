// pt_rays_kernels.h -- ray queries (pt_trace_closest, pt_trace_occluded, include/mi355pt.h): closest hit and occlusion for the caller's rays
// Translation units of their own once more - pt_kernel_rays.hip and, with PT_WATERTIGHT = 1, pt_kernel_rays_wt.hip include this header -
// so that every other `make asm-*` target goes on listing the kernels it listed.  No batch form.  Like the probes and the guide kernels the
// kernel owns no traversal arithmetic: ray_inv -> node4_step<PT_WAVE, PT_LDS_STACK> (short LDS stack, deeper levels in the wave's HBM
// columns) -> leaf_test -> stack_pop, with the probe's bounds around them.  The ray's own bound enters only as the initial h.t.
// What is new:  * ray I/O: a ray is two 16-byte loads, a closest hit one 16-byte store, an occlusion flag a byte store;
//   * any-hit exit (OCCLUDED): a lane whose leaf_test accepted a triangle (h.slot >= 0) is done at once.  tbest never shrinks below the
//     ray's bound in such a walk, so ordering the children buys nothing - node4_step is left as it is;
//   * lane refill (the persistent "while-while" loop of Aila and Laine 2009, without its atomics): a wave owns the contiguous range
//     [blockIdx.x * per_wave, + per_wave) of the rays - a multiple of 64, so what coherence the caller's order has stays inside a wave -
//     and `next`, the first ray not handed out yet, is wave-uniform.  Every round: idle = ballot(the lane holds no ray); when at most
//     A.refill lanes are still walking, every idle lane takes ray next + (its rank among the idle lanes), loads and initialises it, and
//     next += popcount(idle).  Nothing crosses waves.  Then every lane that holds a ray takes ONE step of its walk, and a lane whose walk
//     ended stores its result at once and is idle from the next round on.
// TERMINATION, read off the code: a lane that holds a ray takes a step every round, and a walk is over after at most 2^20 + 1 steps
// (`steps`; the stack bound `cap` comes from the host: 3 * depth4 + 1, + 3 - a walk that runs out of either sets error_flag and its ray
// is reported as a miss); a round in which no lane holds a ray either hands out at least one (next < end: no lane is walking, which is
// <= any A.refill) or leaves the loop; `next` only grows.
#pragma once
#include "pt_instance.h"
#include "pt_trace.h"
#if PT_RAYS_SURFACE
#include "pt_surface.h" // surface mode (pt_trace_surface): the record a lane retires with, and PT_RAYS_KERNEL / _LAUNCH / _GEOMETRY
#elif PT_WATERTIGHT
#define PT_RAYS_KERNEL pt_rays_wt_kernel
#define PT_RAYS_LAUNCH pt_launch_rays_wt
#define PT_RAYS_GEOMETRY pt_rays_geometry_wt
#else
#define PT_RAYS_KERNEL pt_rays_kernel
#define PT_RAYS_LAUNCH pt_launch_rays
#define PT_RAYS_GEOMETRY pt_rays_geometry
#endif
#ifndef PT_RAYS_WAVES_PER_EU
#define PT_RAYS_WAVES_PER_EU 4 // 128 VGPRs, 16 waves per CU at 3 KB of LDS each
#endif
template <bool OCCLUDED, bool EXACT>
__global__ void __launch_bounds__(PT_WAVE, PT_RAYS_WAVES_PER_EU) PT_RAYS_KERNEL(const PtKernelParams P, const PtRaysArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    uint32_t* stack = lds + lane; // stack[level * 64 + lane]
    const int ovf_levels = A.cap > PT_LDS_STACK ? A.cap - PT_LDS_STACK : 0;
    uint32_t PT_AS1* ovf = gp(A.ovf) + (size_t)blockIdx.x * ((size_t)ovf_levels * PT_WAVE) + lane;
    const PtNode4* __restrict__ nodes4 = P.nodes4;
    const PtTri* __restrict__ tris = P.tris;
    const long long first = (long long)blockIdx.x * A.per_wave; // < n: the launcher refuses a grid with an empty range
    const int end = (int)(first + A.per_wave < (long long)A.n ? first + A.per_wave : (long long)A.n);
    int next = (int)first;
    int ray = -1, cur = PT_DONE, sp = 0, steps = 0; // ray < 0: the lane is idle
    v3 o = vs(0.0f), d = vs(0.0f), inv = vs(0.0f);
    Hit h;
    h.t = 0.0f; h.u = 0.0f; h.v = 0.0f; h.id = 0x7fffffff; h.slot = -1;
    for (;;) {
        const unsigned long long m_idle = __ballot(ray < 0);
        const int n_idle = popc64(m_idle);
        if (next < end) {
            if (PT_WAVE - n_idle <= A.refill) {
                const long long i = (long long)next + rank_in(m_idle); // (64-bit: next may be within 63 of 2^31 - 1)
                if (ray < 0 && i < (long long)end) {
                    const f32x4 r0 = ldg4(A.rays, (size_t)(uint32_t)i * 32), r1 = ldg4(A.rays, (size_t)(uint32_t)i * 32 + 16); // {org, tmax}, {dir, not read}
                    o = V(r0.x, r0.y, r0.z);
                    d = V(r1.x, r1.y, r1.z);
                    inv = ray_inv(d);
                    h.t = r0.w < kTMax ? r0.w : kTMax; // NaN and +inf: the library's own bound; a hit at exactly this t is taken (id below)
                    h.u = 0.0f; h.v = 0.0f; h.id = 0x7fffffff; h.slot = -1;
                    cur = P.root; sp = 0; steps = 0;
                    ray = (int)i;
                }
                next = (end - next > n_idle) ? next + n_idle : end;
            }
        } else if (n_idle == PT_WAVE) {
            break;
        }
        if (ray >= 0) {
            if (cur != PT_DONE) {
                // bounded as the probe's walk: a ray needs a few thousand steps, the stack bound comes from the host (3 * depth4 + 1, + 3)
                if (++steps > (1 << 20) || sp + 3 > A.cap) {
                    gp(P.error_flag)[0] = 1u;
                    h.slot = -1; // retired as a miss
                    cur = PT_DONE;
                } else if (cur >= 0) {
                    node4_step<PT_WAVE, PT_LDS_STACK>(nodes4, stack, ovf, o, inv, h.t, cur, sp, EXACT);
                } else {
                    const uint32_t code = ~(uint32_t)cur;
                    leaf_test(tris, (int)(code >> 3), (int)(code & 7u), o, d, h);
                    if ((OCCLUDED && h.slot >= 0) || sp == 0) {
                        cur = PT_DONE;
                    } else {
                        --sp;
                        cur = (int)stack_pop<PT_WAVE, PT_LDS_STACK>(stack, ovf, sp);
                    }
                }
            }
            if (cur == PT_DONE) { // the walk has ended: the result is stored now, the lane is idle from the next round on
                const bool hit = h.slot >= 0;
                if (OCCLUDED) {
                    ((uint8_t PT_AS1*)A.out)[(size_t)(uint32_t)ray] = hit ? (uint8_t)1 : (uint8_t)0;
#if PT_RAYS_SURFACE
                } else if (PT_RAYS_SURFACE) { // surface mode: the 80-byte record of the hit; h.slot < 0 (a miss, a walk out of its bounds): the miss record
                    const SurfaceRecord r = surface_record(P, h.slot, h.u, h.v, h.t, h.id);
                    f32x4 PT_AS1* y = (f32x4 PT_AS1*)((char PT_AS1*)A.out + (size_t)(uint32_t)ray * 80);
                    y[0] = r.hit; y[1] = r.p; y[2] = r.ng; y[3] = r.ns; y[4] = r.base;
#endif
                } else {
                    f32x4 PT_AS1* y = (f32x4 PT_AS1*)((char PT_AS1*)A.out + (size_t)(uint32_t)ray * 16);
                    *y = hit ? (f32x4){h.t, h.u, h.v, __int_as_float(h.id)} : (f32x4){0.0f, 0.0f, 0.0f, __int_as_float(-1)};
                }
                ray = -1;
            }
        }
    }
}

// The instance that serves (occluded, exact), for the geometry function and the launcher alike.
static const void* rays_instance(int occluded, int exact)
{
#if PT_RAYS_SURFACE
    if (occluded) return nullptr; // no such instance: the geometry function and the launcher answer hipErrorInvalidValue
    return exact ? (const void*)PT_RAYS_KERNEL<false, true> : (const void*)PT_RAYS_KERNEL<false, false>;
#else
    if (occluded) return exact ? (const void*)PT_RAYS_KERNEL<true, true> : (const void*)PT_RAYS_KERNEL<true, false>;
    return exact ? (const void*)PT_RAYS_KERNEL<false, true> : (const void*)PT_RAYS_KERNEL<false, false>;
#endif
}

extern "C" hipError_t PT_RAYS_GEOMETRY(int occluded, int exact, PtGeometry* g)
{
    g->block = PT_WAVE;
    g->ns = PT_WAVE;
    g->lds_levels = PT_LDS_STACK;
    g->lds_bytes = (size_t)g->lds_levels * PT_WAVE * 4;
    g->state_words = 0;
#if PT_RAYS_SURFACE
    if (occluded) return hipErrorInvalidValue;
#endif
    return pt_complete_geometry(g, rays_instance(occluded, exact));
}

extern "C" hipError_t PT_RAYS_LAUNCH(const PtKernelParams* p, const PtRaysArgs* a, int occluded, int grid, size_t lds_bytes, hipStream_t stream)
{
    if (grid < 1 || a->n < 1 || a->per_wave < PT_WAVE || (a->per_wave % PT_WAVE) != 0 || a->refill < 0 || a->refill >= PT_WAVE) return hipErrorInvalidValue;
    if ((long long)grid * a->per_wave < (long long)a->n) return hipErrorInvalidValue; // the ranges cover every ray ...
    if ((long long)(grid - 1) * a->per_wave >= (long long)a->n) return hipErrorInvalidValue; // ... and none is empty: the kernel relies on it
#if PT_RAYS_SURFACE
    if (occluded) return hipErrorInvalidValue;
#endif
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel(rays_instance(occluded, p->box_exact), dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
