// pt_rays_kernels.h -- ray queries (pt_trace_closest, pt_trace_occluded, include/mi355pt.h): closest hit and occlusion for the caller's rays
// Translation units of their own once more - pt_kernel_rays.hip and, with PT_WATERTIGHT = 1, pt_kernel_rays_wt.hip include this header -
// so that every other `make asm-*` target goes on listing the kernels it listed.  No batch form.  Like the probes and the guide kernels the
// kernel owns no traversal arithmetic: ray_inv -> node4_step<PT_WAVE, PT_LDS_STACK> (short LDS stack, deeper levels in the wave's HBM
// columns) -> leaf_test -> stack_pop, one bounded step at a time (quad_walk_step, pt_trace.h).  The ray's own bound enters only as the
// initial h.t.
// What is new:  * ray I/O: a ray is two 16-byte loads, a closest hit one 16-byte store, an occlusion flag a byte store;
//   * any-hit exit (OCCLUDED): a lane whose leaf_test accepted a triangle (h.slot >= 0) is done at once.  tbest never shrinks below the
//     ray's bound in such a walk, so ordering the children buys nothing - node4_step is left as it is;
//   * lane refill: the persistent loop of pt_ray_range.h - the wave's range of the rays, the refill of its idle lanes, the ray load and
//     the TERMINATION argument are there; the bounded step of the walk is quad_walk_step (pt_trace.h).  A walk that runs out of its
//     bounds retires its ray as a miss.
#pragma once
#include "pt_instance.h"
#include "pt_ray_range.h"
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
    RayRange R = ray_range(A);
    int ray = -1, cur = PT_DONE, sp = 0, steps = 0; // ray < 0: the lane is idle
    v3 o = vs(0.0f), d = vs(0.0f), inv = vs(0.0f);
    Hit h;
    hit_reset(h, 0.0f);
    const auto start = [&](int i) {
        hit_reset(h, ray_load(A.rays, i, o, d, inv)); // a hit at exactly the ray's bound is taken
        cur = P.root; sp = 0; steps = 0;
        ray = i;
    };
    while (ray_range_refill(R, A.refill, ray < 0, start)) {
        if (ray >= 0) {
            if (cur != PT_DONE && !quad_walk_step<PT_LDS_STACK>(P, nodes4, tris, stack, ovf, A.cap, o, d, inv, h, cur, sp, steps, EXACT, OCCLUDED))
                h.slot = -1; // the walk ran out of its bounds: retired as a miss
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
    const void* fn = rays_instance(occluded, exact);
    if (!fn) return hipErrorInvalidValue;
    return pt_wave_geometry(g, PT_LDS_STACK, 0, fn);
}

extern "C" hipError_t PT_RAYS_LAUNCH(const PtKernelParams* p, const PtRaysArgs* a, int occluded, int grid, size_t lds_bytes, hipStream_t stream)
{
    const void* fn = rays_instance(occluded, p->box_exact);
    if (!fn || !pt_ray_ranges_ok(grid, *a)) return hipErrorInvalidValue;
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel(fn, dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
