// pt_ao.h -- the fused ambient-occlusion kernel of pt_trace_ao (include/mi355pt.h, "ray queries: ambient occlusion").  Translation units
// of their own - pt_kernel_rays_ao.hip and, with PT_WATERTIGHT = 1, pt_kernel_rays_ao_wt.hip include this header - so that every other
// `make asm-*` target goes on listing the kernels it listed; pt_rays_kernels.h is not touched.  Two instances per unit (EXACT 0 / 1).
// The kernel is the persistent loop of pt_ray_range.h around quad_walk_step (pt_trace.h), as the ray kernels of pt_rays_kernels.h are -
// a wave owning a contiguous range of rays and refilling its idle lanes from it - with ONE more piece of per-lane state, the phase `k`:
//   k == AO_PRIMARY  the lane walks the caller's ray to its closest hit (the closest-hit instance's walk, step for step);
//   k >= 0           the lane walks its k-th occlusion ray: origin p, direction ao_direction(nf, rng), bound A.thi; the any-hit exit
//                    applies (a run-time test of k, not a template parameter: both kinds of lane sit in one wave);
//   k == AO_OVERRUN  a walk of the lane ran out of its step or stack bound: error_flag is set, the ray retires as a miss with ao = 1.
// A lane whose PRIMARY walk ends on a hit does not retire: it fetches the three 16-byte loads of PtTri and the first three of PtShade
// (the normals; no material row, no texel) for the hit slot, forms p and nf (ao_surface, pt_ao_math.h), seeds its stream and starts
// occlusion ray 0 in the same round.  A lane whose OCCLUSION walk ends counts the ray if it is clear and starts the next one, or
// retires after the K-th with two 16-byte stores: {t, u, v, prim}, {nf, ao}.  No occlusion ray is ever stored.  A lane in its
// occlusion phase holds a ray (ray >= 0) and so counts as walking for the refill ballot.
// The frame (T, B) of the hemisphere is recomputed from nf per occlusion ray (ao_direction): six registers fewer in the walk than
// keeping it, a normalize and a cross more per K-th of a walk, and the same bits.
// TERMINATION: pt_ray_range.h's argument, with `steps` and the stack bound applying PER WALK (both are reset when a walk starts); a
// lane that holds a ray either takes a step of a walk or ends one, a ray has 1 + K <= 4097 walks, and an overrun retires it at once.
#pragma once
#include "pt_ao_math.h"
#include "pt_instance.h"
#include "pt_ray_range.h"
#if PT_WATERTIGHT
#define PT_AO_KERNEL pt_rays_ao_wt_kernel
#define PT_AO_LAUNCH pt_launch_rays_ao_wt
#define PT_AO_GEOMETRY pt_rays_ao_geometry_wt
#else
#define PT_AO_KERNEL pt_rays_ao_kernel
#define PT_AO_LAUNCH pt_launch_rays_ao
#define PT_AO_GEOMETRY pt_rays_ao_geometry
#endif
#ifndef PT_AO_WAVES_PER_EU
#define PT_AO_WAVES_PER_EU 4 // 128 VGPRs, 16 waves per CU at 3 KB of LDS each
#endif
#define AO_PRIMARY (-1)
#define AO_OVERRUN (-2)
template <bool EXACT>
__global__ void __launch_bounds__(PT_WAVE, PT_AO_WAVES_PER_EU) PT_AO_KERNEL(const PtKernelParams P, const PtAoArgs A)
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
    int k = AO_PRIMARY, clear = 0;
    uint32_t rng = 0u;
    v3 o = vs(0.0f), d = vs(0.0f), inv = vs(0.0f), nf = vs(0.0f);
    f32x4 first_hit = {0.0f, 0.0f, 0.0f, 0.0f}; // the closest hit's record, kept through the occlusion phase
    Hit h;
    hit_reset(h, 0.0f);
    const auto start = [&](int i) {
        hit_reset(h, ray_load(A.r.rays, i, o, d, inv));
        cur = P.root; sp = 0; steps = 0;
        k = AO_PRIMARY;
        ray = i;
    };
    while (ray_range_refill(R, A.r.refill, ray < 0, start)) {
        if (ray >= 0) {
            // the bounds apply per walk; the any-hit exit is an occlusion ray's
            if (cur != PT_DONE && !quad_walk_step<PT_LDS_STACK>(P, nodes4, tris, stack, ovf, A.r.cap, o, d, inv, h, cur, sp, steps, EXACT, k >= 0))
                k = AO_OVERRUN;
            if (cur == PT_DONE) { // a walk has ended: the next one starts now, or the ray retires and the lane is idle from the next round on
                bool retire = true;
                float ao = 1.0f;
                if (k == AO_PRIMARY) {
                    first_hit = (f32x4){0.0f, 0.0f, 0.0f, __int_as_float(-1)};
                    nf = vs(0.0f);
                    if (h.slot >= 0) {
                        const size_t tb = (size_t)(uint32_t)h.slot * sizeof(PtTri);
                        const f32x4 a = ldg4(P.tris, tb), b = ldg4(P.tris, tb + 16), c = ldg4(P.tris, tb + 32);
                        const size_t sb = (size_t)(uint32_t)h.slot * sizeof(PtShade);
                        const f32x4 s0 = ldg4(P.shade, sb), s1 = ldg4(P.shade, sb + 16), s2 = ldg4(P.shade, sb + 32);
                        const AoSurface s = ao_surface(h.u, h.v, V(a.x, a.y, a.z), V(a.w, b.x, b.y), V(b.z, b.w, c.x), V(s0.x, s0.y, s0.z), V(s0.w, s1.x, s1.y),
                                                       V(s1.z, s1.w, s2.x), d, A.flags);
                        first_hit = (f32x4){h.t, h.u, h.v, __int_as_float(h.id)};
                        nf = s.nf;
                        if (s.traced) {
                            o = s.p;
                            rng = rng_init((uint32_t)ray, A.seed);
                            clear = 0;
                            k = 0;
                            retire = false;
                        }
                    }
                } else if (k >= 0) {
                    clear += h.slot < 0 ? 1 : 0;
                    ++k;
                    retire = k == A.n_rays;
                    ao = ao_value(clear, A.n_rays);
                } else { // AO_OVERRUN: a miss
                    first_hit = (f32x4){0.0f, 0.0f, 0.0f, __int_as_float(-1)};
                    nf = vs(0.0f);
                }
                if (retire) {
                    f32x4 PT_AS1* y = (f32x4 PT_AS1*)((char PT_AS1*)A.r.out + (size_t)(uint32_t)ray * 32);
                    y[0] = first_hit;
                    y[1] = (f32x4){nf.x, nf.y, nf.z, ao};
                    ray = -1;
                } else { // occlusion ray k
                    d = ao_direction(nf, rng);
                    inv = ray_inv(d);
                    hit_reset(h, A.thi);
                    cur = P.root; sp = 0; steps = 0;
                }
            }
        }
    }
}

static const void* ao_instance(int exact) { return exact ? (const void*)PT_AO_KERNEL<true> : (const void*)PT_AO_KERNEL<false>; }

extern "C" hipError_t PT_AO_GEOMETRY(int exact, PtGeometry* g)
{
    return pt_wave_geometry(g, PT_LDS_STACK, 0, ao_instance(exact));
}

extern "C" hipError_t PT_AO_LAUNCH(const PtKernelParams* p, const PtAoArgs* a, int grid, size_t lds_bytes, hipStream_t stream)
{
    if (!pt_ray_ranges_ok(grid, a->r)) return hipErrorInvalidValue;
    if (a->n_rays < 1 || a->n_rays > 4096 || (a->flags & ~kAoShadingNormal) != 0 || !(a->thi > 0.0f && a->thi <= kTMax)) return hipErrorInvalidValue;
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel(ao_instance(p->box_exact), dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
