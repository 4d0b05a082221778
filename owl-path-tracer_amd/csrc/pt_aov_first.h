// pt_aov_first.h -- guide pass (pt_render_aov, include/mi355pt.h): first-hit albedo, shading normal, depth and coverage
//
// pt_kernel_aov.hip and, with PT_WATERTIGHT = 1, pt_kernel_aov_wt.hip include this header (`make asm-aov` prints both reports).
// One pixel per lane, one wave per workgroup, n_samples camera rays per pixel, each walked to its closest hit and no further.
// Like the probes the kernel owns no traversal or shading arithmetic: the ray is gen_camera_ray's, the walk is ray_inv -> node4_step<PT_WAVE,
// PT_LDS_STACK> (short LDS stack, deeper levels in the wave's HBM columns) -> leaf_test, stepped by quad_walk_step (pt_trace.h), and what a
// sample contributes comes from the records, the material row and the texture that shade_hit reads, through the same functions.
// The lanes of a wave take an 8 x 8 block of pixels (four per 16-pixel shard tile; pt_shard_pixels deals tiles whose side is a multiple
// of 8, so a block has one owner and a wave that does not own its block has nothing to do): the primary rays of a wave stay together
// through the upper node steps.  BINARY (no quad nodes: option quad = 0 or a tree too deep for them): closest_hit of pt_trace.h, whole
// stack in LDS, Moeller-Trumbore only - the watertight build has no such instance.
// No batch form: pt_render_aov_batch runs the follow kernels (max_follow = 0 gives the first-hit guides).
#pragma once
#include "pt_aov.h"
#if PT_WATERTIGHT
#define PT_AOV_KERNEL pt_aov_wt_kernel
#define PT_AOV_LAUNCH pt_launch_aov_wt
#define PT_AOV_GEOMETRY pt_aov_geometry_wt
#else
#define PT_AOV_KERNEL pt_aov_kernel
#define PT_AOV_LAUNCH pt_launch_aov
#define PT_AOV_GEOMETRY pt_aov_geometry
#endif

template <bool BINARY, bool EXACT>
__global__ void __launch_bounds__(PT_WAVE, PT_AOV_WAVES_PER_EU) PT_AOV_KERNEL(const PtKernelParams P, const PtAovArgs A)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int lane = threadIdx.x;
    uint32_t* stack = lds + lane; // stack[level * 64 + lane]
    const int ovf_levels = A.cap > PT_LDS_STACK ? A.cap - PT_LDS_STACK : 0;
    uint32_t PT_AS1* ovf = gp(A.ovf) + (size_t)blockIdx.x * ((size_t)ovf_levels * PT_WAVE) + lane;
    const PtNode4* __restrict__ nodes4 = P.nodes4;
    const PtTri* __restrict__ tris = P.tris;
    const int nbx = (P.width + 7) >> 3, nby = (P.height + 7) >> 3;
    const float inv_n = 1.0f / (float)A.n_samples;
    for (int b = blockIdx.x; b < nbx * nby; b += gridDim.x) {
        const int bx = b % nbx, by = b / nbx;
        if (((bx * 8) / A.tile + (by * 8) / A.tile) % A.world != A.rank) continue; // another rank's tile (wave-uniform)
        const int px = bx * 8 + (lane & 7), py = by * 8 + (lane >> 3);
        if (px >= P.width || py >= P.height) continue; // the block sticks out of the frame
        PathState ps;
        ps.rng = rng_init((uint32_t)px, (uint32_t)py); // the beauty frame's stream: sample 0 is its first camera ray of this pixel
        v3 s_alb = vs(0.0f), s_nrm = vs(0.0f);
        float s_alpha = 0.0f, s_depth = 0.0f;
        for (int k = 0; k < A.n_samples; ++k) {
            gen_camera_ray(P, px, py, ps); // two draws; nothing else of this pass draws from the stream
            const v3 o = ps.org, d = ps.dir;
            Hit h;
            hit_reset(h, kTMax);
#if !PT_WATERTIGHT
            if (BINARY) {
                Counters cn;
                closest_hit<false, PT_WAVE>(P, stack, o, d, h, cn);
            } else
#endif
            {
                const v3 inv = ray_inv(d);
                int cur = P.root, sp = 0, steps = 0;
                // (a walk out of its bounds ends here too, with the best hit so far: quad_walk_step)
                while (cur != PT_DONE) quad_walk_step<PT_LDS_STACK>(P, nodes4, tris, stack, ovf, A.cap, o, d, inv, h, cur, sp, steps, EXACT, false);
            }
            v3 alb, nrm;
            float alpha, depth;
            aov_sample(P, h.slot, h.u, h.v, h.t, d, alb, alpha, nrm, depth);
            s_alb = s_alb + alb; s_alpha = s_alpha + alpha; // float32, in sample order
            s_nrm = s_nrm + nrm; s_depth = s_depth + depth;
        }
        const size_t ofs = (size_t)px + (size_t)P.width * (size_t)(P.height - 1 - py); // as out_rgb
        f32x4 PT_AS1* y = (f32x4 PT_AS1*)(gp(A.out) + 8 * ofs);                        // two 16-byte stores
        y[0] = (f32x4){s_alb.x * inv_n, s_alb.y * inv_n, s_alb.z * inv_n, s_alpha * inv_n};
        y[1] = (f32x4){s_nrm.x * inv_n, s_nrm.y * inv_n, s_nrm.z * inv_n, s_depth * inv_n};
    }
}

// The instance that serves (binary, exact), for the geometry function and the launcher alike; nullptr: no such instance.
static const void* aov_instance(int binary, int exact)
{
#if PT_WATERTIGHT
    if (binary) return nullptr; // the binary walk has no watertight test
#else
    if (binary) return (const void*)PT_AOV_KERNEL<true, false>;
#endif
    return exact ? (const void*)PT_AOV_KERNEL<false, true> : (const void*)PT_AOV_KERNEL<false, false>;
}

extern "C" hipError_t PT_AOV_GEOMETRY(int binary, int exact, int stack_entries, PtGeometry* g)
{
    const void* fn = aov_instance(binary, exact);
    if (!fn) return hipErrorInvalidValue;
    return pt_wave_geometry(g, binary ? stack_entries : PT_LDS_STACK, 0, fn);
}

extern "C" hipError_t PT_AOV_LAUNCH(const PtKernelParams* p, const PtAovArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream)
{
    if (grid < 1) grid = 1;
    const void* fn = aov_instance(binary, p->box_exact);
    if (!fn) return hipErrorInvalidValue;
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel(fn, dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
