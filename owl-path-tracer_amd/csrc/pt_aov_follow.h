// pt_aov_follow.h -- guide pass, follow mode (pt_render_aov_follow, include/mi355pt.h): the guide ray passes mirrors and glass
//
// Translation units of their own again - pt_kernel_aov_follow.hip and pt_kernel_aov_follow_wt.hip include this header - so
// that `make asm-aov` goes on listing the five first-hit kernels and nothing else.  The frame loop, the pixel blocks, the walk (quad_walk_step, pt_trace.h) and
// every fetch are the first-hit kernel's; what is new is the loop around the walk: a hit on a surface that classifies MIRROR or GLASS
// (aov_classify) sends the ray on from shade_hit's hit point with reflect / refract of pt_device.h, and the tint and the path length
// travel with it.  The loop draws nothing from the stream.
// Registers.  The first-hit instances sit at 119..128 of the 128 VGPRs of four waves per SIMD, and the follow loop adds state that
// lives across the walk: tint (3), path length, and an origin that now differs per lane (3).  The eight per-pixel sums are needed only
// BETWEEN samples, so they live in LDS across the walks - acc[field * 64 + lane] behind the wave's stack, conflict-free like the stack -
// and so do the tint and the path length, which are needed only between two walks of a sample, and the RNG state and the pixel, needed
// only between samples, and the lane's place in its 8 x 8 block: 15 words per lane, 3.75 KB per wave (16 waves per CU: 108 KB of 160 KB together with the stacks).  The accesses
// are volatile: the compiler must not promote the parked words back into registers across the walk (it did, and spilled them to scratch).
// No scratch, 128 VGPRs at the most (`make asm-aov-follow`).
// BATCH BUILD (pt_kernel_aov_follow_batch.hip: PT_BATCH = 1; pt_render_aov_batch).  The same kernel as pt_aov_follow_batch_kernel
// over the 8 x 8 blocks of K frames, frame by frame: a wave's block lies in one frame, so the frame's camera (P.batch_cams) and material
// table (P.materials + frame * n_materials * PT_MAT_STRIDE) are wave-uniform - scalar loads, no per-lane gather as in the render batch -
// and frame f is stored W * H pixels behind frame f - 1.  With PT_BATCH = 0 the preprocessor removes all of it (`make asm-aov-follow-batch`).
// RAY IMAGE BUILD (pt_kernel_aov_rays.hip, pt_kernel_aov_rays_wt.hip: PT_RAYGEN = 1; pt_render_aov_rays).  The same kernel as
// pt_aov_rays_kernel / pt_aov_rays_wt_kernel, quad walk only: a sample starts on the pixel's ray record of the caller's table
// (gen_ray_from, pt_trace.h: a 64-bit per-lane address and four 16-byte loads; the table pointer travels in P.batch_cams, batch_frames
// stays 0) instead of the camera's ray, which is the whole difference.  The gather sits in the sample prologue, between two walks, where
// sums, tint, RNG state and pixel are parked: 118 / 124 / 127 / 128 VGPRs, no scratch (`make asm-aov-rays`).  With PT_RAYGEN = 0 the
// preprocessor removes all of it.
#pragma once
#include "pt_aov.h"
#ifndef PT_BATCH
#define PT_BATCH 0
#endif
#ifndef PT_RAYGEN
#define PT_RAYGEN 0 // 1: pt_kernel_aov_rays.hip / pt_kernel_aov_rays_wt.hip - the camera replaced by a per-pixel ray record (pt_render_aov_rays, "RAY IMAGE BUILD" above)
#endif
#if PT_WATERTIGHT && PT_BATCH
#error "batches have no watertight instances"
#endif
#if PT_RAYGEN && PT_BATCH
#error "batches have no ray-image instances"
#endif
#if PT_RAYGEN && PT_WATERTIGHT
#define PT_AOV_FOLLOW_KERNEL pt_aov_rays_wt_kernel
#define PT_AOV_FOLLOW_LAUNCH pt_launch_aov_rays_wt
#define PT_AOV_FOLLOW_GEOMETRY pt_aov_rays_geometry_wt
#elif PT_RAYGEN
#define PT_AOV_FOLLOW_KERNEL pt_aov_rays_kernel
#define PT_AOV_FOLLOW_LAUNCH pt_launch_aov_rays
#define PT_AOV_FOLLOW_GEOMETRY pt_aov_rays_geometry
#elif PT_WATERTIGHT
#define PT_AOV_FOLLOW_KERNEL pt_aov_follow_wt_kernel
#define PT_AOV_FOLLOW_LAUNCH pt_launch_aov_follow_wt
#define PT_AOV_FOLLOW_GEOMETRY pt_aov_follow_geometry_wt
#elif PT_BATCH
#define PT_AOV_FOLLOW_KERNEL pt_aov_follow_batch_kernel
#define PT_AOV_FOLLOW_LAUNCH pt_launch_aov_follow_batch
#define PT_AOV_FOLLOW_GEOMETRY pt_aov_follow_batch_geometry
#else
#define PT_AOV_FOLLOW_KERNEL pt_aov_follow_kernel
#define PT_AOV_FOLLOW_LAUNCH pt_launch_aov_follow
#define PT_AOV_FOLLOW_GEOMETRY pt_aov_follow_geometry
#endif
#define PT_AS3 __attribute__((address_space(3)))
#define PT_AOV_PARK 15 // LDS words per lane behind the stack: 8 sums, tint r g b, path length, RNG state, px | py << 16, the lane's place in its block
enum { AOV_NONE = 0, AOV_MIRROR = 1, AOV_GLASS = 2 };
namespace {
// Which lobe a guide ray follows: the lobe weights are sample_disney's own expressions (pt_device.h); a NaN field fails every comparison
__device__ __forceinline__ int aov_classify(const Material& m, float roughness_max)
{
    const float dw = (1.0f - m.specular_transmission) * (1.0f - m.metallic);
    const float mw = m.metallic;
    const float cw = 0.25f * m.clearcoat;
    const float gw = (1.0f - m.metallic) * m.specular_transmission;
    if (mw > gw && mw > dw && mw > cw && m.roughness <= roughness_max) return AOV_MIRROR;
    if (gw > mw && gw > dw && gw > cw && m.specular_transmission_roughness <= roughness_max) return AOV_GLASS;
    return AOV_NONE;
}

// One surface of a guide ray (o, d) whose walk ended in h.  Returns true if the ray goes on: o, d, tint updated, dist advanced.  Otherwise
// the sample's contribution is complete: albedo, normal, depth set.  The miss branch is aov_sample's; the fetches are its expressions.
#if PT_BATCH
// (batch instances: mats = the material table of the block's frame, wave-uniform; everything else as below)
__device__ __forceinline__ bool aov_follow_surface(const PtKernelParams& P, const float* mats, const PtAovFollowArgs& F, const Hit& h, int step, v3& o, v3& d, v3& tint,
                                                   float& dist, v3& albedo, v3& normal, float& depth)
#else
__device__ __forceinline__ bool aov_follow_surface(const PtKernelParams& P, const PtAovFollowArgs& F, const Hit& h, int step, v3& o, v3& d, v3& tint, float& dist,
                                                   v3& albedo, v3& normal, float& depth)
#endif
{
    if (h.slot < 0) { // aov_sample's miss branch, expression for expression
        v3 radiance = vs(0.0f);
        if (P.env_use_map && P.env_map.width > 0) {
            float tu, tv;
            uv_on_sphere(d, tu, tv);
            radiance = radiance + tex_nearest(gp(P.env_map.texels), P.env_map.width, P.env_map.height, tu, tv);
        } else if (P.env_use_auto) {
            radiance = radiance + lerp3(vs(1.0f), V(0.5f, 0.7f, 1.0f), 0.5f * (d.y + 1.0f));
        } else {
            // the colour passes an empty asm so that 0 + colour is formed here: hoisted out of the frame loop the three wave-uniform sums
            // sit in VGPRs across every walk, which is what tips the tightest instance into scratch
            float cr = P.env_color[0], cg = P.env_color[1], cb = P.env_color[2];
            asm volatile("" : "+s"(cr), "+s"(cg), "+s"(cb));
            radiance = radiance + V(cr, cg, cb);
        }
        albedo = tint * (radiance * P.env_intensity);
        normal = vs(0.0f);
        depth = dist;
        return false;
    }
    dist = dist + h.t; // float32, in step order
    const size_t tb = (size_t)(uint32_t)h.slot * sizeof(PtTri);
    const f32x4 c = ldg4(P.tris, tb + 32); // {p2.z, id, material, pad}
    const size_t sb = (size_t)(uint32_t)h.slot * sizeof(PtShade);
    const f32x4 s0 = ldg4(P.shade, sb), s1 = ldg4(P.shade, sb + 16), s2 = ldg4(P.shade, sb + 32), s3 = ldg4(P.shade, sb + 48);
    const int mi = __float_as_int(c.z);
    Material mat = material_default();
    int tex_slot = -1;
    if (mi >= 0) {
#if PT_BATCH
        const float PT_AS1* mp = gp(mats) + mi * PT_MAT_STRIDE;
#else
        const float PT_AS1* mp = gp(P.materials) + mi * PT_MAT_STRIDE;
#endif
        mat = material_load(mp);
        tex_slot = __float_as_int(mp[17]);
    }
    const float bx = h.u, by = h.v;
    const float bw = 1.0f - bx - by;
    const v3 v_n = normalize(interp3(bw, bx, by, V(s0.x, s0.y, s0.z), V(s0.w, s1.x, s1.y), V(s1.z, s1.w, s2.x)));
    const bool n_ok = finite_(v_n.x) && finite_(v_n.y) && finite_(v_n.z);
    const bool emits = mat.emission > 0.0f;
    if (!emits && tex_slot >= 0) {
        const float tu = fma_(by, s3.z, fma_(bx, s3.x, bw * s2.z));
        const float tv = fma_(by, s3.w, fma_(bx, s3.y, bw * s2.w));
        const PtTexDesc PT_AS1* tdp = gp(P.textures) + tex_slot;
        mat.base_color = tex_nearest(gp(tdp->texels), tdp->width, tdp->height, tu, tv);
    }
    const int kind = (emits || step == F.max_follow || !n_ok) ? (int)AOV_NONE : aov_classify(mat, F.roughness_max);
    if (kind != AOV_NONE) {
        const v3 wo = -d;
        v3 wi, t2 = tint * mat.base_color;
        bool through = false;
        if (kind == AOV_GLASS) {
            const float ct = dot(wo, v_n);
            through = ct > 0.0f ? refract(wo, v_n, 1.0f / mat.ior, wi) : refract(wo, -v_n, mat.ior, wi);
        }
        if (through) t2 = tint * V(sqrt_(mat.base_color.x), sqrt_(mat.base_color.y), sqrt_(mat.base_color.z));
        else wi = reflect(wo, v_n); // a mirror, or total internal reflection
        const v3 dn = normalize(wi);
        if (finite_(dn.x) && finite_(dn.y) && finite_(dn.z)) {
            const f32x4 a = ldg4(P.tris, tb), b = ldg4(P.tris, tb + 16);
            o = interp3(bw, bx, by, V(a.x, a.y, a.z), V(a.w, b.x, b.y), V(b.z, b.w, c.x)); // shade_hit's v_p: no normal offset
            d = dn;
            tint = t2;
            return true;
        }
    }
    albedo = tint * (emits ? vs(mat.emission) : mat.base_color);
    normal = n_ok ? v_n : vs(0.0f);
    depth = dist;
    return false;
}
} // namespace

template <bool BINARY, bool EXACT>
__global__ void __launch_bounds__(PT_WAVE, PT_AOV_WAVES_PER_EU) PT_AOV_FOLLOW_KERNEL(const PtKernelParams P, const PtAovFollowArgs F)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const PtAovArgs& A = F.a;
    const int lane = threadIdx.x;
    uint32_t* stack = lds + lane; // stack[level * 64 + lane]
    // park[field * 64 + lane]: 0..7 the sums, 8..10 tint, 11 path length; 12 RNG state, 13 pixel, 14 place in the block (LDS address space spelled out: ds_read / ds_write)
    volatile float PT_AS3* park = (volatile float PT_AS3*)(lds + P.lds_levels * PT_WAVE + lane);
    volatile uint32_t PT_AS3* parku = (volatile uint32_t PT_AS3*)park;
    const int ovf_levels = A.cap > PT_LDS_STACK ? A.cap - PT_LDS_STACK : 0;
    uint32_t PT_AS1* ovf = gp(A.ovf) + (size_t)blockIdx.x * ((size_t)ovf_levels * PT_WAVE) + lane;
    const PtNode4* __restrict__ nodes4 = P.nodes4;
    const PtTri* __restrict__ tris = P.tris;
    const int nbx = (P.width + 7) >> 3, nby = (P.height + 7) >> 3;
    parku[14 * PT_WAVE] = (uint32_t)(lane & 7) | ((uint32_t)(lane >> 3) << 16);
#if PT_BATCH
    // K * nbx * nby blocks, frame by frame: a block belongs to ONE frame whatever the height, so the frame, its camera and its material
    // table are wave-uniform.  bf: the block inside its frame - shard, pixels and RNG stream are the single frame's.
    const int nb = nbx * nby;
    for (int bb = blockIdx.x; bb < P.batch_frames * nb; bb += gridDim.x) {
        const int frame = bb / nb, b = bb - frame * nb;
        const int bx = b % nbx, by = b / nbx;
#else
    for (int b = blockIdx.x; b < nbx * nby; b += gridDim.x) {
        const int bx = b % nbx, by = b / nbx;
#endif
        if (((bx * 8) / A.tile + (by * 8) / A.tile) % A.world != A.rank) continue; // another rank's tile (wave-uniform)
        const uint32_t in_block = parku[14 * PT_WAVE];
        const int px = bx * 8 + (int)(in_block & 0xffffu), py = by * 8 + (int)(in_block >> 16);
        if (px >= P.width || py >= P.height) continue; // the block sticks out of the frame
#pragma unroll
        for (int i = 0; i < 8; ++i) park[i * PT_WAVE] = 0.0f;
        parku[12 * PT_WAVE] = rng_init((uint32_t)px, (uint32_t)py);
        parku[13 * PT_WAVE] = (uint32_t)px | ((uint32_t)py << 16); // both below 65536
        for (int k = 0; k < A.n_samples; ++k) {
            PathState ps;
            ps.rng = parku[12 * PT_WAVE];
            const uint32_t pxy = parku[13 * PT_WAVE];
#if PT_BATCH
            gen_camera_ray_from(P, gp(P.batch_cams) + 12 * frame, (int)(pxy & 0xffffu), (int)(pxy >> 16), ps);
#elif PT_RAYGEN
            gen_ray_from(P, gp(P.batch_cams), (int)(pxy & 0xffffu), (int)(pxy >> 16), ps); // the pixel's own ray record: a per-lane gather from the table in HBM
#else
            gen_camera_ray(P, (int)(pxy & 0xffffu), (int)(pxy >> 16), ps); // two draws; the follow loop draws nothing
#endif
            parku[12 * PT_WAVE] = ps.rng;
            v3 o = ps.org, d = ps.dir;
            park[8 * PT_WAVE] = 1.0f; park[9 * PT_WAVE] = 1.0f; park[10 * PT_WAVE] = 1.0f; park[11 * PT_WAVE] = 0.0f;
            v3 alb, nrm;
            float depth;
            for (int step = 0;; ++step) {
                Hit h;
                hit_reset(h, kTMax);
#if !PT_WATERTIGHT && !PT_RAYGEN
                if (BINARY) {
                    Counters cn;
                    closest_hit<false, PT_WAVE>(P, stack, o, d, h, cn);
                } else
#endif
                {
                    const v3 inv = ray_inv(d);
                    int cur = P.root, sp = 0, steps = 0;
                    // the first-hit kernel's walk (a walk out of its bounds ends here too, with the best hit so far: quad_walk_step)
                    while (cur != PT_DONE) quad_walk_step<PT_LDS_STACK>(P, nodes4, tris, stack, ovf, A.cap, o, d, inv, h, cur, sp, steps, EXACT, false);
                }
                if (step == 0 && h.slot >= 0) park[3 * PT_WAVE] = park[3 * PT_WAVE] + 1.0f; // coverage stays first-hit
                v3 tint = V(park[8 * PT_WAVE], park[9 * PT_WAVE], park[10 * PT_WAVE]);
                float dist = park[11 * PT_WAVE];
#if PT_BATCH
                if (!aov_follow_surface(P, P.materials + (size_t)frame * (size_t)(P.n_materials * PT_MAT_STRIDE), F, h, step, o, d, tint, dist, alb, nrm, depth)) break;
#else
                if (!aov_follow_surface(P, F, h, step, o, d, tint, dist, alb, nrm, depth)) break;
#endif
                park[8 * PT_WAVE] = tint.x; park[9 * PT_WAVE] = tint.y; park[10 * PT_WAVE] = tint.z; park[11 * PT_WAVE] = dist;
            }
            // float32, in sample order
            park[0 * PT_WAVE] = park[0 * PT_WAVE] + alb.x; park[1 * PT_WAVE] = park[1 * PT_WAVE] + alb.y; park[2 * PT_WAVE] = park[2 * PT_WAVE] + alb.z;
            park[4 * PT_WAVE] = park[4 * PT_WAVE] + nrm.x; park[5 * PT_WAVE] = park[5 * PT_WAVE] + nrm.y; park[6 * PT_WAVE] = park[6 * PT_WAVE] + nrm.z;
            park[7 * PT_WAVE] = park[7 * PT_WAVE] + depth;
        }
        const uint32_t pxy = parku[13 * PT_WAVE];
#if PT_BATCH
        const size_t ofs = (size_t)frame * ((size_t)P.width * (size_t)P.height) + (size_t)(pxy & 0xffffu) + (size_t)P.width * (size_t)(P.height - 1 - (int)(pxy >> 16));
#else
        const size_t ofs = (size_t)(pxy & 0xffffu) + (size_t)P.width * (size_t)(P.height - 1 - (int)(pxy >> 16)); // as out_rgb
#endif
        f32x4 PT_AS1* y = (f32x4 PT_AS1*)(gp(A.out) + 8 * ofs);                        // two 16-byte stores
        y[0] = (f32x4){park[0 * PT_WAVE] * F.inv_n, park[1 * PT_WAVE] * F.inv_n, park[2 * PT_WAVE] * F.inv_n, park[3 * PT_WAVE] * F.inv_n};
        y[1] = (f32x4){park[4 * PT_WAVE] * F.inv_n, park[5 * PT_WAVE] * F.inv_n, park[6 * PT_WAVE] * F.inv_n, park[7 * PT_WAVE] * F.inv_n};
    }
}

// The instance that serves (binary, exact), for the geometry function and the launcher alike; nullptr: no such instance.
static const void* aov_follow_instance(int binary, int exact)
{
#if PT_WATERTIGHT || PT_RAYGEN
    if (binary) return nullptr; // the binary walk has no watertight test, and no ray-image instance
#else
    if (binary) return (const void*)PT_AOV_FOLLOW_KERNEL<true, false>;
#endif
    return exact ? (const void*)PT_AOV_FOLLOW_KERNEL<false, true> : (const void*)PT_AOV_FOLLOW_KERNEL<false, false>;
}

extern "C" hipError_t PT_AOV_FOLLOW_GEOMETRY(int binary, int exact, int stack_entries, PtGeometry* g)
{
    const void* fn = aov_follow_instance(binary, exact);
    if (!fn) return hipErrorInvalidValue;
    return pt_wave_geometry(g, binary ? stack_entries : PT_LDS_STACK, PT_AOV_PARK, fn); // the stack, then the parked state
}

extern "C" hipError_t PT_AOV_FOLLOW_LAUNCH(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream)
{
    if (grid < 1) grid = 1;
#if PT_BATCH
    if (p->batch_frames < 1 || p->batch_cams == nullptr) return hipErrorInvalidValue; // (pt_launch_aov_follow_batch: frames, cameras and tables as pt_launch_render_batch)
#endif
#if PT_RAYGEN
    if (p->batch_frames != 0 || p->batch_cams == nullptr) return hipErrorInvalidValue; // (pt_launch_aov_rays*: the table in the batch cameras' place, as pt_launch_render_rayimage)
#endif
    const void* fn = aov_follow_instance(binary, p->box_exact);
    if (!fn) return hipErrorInvalidValue;
    void* args[] = {(void*)p, (void*)a};
    (void)hipLaunchKernel(fn, dim3(grid), dim3(PT_WAVE), args, lds_bytes, stream);
    return hipGetLastError();
}
