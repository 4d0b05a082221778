// pt_launch.h -- prototypes of the kernel launchers (defined in the .hip units: pt_kernel.hip, the family headers it names, pt_lbvh.hip, ...; stubbed in pt_nogpu_stubs.cpp for the
// host-side sanitizer build) as pt_scene.cpp / pt_render.cpp / pt_guides.cpp / pt_debug.cpp / pt_comm.cpp call them.  ONE declaration for definition, stub and caller: the functions
// have C linkage, so a mismatched parameter list would link and then misbehave (round-3 advisor finding).
// The same holds inside a family: its *_geometry function (what the host sizes LDS and overflow columns from, and reports in pt_stats)
// and its launcher (what the GPU runs) must mean the same kernel instance, and nothing at link time says so.  Each walking family
// therefore has ONE function that maps the selector arguments to the instance, and both ask it; what every *_geometry function asks the
// runtime about that instance - registers, occupancy, and the refusal of one that spills - is pt_instance.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pt_types.h"

// Launch geometry of one render instance (pt_kernel_geometry)
struct PtGeometry {
    int block;              // threads per workgroup
    int ns;                 // pixels a workgroup keeps in flight (wavefront kernel: path slots per wave)
    size_t lds_bytes;       // dynamic LDS per workgroup
    int lds_levels;         // stack levels kept in LDS (PtKernelParams::lds_levels)
    size_t state_words;     // global slot-state words per workgroup (0: none)
    int vgprs;
    int max_blocks_per_cu;  // occupancy at lds_bytes
};

// Ray probes of pt_debug_eval (pt_probes.h): op = PT_PROBE_QUAD / PT_PROBE_QUAD_OVF / PT_PROBE_GROUP + slab form (0: fma, 1: subtracting).
// in: o[3], d[3] per ray; out: PT_PROBE_OUT floats per ray (layout in include/mi355pt.h).
enum { PT_PROBE_FIRST = 30, PT_PROBE_QUAD = 30, PT_PROBE_QUAD_OVF = 32, PT_PROBE_GROUP = 34, PT_PROBE_LAST = 35 };
#define PT_PROBE_OUT 6
#define PT_DEBUG_OP_CLOSEST_HIT 21 // the validation kernel's closest-hit op (PT_OP_CLOSEST_HIT, pt_kernel_aux.hip): Moeller-Trumbore only
#define PT_PROBE_GROUP_SLOTS 24 // path slots of a wave of the group probe: three rays per group, so groups park and resume
#define PT_PROBE_GROUP_RAYS 100 // rays per wave of the group probe: neither a multiple of 8 nor of 64

// pt_refit.hip: the device side of pt_update_vertices.  Device pointers except level_ofs (host: n_levels + 1 offsets into level_nodes).
#define PT_REFIT_PARTIALS 1024 // blocks of the first stage of the extent reduction, at most
struct PtRefitArgs {
    PtNode* nodes;
    PtNode4* nodes4;
    PtNode8* nodes8;
    PtTri* tris;
    PtShade* shade;
    const float* verts;           // the concatenated vertex arrays of the meshes
    const float* normals;         // the concatenated normal arrays; null: the shading records keep their normals
    const int32_t* tri_vi;        // 4 per leaf-order slot (PtRefit::tri_vi, pt_bvh.h)
    const int32_t* level_nodes;   // binary nodes sorted by height
    const int32_t* src4;          // per quad slot: 2 * node + side of the binary box it copies, -1 empty
    const int32_t* src8;          // per oct slot
    float* ws;                    // pt_refit_workspace_bytes(): [0] = pad, [1] = collapsed slivers (uint32) once the launches have run
    const int32_t* level_ofs;
    int32_t n_slots, n_levels, n_slots4, n_slots8;
};

// Guide pass (pt_render_aov; pt_aov_first.h): what the guide kernels take beside the scene and the camera in PtKernelParams.
struct PtAovArgs {
    float* out;        // W*H*8 floats, cleared by the caller: {albedo r, g, b, alpha, normal x, y, z, depth} per pixel, framebuffer order
    uint32_t* ovf;     // quad walk: the waves' HBM stack columns, (cap - PT_LDS_STACK) * 64 words per workgroup (none when cap <= PT_LDS_STACK)
    int32_t n_samples;
    int32_t cap;       // quad walk: stack levels a lane may use (stack bound + the three pushes of a step)
    int32_t rank, world, tile; // pixel shard (pt_shard_pixels: tile a multiple of 8, tile (tx, ty) belongs to rank (tx + ty) % world)
    int32_t pad;
};
// Follow mode of the guide pass (pt_render_aov_follow; pt_aov_follow.h): the first-hit pass's arguments and pt_aov_params
struct PtAovFollowArgs {
    PtAovArgs a;
    int32_t max_follow;  // 0..8 specular surfaces a guide ray may pass
    float roughness_max; // a surface rougher than this is not followed
    float inv_n;         // 1.0f / (float)n_samples, formed on the host (IEEE division, the first-hit kernel's value): a wave-uniform float costs a VGPR
    int32_t pad;
};

// Ray queries (pt_trace_closest, pt_trace_occluded; pt_rays_kernels.h): what the ray kernels take beside the scene in PtKernelParams.
struct PtRaysArgs {
    const void* rays;  // n pt_ray records (include/mi355pt.h: org, tmax, dir, one float that is not read), 16-byte aligned
    void* out;         // closest: n pt_ray_hit {t, u, v, prim}, 16-byte aligned; occluded: n bytes; surface: n pt_surface (80 bytes), 16-byte aligned
    uint32_t* ovf;     // the waves' HBM stack columns, (cap - PT_LDS_STACK) * 64 words per workgroup (none when cap <= PT_LDS_STACK)
    int32_t n;         // rays (< 2^31)
    int32_t per_wave;  // rays of a workgroup's range, a multiple of 64: workgroup b owns [b * per_wave, min(n, (b + 1) * per_wave))
    int32_t cap;       // stack levels a lane may use (stack bound + the three pushes of a step)
    int32_t refill;    // option "rays_refill", 0..63: idle lanes take new rays when at most this many lanes are still walking
};
// Ambient occlusion (pt_trace_ao; pt_ao.h): the ray kernels' arguments (r.out: n pt_ao_hit of 32 bytes, 16-byte aligned) and pt_ao_params
struct PtAoArgs {
    PtRaysArgs r;
    int32_t n_rays;    // K, 1..4096 occlusion rays per hit
    int32_t flags;     // PT_AO_SHADING_NORMAL
    float thi;         // the occlusion rays' bound: radius < 1e10f ? radius : 1e10f, formed on the host
    uint32_t seed;     // second word of rng_init(ray index, seed)
};
// The first K hits (pt_trace_hits; pt_hits.h): the ray kernels' arguments (r.out: n * k pt_ray_hit, 16-byte aligned) and K
#define PT_HITS_K_MAX 16 // PT_HITS_MAX of include/mi355pt.h
struct PtHitsArgs {
    PtRaysArgs r;
    int32_t k;         // K, 1..PT_HITS_K_MAX records per ray
    int32_t pad[3];
};

// Denoiser (pt_denoise; pt_denoise.hip): what its three kernels take.  The host fills everything but the record pointers, which
// pt_launch_denoise carves out of ws; the constants are include/mi355pt.h's "host constants" (pti::denoise_constants).
struct PtDenoiseArgs {
    const float* rgb;       // W*H*3 floats, framebuffer order (may equal out_rgb)
    const float* aov;       // W*H*8 floats of the guide pass, 16-byte aligned
    float* out_rgb;         // W*H*3 floats
    uint32_t* out_rgba8;    // W*H, or null
    void* ws;               // pt_denoise_workspace_bytes(W, H), 16-byte aligned
    float4* col[2];         // colour r g b + kz, ping-pong
    float4* nz;             // normal x y z + depth
    float4* alb;            // albedo r g b
    int32_t width, height, iterations, flags;
    float sigma_depth, kn, ka, pad;
    float kc[8];            // per iteration
};

// Variance-guided denoiser (pt_denoise_var, pt_accum_denoise; pt_denoise_var.hip): what its prepare, iteration and finish kernels take.
// As PtDenoiseArgs; the colour record carries the summed variance v instead of kz, which moves to the albedo record.
struct PtDenoiseVarArgs {
    const float* rgb;       // W*H*3 floats, framebuffer order (may equal out_rgb)
    const float* var;       // W*H*3 floats: per-channel variance of rgb
    const float* aov;       // W*H*8 floats of the guide pass, 16-byte aligned
    float* out_rgb;         // W*H*3 floats
    uint32_t* out_rgba8;    // W*H, or null
    void* ws;               // pt_denoise_var_workspace_bytes(W, H), 16-byte aligned
    float4* col[2];         // colour r g b + v, ping-pong
    float4* nz;             // normal x y z + depth
    float4* alb;            // albedo r g b + kz
    int32_t width, height, iterations, flags;
    float sigma_depth, kn, ka, s2; // s2 = sigma_color^2 (+infinity: no colour term)
};
// ... and its variance kernel over an accumulation's state (arrays by launch id x + W * y, as PtAccumArgs): out_var in framebuffer order.
struct PtAccumVarArgs {
    const float* sum;
    const float* half;
    const uint32_t* n;
    const uint32_t* n_half;
    const uint8_t* owned;
    float* out_var;          // W*H*3
    uint32_t n_frame;        // W*H
    int32_t width, height, pad;
};

// Progressive accumulation (pt_accum_*; pt_accum.hip): what its two kernels take.  Every per-pixel array is indexed by the launch id
// x + W * y (the render kernel's index into rng_state / accum) except the two images, which are in framebuffer order.
struct PtAccumArgs {
    const float* sum;        // W*H*3: the render kernel's accum
    float* seen;             // W*H*3: sum as of the pixel's last resolve
    float* half;             // W*H*3: the samples of every second pass
    uint32_t* n;             // samples, samples in half, passes
    uint32_t* n_half;
    uint32_t* passes;
    float* noise;            // W*H
    const uint8_t* owned;    // 1: a pixel of this context's shard
    const uint8_t* active;   // 1: took part in this add (select's flags); not read with all_active
    float* out_rgb;          // W*H*3
    uint32_t* out_rgba8;     // W*H
    uint32_t n_frame;        // W*H
    int32_t width, height, n_samples, all_active;
};
struct PtAccumSelectArgs {
    const uint32_t* queue;   // the shard's pixel queue
    const float* noise;
    const uint32_t* n;
    uint8_t* active;         // by id, written for every queue entry
    uint32_t* ids_out;       // n_queue entries: the active ids, compacted
    uint32_t* count;         // their number; 0 on entry, alone on its cache line
    uint32_t n_queue, cap;   // cap = max_pixel_samples (0: none)
    float threshold;         // noise_threshold (0: none)
    int32_t pad;
};

// Reprojection of the accumulation (pt_accum_reproject; pt_accum_reproject.hip): the kernel gathers the state of every owned pixel's source
// from one set of buffers into the other and resolves it.  Arrays by launch id except the guides and the two images (framebuffer order).
// What the per-pixel definition (pt_accum_math.h, accum_reproject_source / accum_reproject_history) takes beside the pixel: the new
// camera, the old one with the header's host constants, the parameters.
struct PtAccumReproject {
    float o[3], llc[3], hor[3], ver[3];    // new camera
    float oo[3], a[3], ho[3], vo[3], N[3]; // old camera: origin, a = llc' - o', h', v', N = cross(h', v')
    float inn, na;                         // 1 / dot(N, N), dot(N, a)
    float depth_tol, normal_min, albedo_tol;
    int32_t width, height, max_history;
};
struct PtAccumReprojectArgs {
    PtAccumReproject R;
    const float* aov_prev;   // W*H*8 floats each, 16-byte aligned; may be the same buffer
    const float* aov_cur;
    const uint8_t* owned;
    const float* sum_in;     // the state before the call: read at the source
    const float* half_in;
    const uint32_t* n_in;
    const uint32_t* n_half_in;
    const uint32_t* passes_in;
    float* sum_out;          // the state after it: written at the pixel; none of these is one of the inputs
    float* half_out;
    uint32_t* n_out;
    uint32_t* n_half_out;
    uint32_t* passes_out;
    float* seen;             // = sum_out; the kernel does not read it
    float* noise;
    float* out_rgb;
    uint32_t* out_rgba8;
    uint32_t n_frame;        // W*H
    int32_t pad;
};

// Upsampling (pt_upsample; pt_upsample.hip): what its two kernels take.  The host fills everything but the record pointers, which
// pt_launch_upsample carves out of ws; the constants are include/mi355pt.h's "host constants" (pti::upsample_constants).
struct PtUpsampleArgs {
    const float* rgb_lo;    // w*h*3 floats, framebuffer order
    const float* aov_lo;    // w*h*8 floats of the guide pass at the low size, 16-byte aligned
    const float* aov_hi;    // W*H*8 floats of the guide pass at the high size, 16-byte aligned
    float* out_rgb;         // W*H*3 floats
    uint32_t* out_rgba8;    // W*H, or null
    void* ws;               // pt_upsample_workspace_bytes(w, h), 16-byte aligned
    float4* col;            // low records: colour r g b (divided by the albedo divisor with the flag)
    float4* nz;             // normal x y z + depth
    float4* alb;            // albedo r g b
    int32_t w, h, W, H;
    int32_t taps, flags;
    float sigma_depth, rx, ry, kn, ka, ir;
};

extern "C" {
// pt_upsample.hip: prepare (over the low frame) + upsample (over the high frame) on `stream`; the geometry is the upsample kernel's
// (grid = its workgroups for a W x H frame), hipErrorInvalidConfiguration if one of the two kernels needs scratch
size_t pt_upsample_workspace_bytes(int w, int h);
hipError_t pt_upsample_geometry(int W, int H, PtGeometry* g, int* grid);
hipError_t pt_launch_upsample(const PtUpsampleArgs* a, hipStream_t stream);
// pt_accum_reproject.hip: geometry of the reproject kernel (block, vgprs; *grid = its workgroups for a W x H frame);
// hipErrorInvalidConfiguration if it needs scratch
hipError_t pt_accum_reproject_geometry(int W, int H, PtGeometry* g, int* grid);
hipError_t pt_launch_accum_reproject(const PtAccumReprojectArgs* a, hipStream_t stream);
// pt_accum.hip: geometry of the resolve kernel (block, vgprs); hipErrorInvalidConfiguration if one of the two kernels needs scratch
hipError_t pt_accum_geometry(PtGeometry* g);
hipError_t pt_launch_accum_resolve(const PtAccumArgs* a, hipStream_t stream);
hipError_t pt_launch_accum_select(const PtAccumSelectArgs* a, hipStream_t stream);
// pt_denoise.hip: prepare + `iterations` iteration launches + finish on `stream`; the geometry is the iteration kernel's (grid = its
// workgroups for a W x H frame), hipErrorInvalidConfiguration if one of the three kernels needs scratch
size_t pt_denoise_workspace_bytes(int W, int H);
hipError_t pt_denoise_geometry(int W, int H, PtGeometry* g, int* grid);
hipError_t pt_launch_denoise(const PtDenoiseArgs* a, hipStream_t stream);
// pt_denoise_var.hip: the variance-guided filter, same conventions (prepare + `iterations` launches + finish); the geometry is the
// iteration kernel's, hipErrorInvalidConfiguration if one of the FOUR kernels (the variance kernel included) needs scratch
size_t pt_denoise_var_workspace_bytes(int W, int H);
hipError_t pt_denoise_var_geometry(int W, int H, PtGeometry* g, int* grid);
hipError_t pt_launch_denoise_var(const PtDenoiseVarArgs* a, hipStream_t stream);
hipError_t pt_launch_accum_variance(const PtAccumVarArgs* a, hipStream_t stream);
// pt_denoise_batch.hip: the kernels of pt_denoise.hip over K frames of one size, back to back in every caller buffer (the pointers of *a are the first frame's),
// frame in blockIdx.z: 1 <= K <= 65535; workspace and grid cover all K frames
size_t pt_denoise_batch_workspace_bytes(int W, int H, int K);
hipError_t pt_denoise_batch_geometry(int W, int H, int K, PtGeometry* g, int* grid);
hipError_t pt_launch_denoise_batch(const PtDenoiseArgs* a, int K, hipStream_t stream);
// pt_kernel_aov.hip / pt_kernel_aov_wt.hip: the guide kernels.  binary = 1: the one-level walk over PtNode[] (closest_hit of pt_trace.h; Moeller-
// Trumbore only: the watertight build has no such instance and answers hipErrorInvalidValue).  Geometry: block, lds_bytes, lds_levels and
// vgprs of the instance; hipErrorInvalidConfiguration if it needs scratch.
hipError_t pt_launch_aov(const PtKernelParams* p, const PtAovArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_geometry(int binary, int exact, int stack_entries, PtGeometry* g);
hipError_t pt_launch_aov_wt(const PtKernelParams* p, const PtAovArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_geometry_wt(int binary, int exact, int stack_entries, PtGeometry* g);
// pt_kernel_rays.hip / pt_kernel_rays_wt.hip: the ray kernels (quad walk only; slab form by p->box_exact).  Geometry: block, lds_bytes,
// lds_levels, vgprs and max_blocks_per_cu of the instance; hipErrorInvalidConfiguration if it needs scratch.
hipError_t pt_launch_rays(const PtKernelParams* p, const PtRaysArgs* a, int occluded, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_geometry(int occluded, int exact, PtGeometry* g);
hipError_t pt_launch_rays_wt(const PtKernelParams* p, const PtRaysArgs* a, int occluded, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_geometry_wt(int occluded, int exact, PtGeometry* g);
// pt_kernel_rays_surface.hip / pt_kernel_rays_surface_wt.hip: the surface instances of the ray kernels (pt_trace_surface; a->out: n pt_surface
// records of 80 bytes, 16-byte aligned), same conventions; closest hit only: occluded = 1 answers hipErrorInvalidValue
hipError_t pt_launch_rays_surface(const PtKernelParams* p, const PtRaysArgs* a, int occluded, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_surface_geometry(int occluded, int exact, PtGeometry* g);
hipError_t pt_launch_rays_surface_wt(const PtKernelParams* p, const PtRaysArgs* a, int occluded, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_surface_geometry_wt(int occluded, int exact, PtGeometry* g);
// pt_kernel_rays_ao.hip / pt_kernel_rays_ao_wt.hip: the fused ambient-occlusion kernels (pt_trace_ao; pt_ao.h), same conventions
hipError_t pt_launch_rays_ao(const PtKernelParams* p, const PtAoArgs* a, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_ao_geometry(int exact, PtGeometry* g);
hipError_t pt_launch_rays_ao_wt(const PtKernelParams* p, const PtAoArgs* a, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_ao_geometry_wt(int exact, PtGeometry* g);
// pt_kernel_rays_hits.hip / pt_kernel_rays_hits_wt.hip: the first-K-hits kernels (pt_trace_hits; pt_hits.h), same conventions; the geometry is that
// of a launch with k records per ray (lds_bytes grows with k: four words per record and lane behind the stack)
hipError_t pt_launch_rays_hits(const PtKernelParams* p, const PtHitsArgs* a, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_hits_geometry(int exact, int k, PtGeometry* g);
hipError_t pt_launch_rays_hits_wt(const PtKernelParams* p, const PtHitsArgs* a, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_rays_hits_geometry_wt(int exact, int k, PtGeometry* g);
// pt_kernel_points.hip: the point kernel (pt_closest_point), one instance.  a: the ray kernels' arguments with a->rays = n pt_point records
// (16 bytes), a->out = n pt_point_hit (32 bytes), both 16-byte aligned, and a->cap in stack ENTRIES of pt_points_entry_words() words each:
// a->ovf holds (cap * words - g->lds_levels) * 64 words per workgroup, g->lds_levels being the words of a lane's stack kept in LDS
hipError_t pt_launch_points(const PtKernelParams* p, const PtRaysArgs* a, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_points_geometry(PtGeometry* g);
int pt_points_entry_words(void);
// pt_kernel_aov_follow.hip / pt_kernel_aov_follow_wt.hip: the follow kernels, same conventions; lds_bytes covers the stack and the state a lane parks behind it
hipError_t pt_launch_aov_follow(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_follow_geometry(int binary, int exact, int stack_entries, PtGeometry* g);
hipError_t pt_launch_aov_follow_wt(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_follow_geometry_wt(int binary, int exact, int stack_entries, PtGeometry* g);
// pt_kernel_aov_follow_batch.hip: the batch instances of the follow kernels over the blocks of p->batch_frames frames (p->batch_cams, p->materials =
// the first frame's table, a->out = the first frame's buffers; PtKernelParams::batch_*), same conventions
hipError_t pt_launch_aov_follow_batch(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_follow_batch_geometry(int binary, int exact, int stack_entries, PtGeometry* g);
// pt_kernel_aov_rays.hip / pt_kernel_aov_rays_wt.hip: the ray-image instances of the follow kernels (p->batch_cams = the table of W * H pt_ray_gen
// records, p->batch_frames = 0; PtKernelParams::batch_cams), same conventions; quad walk only: binary = 1 answers hipErrorInvalidValue
hipError_t pt_launch_aov_rays(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_rays_geometry(int binary, int exact, int stack_entries, PtGeometry* g);
hipError_t pt_launch_aov_rays_wt(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
hipError_t pt_aov_rays_geometry_wt(int binary, int exact, int stack_entries, PtGeometry* g);
size_t pt_refit_workspace_bytes(void);
// gather, extent, one refit launch per level, propagate - all on `stream`, `first` recorded before the first kernel, `last` after the last
hipError_t pt_launch_refit(const PtRefitArgs* a, hipEvent_t first, hipEvent_t last, hipStream_t stream);
// scratch: quad probe with overflow: the waves' HBM stack columns; group probe: the waves' park areas (pt_probe_group_state_words each)
hipError_t pt_launch_probe(const PtKernelParams* p, int op, const float* in, int in_stride, float* out, int out_stride, long long n, int grid, size_t lds_bytes,
                           uint32_t* scratch, hipStream_t stream);
int pt_probe_lds_stack(void);                                // PT_LDS_STACK of this build
size_t pt_probe_group_lds_bytes(int lds_levels, int ns);
size_t pt_probe_group_state_words(void);
hipError_t pt_launch_render(const PtKernelParams* p, const PtKernelParams* d_params, int variant, int grid, size_t lds_bytes, hipStream_t stream, int count);
hipError_t pt_launch_debug(const PtKernelParams* p, int op, const float* in, int in_stride, float* out, int out_stride, long long n, size_t lds_bytes,
                           hipStream_t stream);
size_t pt_sort_scratch_bytes(uint32_t n);
hipError_t pt_launch_plan_tiers(const uint32_t* scratch, uint32_t n, int capacity, int ns, int force, uint32_t* tiers, hipStream_t stream);
hipError_t pt_launch_sort_pixels(const uint8_t* cost_img, int W, int H, int radius, const uint32_t* in, uint32_t* out, uint32_t n, uint32_t c0, uint32_t* scratch,
                                 uint8_t* bucket, hipStream_t stream);
hipError_t pt_kernel_geometry(int variant, int count, int stack_entries, int group_entries, int want_ns, int exact, PtGeometry* g);
// pt_kernel_batch.hip: the batch instances of the wavefront kernel (variants 2 and 3 and the instrumented instance; PtKernelParams::batch_*)
hipError_t pt_launch_render_batch(const PtKernelParams* p, const PtKernelParams* d_params, int variant, int grid, size_t lds_bytes, hipStream_t stream, int count);
hipError_t pt_batch_kernel_geometry(int variant, int count, int stack_entries, int group_entries, int want_ns, int exact, PtGeometry* g);
// pt_kernel_rayimage.hip: the ray-image instances of the wavefront kernel (variants 2 and 3 and the instrumented instance; the table of W * H
// pt_ray_gen records, 16-byte aligned, in PtKernelParams::batch_cams with batch_frames = 0)
hipError_t pt_launch_render_rayimage(const PtKernelParams* p, const PtKernelParams* d_params, int variant, int grid, size_t lds_bytes, hipStream_t stream, int count);
hipError_t pt_rayimage_kernel_geometry(int variant, int count, int stack_entries, int group_entries, int want_ns, int exact, PtGeometry* g);
// pt_kernel_wt.hip: the watertight instances of the wavefront kernel (variants 2 and 3 and the instrumented instance) and of the ray probes
hipError_t pt_launch_render_wt(const PtKernelParams* p, const PtKernelParams* d_params, int variant, int grid, size_t lds_bytes, hipStream_t stream, int count);
hipError_t pt_wt_kernel_geometry(int variant, int count, int stack_entries, int group_entries, int want_ns, int exact, PtGeometry* g);
hipError_t pt_launch_probe_wt(const PtKernelParams* p, int op, const float* in, int in_stride, float* out, int out_stride, long long n, int grid, size_t lds_bytes,
                              uint32_t* scratch, hipStream_t stream);
int pt_debug_block(void);
// pt_kernel_aux.hip: the lane-per-pixel variant (pt_launch_render / pt_kernel_geometry forward variant 1 to these)
hipError_t pt_launch_render_lane(const PtKernelParams* p, int grid, size_t lds_bytes, hipStream_t stream, int count);
hipError_t pt_lane_kernel_geometry(int count, int stack_entries, PtGeometry* g);
hipError_t pt_launch_store_params(const PtKernelParams* p, PtKernelParams* d_dst, hipStream_t stream);
hipError_t pt_launch_pack_rgba8(const float* rgb, uint32_t* out, long long n, hipStream_t stream);
// pt_lbvh.hip
size_t pt_lbvh_workspace_bytes(int n);
hipError_t pt_lbvh_build_device(const float* d_pos, int n, int leaf_size, void* d_workspace, size_t workspace_bytes, PtNode* d_nodes, uint32_t* d_order, int32_t* h_root,
                                int32_t* h_n_nodes, int32_t* h_height, int32_t* h_max_leaf, float* h_pad, hipStream_t stream);
size_t pt_ploc_workspace_bytes(int n);
hipError_t pt_ploc_build_device(const float* d_pos, int n, int radius, void* d_workspace, size_t workspace_bytes, int* h_child, float* h_box, int* h_count,
                                uint32_t* h_order, int32_t* h_root, int32_t* h_rounds, hipStream_t stream);
}
