// pt_guides.cpp -- what goes with a frame: the guide pass (pt_render_aov*: first hit or follow mode, one frame or the frames of a batch)
// the denoiser (pt_denoise*, one frame or a batch) and the variance-guided denoiser (pt_denoise_var*, and pt_accum_denoise* /
// pt_accum_variance on the context's accumulation) and the upsampling (pt_upsample*), each ONE device path behind its asynchronous and
// blocking entry points.
// None reads the render's pixel queue or touches its buffers and state (d_laps, slots): their own are d_aov_ws, d_dn_ws, d_dn_var and d_up_ws.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_internal.h"
#include "pt_launch.h"

using namespace pti;

namespace pti {

// (pt_internal.h; pt_accum_host.cpp ends its reproject pass with it as well)
void note_pass(pt_ctx* c, int W, int H, int launches, int grid, const PtGeometry& g, int stack_entries, bool aov_flag)
{
    LastFrame& L = c->last;
    L.ev_pending = true;
    L.flag_pending = false;
    L.aov_flag_pending = aov_flag;
    L.launches = launches;
    L.sorted = false;
    L.w = W;
    L.h = H;
    L.seqs = 1; // (d_seq_flags is the render batch's)
    c->stats.express_pixels = c->stats.whole_pixels = c->stats.prepass_spp = 0;
    c->stats.grid = grid;
    c->stats.vgprs = g.vgprs;
    c->stats.lds_bytes = (int)g.lds_bytes;
    c->stats.block = g.block;
    c->stats.stack_entries = stack_entries;
}

} // namespace pti

namespace {

// ---- guide pass (pt_render_aov*) -------------------------------------------------------------------------------------------
// The instances of the guide kernel (pt_launch.h), by [follow mode][watertight][batch].  The first-hit kernel takes the PtAovArgs a
// PtAovFollowArgs begins with.  There are no batch instances of the first-hit kernel and no watertight batch instances: no entry point
// asks for the first, check_aov_batch_args refuses the second.
using AovGeometry = hipError_t (*)(int binary, int exact, int stack_entries, PtGeometry* g);
using AovLaunch = hipError_t (*)(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream);
template <auto launch> hipError_t first_hit(const PtKernelParams* p, const PtAovFollowArgs* a, int binary, int grid, size_t lds_bytes, hipStream_t stream)
{
    return launch(p, &a->a, binary, grid, lds_bytes, stream);
}
const struct AovInstance { AovGeometry geometry; AovLaunch launch; } kAovInstance[2][2][2] = {
    {{{pt_aov_geometry, first_hit<pt_launch_aov>}, {}}, {{pt_aov_geometry_wt, first_hit<pt_launch_aov_wt>}, {}}},
    {{{pt_aov_follow_geometry, pt_launch_aov_follow}, {pt_aov_follow_batch_geometry, pt_launch_aov_follow_batch}}, {{pt_aov_follow_geometry_wt, pt_launch_aov_follow_wt}, {}}},
};

// The ray-image instances of the follow kernel (pt_render_aov_rays), by [watertight]: quad walk only, single frames only.
const AovInstance kAovRaysInstance[2] = {{pt_aov_rays_geometry, pt_launch_aov_rays}, {pt_aov_rays_geometry_wt, pt_launch_aov_rays_wt}};

// What a guide pass renders: ONE frame from `cam` on the single-frame kernels, or frames [0, n_frames) of a batch (frames != null) on
// the batch instances, their buffers back to back in d_out (W*H*8 floats per frame), or ONE frame over a ray image (cam and frames null)
// on the ray-image instances.
struct AovJob {
    const pt_camera* cam;
    const pt_frame* frames;
    int n_frames, W, H, n_samples;
    const pt_aov_params* follow; // follow mode with these parameters (checked by the caller, check_aov_params); null: the first-hit kernel
    void* d_out;
    hipStream_t stream;
    bool reduce;                 // with a communicator: ONE sum-reduce onto rank 0 per launch sequence, over all of its frames
    // a ray image (pt_render_aov_rays; follow != null): the table of W * H pt_ray_gen records in HBM; far_o: its largest |org| component, which
    // decides the slab form as the camera's origin does in walk_params (+infinity: unknown, rays_image_device of pt_render.cpp); host_rays:
    // the blocking form's table, staged in d_ray_image first
    const void* d_rays = nullptr;
    float far_o = 0.0f;
    const pt_ray_gen* host_rays = nullptr;
};

// One launch of the guide kernel per launch sequence over the 8 x 8 pixel blocks of its frames - a single frame is one sequence, a batch
// is cut as pt_render_batch cuts it (batch_max_frames), the blocks of a sequence being those of its frames one after the other.  The
// kernel itself skips the blocks of other ranks' tiles, so the pass needs no pixel queue.
int aov_device(pt_ctx* c, const AovJob& j)
{
    // refusals first: nothing is enqueued or allocated before them
    // quad: without the quad walk (quad_walk_available) the guide pass runs the binary walk
    const bool batch = j.frames != nullptr, rays = j.d_rays != nullptr, quad = quad_walk_available(c), wt = c->opt.watertight != 0;
    const int W = j.W, H = j.H, n_frames = batch ? j.n_frames : 1, binary = quad ? 0 : 1;
    hipStream_t stream = j.stream;
    int rc;
    if (rays && !quad) return fail(c, PT_E_INVALID, "pt_render_aov_rays: the guide pass over a ray image needs quad nodes"); // (check_aov_rays_args, by name)
    if (!quad && wt)
        return fail(c, PT_E_INVALID, "%s: without quad nodes (option quad = 0, or a tree too deep for them) the guide pass runs the binary walk, which has no watertight test (option watertight = 1)", j.follow ? "pt_render_aov_follow" : "pt_render_aov");
    if (quad && (rc = check_quad_walk_size(c, "guide"))) return rc;
    const int64_t kmax = batch ? batch_max_frames(W, H, c->opt.batch_frames) : 1;
    if (kmax < 1) return fail(c, PT_E_LIMIT, "pt_render_aov_batch: one %dx%d frame already exceeds a launch sequence (< 2^24 pixels)", W, H);
    pt_camera ray_cam{}; // a ray image has no camera: walk_params reads the origin alone, the kernel nothing of P.cam
    ray_cam.origin[0] = j.far_o;
    const pt_camera* cam0 = rays ? &ray_cam : (batch ? &j.frames[0].camera : j.cam);
    PtKernelParams P;
    walk_params(c, cam0, P); // the scene, the slab form ("box_exact" as the render; of a batch: chosen per launch sequence below)
    ray_cam.origin[0] = 0.0f;
    P.nodes8 = nullptr;
    P.groups = 0;
    if (quad) {
        quad_walk_params(c, P);
    } else {
        P.nodes4 = nullptr;
        P.root = c->scene.bvh.root;
        P.stack_entries = c->scene.bvh.depth < 1 ? 1 : c->scene.bvh.depth;
    }
    const AovInstance& inst = rays ? kAovRaysInstance[wt] : kAovInstance[j.follow != nullptr][wt][batch];
    if (rays) P.batch_cams = (const float*)j.d_rays; // (batch_frames stays 0: pt_launch_aov_rays checks both)
    // both slab forms may run in one batch: neither may spill, and they share the launch geometry (block, LDS)
    PtGeometry g{}, gx{};
    hipError_t ge = inst.geometry(binary, batch ? 0 : P.box_exact, P.stack_entries, &g);
    if (ge == hipSuccess && batch && quad) ge = inst.geometry(0, 1, P.stack_entries, &gx);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the %sguide kernel spills registers to scratch; such builds are refused (pt_kernel.hip)", batch ? "batch " : "");
    HIP_TRY(c, ge);
    if (g.max_blocks_per_cu < 1) return fail(c, PT_E_LIMIT, "guide kernel does not fit a CU (LDS %zu bytes, BVH depth %d)", g.lds_bytes, c->scene.bvh.depth);
    const int tile = shard_tile(c->tile);
    // (a batch's shard: check_aov_batch_args, before the device is asked for)
    if (!batch && pt_shard_pixels(W, H, tile, c->rank, c->world, nullptr, 0) < 0) return fail(c, PT_E_INVALID, "invalid pixel shard (%d of %d)", c->rank, c->world);
    const long n_blocks = (long)((W + 7) / 8) * (long)((H + 7) / 8); // of one frame
    auto grid_of = [&](int K) { return (int)std::max(1L, std::min((long)K * n_blocks, (long)c->num_cus * 32)); }; // a few rounds of resident waves: the blocks differ in cost
    PtAovFollowArgs F{};
    PtAovArgs& A = F.a;
    A.cap = quad ? P.stack_entries + 3 : 0;
    const int k_first = (int)std::min<int64_t>(kmax, n_frames); // the longest sequence has the most workgroups
    if ((rc = walk_workspace(c, A.cap, g.lds_levels, grid_of(k_first), stream, P, &A.ovf))) return rc; // one bound flag for every sequence (the binary walk: cap 0, no columns)
    if (batch && (rc = stage_batch_tables(c, j.frames, n_frames, stream))) return rc;
    const size_t npx = (size_t)W * H;
    HIP_TRY(c, hipMemsetAsync(j.d_out, 0, (size_t)n_frames * npx * 8 * sizeof(float), stream)); // pixels of other ranks stay 0
    P.lds_levels = g.lds_levels;
    std::memcpy(P.cam, cam0, sizeof(float) * 12); // (a batch does not read it: every frame's camera comes from batch_cams)
    P.width = W;
    P.height = H;
    A.n_samples = j.n_samples;
    A.rank = c->rank; A.world = c->world; A.tile = tile;
    if (j.follow) {
        F.max_follow = j.follow->max_follow;
        F.roughness_max = j.follow->roughness_max;
        F.inv_n = 1.0f / (float)j.n_samples;
    }
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    int n_seq = 0;
    for (int f0 = 0; f0 < n_frames; ++n_seq) {
        const int K = (int)std::min<int64_t>(kmax, n_frames - f0);
        if (batch) {
            // one slab form per launch sequence: the subtracting one if ANY of its cameras is beyond the switch of walk_params (batch_sequence)
            P.box_exact = 0;
            for (int f = 0; f < K && !P.box_exact; ++f) {
                PtKernelParams Q;
                walk_params(c, &j.frames[f0 + f].camera, Q);
                P.box_exact = Q.box_exact;
            }
            if (quad && P.box_exact) g.vgprs = gx.vgprs; // stats: the exact instance's if any sequence ran it
            P.batch_frames = K;
            P.batch_cams = (const float*)c->d_batch_cams.p + (size_t)12 * f0;
            P.materials = (const float*)c->d_batch_mats.p + (size_t)f0 * c->scene.n_materials * PT_MAT_STRIDE;
        }
        A.out = (float*)j.d_out + (size_t)f0 * npx * 8;
        HIP_TRY(c, inst.launch(&P, &F, binary, grid_of(K), g.lds_bytes, stream));
        HIP_TRY(c, hipEventRecord(c->ev1, stream)); // (after the last kernel: the earlier sequences' reduces lie inside kernel_ms, as pt_render_batch's)
        // one non-zero contributor per pixel, so the sum is exact
        if (j.reduce && c->comm && (rc = reduce_sum(c, A.out, (size_t)K * npx * 8, stream))) return rc;
        f0 += K;
    }
    note_pass(c, W, H, n_seq, grid_of(k_first), g, P.stack_entries, true); // launches = launch sequences
    return PT_OK;
}

// The asynchronous entry points, after their checks: on the caller's stream (null: the context's), no reduce.
int aov_async(pt_ctx* c, AovJob j, void* d_out_aov, void* stream_v)
{
    j.d_out = d_out_aov;
    j.reduce = false;
    return async_call_on(c, stream_v, [&](hipStream_t stream) {
        j.stream = stream;
        return aov_device(c, j);
    });
}

// The blocking entry points, after their checks: into d_aov, reduced, and from there to the host buffer of the root (with a
// communicator attached only rank 0 receives the buffers, as pt_render).
int aov_blocking(pt_ctx* c, AovJob j, float* out_aov)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const bool root = !c->comm || c->comm_rank == 0;
    const size_t n_floats = (size_t)(j.frames ? j.n_frames : 1) * (size_t)j.W * (size_t)j.H * 8;
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_aov, n_floats * 4))) return rc;
        j.d_out = c->d_aov.p;
        j.stream = c->stream;
        j.reduce = true;
        if (j.host_rays) { // a ray image: the table staged where pt_render_rays stages it
            const size_t bytes = (size_t)j.W * (size_t)j.H * sizeof(pt_ray_gen);
            if ((rc = ensure(c, c->d_ray_image, bytes))) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->d_ray_image.p, j.host_rays, bytes, hipMemcpyHostToDevice, c->stream));
            j.d_rays = c->d_ray_image.p;
        }
        if ((rc = aov_device(c, j))) return rc;
        return drain(c, {{root ? out_aov : nullptr, c->d_aov.p, n_floats * 4}});
    });
}

// What the guide batch refuses before anything is touched or enqueued, a host-only context last (who: the entry point; *eff = the
// parameters in effect).  The tables are staged, the batch is cut and the instances are chosen in aov_device.
int check_aov_batch_args(pt_ctx* c, const char* who, const pt_frame* frames, int n_frames, int n_materials, int W, int H, const pt_aov_params* p, pt_aov_params* eff)
{
    if (n_frames < 1 || !frames) return fail(c, PT_E_INVALID, "%s: a batch needs at least one frame (n_frames %d%s)", who, n_frames, frames ? "" : ", frames NULL");
    int rc;
    if ((rc = check_aov_params(c, p, who, eff))) return rc;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    if (n_materials != c->scene.n_materials) return fail(c, PT_E_INVALID, "%s: %d materials per frame, the scene has %d", who, n_materials, c->scene.n_materials);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (int64_t)W * H > (int64_t)0x7fffffff) return fail(c, PT_E_INVALID, "%s: bad guide pass size %dx%d", who, W, H);
    if (c->opt.watertight) return fail(c, PT_E_INVALID, "%s: batches have no watertight instances (option watertight = 1); render the guides frame by frame or set watertight = 0", who);
    if (pt_shard_pixels(W, H, shard_tile(c->tile), c->rank, c->world, nullptr, 0) < 0) return fail(c, PT_E_INVALID, "%s: invalid pixel shard (%d of %d)", who, c->rank, c->world);
    return need_device(c);
}

// What the two forms of the guide pass over a ray image refuse alike before anything is touched, a host-only context last (device: rays
// and out are device pointers, and the host cannot look at the records).  The table's checks are pt_render_rays' (pt_render.cpp), the
// parameters' and the sizes' pt_render_aov_follow's.
int check_aov_rays_args(pt_ctx* c, const char* who, const void* rays, int W, int H, const pt_aov_params* p, const void* out_aov, bool device, pt_aov_params* eff)
{
    int rc;
    if ((rc = check_ray_ptrs(c, who, rays, out_aov, device ? "d_out_aov" : "out_aov", device))) return rc;
    if (device && ((uintptr_t)out_aov & 15u)) return fail(c, PT_E_INVALID, "%s: d_out_aov is not 16-byte aligned (a guide record is two 16-byte stores)", who);
    if ((rc = check_aov_params(c, p, who, eff))) return rc;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (int64_t)W * H > (int64_t)0x7fffffff) return fail(c, PT_E_INVALID, "%s: bad guide pass size %dx%d", who, W, H);
    // the ray-image instances walk the quad nodes - or a root that is itself a leaf - and nothing else (as the ray queries, pt_rays_host.cpp)
    if (!quad_walk_available(c))
        return fail(c, PT_E_INVALID, "%s: the guide pass over a ray image needs quad nodes (%s); there are no binary-walk instances", who, !c->opt.quad ? "option quad = 0" : "the tree is too deep for them");
    if ((rc = check_ray_table(c, who, rays, W, H, device, true))) return rc;
    return need_device(c);
}

// ---- denoiser (pt_denoise*) ------------------------------------------------------------------------------------------------
// The filter over device buffers: prepare, L iteration launches, finish.  It reads no scene; its records live in d_dn_ws.  batch = false:
// one frame on the kernels of pt_denoise.hip.  batch = true: n_frames frames of W x H, back to back in every buffer, on those of
// pt_denoise_batch.hip, cut into launch sequences as pt_render_batch cuts a batch (batch_max_frames) - ONE workspace for the frames of
// a sequence, which the next sequence reuses in stream order.
struct DenoiseJob {
    bool batch;
    int n_frames, W, H;
    pt_denoise_params prm; // checked by the caller (check_denoise_args)
};

int denoise_device(pt_ctx* c, const DenoiseJob& j, const void* d_rgb, const void* d_aov, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    const int W = j.W, H = j.H, n_frames = j.batch ? j.n_frames : 1;
    const int64_t kmax = j.batch ? batch_max_frames(W, H, c->opt.batch_frames) : 1;
    if (kmax < 1) return fail(c, PT_E_LIMIT, "pt_denoise_batch: one %dx%d frame already exceeds a launch sequence (< 2^24 pixels)", W, H);
    const int k_first = (int)std::min<int64_t>(kmax, n_frames);
    PtGeometry g{};
    int grid = 0;
    const hipError_t ge = j.batch ? pt_denoise_batch_geometry(W, H, k_first, &g, &grid) : pt_denoise_geometry(W, H, &g, &grid);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the %sdenoise kernels spills registers to scratch; such builds are refused (pt_denoise.hip)", j.batch ? "batch " : "");
    HIP_TRY(c, ge);
    int rc;
    if ((rc = ensure(c, c->d_dn_ws, j.batch ? pt_denoise_batch_workspace_bytes(W, H, k_first) : pt_denoise_workspace_bytes(W, H)))) return rc; // (growing it first waits on the host for what is in flight)
    PtDenoiseArgs A{};
    A.ws = c->d_dn_ws.p;
    A.width = W;
    A.height = H;
    A.iterations = j.prm.iterations;
    A.flags = j.prm.flags;
    A.sigma_depth = j.prm.sigma_depth;
    denoise_constants(j.prm, &A.kn, &A.ka, A.kc);
    const size_t npx = (size_t)W * H;
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    int n_seq = 0;
    for (int f0 = 0; f0 < n_frames; ++n_seq) {
        const int K = (int)std::min<int64_t>(kmax, n_frames - f0);
        A.rgb = (const float*)d_rgb + (size_t)f0 * npx * 3;
        A.aov = (const float*)d_aov + (size_t)f0 * npx * 8;
        A.out_rgb = (float*)d_out_rgb + (size_t)f0 * npx * 3;
        A.out_rgba8 = d_out_rgba8 ? (uint32_t*)d_out_rgba8 + (size_t)f0 * npx : nullptr;
        HIP_TRY(c, j.batch ? pt_launch_denoise_batch(&A, K, stream) : pt_launch_denoise(&A, stream));
        f0 += K;
    }
    HIP_TRY(c, hipEventRecord(c->ev1, stream)); // kernel_ms: from the first to the last filter kernel
    note_pass(c, W, H, n_seq * (j.prm.iterations + 2), grid, g, 0, false);
    return PT_OK;
}

int denoise_async(pt_ctx* c, const DenoiseJob& j, const void* d_rgb, const void* d_aov, void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return denoise_device(c, j, d_rgb, d_aov, d_out_rgb, d_out_rgba8, stream); });
}

// Host buffers: staged in d_dn_rgb / d_dn_aov, filtered in place on the staging copy, and back.
int denoise_blocking(pt_ctx* c, const DenoiseJob& j, const float* rgb, const float* aov, float* out_rgb, uint32_t* out_rgba8)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)(j.batch ? j.n_frames : 1) * (size_t)j.W * (size_t)j.H;
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_dn_rgb, npx * 12)) || (rc = ensure(c, c->d_dn_aov, npx * 32))) return rc;
        if (out_rgba8 && (rc = ensure(c, c->d_dn_out8, npx * 4))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_dn_rgb.p, rgb, npx * 12, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_dn_aov.p, aov, npx * 32, hipMemcpyHostToDevice, c->stream));
        if ((rc = denoise_device(c, j, c->d_dn_rgb.p, c->d_dn_aov.p, c->d_dn_rgb.p, out_rgba8 ? c->d_dn_out8.p : nullptr, c->stream))) return rc;
        return drain(c, {{out_rgb, c->d_dn_rgb.p, npx * 12}, {out_rgba8, c->d_dn_out8.p, npx * 4}});
    });
}

// ---- upsampling (pt_upsample*) -----------------------------------------------------------------------------------------------
// A w x h frame and its guides to W x H under the high guides, over device buffers: prepare over the low frame, the upsample kernel over
// the high one (pt_upsample.hip).  It reads no scene; its records live in d_up_ws.
struct UpsampleJob {
    int w, h, W, H;
    pt_upsample_params prm; // checked by the caller (check_upsample_args)
};

int upsample_device(pt_ctx* c, const UpsampleJob& j, const void* d_rgb_lo, const void* d_aov_lo, const void* d_aov_hi, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    PtGeometry g{};
    int grid = 0;
    const hipError_t ge = pt_upsample_geometry(j.W, j.H, &g, &grid);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the upsample kernels spills registers to scratch; such builds are refused (pt_upsample.hip)");
    HIP_TRY(c, ge);
    int rc;
    if ((rc = ensure(c, c->d_up_ws, pt_upsample_workspace_bytes(j.w, j.h)))) return rc; // (growing it first waits on the host for what is in flight)
    PtUpsampleArgs A{};
    A.rgb_lo = (const float*)d_rgb_lo;
    A.aov_lo = (const float*)d_aov_lo;
    A.aov_hi = (const float*)d_aov_hi;
    A.out_rgb = (float*)d_out_rgb;
    A.out_rgba8 = (uint32_t*)d_out_rgba8;
    A.ws = c->d_up_ws.p;
    A.w = j.w; A.h = j.h; A.W = j.W; A.H = j.H;
    A.taps = j.prm.taps;
    A.flags = j.prm.flags;
    A.sigma_depth = j.prm.sigma_depth;
    upsample_constants(j.prm, j.w, j.h, j.W, j.H, &A.rx, &A.ry, &A.kn, &A.ka, &A.ir);
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    HIP_TRY(c, pt_launch_upsample(&A, stream));
    HIP_TRY(c, hipEventRecord(c->ev1, stream)); // kernel_ms: from the first to the last kernel
    note_pass(c, j.W, j.H, 2, grid, g, 0, false);
    return PT_OK;
}

int upsample_async(pt_ctx* c, const UpsampleJob& j, const void* d_rgb_lo, const void* d_aov_lo, const void* d_aov_hi, void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return upsample_device(c, j, d_rgb_lo, d_aov_lo, d_aov_hi, d_out_rgb, d_out_rgba8, stream); });
}

// Host buffers: the low frame and its guides staged in d_up_rgb / d_up_aov, the high guides in d_dn_aov, the result in d_dn_rgb (and
// d_dn_out8), and back.
int upsample_blocking(pt_ctx* c, const UpsampleJob& j, const float* rgb_lo, const float* aov_lo, const float* aov_hi, float* out_rgb, uint32_t* out_rgba8)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_lo = (size_t)j.w * (size_t)j.h, n_hi = (size_t)j.W * (size_t)j.H;
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_up_rgb, n_lo * 12)) || (rc = ensure(c, c->d_up_aov, n_lo * 32)) || (rc = ensure(c, c->d_dn_aov, n_hi * 32)) || (rc = ensure(c, c->d_dn_rgb, n_hi * 12))) return rc;
        if (out_rgba8 && (rc = ensure(c, c->d_dn_out8, n_hi * 4))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_up_rgb.p, rgb_lo, n_lo * 12, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_up_aov.p, aov_lo, n_lo * 32, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(c->d_dn_aov.p, aov_hi, n_hi * 32, hipMemcpyHostToDevice, c->stream));
        if ((rc = upsample_device(c, j, c->d_up_rgb.p, c->d_up_aov.p, c->d_dn_aov.p, c->d_dn_rgb.p, out_rgba8 ? c->d_dn_out8.p : nullptr, c->stream))) return rc;
        return drain(c, {{out_rgb, c->d_dn_rgb.p, n_hi * 12}, {out_rgba8, c->d_dn_out8.p, n_hi * 4}});
    });
}

// ---- variance-guided denoiser (pt_denoise_var*, pt_accum_denoise*, pt_accum_variance) ------------------------------------------
// The variance kernel over the accumulation's state, into d_out_var (W*H*3 floats, framebuffer order).  It reads the state and writes none.
int accum_variance_launch(pt_ctx* c, void* d_out_var, hipStream_t stream)
{
    const Accum& a = *c->acc;
    PtAccumVarArgs V{};
    V.sum = (const float*)a.sum.p;
    V.half = (const float*)a.half.p;
    V.n = (const uint32_t*)a.n.p;
    V.n_half = (const uint32_t*)a.n_half.p;
    V.owned = (const uint8_t*)a.owned.p;
    V.out_var = (float*)d_out_var;
    V.n_frame = (uint32_t)a.w * (uint32_t)a.h;
    V.width = a.w;
    V.height = a.h;
    HIP_TRY(c, pt_launch_accum_variance(&V, stream));
    return PT_OK;
}

// The filter over device buffers, ONE path: prepare, L iteration launches, finish on the kernels of pt_denoise_var.hip, its records in
// d_dn_ws like pt_denoise's.  accum: the frame is the context's accumulation - the variance kernel first (its map in d_dn_var), the colour
// resolve's own image; d_rgb and d_var are not looked at.
struct DenoiseVarJob {
    bool accum;
    int W, H;
    pt_denoise_params prm; // checked by the caller (check_denoise_args)
};

int denoise_var_device(pt_ctx* c, const DenoiseVarJob& j, const void* d_rgb, const void* d_var, const void* d_aov, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    const int W = j.W, H = j.H;
    PtGeometry g{};
    int grid = 0;
    const hipError_t ge = pt_denoise_var_geometry(W, H, &g, &grid);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the variance-guided denoise kernels spills registers to scratch; such builds are refused (pt_denoise_var.hip)");
    HIP_TRY(c, ge);
    const size_t npx = (size_t)W * H;
    int rc;
    if ((rc = ensure(c, c->d_dn_ws, pt_denoise_var_workspace_bytes(W, H)))) return rc; // (growing it first waits on the host for what is in flight)
    if (j.accum && (rc = ensure(c, c->d_dn_var, npx * 12))) return rc;
    PtDenoiseVarArgs A{};
    A.rgb = (const float*)(j.accum ? c->acc->out.p : d_rgb);
    A.var = (const float*)(j.accum ? c->d_dn_var.p : d_var);
    A.aov = (const float*)d_aov;
    A.out_rgb = (float*)d_out_rgb;
    A.out_rgba8 = (uint32_t*)d_out_rgba8;
    A.ws = c->d_dn_ws.p;
    A.width = W;
    A.height = H;
    A.iterations = j.prm.iterations;
    A.flags = j.prm.flags;
    A.sigma_depth = j.prm.sigma_depth;
    float kc_unused[8];
    denoise_constants(j.prm, &A.kn, &A.ka, kc_unused);
    A.s2 = j.prm.sigma_color * j.prm.sigma_color;
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    if (j.accum && (rc = accum_variance_launch(c, c->d_dn_var.p, stream))) return rc;
    HIP_TRY(c, pt_launch_denoise_var(&A, stream));
    HIP_TRY(c, hipEventRecord(c->ev1, stream)); // kernel_ms: from the first to the last kernel
    note_pass(c, W, H, j.prm.iterations + 2 + (j.accum ? 1 : 0), grid, g, 0, false);
    return PT_OK;
}

int denoise_var_async(pt_ctx* c, const DenoiseVarJob& j, const void* d_rgb, const void* d_var, const void* d_aov, void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return denoise_var_device(c, j, d_rgb, d_var, d_aov, d_out_rgb, d_out_rgba8, stream); });
}

// Host buffers: staged in d_dn_rgb / d_dn_var / d_dn_aov, filtered into d_dn_rgb, and back.  accum: only the guides are staged.
int denoise_var_blocking(pt_ctx* c, const DenoiseVarJob& j, const float* rgb, const float* var, const float* aov, float* out_rgb, uint32_t* out_rgba8)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)j.W * (size_t)j.H;
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_dn_rgb, npx * 12)) || (rc = ensure(c, c->d_dn_aov, npx * 32)) || (rc = ensure(c, c->d_dn_var, npx * 12))) return rc;
        if (out_rgba8 && (rc = ensure(c, c->d_dn_out8, npx * 4))) return rc;
        if (!j.accum) {
            HIP_TRY(c, hipMemcpyAsync(c->d_dn_rgb.p, rgb, npx * 12, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(c->d_dn_var.p, var, npx * 12, hipMemcpyHostToDevice, c->stream));
        }
        HIP_TRY(c, hipMemcpyAsync(c->d_dn_aov.p, aov, npx * 32, hipMemcpyHostToDevice, c->stream));
        if ((rc = denoise_var_device(c, j, c->d_dn_rgb.p, c->d_dn_var.p, c->d_dn_aov.p, c->d_dn_rgb.p, out_rgba8 ? c->d_dn_out8.p : nullptr, c->stream))) return rc;
        return drain(c, {{out_rgb, c->d_dn_rgb.p, npx * 12}, {out_rgba8, c->d_dn_out8.p, npx * 4}});
    });
}

// What the two forms of pt_accum_denoise refuse alike before anything is touched, a host-only context last; j->W, H = the accumulation's.
int check_accum_denoise_args(pt_ctx* c, const char* who, const void* aov, const pt_denoise_params* p, const void* out_rgb, DenoiseVarJob* j)
{
    int rc;
    if ((rc = need_accum(c, who))) return rc;
    const Accum& a = *c->acc;
    if ((uint64_t)a.n_owned != (uint64_t)a.w * (uint64_t)a.h)
        return fail(c, PT_E_INVALID, "%s: the accumulation's pixel shard (%d of %d) owns %u of the frame's %lld pixels; the filter needs every pixel", who, a.rank, a.world, a.n_owned, (long long)a.w * a.h);
    if ((rc = refuse_comm(c, who))) return rc;
    if (!aov || !out_rgb) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !aov ? "aov" : "out_rgb");
    j->accum = true;
    j->W = a.w;
    j->H = a.h;
    if ((rc = check_denoise_args(c, who, a.w, a.h, p, &j->prm, pt_denoise_var_default_params))) return rc;
    return need_device(c);
}

// What the two forms of the denoise batch refuse alike before anything is touched, a host-only context last.
int check_denoise_batch_args(pt_ctx* c, const char* who, int32_t n_frames, int32_t W, int32_t H, const pt_denoise_params* p, pt_denoise_params* eff)
{
    if (n_frames < 1) return fail(c, PT_E_INVALID, "%s: a batch needs at least one frame (n_frames %d)", who, n_frames);
    int rc;
    if ((rc = check_denoise_args(c, who, W, H, p, eff))) return rc;
    return need_device(c);
}

} // namespace

extern "C" {

int pt_render_aov_device(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, int32_t n_samples, void* d_out_aov, void* stream_v)
{
    if (!c || !cam || !d_out_aov) return PT_E_INVALID;
    int rc;
    if ((rc = need_device(c)) || (rc = check_render_args(c, W, H, n_samples, 0))) return rc;
    return aov_async(c, AovJob{cam, nullptr, 1, W, H, n_samples, nullptr}, d_out_aov, stream_v);
}

int pt_render_aov_follow_device(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, const pt_aov_params* p, void* d_out_aov, void* stream_v)
{
    if (!c || !cam || !d_out_aov) return PT_E_INVALID;
    pt_aov_params prm;
    int rc;
    if ((rc = need_device(c)) || (rc = check_aov_params(c, p, "pt_render_aov_follow_device", &prm)) || (rc = check_render_args(c, W, H, prm.n_samples, 0))) return rc;
    return aov_async(c, AovJob{cam, nullptr, 1, W, H, prm.n_samples, &prm}, d_out_aov, stream_v);
}

int pt_render_aov(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, int32_t n_samples, float* out_aov)
{
    // with a communicator attached only rank 0 receives the buffers (as pt_render)
    const bool root = !c || !c->comm || c->comm_rank == 0;
    if (!c || !cam || (root && !out_aov)) return PT_E_INVALID;
    int rc;
    if ((rc = need_device(c)) || (rc = check_render_args(c, W, H, n_samples, 0))) return rc;
    return aov_blocking(c, AovJob{cam, nullptr, 1, W, H, n_samples, nullptr}, out_aov);
}

int pt_render_aov_follow(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, const pt_aov_params* p, float* out_aov)
{
    const bool root = !c || !c->comm || c->comm_rank == 0;
    if (!c || !cam || (root && !out_aov)) return PT_E_INVALID;
    pt_aov_params prm;
    int rc;
    if ((rc = need_device(c)) || (rc = check_aov_params(c, p, "pt_render_aov_follow", &prm)) || (rc = check_render_args(c, W, H, prm.n_samples, 0))) return rc;
    return aov_blocking(c, AovJob{cam, nullptr, 1, W, H, prm.n_samples, &prm}, out_aov);
}

int pt_render_aov_batch_device(pt_ctx* c, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t W, int32_t H, const pt_aov_params* p, void* d_out_aov,
                               void* stream_v)
{
    if (!c) return PT_E_INVALID;
    if (!d_out_aov) return fail(c, PT_E_INVALID, "pt_render_aov_batch_device: NULL d_out_aov");
    pt_aov_params prm;
    int rc;
    if ((rc = check_aov_batch_args(c, "pt_render_aov_batch_device", frames, n_frames, n_materials, W, H, p, &prm))) return rc;
    return aov_async(c, AovJob{nullptr, frames, n_frames, W, H, prm.n_samples, &prm}, d_out_aov, stream_v);
}

int pt_render_aov_batch(pt_ctx* c, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t W, int32_t H, const pt_aov_params* p, float* out_aov)
{
    if (!c) return PT_E_INVALID;
    const bool root = !c->comm || c->comm_rank == 0;
    if (root && !out_aov) return fail(c, PT_E_INVALID, "pt_render_aov_batch: NULL out_aov");
    pt_aov_params prm;
    int rc;
    if ((rc = check_aov_batch_args(c, "pt_render_aov_batch", frames, n_frames, n_materials, W, H, p, &prm))) return rc;
    return aov_blocking(c, AovJob{nullptr, frames, n_frames, W, H, prm.n_samples, &prm}, out_aov);
}

int pt_render_aov_rays_device(pt_ctx* c, const void* d_rays, int32_t W, int32_t H, const pt_aov_params* p, void* d_out_aov, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    pt_aov_params prm;
    int rc;
    if ((rc = check_aov_rays_args(c, "pt_render_aov_rays_device", d_rays, W, H, p, d_out_aov, true, &prm))) return rc;
    AovJob j{nullptr, nullptr, 1, W, H, prm.n_samples, &prm};
    j.d_rays = d_rays;
    j.far_o = INFINITY; // the records are the caller's and unknown here: the slab form that holds at any distance, unless the option chooses
    return aov_async(c, j, d_out_aov, stream_v);
}

int pt_render_aov_rays(pt_ctx* c, const pt_ray_gen* rays, int32_t W, int32_t H, const pt_aov_params* p, float* out_aov)
{
    if (!c) return PT_E_INVALID;
    pt_aov_params prm;
    int rc;
    if ((rc = check_aov_rays_args(c, "pt_render_aov_rays", rays, W, H, p, out_aov, false, &prm))) return rc;
    AovJob j{nullptr, nullptr, 1, W, H, prm.n_samples, &prm};
    j.host_rays = rays;
    j.d_rays = rays; // (a ray image; aov_blocking puts the staged table here)
    j.far_o = ray_table_far_o(rays, (size_t)W * (size_t)H);
    return aov_blocking(c, j, out_aov);
}

int pt_denoise_device(pt_ctx* c, const void* d_rgb, const void* d_aov, int32_t W, int32_t H, const pt_denoise_params* p, void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    if (!d_rgb || !d_aov || !d_out_rgb) return fail(c, PT_E_INVALID, "pt_denoise_device: NULL %s", !d_rgb ? "d_rgb" : (!d_aov ? "d_aov" : "d_out_rgb"));
    int rc;
    DenoiseJob j{false, 1, W, H};
    if ((rc = need_device(c)) || (rc = check_denoise_args(c, "pt_denoise_device", W, H, p, &j.prm))) return rc;
    return denoise_async(c, j, d_rgb, d_aov, d_out_rgb, d_out_rgba8, stream_v);
}

int pt_denoise(pt_ctx* c, const float* rgb, const float* aov, int32_t W, int32_t H, const pt_denoise_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    if (!rgb || !aov || !out_rgb) return fail(c, PT_E_INVALID, "pt_denoise: NULL %s", !rgb ? "rgb" : (!aov ? "aov" : "out_rgb"));
    int rc;
    DenoiseJob j{false, 1, W, H};
    if ((rc = need_device(c)) || (rc = check_denoise_args(c, "pt_denoise", W, H, p, &j.prm))) return rc;
    return denoise_blocking(c, j, rgb, aov, out_rgb, out_rgba8);
}

int pt_upsample_device(pt_ctx* c, const void* d_rgb_lo, const void* d_aov_lo, int32_t w, int32_t h, const void* d_aov_hi, int32_t W, int32_t H, const pt_upsample_params* p,
                       void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    if (!d_rgb_lo || !d_aov_lo || !d_aov_hi || !d_out_rgb)
        return fail(c, PT_E_INVALID, "pt_upsample_device: NULL %s", !d_rgb_lo ? "d_rgb_lo" : (!d_aov_lo ? "d_aov_lo" : (!d_aov_hi ? "d_aov_hi" : "d_out_rgb")));
    int rc;
    UpsampleJob j{w, h, W, H};
    if ((rc = check_upsample_args(c, "pt_upsample_device", w, h, W, H, p, &j.prm)) || (rc = need_device(c))) return rc;
    return upsample_async(c, j, d_rgb_lo, d_aov_lo, d_aov_hi, d_out_rgb, d_out_rgba8, stream_v);
}

int pt_upsample(pt_ctx* c, const float* rgb_lo, const float* aov_lo, int32_t w, int32_t h, const float* aov_hi, int32_t W, int32_t H, const pt_upsample_params* p, float* out_rgb,
                uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    if (!rgb_lo || !aov_lo || !aov_hi || !out_rgb) return fail(c, PT_E_INVALID, "pt_upsample: NULL %s", !rgb_lo ? "rgb_lo" : (!aov_lo ? "aov_lo" : (!aov_hi ? "aov_hi" : "out_rgb")));
    int rc;
    UpsampleJob j{w, h, W, H};
    if ((rc = check_upsample_args(c, "pt_upsample", w, h, W, H, p, &j.prm)) || (rc = need_device(c))) return rc;
    return upsample_blocking(c, j, rgb_lo, aov_lo, aov_hi, out_rgb, out_rgba8);
}

int pt_denoise_var_device(pt_ctx* c, const void* d_rgb, const void* d_var, const void* d_aov, int32_t W, int32_t H, const pt_denoise_params* p, void* d_out_rgb, void* d_out_rgba8,
                          void* stream_v)
{
    if (!c) return PT_E_INVALID;
    if (!d_rgb || !d_var || !d_aov || !d_out_rgb) return fail(c, PT_E_INVALID, "pt_denoise_var_device: NULL %s", !d_rgb ? "d_rgb" : (!d_var ? "d_var" : (!d_aov ? "d_aov" : "d_out_rgb")));
    int rc;
    DenoiseVarJob j{false, W, H};
    if ((rc = check_denoise_args(c, "pt_denoise_var_device", W, H, p, &j.prm, pt_denoise_var_default_params)) || (rc = need_device(c))) return rc;
    return denoise_var_async(c, j, d_rgb, d_var, d_aov, d_out_rgb, d_out_rgba8, stream_v);
}

int pt_denoise_var(pt_ctx* c, const float* rgb, const float* var, const float* aov, int32_t W, int32_t H, const pt_denoise_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    if (!rgb || !var || !aov || !out_rgb) return fail(c, PT_E_INVALID, "pt_denoise_var: NULL %s", !rgb ? "rgb" : (!var ? "var" : (!aov ? "aov" : "out_rgb")));
    int rc;
    DenoiseVarJob j{false, W, H};
    if ((rc = check_denoise_args(c, "pt_denoise_var", W, H, p, &j.prm, pt_denoise_var_default_params)) || (rc = need_device(c))) return rc;
    return denoise_var_blocking(c, j, rgb, var, aov, out_rgb, out_rgba8);
}

int pt_accum_denoise_device(pt_ctx* c, const void* d_aov, const pt_denoise_params* p, void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    int rc;
    DenoiseVarJob j{};
    if ((rc = check_accum_denoise_args(c, "pt_accum_denoise_device", d_aov, p, d_out_rgb, &j))) return rc;
    return denoise_var_async(c, j, nullptr, nullptr, d_aov, d_out_rgb, d_out_rgba8, stream_v);
}

int pt_accum_denoise(pt_ctx* c, const float* aov, const pt_denoise_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    int rc;
    DenoiseVarJob j{};
    if ((rc = check_accum_denoise_args(c, "pt_accum_denoise", aov, p, out_rgb, &j))) return rc;
    return denoise_var_blocking(c, j, nullptr, nullptr, aov, out_rgb, out_rgba8);
}

int pt_accum_variance(pt_ctx* c, float* out_var)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = need_accum(c, "pt_accum_variance"))) return rc;
    if (!out_var) return fail(c, PT_E_INVALID, "pt_accum_variance: NULL out_var");
    if ((rc = need_device(c)) || (rc = wait_idle(c))) return rc;
    const Accum& a = *c->acc;
    const size_t npx = (size_t)a.w * a.h;
    PtGeometry g{};
    int grid = 0;
    const hipError_t ge = pt_denoise_var_geometry(a.w, a.h, &g, &grid);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the variance-guided denoise kernels spills registers to scratch; such builds are refused (pt_denoise_var.hip)");
    HIP_TRY(c, ge);
    if ((rc = ensure(c, c->d_dn_var, npx * 12)) || (rc = accum_variance_launch(c, c->d_dn_var.p, c->stream))) return rc;
    HIP_TRY(c, hipMemcpyAsync(out_var, c->d_dn_var.p, npx * 12, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return check_watchdog(c);
}

int pt_denoise_batch_device(pt_ctx* c, const void* d_rgb, const void* d_aov, int32_t n_frames, int32_t W, int32_t H, const pt_denoise_params* p, void* d_out_rgb,
                            void* d_out_rgba8, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    if (!d_rgb || !d_aov || !d_out_rgb) return fail(c, PT_E_INVALID, "pt_denoise_batch_device: NULL %s", !d_rgb ? "d_rgb" : (!d_aov ? "d_aov" : "d_out_rgb"));
    int rc;
    DenoiseJob j{true, n_frames, W, H};
    if ((rc = check_denoise_batch_args(c, "pt_denoise_batch_device", n_frames, W, H, p, &j.prm))) return rc;
    return denoise_async(c, j, d_rgb, d_aov, d_out_rgb, d_out_rgba8, stream_v);
}

int pt_denoise_batch(pt_ctx* c, const float* rgb, const float* aov, int32_t n_frames, int32_t W, int32_t H, const pt_denoise_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    if (!rgb || !aov || !out_rgb) return fail(c, PT_E_INVALID, "pt_denoise_batch: NULL %s", !rgb ? "rgb" : (!aov ? "aov" : "out_rgb"));
    int rc;
    DenoiseJob j{true, n_frames, W, H};
    if ((rc = check_denoise_batch_args(c, "pt_denoise_batch", n_frames, W, H, p, &j.prm))) return rc;
    return denoise_blocking(c, j, rgb, aov, out_rgb, out_rgba8);
}

} // extern "C"
