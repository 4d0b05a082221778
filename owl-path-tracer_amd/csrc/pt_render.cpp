// pt_render.cpp -- a frame, from the pixel queue to the read-back: the plan of its launches, its buffers and parameters, the launches,
// batches of frames (pt_render_batch), ray images (pt_render_rays), pt_render / pt_render_device, pt_synchronize, the watchdog check and the drain that ends every
// blocking call (the guide pass and the denoiser are pt_guides.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "pt_internal.h"
#include "pt_launch.h"
#include "pt_tiers.h"

using namespace pti;

namespace pti {

void fill_params(pt_ctx* c, PtKernelParams& P)
{
    std::memset(&P, 0, sizeof(P));
    P.nodes = (const PtNode*)c->d_nodes.p;
    P.tris = (const PtTri*)c->d_tris.p;
    P.shade = (const PtShade*)c->d_shade.p;
    P.materials = (const float*)c->d_materials.p;
    P.textures = (const PtTexDesc*)c->d_texdesc.p;
    P.env_map.texels = c->scene.env_map.w > 0 ? (const uint32_t*)c->d_env.p : nullptr;
    P.env_map.width = c->scene.env_map.w;
    P.env_map.height = c->scene.env_map.h;
    for (int i = 0; i < 3; ++i) P.env_color[i] = c->scene.env.color[i];
    P.env_intensity = c->scene.env.intensity;
    P.env_use_map = c->scene.env.use_map;
    P.env_use_auto = c->scene.env.use_auto;
    P.root = c->scene.bvh.root;
    P.n_tris = (int)c->scene.bvh.tris.size();
    P.n_materials = c->scene.n_materials;
    P.stack_entries = c->scene.bvh.depth < 1 ? 1 : c->scene.bvh.depth;
    for (int i = 0; i < 8; ++i) P.tune[i] = c->opt.tune[i];
}

// After the render stream has drained: did a wave's watchdog fire (pt_kernel.hip, PT_WATCHDOG_ROUNDS)?  The image is then incomplete.
int check_watchdog(pt_ctx* c)
{
    if (c->last.aov_flag_pending && c->d_aov_ws.p) { // the last call was a guide pass or a ray query: its walks' step and stack bound (pt_kernel.hip, pt_aov_kernel / pt_rays_kernel)
        uint32_t fired = 0;
        HIP_TRY(c, hipMemcpy(&fired, c->d_aov_ws.p, 4, hipMemcpyDeviceToHost));
        c->last.aov_flag_pending = false;
        if (fired) return fail(c, PT_E_HIP, "guide pass or ray query: a walk ran out of its step or stack bound; the buffers are incomplete");
    }
    if (c->opt.kernel != 2 || !c->d_laps.p || !c->last.flag_pending) return PT_OK;
    uint32_t wd = 0;
    HIP_TRY(c, hipMemcpy(&wd, c->d_laps.p, 4, hipMemcpyDeviceToHost));
    if (c->last.seqs > 1 && c->d_seq_flags.p) { // a batch: the flags of its earlier launch sequences (the next sequence clears d_laps)
        std::vector<uint32_t> fl((size_t)c->last.seqs - 1);
        HIP_TRY(c, hipMemcpy(fl.data(), c->d_seq_flags.p, fl.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t v : fl) wd |= v;
    }
    c->last.flag_pending = false;
    c->last.watchdog_fired = wd != 0;
    if (wd) return fail(c, PT_E_HIP, "render kernel watchdog fired (scheduler made no progress); the image is incomplete");
    return PT_OK;
}

// The scene (fill_params) and the tree walks of the wavefront kernel for a frame from `cam`.
void walk_params(pt_ctx* c, const pt_camera* cam, PtKernelParams& P)
{
    fill_params(c, P);
    {   // the fma form of the slab test (pt_kernel.hip, node4_step) displaces a plane by |o| 2^-24; the boxes are padded by 1e-5 x the scene
        // extent (bvh.pad): exact form when the camera is so far from the origin that this would eat a quarter of the padding
        const float reach = c->scene.bvh.pad * 4194304.0f; // pad x 2^22 = 42 scene extents
        float far_o = 0.0f;
        for (int a = 0; a < 3; ++a) far_o = std::max(far_o, std::fabs(cam->origin[a]));
        P.box_exact = (c->opt.box_exact > 0 || (c->opt.box_exact < 0 && !(far_o <= reach))) ? 1 : 0;
    }
    if (c->opt.kernel == 2 && c->opt.quad && !c->scene.nodes4.empty()) quad_walk_params(c, P); // the wavefront kernel walks the quad nodes
    if (c->opt.kernel == 2 && c->opt.groups && !c->scene.nodes8.empty()) { // group walk of sparse waves (oct nodes)
        P.nodes8 = (const PtNode8*)c->d_nodes8.p;
        P.root8 = c->scene.root8;
        P.groups = c->opt.groups;
    }
}

// ---- one-wave quad walks (pt_internal.h) --------------------------------------------------------------------------------
// The quad instances walk the scene's quad nodes, or a root that is itself a leaf (a scene of a few triangles has no nodes at all: root4
// is the leaf reference, the walk is one leaf step and touches no node).  Only a tree too deep for quad nodes (nodes4 cleared,
// root4 >= 0) and option quad = 0 leave them without a walk.
bool quad_walk_available(const pt_ctx* c) { return c->opt.quad && (!c->scene.nodes4.empty() || c->scene.root4 < 0); }

// The quad walk's own root and stack bound: up to three pushes per step.
void quad_walk_params(pt_ctx* c, PtKernelParams& P)
{
    P.nodes4 = (const PtNode4*)c->d_nodes4.p;
    P.root = c->scene.root4;
    P.stack_entries = 3 * c->scene.depth4 + 1;
}

int check_quad_walk_size(pt_ctx* c, const char* kernel)
{
    if (c->scene.bvh.tris.size() * sizeof(PtTri) > 0xffffffffull || c->scene.nodes4.size() * sizeof(PtNode4) > 0xffffffffull)
        return fail(c, PT_E_LIMIT, "the %s kernel needs triangle records and quad nodes below 4 GiB each (%zu triangle slots, %zu quad nodes)", kernel, c->scene.bvh.tris.size(), c->scene.nodes4.size());
    return PT_OK;
}

int shard_tile(int tile) { return ((tile < 8 ? 8 : tile) + 7) & ~7; }

int walk_workspace(pt_ctx* c, int cap, int lds_levels, int grid, hipStream_t stream, PtKernelParams& P, uint32_t** ovf)
{
    const size_t ovf_words = (size_t)std::max(0, cap - lds_levels) * 64 * (size_t)grid;
    int rc;
    if ((rc = ensure(c, c->d_aov_ws, (kWalkFlagWords + ovf_words) * 4))) return rc; // (growing it first waits on the host for what is in flight)
    HIP_TRY(c, hipMemsetAsync(c->d_aov_ws.p, 0, kWalkFlagWords * 4, stream));
    P.error_flag = (uint32_t*)c->d_aov_ws.p;
    *ovf = (uint32_t*)c->d_aov_ws.p + kWalkFlagWords;
    return PT_OK;
}

// What pt_render_device and a batch refuse alike, before anything is enqueued.  n_materials: rows of a batch's per-frame tables, compared
// with the scene's between the two (nullptr: a single frame brings no table).
int check_render_args(pt_ctx* c, int W, int H, int max_samples, int max_depth, const int32_t* n_materials)
{
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "no geometries (pt_upload_scene not called)");
    if (n_materials && *n_materials != c->scene.n_materials) return fail(c, PT_E_INVALID, "pt_render_batch: %d materials per frame, the scene has %d", *n_materials, c->scene.n_materials);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || max_samples <= 0 || max_depth < 0 || max_depth > 63 || (int64_t)W * H > (int64_t)0x7fffffff)
        return fail(c, PT_E_INVALID, "bad render size %dx%d spp %d depth %d (depth must be 0..63)", W, H, max_samples, max_depth);
    return PT_OK;
}

// A ray image's pointers (pt_render_rays*, pt_render_aov_rays*): NULL table or output, a device table that is not 16-byte aligned.
int check_ray_ptrs(pt_ctx* c, const char* who, const void* rays, const void* out, const char* out_name, bool device)
{
    if (!rays || !out) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !rays ? (device ? "d_rays" : "rays") : out_name);
    if (device && ((uintptr_t)rays & 15u)) return fail(c, PT_E_INVALID, "%s: d_rays is not 16-byte aligned (a record is four 16-byte loads)", who);
    return PT_OK;
}

// A ray image's table, after the sizes: a communicator (comm: the entry points; the twin renders none), and - where the host can read
// the W * H records - a record that is not finite or has no direction to normalize.
int check_ray_table(pt_ctx* c, const char* who, const void* rays, int W, int H, bool device, bool comm)
{
    if (comm && c->comm) return fail(c, PT_E_INVALID, "%s: a context with a communicator renders no ray images yet (render the ranks' shards with pt_set_pixel_shard and reduce them yourself)", who);
    if (!device) { // the records themselves: finite, and a direction to normalize
        const pt_ray_gen* r = (const pt_ray_gen*)rays;
        const int64_t n = (int64_t)W * H;
        for (int64_t i = 0; i < n; ++i) {
            const float* v[4] = {r[i].org, r[i].dir, r[i].du, r[i].dv};
            static const char* const name[4] = {"org", "dir", "du", "dv"};
            for (int k = 0; k < 4; ++k)
                if (!std::isfinite(v[k][0]) || !std::isfinite(v[k][1]) || !std::isfinite(v[k][2]))
                    return fail(c, PT_E_INVALID, "%s: record %lld (pixel %lld, %lld): %s is not finite", who, (long long)i, (long long)(i % W), (long long)(i / W), name[k]);
            if (r[i].dir[0] == 0.0f && r[i].dir[1] == 0.0f && r[i].dir[2] == 0.0f)
                return fail(c, PT_E_INVALID, "%s: record %lld (pixel %lld, %lld): dir is 0", who, (long long)i, (long long)(i % W), (long long)(i / W));
        }
    }
    return PT_OK;
}

// The largest |org| component of a host table: what decides the slab form of a ray image as the camera's origin does in walk_params.
float ray_table_far_o(const pt_ray_gen* rays, size_t n)
{
    float far_o = 0.0f;
    for (size_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) far_o = std::max(far_o, std::fabs(rays[i].org[a]));
    return far_o;
}

// ---- batches (pt_render_batch) ------------------------------------------------------------------------------------------
// K frames of the uploaded scene are stacked into a virtual image of W x (K * H) and rendered by ONE launch sequence over the queue of
// that image (pt_kernel_batch.hip).  What bounds K, from the code that sets each limit:
//   * a path slot holds its pixel as x | y << 16 (pt_kernel.hip, S_PIX) and pt_render_device accepts heights up to 65535: K * H <= 65535;
//   * plan_chunks refuses n_pixels >= 2^24 (the express ticket space): K * W * H < 2^24, taken for the whole frame whatever the rank's
//     shard, so that every rank of a communicator cuts a batch alike (one reduce per launch sequence on each).  With n_chunks <= 255
//     this also keeps the (pixel, chunk) tickets below plan_chunks' bound (2^24 * 255 < 0xfff00000);
//   * option "batch_frames" (> 0).
int64_t batch_max_frames(int W, int H, int max_frames)
{
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return 0;
    int64_t k = 65535 / H;
    k = std::min<int64_t>(k, ((int64_t)(1 << 24) - 1) / ((int64_t)W * H));
    if (max_frames > 0) k = std::min<int64_t>(k, max_frames);
    return k;
}

// Every frame's camera and material table (the 17 floats of the caller + the context's texture slot per row) in HBM, once per batch:
// d_batch_cams / d_batch_mats, which pt_render_batch and pt_render_aov_batch share.  The copies go on `stream`, which the caller has
// ordered after the context's last asynchronous call (async_call / blocking_call) - an earlier batch may still read the tables there -
// and the call waits for them on the host.
int stage_batch_tables(pt_ctx* c, const pt_frame* frames, int n_frames, hipStream_t stream)
{
    int rc;
    const size_t row = (size_t)c->scene.n_materials * PT_MAT_STRIDE;
    c->batch_cams_h.resize((size_t)n_frames * 12);
    c->batch_mats_h.assign((size_t)n_frames * row, 0.0f);
    for (int f = 0; f < n_frames; ++f) {
        std::memcpy(&c->batch_cams_h[(size_t)f * 12], &frames[f].camera, 48);
        float* dst = c->batch_mats_h.data() + (size_t)f * row;
        if (!frames[f].materials) { // the context's current table
            if (row) std::memcpy(dst, c->scene.materials.data(), row * sizeof(float));
            continue;
        }
        for (int i = 0; i < c->scene.n_materials; ++i) material_row(c, dst + (size_t)i * PT_MAT_STRIDE, frames[f].materials + (size_t)i * PT_MAT_FLOATS, i);
    }
    if ((rc = ensure(c, c->d_batch_cams, c->batch_cams_h.size() * 4)) || (rc = ensure(c, c->d_batch_mats, c->batch_mats_h.size() * 4))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_batch_cams.p, c->batch_cams_h.data(), c->batch_cams_h.size() * 4, hipMemcpyHostToDevice, stream));
    if (row) HIP_TRY(c, hipMemcpyAsync(c->d_batch_mats.p, c->batch_mats_h.data(), c->batch_mats_h.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(c, hipStreamSynchronize(stream)); // (as pt_set_materials: the staging vectors are the context's and may be refilled by the next call)
    return PT_OK;
}

// The end of every blocking call, after its kernels and its reduce are enqueued on the context's stream: the copies to the caller's host
// buffers between evr and evd (one with dst null is a buffer this caller does not receive: not the root, no RGBA8 asked for), the drain,
// the two times of pt_stats and the watchdog.
int drain(pt_ctx* c, std::initializer_list<D2H> copies)
{
    // kernels end (ev1) .. here: this rank's share of the reduce, incl. waiting for the slowest rank (of a batch: the last launch
    // sequence's reduce; the earlier ones lie inside kernel_ms)
    HIP_TRY(c, hipEventRecord(c->evr, c->stream));
    for (const D2H& d : copies)
        if (d.dst) HIP_TRY(c, hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->evd, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->last.stream = nullptr; // drained: the blocking call was ordered after the last asynchronous one (order_after_last)
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev1, c->evr));
    c->stats.reduce_ms = ms;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->evr, c->evd));
    c->stats.d2h_ms = ms;
    return check_watchdog(c);
}

} // namespace pti

namespace {

// frames > 1 (pt_render_batch): the queue of the virtual image of W x (frames * H) - the shard of ONE frame, repeated per frame with the
// ids moved down by the frames above it (id = x + W * (f * H + y)): a rank owns the same tiles in every frame.
// stream: the one the call enqueues on - an earlier launch sequence of the same batch may still read the queue there.
int ensure_queue(pt_ctx* c, int W, int H, int frames, hipStream_t stream)
{
    const QueueKey key{W, H, frames, c->rank, c->world, c->tile};
    if (c->queue_valid && c->queue == key) return PT_OK;
    const int64_t n1 = pt_shard_pixels(W, H, c->tile, c->rank, c->world, nullptr, 0);
    if (n1 < 0) return fail(c, PT_E_INVALID, "invalid pixel shard (%d of %d)", c->rank, c->world);
    const int64_t n = n1 * frames;
    int rc = wait_idle(c); // d_pixels is rewritten in place: after the frame in flight, whichever stream it is on ...
    if (rc) return rc;
    if (stream != c->stream) HIP_TRY(c, hipStreamSynchronize(stream)); // ... and after what this call itself has enqueued so far
    std::vector<uint32_t> ids((size_t)n);
    pt_shard_pixels(W, H, c->tile, c->rank, c->world, ids.data(), n1);
    for (int f = 1; f < frames; ++f)
        for (int64_t i = 0; i < n1; ++i) ids[(size_t)(f * n1 + i)] = ids[(size_t)i] + (uint32_t)f * (uint32_t)W * (uint32_t)H;
    if ((rc = upload(c, c->d_pixels, ids.data(), ids.size() * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // ids is a local
    c->n_pixels = (uint32_t)n;
    c->queue = key;
    c->queue_valid = true;
    return PT_OK;
}

#ifndef PT_DEFAULT_NS
#define PT_DEFAULT_NS 96 // path slots per wave of the wavefront kernel: 16 waves/CU up to 104; 64..255 swept on C4 (profiles/r01_summary.md), 88..104 within 1 %
#endif
static_assert(PT_DEFAULT_NS >= 16 && PT_DEFAULT_NS <= 252, "PT_DEFAULT_NS: 16..252 path slots per wave");

// Chunk schedule of one wavefront launch over `total` samples per pixel: n_full chunks of `chunk` samples, then the rest in
// halving chunks (rem/2, rem/4, ... >= tail_min).  A frame ends when its slowest in-flight work item ends, so the
// last items must be short (profiles/r01_summary.md, "wind-down").
struct Schedule { int chunk = 0, n_full = 0, n_chunks = 1, tail_len[PT_MAX_TAIL_CHUNKS] = {}; };

Schedule make_schedule(int total, int chunk, int rem_min, int tail_min)
{
    Schedule sc;
    sc.chunk = std::max(1, std::min(chunk, total));
    sc.n_full = total / sc.chunk;
    int rem = total - sc.n_full * sc.chunk;
    if (tail_min > 0 && sc.n_full > 0 && rem < rem_min) { --sc.n_full; rem += sc.chunk; }
    int n_tail = 0;
    while (rem > 0) {
        int len = rem;
        if (tail_min > 0 && rem > tail_min && n_tail < PT_MAX_TAIL_CHUNKS - 1) len = std::max(tail_min, (rem + 1) / 2);
        sc.tail_len[n_tail++] = len;
        rem -= len;
    }
    sc.n_chunks = sc.n_full + n_tail;
    return sc;
}

// What one frame launches, decided before any buffer is sized (plan_frame).
// kernel 1 (lane-per-pixel): optional spp chunks = separate launches.
// Wavefront kernel, schedule 1 (default): a short cost pre-pass (pre samples of every pixel, rays counted), a counting sort of the
// pixel queue by that cost, then ONE persistent launch over the cost-ordered queue whose first chunk is sticky_pct % of the remaining
// samples (a slot keeps its pixel, no hand-offs, expensive pixels start first) and whose last samples go round in halving chunks
// through the per-chunk rings, so that the frame ends on ~n_pixels short work items.
// schedule 0 (or spp_per_launch, which the resumability tests use): one launch, chunk_spp chunks + halving tail.
// All schedules give the same image bit for bit (a pixel's stream does not depend on who renders it, or when).
// The families of the render kernel (pt_launch.h), one build of pt_kernel.hip each.  A frame runs ONE: the caller asks for kBatch or
// kRayImage before plan_frame, which turns kFrame into kWatertight with option "watertight" and refuses the combinations that have no build.
enum RenderFamily { kFrame, kWatertight, kBatch, kRayImage };
const struct RenderInstance {
    hipError_t (*geometry)(int variant, int count, int stack_entries, int group_entries, int want_ns, int exact, PtGeometry* g);
    hipError_t (*launch)(const PtKernelParams* p, const PtKernelParams* d_params, int variant, int grid, size_t lds_bytes, hipStream_t stream, int count);
} kRenderInstance[4] = {{pt_kernel_geometry, pt_launch_render}, {pt_wt_kernel_geometry, pt_launch_render_wt}, {pt_batch_kernel_geometry, pt_launch_render_batch},
                        {pt_rayimage_kernel_geometry, pt_launch_render_rayimage}};

struct FramePlan {
    RenderFamily family = kFrame;   // whose geometry sized the frame and whose launcher runs it
    int variant = 0, use_count = 0; // instance of that family and whether it is the instrumented one
    PtGeometry geo{};               // its launch geometry
    int bpc = 0, grid = 0;          // workgroups per CU, of the (main) launch
    int ring_grid = 0;              // with a tier plan: the workgroups of the ring schedule (the plan's fallback; the pre-pass launches these)
    bool sorted = false;            // cost pre-pass, queue sort, main launch
    bool tiers = false;             // ... whose main launch has a whole-pixel tier plan prepared (pt_plan_tiers_kernel)
    int pre = 0;                    // samples of the cost pre-pass
    int n_launch = 1, S = 0;        // launches; samples per launch (kernel 1)
    Schedule sc;                    // chunk schedule of the (main) wavefront launch
    int tail_min = 16;              // smallest chunk of its halving tail
    size_t lap_ticks_ofs = 0;       // where the timelines start in d_laps (plan_chunks)
    uint32_t n_express = 0;         // express pixels (pt_kernel.hip, take_ticket), their waves and pixels per express wave
    int express_waves = 0, ns_express = 0;
    int sample_base = 0;            // an add of the progressive accumulation that continues its pixels (accum_frame): every launch has sample_begin != 0
};

// Samples, chunks and express pixels of a wavefront frame whose launch geometry plan_frame has fixed.
int plan_chunks(pt_ctx* c, bool group_walk, int max_samples, FramePlan& f)
{
    f.tail_min = c->opt.chunk_tail_min >= 0 ? c->opt.chunk_tail_min : 16; // (automatic: set per schedule below)
    f.S = max_samples;
    f.n_launch = f.sorted ? 2 : 1;
    const int ns = f.geo.ns;
    if (f.sorted) {
        const int rest = max_samples - f.pre;
        // Share of a pixel's remaining samples that its first slot renders in one go.  With many more pixels than slots the
        // frame is throughput-bound and hand-offs are pure overhead: 80 %; with fewer pixels per slot 50-65 % (a launch whose
        // pixels all have a slot and whose costs have a tail runs the tier schedule instead).
        int sticky = c->opt.sticky_pct;
        if (sticky < 1) {
            const double ratio = (double)c->n_pixels / ((double)c->num_cus * (double)f.bpc * (double)ns);
            sticky = (int)std::min(80.0, 50.0 + 6.0 * ratio); // (rounds 1-2, queue ordered by rays: 10-75, rising with the ratio; re-swept with the
                                                             // queue ordered by time: C4 80, 1/2 shard and C3 65, 1/4 shard 50-65, C2 60 - r3_ab57/58.log)
        }
        // With the queue ordered by the TIME of a pixel's samples the hand-offs of the tail buy little and every lap is a barrier of
        // sorts: the last quarter goes in two chunks, not five (C4 528 -> 500 ms, C3 161 -> 153; smallest tail chunk 16 / 32 / 64 / 128
        // of 1016 samples: 528 / 515 / 505 / 498 ms; profiles/r03_logs/r3_ab54.log).
        if (c->opt.chunk_tail_min < 0) f.tail_min = std::max(16, rest / 8);
        const int big = std::max(1, (int)((int64_t)rest * sticky / 100));
        f.sc = make_schedule(rest, big, rest - big, f.tail_min);
    } else {
        const int chunk = std::min(c->opt.spp_per_launch > 0 ? c->opt.spp_per_launch : c->opt.chunk_spp, std::min(max_samples, 65535));
        f.sc = make_schedule(max_samples, chunk, 1, f.tail_min);
    }
    const int n_chunks = f.sc.n_chunks;
    // Layout of d_laps (never a plain store in a cache line that also holds device-scope atomics): [0] watchdog flag | +256 B: ring fill
    // counters (n_chunks + 1, + the pre-pass's spare) | 256-B aligned: diagnostics timelines of the two launches.
    f.lap_ticks_ofs = ((256 + (size_t)(n_chunks + 3) * 4 + 255) / 256) * 256;
    if ((uint64_t)c->n_pixels * (uint64_t)n_chunks >= 0xfff00000ull) return fail(c, PT_E_LIMIT, "too many (pixel, chunk) tickets");
    if (n_chunks > 255 || c->n_pixels >= (1u << 24)) return fail(c, PT_E_LIMIT, "the wavefront kernel needs n_chunks <= 255 and < 2^24 pixels per rank (raise chunk_spp)");
    // Express pixels (pt_kernel.hip, take_ticket): the most expensive entries of the cost-ordered queue get waves of their own when the
    // frame is bound by its longest sample chains, i.e. when (nearly) every pixel is in flight from the start - few pixels per path slot
    // (a shard of a multi-GPU frame, a small image).  A throughput-bound frame (many pixels per slot) has none: sparse waves would only
    // take wave slots from it.  Options "express_permille" (-1 = automatic: 10 per mille up to 1.5 pixels per slot, 0 from 4),
    // "ns_express" (8 pixels per express wave), at most an eighth of the waves.
    if (f.sorted && group_walk && n_chunks <= 254 && (uint64_t)c->n_pixels * (uint64_t)n_chunks < 0xE0000000ull) {
        int& rgrid = f.tiers ? f.ring_grid : f.grid; // the workgroups of the ring schedule (with a tier plan the launch has all resident ones)
        const double ratio = (double)c->n_pixels / ((double)rgrid * (double)ns);
        double permille = c->opt.express_permille >= 0 ? (double)c->opt.express_permille : (ratio <= 1.5 ? 10.0 : (ratio >= 4.0 ? 0.0 : 10.0 * (4.0 - ratio) / 2.5));
        const int nse = std::max(1, std::min(c->opt.ns_express, ns));
        uint64_t want = (uint64_t)((double)c->n_pixels * permille / 1000.0);
        const int capacity = c->num_cus * f.bpc;
        // at most an eighth of the ring schedule's waves, or what the bulk leaves free.  (Round 4 tried up to 60 % of the waves for 1-15 % of the
        // pixels at 8-48 per wave, also with the grid oversubscribed by the express waves: world 2 351 -> 400-470 ms, world 4 269 -> 300-370,
        // profiles/r04_notes.md 5.)
        const int cap_waves = std::max(rgrid / 8, std::min(capacity / 2, capacity - rgrid));
        want = std::min<uint64_t>(want, (uint64_t)cap_waves * (uint64_t)nse);
        if (want > 0 && want < c->n_pixels) {
            f.n_express = (uint32_t)want;
            f.express_waves = (int)((want + (uint64_t)nse - 1) / (uint64_t)nse);
            f.ns_express = nse;
            // wave slots the bulk does not fill (a shard, a small image) hold the express waves on top of the bulk's
            rgrid = std::min(capacity, (int)(((long)c->n_pixels - (long)f.n_express + ns - 1) / ns) + f.express_waves);
        }
    }
    return PT_OK;
}

// The launch plan of a frame from the context's options, the pixel queue, the device and the tree bounds in P.  Its only device
// interaction is the geometry query of the kernel instance; every PT_E_LIMIT refusal of a render happens here.
int plan_frame(pt_ctx* c, const PtKernelParams& P, int max_samples, FramePlan& f)
{
    // variant of the launch: the wavefront kernel's product instance (2) unless it needs scratch in this build - then its fallback
    // instance with the larger register budget (3): slower (12 instead of 16 waves per CU), the same arithmetic
    // (the one-level walk over PtNode[] - option quad = 0, or a tree too deep for the quad walk's stack bound - is compiled into the
    // instrumented instance only: the product instance is kept small for the instruction cache)
    // option "watertight": the same three instances from pt_kernel_wt.hip, chosen and refused by the same rules (a 128-VGPR watertight
    // instance that needs scratch falls back to the 168-VGPR one, a fallback that needs it too is PT_E_LIMIT below)
    const bool wt = c->opt.watertight != 0;
    if (wt && c->opt.kernel != 2) return fail(c, PT_E_INVALID, "watertight = 1: the lane-per-pixel kernel (option kernel = 1) has no watertight form");
    if (wt && f.family == kRayImage) return fail(c, PT_E_INVALID, "pt_render_rays: ray images have no watertight instances (option watertight = 1); set watertight = 0");
    if (wt && f.family == kBatch) return fail(c, PT_E_INVALID, "pt_render_batch: batches have no watertight instances (option watertight = 1); render the frames one by one or set watertight = 0");
    if (wt) f.family = kWatertight;
    f.use_count = (c->opt.count || (c->opt.kernel == 2 && !P.nodes4)) ? 1 : 0;
    f.variant = c->opt.kernel == 2 && c->opt.fallback && !f.use_count ? 3 : c->opt.kernel;
    // the wavefront kernel's quad-node and leaf steps address their records with 32-bit byte offsets from the buffer base (node4_step, leaf_test)
    int rc;
    if (c->opt.kernel == 2 && (rc = check_quad_walk_size(c, "wavefront"))) return rc;
    // The wavefront kernel keeps `ns` pixels in flight per wave; shrink ns when the image is too small to give every resident wave a
    // full set (e.g. 512x512 over 4096 waves), otherwise use the default.
    const int group_entries = P.nodes8 ? 7 * c->scene.depth8 + 1 : 0;
    int want_ns = c->opt.slots_per_wave > 0 ? c->opt.slots_per_wave : PT_DEFAULT_NS;
    const PtGeometry& g = f.geo;
    auto geometry = [&] { return kRenderInstance[f.family].geometry(f.variant, f.use_count, P.stack_entries, group_entries, want_ns, P.box_exact, &f.geo); };
    hipError_t ge = geometry();
    if (ge == hipErrorInvalidConfiguration && f.variant == 2 && !f.use_count) {
        f.variant = 3;
        ge = geometry();
    }
    if (ge == hipErrorInvalidConfiguration)
        return fail(c, PT_E_LIMIT, f.use_count ? "the instrumented instance of the render kernel needs scratch in this build; such builds rendered wrong pixels and are refused (pt_kernel.hip; tests/test_abi_host.py reads hipcc's resource report)"
                                               : "this build of the render kernel spills registers to scratch even in its fallback instance; such builds rendered wrong pixels and are refused (pt_kernel.hip)");
    HIP_TRY(c, ge);
    if (c->opt.kernel == 2 && c->opt.slots_per_wave == 0 && g.max_blocks_per_cu > 0) {
        // small images: fewer slots per wave so that at least 8 waves per CU have pixels (never below 64)
        const long fit = (long)c->n_pixels / ((long)c->num_cus * 8);
        if (fit < want_ns) {
            want_ns = (int)std::max(64L, fit);
            HIP_TRY(c, geometry());
        }
    }
    if (g.max_blocks_per_cu < 1) return fail(c, PT_E_LIMIT, "render kernel does not fit a CU (LDS %zu bytes, BVH depth %d)", g.lds_bytes, c->scene.bvh.depth);
    f.bpc = c->opt.blocks_per_cu > 0 ? std::min(c->opt.blocks_per_cu, g.max_blocks_per_cu) : g.max_blocks_per_cu;
    const long capacity = (long)c->num_cus * f.bpc;
    const int per_wg = c->opt.kernel == 1 ? g.block : g.ns; // never more path slots than pixels: a pixel's chunks are sequential
    f.grid = (int)std::max(1L, std::min(((long)c->n_pixels + per_wg - 1) / per_wg, capacity));
    f.pre = c->opt.prepass_spp > 0 ? c->opt.prepass_spp : 8; // samples of the cost pre-pass
    f.sorted = c->opt.kernel == 2 && c->opt.schedule == 1 && c->opt.spp_per_launch == 0 && max_samples >= 4 * f.pre && max_samples <= 65535;
    // Whole-pixel schedule (pt_kernel.hip, TIERS): when every pixel can have a path slot from the start, the main launch hands out
    // pixels instead of (pixel, chunk) tickets, and every wave serves one cost class with as few pixels as that class needs - the plan
    // is made on the device from the histogram of the counting sort (pt_plan_tiers_kernel).  Option "whole": -1 automatic, 0 never.
    if (f.sorted && P.nodes8 && c->opt.whole != 0 && c->opt.slots_per_wave == 0) {
        for (int nsd = 96; nsd <= 104 && !f.tiers; nsd += 8) { // 16 waves per CU up to 104 slots
            if (c->opt.whole < 1 && (long)c->n_pixels + (long)PT_MAX_TIERS * nsd > capacity * nsd) continue; // (one partly filled wave per class)
            want_ns = nsd;
            HIP_TRY(c, geometry());
            if (g.max_blocks_per_cu >= f.bpc && g.ns == nsd) {
                f.tiers = true;
                f.ring_grid = (int)std::max(1L, std::min(((long)c->n_pixels + g.ns - 1) / g.ns, capacity)); // what the ring schedule would launch
                f.grid = (int)capacity;
            }
        }
        if (!f.tiers) {
            want_ns = PT_DEFAULT_NS;
            HIP_TRY(c, geometry());
        }
    }
    // the tier plan lives on the cost estimate: twice the samples (1/8 shard of C4 218 -> 201 ms; a throughput-bound frame gains nothing)
    if (f.tiers && c->opt.prepass_spp == 0 && max_samples >= 4 * 16) f.pre = 16;
    if (c->opt.kernel == 1) {
        f.S = std::min(c->opt.spp_per_launch > 0 ? std::min(c->opt.spp_per_launch, max_samples) : max_samples, 65535);
        f.n_launch = (max_samples + f.S - 1) / f.S;
        return PT_OK;
    }
    return plan_chunks(c, P.nodes8 != nullptr, max_samples, f);
}

// Every device buffer of a frame sized from its plan, and every clear it needs: all of it is enqueued before the frame's first event.
// (H: rows of the launch's image - of the virtual image of a batch's launch sequence; first = false: a later launch sequence of a batch,
// whose work counters go on counting)
int frame_buffers(pt_ctx* c, const FramePlan& f, int W, int H, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream, bool first = true)
{
    int rc;
    const int n_chunks = f.sc.n_chunks;
    if (f.geo.state_words && (rc = ensure(c, c->d_slots, f.geo.state_words * 4 * (size_t)f.grid))) return rc;
    if (f.sorted) {
        if ((rc = ensure(c, c->d_cost, (size_t)W * H))) return rc; // cost image; zero where this rank owns nothing
        if ((rc = ensure(c, c->d_bucket, (size_t)c->n_pixels))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_cost.p, 0, (size_t)W * H, stream));
        if ((rc = ensure(c, c->d_sorted, (size_t)c->n_pixels * 4))) return rc;
        if ((rc = ensure(c, c->d_sort_scratch, pt_sort_scratch_bytes(c->n_pixels)))) return rc;
    }
    if (c->opt.kernel == 2) {
        // one ring of ready pixels per chunk index: ring c holds, in completion order of chunk c - 1, the pixels whose chunk c
        // may start.  d_laps = watchdog flag + one fill counter per ring (layout: plan_chunks, lap_ticks_ofs).
        const size_t laps_bytes = f.lap_ticks_ofs + ((size_t)PT_LAP_REGION(n_chunks) + (size_t)PT_LAP_REGION(1)) * 8;
        if ((rc = ensure(c, c->d_laps, laps_bytes))) return rc;
        if ((rc = ensure(c, c->d_ring, (size_t)c->n_pixels * 4 * (size_t)n_chunks))) return rc;
        HIP_TRY(c, hipMemsetAsync(c->d_laps.p, 0, laps_bytes, stream));
        if (n_chunks > 1) HIP_TRY(c, hipMemsetAsync(c->d_ring.p, 0, (size_t)c->n_pixels * 4 * (size_t)n_chunks, stream));
        if ((rc = ensure(c, c->d_params, sizeof(PtKernelParams) * (size_t)f.n_launch))) return rc;
    }
    if ((rc = ensure(c, c->d_heads, (size_t)f.n_launch * PT_HEADS_WORDS * 4))) return rc; // per launch: the ticket counter, the express counter 256 bytes on, the tier counters
    HIP_TRY(c, hipMemsetAsync(c->d_heads.p, 0, (size_t)f.n_launch * PT_HEADS_WORDS * 4, stream));
    if (f.tiers && (rc = ensure(c, c->d_tiers, (1 + PT_MAX_TIERS * PT_TIER_WORDS) * 4))) return rc;
    if (d_out_rgb) HIP_TRY(c, hipMemsetAsync(d_out_rgb, 0, (size_t)W * H * 3 * sizeof(float), stream)); // (null: accum_frame, whose launches write no framebuffer)
    if (d_out_rgba8) HIP_TRY(c, hipMemsetAsync(d_out_rgba8, 0, (size_t)W * H * 4, stream));
    if (f.n_launch > 1 || n_chunks > 1) {
        if ((rc = ensure(c, c->d_rng, (size_t)W * H * 4))) return rc;
        if ((rc = ensure(c, c->d_accum, (size_t)W * H * 12))) return rc;
    }
    if (f.use_count) {
        if ((rc = ensure(c, c->d_counters, sizeof(PtCounters)))) return rc;
        if (first) HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(PtCounters), stream));
    }
    if (c->opt.latency && f.sorted) {
        if ((rc = ensure(c, c->d_dbg_start, (size_t)W * H * 8))) return rc; // + rays per pixel (instrumented instance)
        HIP_TRY(c, hipMemsetAsync(c->d_dbg_start.p, 0, (size_t)W * H * 8, stream));
    }
    return PT_OK;
}

// The parameters every launch of the frame shares (P holds the scene and the tree walk already: fill_params, pt_render_device).
void frame_params(pt_ctx* c, const FramePlan& f, const pt_camera* cam, int W, int H, int max_samples, int max_depth, void* d_out_rgb, void* d_out_rgba8,
                  PtKernelParams& P)
{
    P.lds_levels = f.geo.lds_levels;
    P.ns = f.geo.ns;
    P.slot_state = f.geo.state_words ? (uint32_t*)c->d_slots.p : nullptr;
    std::memcpy(P.cam, cam, sizeof(float) * 12);
    P.pixel_ids = (const uint32_t*)c->d_pixels.p;
    P.n_pixels = c->n_pixels;
    P.rng_state = (uint32_t*)c->d_rng.p;
    P.accum = (float*)c->d_accum.p;
    P.out_rgb = (float*)d_out_rgb;
    P.out_rgba8 = (uint32_t*)d_out_rgba8;
    P.counters = f.use_count ? (PtCounters*)c->d_counters.p : nullptr;
    P.width = W;
    P.height = H;
    P.max_samples = max_samples;
    P.max_depth = max_depth;
    P.ring = (uint32_t*)c->d_ring.p;
    P.ring_tail = c->d_laps.p ? (uint32_t*)c->d_laps.p + 64 : nullptr;
    P.error_flag = (uint32_t*)c->d_laps.p;
    P.lap_ticks = (unsigned long long*)((char*)c->d_laps.p + f.lap_ticks_ofs);
    P.timeline = c->opt.timeline;
    if (c->opt.latency && f.sorted) P.dbg_cost = (uint8_t*)c->d_cost.p;
    P.census_mode = c->opt.census_mode;
    P.chunk_spp = f.sc.chunk;
    P.n_chunks = f.sc.n_chunks;
    P.n_full = f.sc.n_full;
    for (int i = 0; i < PT_MAX_TAIL_CHUNKS; ++i) P.tail_len[i] = f.sc.tail_len[i];
    P.n_tickets = c->n_pixels * (uint32_t)f.sc.n_chunks;
    P.ns_express = f.ns_express;
}

// What launch l of the frame changes in P: its samples, and with a cost pre-pass (sorted) launch 0 is that pre-pass over the queue in
// shard order, one chunk per pixel, and launch 1 everything else over the cost-ordered queue, expensive pixels first.
void launch_params(pt_ctx* c, const FramePlan& f, int l, int max_samples, PtKernelParams& P)
{
    P.queue_head = (uint32_t*)c->d_heads.p + PT_HEADS_WORDS * l;
    if (!f.sorted) {
        P.sample_begin = f.sample_base + l * f.S;
        P.sample_count = std::min(f.S, max_samples - l * f.S);
        return;
    }
    const bool pre = l == 0;
    const int n_chunks = f.sc.n_chunks;
    P.sample_begin = f.sample_base + (pre ? 0 : f.pre);
    P.sample_count = pre ? f.pre : max_samples - f.pre;
    P.pixel_ids = pre ? (const uint32_t*)c->d_pixels.p : (const uint32_t*)c->d_sorted.p;
    P.cost_out = pre ? (uint8_t*)c->d_cost.p : nullptr;
    P.dbg_start = (!pre && c->opt.latency) ? (uint32_t*)c->d_dbg_start.p : nullptr;
    P.lap_ticks = (unsigned long long*)((char*)c->d_laps.p + f.lap_ticks_ofs) + (pre ? PT_LAP_REGION(n_chunks) : 0); // the pre-pass's block follows the main launch's
    P.ring_tail = (uint32_t*)c->d_laps.p + 64 + (pre ? n_chunks : 0); // the pre-pass only uses its [1]: the spare counter
    P.chunk_spp = pre ? P.sample_count : f.sc.chunk;
    P.n_chunks = pre ? 1 : n_chunks;
    P.n_full = pre ? 1 : f.sc.n_full;
    P.n_tickets = pre ? c->n_pixels : (c->n_pixels - f.n_express) * (uint32_t)n_chunks;
    P.n_express = pre ? 0 : f.n_express;
    P.express_waves = pre ? 0 : f.express_waves;
    // the tier plan decides on the device: pixels by cost class (then none of the above is used), or the ring schedule as prepared
    P.tiers = (!pre && f.tiers) ? (const uint32_t*)c->d_tiers.p : nullptr;
    if (!pre && f.tiers) P.ring_grid = f.ring_grid;
}

// End of a frame or launch sequence, after its last launch (f == nullptr: a rank that owns no pixel and launched nothing): the one place
// that writes what pt_synchronize, pt_get_stats and the diagnostics readers look at.  The kernel's own figures (registers, block, LDS,
// chunks) stay those of the last frame that ran one.  first = false: a later launch sequence of a batch, which adds its launches and
// its sequence to what the earlier ones left.  (flag_pending then says that SOME sequence ran kernels, which is the same as "this one
// did": every sequence of a batch has the queue of one frame's shard, repeated per frame - ensure_queue - so a rank without a tile
// runs no kernel in any of them and a rank with one runs kernels in all.)
int finish_frame(pt_ctx* c, hipStream_t stream, int W, int H, const FramePlan* f, int stack_entries, bool first = true)
{
    HIP_TRY(c, hipEventRecord(c->ev1, stream));
    LastFrame& L = c->last;
    L.ev_pending = true;
    L.flag_pending = (!first && L.flag_pending) || f != nullptr;
    L.launches = (first ? 0 : L.launches) + (f ? f->n_launch : 0);
    L.sorted = f && f->sorted;
    L.w = W;
    L.h = H;
    L.seqs = first ? 1 : L.seqs + 1;
    L.aov_flag_pending = false;
    c->stats.express_pixels = f ? (int32_t)f->n_express : 0;
    c->stats.whole_pixels = f && f->tiers ? (int32_t)c->n_pixels : 0;
    c->stats.prepass_spp = f && f->sorted ? f->pre : 0;
    c->stats.grid = f ? f->grid : 0;
    if (!f) return PT_OK;
    if (c->opt.kernel == 2) { // (d_laps keeps the layout of the last wavefront frame)
        L.chunks = f->sc.n_chunks;
        L.lap_ticks_ofs = f->lap_ticks_ofs;
    }
    c->stats.vgprs = f->geo.vgprs;
    c->stats.kernel_variant = f->variant;
    c->stats.lds_bytes = (int)f->geo.lds_bytes;
    c->stats.block = f->geo.block;
    c->stats.stack_entries = stack_entries;
    return PT_OK;
}

// The frame of a rank that owns no tile (fewer tiles than ranks, e.g. 64x64 / tile 16 at world 8): all zeros, and no kernel runs.
// (Round-3 advisor finding: the main launch of such a rank read a tier table nobody had written - the sort and the plan kernel return
// early for an empty queue.)  first = false: a later launch sequence of a batch, whose work counters go on counting.
int empty_frame(pt_ctx* c, hipStream_t stream, int W, int H, void* d_out_rgb, void* d_out_rgba8, bool first = true)
{
    HIP_TRY(c, hipMemsetAsync(d_out_rgb, 0, (size_t)W * H * 3 * sizeof(float), stream));
    if (d_out_rgba8) HIP_TRY(c, hipMemsetAsync(d_out_rgba8, 0, (size_t)W * H * 4, stream));
    if (first && c->opt.count && c->d_counters.p) HIP_TRY(c, hipMemsetAsync(c->d_counters.p, 0, sizeof(PtCounters), stream));
    return finish_frame(c, stream, W, H, nullptr, 0, first);
}

// The launches of a planned frame (H: rows of the launch's image, see frame_buffers).  mark_prepass: record evm after the queue sort
// (a batch does so in its first launch sequence only: pt_stats.prepass_ms).
int run_launches(pt_ctx* c, const FramePlan& f, PtKernelParams& P, int W, int H, int max_samples, hipStream_t stream, bool mark_prepass)
{
    for (int l = 0; l < f.n_launch; ++l) {
        launch_params(c, f, l, max_samples, P);
        if (f.sorted && l == 1) { // the queue in cost order (and the tier plan) from the pre-pass's cost image
            // ... or from the image a test has set for launch sequences of this size (pt_debug_set_cost_image): the pre-pass ran, its costs are replaced
            if (c->cost_image_w == W && c->cost_image_h == H)
                HIP_TRY(c, hipMemcpyAsync(c->d_cost.p, c->d_cost_image.p, (size_t)W * H, hipMemcpyDeviceToDevice, stream));
            HIP_TRY(c, pt_launch_sort_pixels((const uint8_t*)c->d_cost.p, W, H, c->opt.cost_radius, (const uint32_t*)c->d_pixels.p, (uint32_t*)c->d_sorted.p,
                                             c->n_pixels, (uint32_t)f.pre, (uint32_t*)c->d_sort_scratch.p, (uint8_t*)c->d_bucket.p, stream));
            if (f.tiers) HIP_TRY(c, pt_launch_plan_tiers((const uint32_t*)c->d_sort_scratch.p, c->n_pixels, f.grid, f.geo.ns, c->opt.whole > 0, (uint32_t*)c->d_tiers.p, stream));
            if (mark_prepass) HIP_TRY(c, hipEventRecord(c->evm, stream));
        }
        const PtKernelParams* dP = (const PtKernelParams*)c->d_params.p + l; // one block per launch: launch l+1's copy never races launch l
        if (c->opt.kernel == 2) HIP_TRY(c, pt_launch_store_params(&P, (PtKernelParams*)dP, stream)); // by value: P is reused for the next launch
        // (with a tier plan prepared only the main launch has every resident workgroup; the pre-pass measures the pixels' costs in waves
        // as dense as the ring schedule's - C2 74.3 -> 71 ms, 1/8 shard 198 -> 194)
        const int grid = (f.tiers && l == 0) ? f.ring_grid : f.grid;
        HIP_TRY(c, kRenderInstance[f.family].launch(&P, dP, f.variant, grid, f.geo.lds_bytes, stream, f.use_count));
    }
    return PT_OK;
}

struct BatchArgs {
    const pt_frame* frames;
    int n_frames, W, H, max_samples, max_depth;
};

// One launch sequence: frames [f0, f0 + K) of the batch into d_out_rgb / d_out_rgba8 (already offset to frame f0); first: of the batch.
int batch_sequence(pt_ctx* c, const BatchArgs& a, int f0, int K, bool first, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    const int W = a.W, H = a.H, Hv = K * a.H;
    int rc = ensure_queue(c, W, H, K, stream);
    if (rc) return rc;
    if (c->n_pixels == 0) return empty_frame(c, stream, W, Hv, d_out_rgb, d_out_rgba8, first);
    PtKernelParams P;
    walk_params(c, &a.frames[f0].camera, P);
    // one slab form per launch sequence: the subtracting one if ANY of its cameras is beyond the switch of walk_params (boxes only
    // have to be conservative, so no image changes)
    for (int f = 1; f < K && !P.box_exact; ++f) {
        PtKernelParams Q;
        walk_params(c, &a.frames[f0 + f].camera, Q);
        P.box_exact = Q.box_exact;
    }
    FramePlan f;
    f.family = kBatch;
    if ((rc = plan_frame(c, P, a.max_samples, f))) return rc;
    if ((rc = frame_buffers(c, f, W, Hv, d_out_rgb, d_out_rgba8, stream, first))) return rc;
    frame_params(c, f, &a.frames[f0].camera, W, H, a.max_samples, a.max_depth, d_out_rgb, d_out_rgba8, P);
    P.batch_frames = K;
    P.batch_cams = (const float*)c->d_batch_cams.p + (size_t)12 * f0;
    P.materials = (const float*)c->d_batch_mats.p + (size_t)f0 * c->scene.n_materials * PT_MAT_STRIDE;
    if ((rc = run_launches(c, f, P, W, Hv, a.max_samples, stream, first))) return rc;
    return finish_frame(c, stream, W, Hv, &f, P.stack_entries, first);
}

// The whole batch on `stream`; with reduce = true (pt_render_batch) one pt_reduce_framebuffer per launch sequence over all of its frames.
int batch_device(pt_ctx* c, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth,
                 void* d_out_rgb, void* d_out_rgba8, void* d_reduce_rgba8, hipStream_t stream, bool reduce)
{
    if (n_frames < 1 || !frames) return fail(c, PT_E_INVALID, "pt_render_batch: a batch needs at least one frame (n_frames %d%s)", n_frames, frames ? "" : ", frames NULL");
    int rc = check_render_args(c, W, H, max_samples, max_depth, &n_materials);
    if (rc) return rc;
    // what only exists for one frame at a time is refused by name, never rendered by a loop of single frames
    if (c->opt.kernel != 2) return fail(c, PT_E_INVALID, "pt_render_batch: the lane-per-pixel kernel (option kernel = 1) has no batch form");
    if (c->opt.watertight) return fail(c, PT_E_INVALID, "pt_render_batch: batches have no watertight instances (option watertight = 1); render the frames one by one or set watertight = 0");
    if (c->opt.latency) return fail(c, PT_E_INVALID, "pt_render_batch: the per-pixel latency diagnostics (option latency) are per frame; switch them off for a batch");
    if (c->opt.timeline) return fail(c, PT_E_INVALID, "pt_render_batch: the chunk timeline (option timeline) is per frame; switch it off for a batch");
    if ((rc = need_device(c))) return rc;
    const int64_t kmax = batch_max_frames(W, H, c->opt.batch_frames);
    if (kmax < 1) return fail(c, PT_E_LIMIT, "pt_render_batch: one %dx%d frame already exceeds a launch sequence (< 2^24 pixels)", W, H);
    HIP_TRY(c, hipSetDevice(c->device));
    const int n_seq = (int)((n_frames + kmax - 1) / kmax);
    if ((rc = ensure(c, c->d_seq_flags, (size_t)n_seq * 4))) return rc;
    if ((rc = stage_batch_tables(c, frames, n_frames, stream))) return rc;
    const BatchArgs a{frames, n_frames, W, H, max_samples, max_depth};
    const size_t npx = (size_t)W * H;
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    for (int s = 0, f0 = 0; f0 < n_frames; ++s) {
        const int K = (int)std::min<int64_t>(kmax, n_frames - f0);
        float* o = (float*)d_out_rgb + (size_t)f0 * npx * 3;
        uint32_t* o8 = d_out_rgba8 ? (uint32_t*)d_out_rgba8 + (size_t)f0 * npx : nullptr;
        if ((rc = batch_sequence(c, a, f0, K, s == 0, o, o8, stream))) return rc;
        // the sequence's watchdog flag, kept for check_watchdog: the next sequence clears the block it lives in
        if (f0 + K < n_frames && c->d_laps.p && c->last.flag_pending) HIP_TRY(c, hipMemcpyAsync((uint32_t*)c->d_seq_flags.p + s, c->d_laps.p, 4, hipMemcpyDeviceToDevice, stream));
        else if (f0 + K < n_frames) HIP_TRY(c, hipMemsetAsync((uint32_t*)c->d_seq_flags.p + s, 0, 4, stream));
        if (reduce && c->comm) {
            uint32_t* r8 = d_reduce_rgba8 ? (uint32_t*)d_reduce_rgba8 + (size_t)f0 * npx : nullptr;
            if ((rc = reduce_framebuffer(c, o, r8, (int64_t)K * (int64_t)npx, stream))) return rc;
        }
        f0 += K;
    }
    return PT_OK;
}

// The end of pt_render and pt_render_batch: npx pixels from d_out / d_out8 to the root's host buffers.
int read_back(pt_ctx* c, bool root, float* out_rgb, uint32_t* out_rgba8, size_t npx)
{
    return drain(c, {{root ? out_rgb : nullptr, c->d_out.p, npx * 12}, {root ? out_rgba8 : nullptr, c->d_out8.p, npx * 4}});
}

// One frame on `stream`, which the caller has ordered after the context's last asynchronous call (order_after_last).
int render_device(pt_ctx* c, const pt_camera* cam, int W, int H, int max_samples, int max_depth, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    int rc;
    if ((rc = ensure_queue(c, W, H, 1, stream))) return rc;
    if (c->n_pixels == 0) {
        HIP_TRY(c, hipEventRecord(c->ev0, stream));
        return empty_frame(c, stream, W, H, d_out_rgb, d_out_rgba8);
    }

    PtKernelParams P;
    walk_params(c, cam, P);
    FramePlan f;
    if ((rc = plan_frame(c, P, max_samples, f))) return rc;
    if ((rc = frame_buffers(c, f, W, H, d_out_rgb, d_out_rgba8, stream))) return rc;
    frame_params(c, f, cam, W, H, max_samples, max_depth, d_out_rgb, d_out_rgba8, P);

    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    if ((rc = run_launches(c, f, P, W, H, max_samples, stream, true))) return rc;
    return finish_frame(c, stream, W, H, &f, P.stack_entries);
}

// ---- ray images (pt_render_rays) ----------------------------------------------------------------------------------------
// What both forms refuse before anything is touched, a host-only context last (who: the entry point; device: rays is a device pointer,
// whose records the host cannot look at).  The table's own checks are check_ray_ptrs / check_ray_table above, which the guide pass over a
// ray image shares (pt_render_aov_rays, pt_guides.cpp).
int check_ray_image_args(pt_ctx* c, const char* who, const void* rays, int W, int H, int max_samples, int max_depth, const void* out_rgb, bool device)
{
    int rc;
    if ((rc = check_ray_ptrs(c, who, rays, out_rgb, device ? "d_out_rgb" : "out_rgb", device))) return rc;
    if ((rc = check_render_args(c, W, H, max_samples, max_depth))) return rc;
    // what only exists for a camera's frame is refused by name, never rendered some other way
    if (c->opt.kernel != 2) return fail(c, PT_E_INVALID, "%s: the lane-per-pixel kernel (option kernel = 1) has no ray-image form", who);
    if (c->opt.watertight) return fail(c, PT_E_INVALID, "%s: ray images have no watertight instances (option watertight = 1); set watertight = 0", who);
    if (c->opt.latency) return fail(c, PT_E_INVALID, "%s: the per-pixel latency diagnostics (option latency) belong to pt_render; switch them off for a ray image", who);
    if (c->opt.timeline) return fail(c, PT_E_INVALID, "%s: the chunk timeline (option timeline) belongs to pt_render; switch it off for a ray image", who);
    if ((rc = check_ray_table(c, who, rays, W, H, device, true))) return rc;
    return need_device(c);
}

// One frame over the ray image at d_rays on `stream`, which the caller has ordered after the context's last asynchronous call: render_device
// with the ray-image instances (kRayImage) and the table in the batch cameras' place.  far_o: the largest |org| component of the
// table, which decides the slab form as the camera's origin does in walk_params (+infinity: unknown, the subtracting form unless
// option "box_exact" = 0 asks for the other).
int rays_image_device(pt_ctx* c, const void* d_rays, float far_o, int W, int H, int max_samples, int max_depth, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    int rc;
    if ((rc = ensure_queue(c, W, H, 1, stream))) return rc;
    if (c->n_pixels == 0) {
        HIP_TRY(c, hipEventRecord(c->ev0, stream));
        return empty_frame(c, stream, W, H, d_out_rgb, d_out_rgba8);
    }

    pt_camera cam{}; // no camera: walk_params reads the origin alone, the kernel nothing of P.cam
    cam.origin[0] = far_o;
    PtKernelParams P;
    walk_params(c, &cam, P);
    FramePlan f;
    f.family = kRayImage;
    if ((rc = plan_frame(c, P, max_samples, f))) return rc;
    if ((rc = frame_buffers(c, f, W, H, d_out_rgb, d_out_rgba8, stream))) return rc;
    cam.origin[0] = 0.0f;
    frame_params(c, f, &cam, W, H, max_samples, max_depth, d_out_rgb, d_out_rgba8, P);
    P.batch_cams = (const float*)d_rays; // (batch_frames stays 0: pt_launch_render_rayimage checks both)

    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    if ((rc = run_launches(c, f, P, W, H, max_samples, stream, true))) return rc;
    return finish_frame(c, stream, W, H, &f, P.stack_entries);
}

} // namespace

namespace pti {

// An add of the progressive accumulation (pt_accum_host.cpp) is the frame path above with four differences: the pixel queue is the one
// the add has put into d_pixels / n_pixels (its active set); rng_state / accum are the accumulation's own; a continuing add starts every
// launch at sample_begin != 0, so start_chunk loads the pixel's state instead of seeding it (pt_kernel.hip: the only two uses of
// sample_begin are that test and the one below); and max_samples is a value no launch reaches (sample_begin + sample_count <= 2 * 65536),
// so finish_chunk always stores the state and never writes a framebuffer.  n_samples < 4 * prepass_spp takes the unsorted schedule,
// larger adds the pre-pass, the sort and - on small active sets - tiers and express pixels, exactly as plan_frame decides for a shard.
int accum_frame(pt_ctx* c, const pt_camera* cam, int W, int H, int n_samples, int max_depth, bool first_add, uint32_t* d_rng, float* d_sum, hipStream_t stream,
                bool ev0_recorded, const std::function<int()>& resolve)
{
    int rc;
    if (c->n_pixels == 0) { // an empty active set: resolve alone
        if (!ev0_recorded) HIP_TRY(c, hipEventRecord(c->ev0, stream));
        if ((rc = resolve())) return rc;
        return finish_frame(c, stream, W, H, nullptr, 0);
    }
    PtKernelParams P;
    walk_params(c, cam, P);
    FramePlan f;
    f.sample_base = first_add ? 0 : 65536;
    if ((rc = plan_frame(c, P, n_samples, f))) return rc;
    if ((rc = frame_buffers(c, f, W, H, nullptr, nullptr, stream))) return rc;
    frame_params(c, f, cam, W, H, 0x7fffffff, max_depth, nullptr, nullptr, P);
    P.rng_state = d_rng;
    P.accum = d_sum;
    if (!ev0_recorded) HIP_TRY(c, hipEventRecord(c->ev0, stream));
    if ((rc = run_launches(c, f, P, W, H, n_samples, stream, true))) return rc;
    if ((rc = resolve())) return rc;
    return finish_frame(c, stream, W, H, &f, P.stack_entries);
}

} // namespace pti

extern "C" {

int pt_render_device(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth, void* d_out_rgb,
                     void* d_out_rgba8, void* stream_v)
{
    if (!c || !cam || !d_out_rgb) return PT_E_INVALID;
    int rc;
    if ((rc = need_device(c)) || (rc = check_render_args(c, W, H, max_samples, max_depth))) return rc;
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return render_device(c, cam, W, H, max_samples, max_depth, d_out_rgb, d_out_rgba8, stream); });
}

int pt_synchronize(pt_ctx* c)
{
    if (!c) return PT_E_INVALID;
    if (c->host_only) return PT_OK;
    int rc = wait_idle(c);
    if (rc) return rc;
    return check_watchdog(c);
}

int pt_render(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth, float* out_rgb, uint32_t* out_rgba8)
{
    // with a communicator attached (pt_comm_init_rank) only rank 0 receives the frame; the other ranks may pass NULL
    const bool root = !c || !c->comm || c->comm_rank == 0;
    if (!c || !cam || (root && !out_rgb)) return PT_E_INVALID;
    int rc = need_device(c);
    if (rc) return rc;
    if (W <= 0 || H <= 0) return fail(c, PT_E_INVALID, "bad render size %dx%d", W, H);
    if ((rc = check_render_args(c, W, H, max_samples, max_depth))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)W * H;
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_out, npx * 12))) return rc;
        if (out_rgba8 && (rc = ensure(c, c->d_out8, npx * 4))) return rc;
        // with a communicator the RGBA8 image is made from the reduced float frame on the root (pt_reduce_framebuffer): every rank
        // enqueues the same single collective whatever buffers its caller passed
        rc = render_device(c, cam, W, H, max_samples, max_depth, c->d_out.p, (out_rgba8 && !c->comm) ? c->d_out8.p : nullptr, c->stream);
        if (rc) return rc;
        // N ranks: the one collective of the path - RCCL sum-reduce of the float3 framebuffer onto rank 0 (pt_comm.cpp)
        if (c->comm && (rc = reduce_framebuffer(c, c->d_out.p, (root && out_rgba8) ? c->d_out8.p : nullptr, (int64_t)npx, c->stream))) return rc;
        return read_back(c, root, out_rgb, out_rgba8, npx);
    });
}

int pt_render_rays_device(pt_ctx* c, const void* d_rays, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth, void* d_out_rgb, void* d_out_rgba8,
                          void* stream_v)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = check_ray_image_args(c, "pt_render_rays_device", d_rays, W, H, max_samples, max_depth, d_out_rgb, true))) return rc;
    // the records are the caller's and unknown here: the slab form that holds at any distance, unless the option chooses
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return rays_image_device(c, d_rays, INFINITY, W, H, max_samples, max_depth, d_out_rgb, d_out_rgba8, stream); });
}

int pt_render_rays(pt_ctx* c, const pt_ray_gen* rays, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = check_ray_image_args(c, "pt_render_rays", rays, W, H, max_samples, max_depth, out_rgb, false))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)W * H;
    const float far_o = ray_table_far_o(rays, npx);
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_out, npx * 12)) || (rc = ensure(c, c->d_ray_image, npx * sizeof(pt_ray_gen)))) return rc;
        if (out_rgba8 && (rc = ensure(c, c->d_out8, npx * 4))) return rc;
        HIP_TRY(c, hipMemcpyAsync(c->d_ray_image.p, rays, npx * sizeof(pt_ray_gen), hipMemcpyHostToDevice, c->stream));
        if ((rc = rays_image_device(c, c->d_ray_image.p, far_o, W, H, max_samples, max_depth, c->d_out.p, out_rgba8 ? c->d_out8.p : nullptr, c->stream))) return rc;
        return read_back(c, true, out_rgb, out_rgba8, npx);
    });
}

int pt_render_batch_device(pt_ctx* c, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth,
                           void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    if (!c || !d_out_rgb) return PT_E_INVALID;
    if (c->host_only) return batch_device(c, frames, n_frames, n_materials, W, H, max_samples, max_depth, d_out_rgb, d_out_rgba8, nullptr, nullptr, false); // (refused there, with its message)
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return batch_device(c, frames, n_frames, n_materials, W, H, max_samples, max_depth, d_out_rgb, d_out_rgba8, nullptr, stream, false); });
}

int pt_render_batch(pt_ctx* c, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t W, int32_t H, int32_t max_samples, int32_t max_depth,
                    float* out_rgb, uint32_t* out_rgba8)
{
    // with a communicator attached only rank 0 receives the frames (as pt_render)
    const bool root = !c || !c->comm || c->comm_rank == 0;
    if (!c || (root && !out_rgb)) return PT_E_INVALID;
    // with a communicator the RGBA8 frames are made from the reduced float frames on the root, one reduce per launch sequence
    auto batch = [&] {
        return batch_device(c, frames, n_frames, n_materials, W, H, max_samples, max_depth, c->d_out.p, (out_rgba8 && !c->comm) ? c->d_out8.p : nullptr,
                            (root && out_rgba8 && c->comm) ? c->d_out8.p : nullptr, c->stream, true);
    };
    if (n_frames < 1 || W <= 0 || H <= 0 || c->host_only) return batch(); // refused there, with its message, before anything is enqueued
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)n_frames * (size_t)W * (size_t)H;
    return blocking_call(c, [&]() -> int {
        int rc;
        if ((rc = ensure(c, c->d_out, npx * 12))) return rc;
        if (out_rgba8 && (rc = ensure(c, c->d_out8, npx * 4))) return rc;
        if ((rc = batch())) return rc;
        return read_back(c, root, out_rgb, out_rgba8, npx);
    });
}

int64_t pt_debug_plan_batch(int32_t W, int32_t H, int32_t n_frames, int32_t max_frames, int32_t* out, int64_t cap)
{
    if (n_frames < 1 || max_frames < 0 || W <= 0 || H <= 0 || W > 65535 || H > 65535 || cap < 0) return PT_E_INVALID;
    const int64_t kmax = batch_max_frames(W, H, max_frames);
    if (kmax < 1) return PT_E_LIMIT;
    int64_t n = 0;
    for (int64_t f0 = 0; f0 < n_frames; f0 += kmax, ++n)
        if (out && n < cap) out[n] = (int32_t)std::min<int64_t>(kmax, n_frames - f0);
    return n;
}

} // extern "C"
