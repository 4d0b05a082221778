// pt_debug.cpp -- what looks into the device for the tests: pt_debug_eval with the ray probes, and the readers of the diagnostics a
// frame leaves behind (queue, chunk timeline, tier plan, finish ticks), and the cost image a test sets in place of the measured one.
#include <algorithm>
#include <cstring>
#include <vector>

#include "pt_internal.h"
#include "pt_launch.h"
#include "pt_tiers.h"

using namespace pti;

namespace {

// The ray probes of pt_debug_eval (ops >= PT_PROBE_FIRST, pt_launch.h): rays already uploaded to d_dbg_in, d_dbg_out sized and cleared; P
// holds the scene (fill_params).  The probes walk the quad / oct nodes with the device functions of the render kernel (pt_kernel.hip); a
// scene without those nodes is an error, never another walk.
int probe_eval(pt_ctx* c, PtKernelParams& P, int op, int in_stride, float* out, int out_stride, int64_t n)
{
    if (op > PT_PROBE_LAST) return fail(c, PT_E_INVALID, "pt_debug_eval: unknown op %d", op);
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_debug_eval: ray probe before pt_upload_scene");
    if (in_stride < 6 || out_stride < PT_PROBE_OUT) return fail(c, PT_E_INVALID, "ray probe: 6 floats in, %d out per ray", PT_PROBE_OUT);
    const bool group = op >= PT_PROBE_GROUP;
    P.box_exact = (op - PT_PROBE_FIRST) & 1;
    int grid = 0;
    size_t lds = 0, scratch_words = 0;
    if (!group) {
        if (c->scene.nodes4.empty() && c->scene.root4 >= 0) return fail(c, PT_E_LIMIT, "ray probe: the scene has no quad nodes (tree too deep for the quad walk)");
        quad_walk_params(c, P);
        const bool overflow = op >= PT_PROBE_QUAD_OVF;
        const int levels = P.stack_entries + 3; // the LDS-only step stores three entries above the top whether or not it pushes them
        grid = (int)std::min<int64_t>((n + 63) / 64, 2048);
        P.lds_levels = overflow ? std::min(levels, pt_probe_lds_stack()) : levels;
        lds = (size_t)P.lds_levels * 64 * 4;
        scratch_words = overflow ? (size_t)std::max(0, levels - P.lds_levels) * 64 * (size_t)grid : 0;
    } else {
        if (c->scene.nodes8.empty() && c->scene.root8 >= 0) return fail(c, PT_E_LIMIT, "ray probe: the scene has no oct nodes (tree too deep for the group walk)");
        P.nodes8 = (const PtNode8*)c->d_nodes8.p;
        P.root8 = c->scene.root8;
        P.groups = 2;
        P.ns = PT_PROBE_GROUP_SLOTS;
        P.lds_levels = std::max(1, (7 * c->scene.depth8 + 1 + 7) / 8);
        grid = (int)((n + PT_PROBE_GROUP_RAYS - 1) / PT_PROBE_GROUP_RAYS);
        lds = pt_probe_group_lds_bytes(P.lds_levels, P.ns);
        scratch_words = pt_probe_group_state_words() * (size_t)grid;
    }
    DevBuf d_scratch; // overflow columns / park areas, then the watchdog flag
    int rc = ensure(c, d_scratch, (scratch_words + 64) * 4);
    if (rc) return rc;
    uint32_t* flag = (uint32_t*)d_scratch.p + scratch_words;
    P.error_flag = flag;
    uint32_t fired = 0;
    hipError_t e = hipMemsetAsync(flag, 0, 4, c->stream);
    // option "watertight": the same probe kernels around the watertight instances of leaf_test / traverse_groups (pt_kernel_wt.hip)
    if (e == hipSuccess) e = (c->opt.watertight ? pt_launch_probe_wt : pt_launch_probe)(&P, op, (const float*)c->d_dbg_in.p, in_stride, (float*)c->d_dbg_out.p, out_stride, (long long)n, grid, lds, (uint32_t*)d_scratch.p, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, c->d_dbg_out.p, (size_t)n * out_stride * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&fired, flag, 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, PT_E_HIP, "ray probe %d failed: %s", op, hipGetErrorString(e));
    if (fired) return fail(c, PT_E_HIP, "ray probe %d: a walk ran out of its step or stack bound; the results are incomplete", op);
    return PT_OK;
}

// Before a reader of device-side diagnostics copies anything: the context's GPU current and the last frame complete, on whichever
// stream it was enqueued.
int drain(pt_ctx* c) { return wait_idle(c); }

} // namespace

extern "C" {

int64_t pt_debug_read_queue(pt_ctx* c, uint32_t* queue_ids, uint32_t* input_ids, uint8_t* cost, int64_t cap)
{
    if (!c) return PT_E_INVALID;
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: pt_debug_read_queue needs the GPU");
    if (!c->last.sorted) return 0;
    const int64_t n = std::min<int64_t>(cap, c->n_pixels);
    if (int rc = drain(c)) return rc;
    if (queue_ids) HIP_TRY(c, hipMemcpy(queue_ids, c->d_sorted.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (input_ids) HIP_TRY(c, hipMemcpy(input_ids, c->d_pixels.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (cost) { // cost image -> cost of each input queue entry
        std::vector<uint8_t> img((size_t)c->last.w * (size_t)c->last.h);
        std::vector<uint32_t> ids((size_t)n);
        HIP_TRY(c, hipMemcpy(img.data(), c->d_cost.p, img.size(), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(ids.data(), c->d_pixels.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) cost[i] = ids[(size_t)i] < img.size() ? img[ids[(size_t)i]] : 0;
    }
    return n;
}

int pt_debug_set_cost_image(pt_ctx* c, const uint8_t* img, int32_t W, int32_t H)
{
    if (!c) return PT_E_INVALID;
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: pt_debug_set_cost_image needs the GPU");
    if (img && (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (int64_t)W * H > (int64_t)0x7fffffff)) // the sizes of check_render_args
        return fail(c, PT_E_INVALID, "pt_debug_set_cost_image: bad image size %dx%d", W, H);
    if (int rc = drain(c)) return rc; // a frame in flight may still copy the image that is replaced here
    c->cost_image_w = c->cost_image_h = 0;
    if (!img) return PT_OK; // back to the measured costs (the buffer stays the context's until pt_destroy)
    if (int rc = upload(c, c->d_cost_image, img, (size_t)W * H)) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // img is the caller's
    c->cost_image_w = W;
    c->cost_image_h = H;
    return PT_OK;
}

int64_t pt_debug_read_laps(pt_ctx* c, uint64_t* ticks, int64_t cap)
{
    if (!c || !ticks) return PT_E_INVALID;
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: pt_debug_read_laps needs the GPU");
    if (c->opt.kernel != 2 || !c->d_laps.p) return 0;
    const int nt = 3 * (c->last.chunks + 1);
    std::vector<uint64_t> blk((size_t)PT_LAP_REGION(c->last.chunks));
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(blk.data(), (char*)c->d_laps.p + c->last.lap_ticks_ofs, blk.size() * 8, hipMemcpyDeviceToHost));
    int64_t n = 0; // the timeline, then the 64 latency accumulators, without the padding between them
    for (int i = 0; i < nt && n < cap; ++i) ticks[n++] = blk[(size_t)i];
    for (int i = 0; i < 64 && n < cap; ++i) ticks[n++] = blk[(size_t)PT_LAP_DIAG_OFS(c->last.chunks) + i];
    return n;
}

int64_t pt_debug_plan_tiers(const uint32_t* bucket_pixels, int32_t capacity, int32_t ns, int32_t force, uint32_t* words, int64_t cap)
{
    if (!bucket_pixels || !words || capacity < 1 || ns < 4 || ns > 255 || cap < 1 + PT_MAX_TIERS * PT_TIER_WORDS) return PT_E_INVALID;
    uint32_t start[PT_SORT_BUCKETS + 1];
    uint64_t run = 0;
    for (int b = 0; b < PT_SORT_BUCKETS; ++b) { start[b] = (uint32_t)run; run += bucket_pixels[b]; }
    if (run == 0 || run >= (1ull << 31)) return PT_E_INVALID;
    start[PT_SORT_BUCKETS] = (uint32_t)run;
    std::memset(words, 0, (size_t)(1 + PT_MAX_TIERS * PT_TIER_WORDS) * 4);
    pt_plan_tiers(start, capacity, ns, force, words); // the code of pt_plan_tiers_kernel, on the host
    return 1 + (int64_t)words[0] * PT_TIER_WORDS;
}

int64_t pt_debug_read_tiers(pt_ctx* c, uint32_t* words, int64_t cap)
{
    if (!c || !words) return PT_E_INVALID;
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: pt_debug_read_tiers needs the GPU");
    if (!c->stats.whole_pixels || !c->d_tiers.p) return 0;
    const int64_t n = std::min<int64_t>(cap, 1 + PT_MAX_TIERS * PT_TIER_WORDS);
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(words, c->d_tiers.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int64_t pt_debug_read_finish(pt_ctx* c, uint32_t* ticks, int64_t cap)
{
    if (!c || !ticks) return PT_E_INVALID;
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: pt_debug_read_finish needs the GPU");
    if (c->opt.kernel != 2 || !c->opt.latency || !c->last.sorted || !c->d_dbg_start.p) return 0;
    const int64_t n = std::min<int64_t>(cap, 2 * (int64_t)c->last.w * c->last.h);
    if (int rc = drain(c)) return rc;
    HIP_TRY(c, hipMemcpy(ticks, c->d_dbg_start.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return n;
}

int pt_debug_eval(pt_ctx* c, int32_t op, const float* in, int32_t in_stride, float* out, int32_t out_stride, int64_t n)
{
    if (!c || !in || !out || n < 0 || in_stride < 1 || out_stride < 1) return PT_E_INVALID;
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: pt_debug_eval needs the GPU");
    if (n == 0) return PT_OK;
    int rc;
    if ((rc = wait_idle(c))) return rc; // the probes run on the context's stream: after a frame in flight on a caller's
    if ((rc = upload(c, c->d_dbg_in, in, (size_t)n * in_stride * 4))) return rc;
    if ((rc = ensure(c, c->d_dbg_out, (size_t)n * out_stride * 4))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_dbg_out.p, 0, (size_t)n * out_stride * 4, c->stream));
    PtKernelParams P;
    fill_params(c, P);
    if (op >= PT_PROBE_FIRST) return probe_eval(c, P, op, in_stride, out, out_stride, n);
    if (op == PT_DEBUG_OP_CLOSEST_HIT && c->opt.watertight)
        return fail(c, PT_E_INVALID, "pt_debug_eval: the validation kernel's closest-hit op (21) has no watertight form (option watertight = 1); use the ray probes 30..35");
    if (!c->have_scene) { P.root = -1; P.stack_entries = 1; }
    size_t lds = (size_t)P.stack_entries * pt_debug_block() * 4;
    HIP_TRY(c, pt_launch_debug(&P, op, (const float*)c->d_dbg_in.p, in_stride, (float*)c->d_dbg_out.p, out_stride, (long long)n, lds, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out, c->d_dbg_out.p, (size_t)n * out_stride * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

} // extern "C"
