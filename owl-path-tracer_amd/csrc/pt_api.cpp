// pt_api.cpp -- the C-ABI declared in include/mi355pt.h (host side, HIP runtime): context lifetime, options, statistics, errors, pixel
// shards and the camera; with pt_scene.cpp (scene), pt_render.cpp (frames), pt_guides.cpp (guide pass, denoiser), pt_debug.cpp (probes, readers) and pt_comm.cpp (N GPUs).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "pt_internal.h"

static std::string g_create_error; // pt_last_error(NULL): why the last pt_create / pt_group_create returned NULL

namespace pti {

int fail(pt_ctx* c, int code, const char* fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

int ensure(pt_ctx* c, DevBuf& b, size_t bytes)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return PT_OK;
    if (b.p) { // a buffer grows: nothing in flight may still use the old one (a frame on a caller's stream included)
        int rc = wait_idle(c);
        if (rc) return rc;
        HIP_TRY(c, hipFree(b.p));
    }
    b.p = nullptr;
    b.cap = 0;
    HIP_TRY(c, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return PT_OK;
}

int upload(pt_ctx* c, DevBuf& b, const void* src, size_t bytes)
{
    int rc = ensure(c, b, bytes);
    if (rc) return rc;
    if (bytes) HIP_TRY(c, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return PT_OK;
}

int order_after_last(pt_ctx* c, hipStream_t stream)
{
    if (c->last.stream && c->last.stream != stream) HIP_TRY(c, hipStreamWaitEvent(stream, c->evo, 0));
    return PT_OK;
}

int mark_last(pt_ctx* c, hipStream_t stream)
{
    HIP_TRY(c, hipEventRecord(c->evo, stream));
    c->last.stream = stream;
    return PT_OK;
}

int wait_idle(pt_ctx* c)
{
    if (c->host_only) return PT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->last.stream && c->last.stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->last.stream)); // an asynchronous call on a caller's stream
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->last.stream = nullptr; // (the caller's stream is not looked at again: it may be destroyed from here on)
    return PT_OK;
}

int need_device(pt_ctx* c)
{
    if (c->host_only) return fail(c, PT_E_NO_DEVICE, "host-only context: the HIP render path is required and there is no CPU fallback");
    return PT_OK;
}

} // namespace pti

using namespace pti;

extern "C" {

int pt_abi_version(void) { return PT_ABI_VERSION; }

const char* pt_last_error(const pt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

pt_ctx* pt_create(const pt_config* cfg)
{
    int dev = cfg ? cfg->device : 0;
    pt_ctx* c = new pt_ctx();
    c->device = dev;
    if (dev < 0) { // host-only validation context: scene/BVH/sharding work, every render call fails loudly
        c->host_only = true;
        return c;
    }
    auto refuse = [c]() -> pt_ctx* { delete c; return nullptr; }; // (pt_last_error(NULL) has the reason)
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0 || dev >= n) {
        fail(nullptr, PT_E_NO_DEVICE, "no usable HIP device (count=%d, requested=%d): %s", n, dev, hipGetErrorString(e));
        return refuse();
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        fail(nullptr, PT_E_NO_DEVICE, "hipSetDevice/hipGetDeviceProperties failed for device %d", dev);
        return refuse();
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fail(nullptr, PT_E_NO_DEVICE, "device %d is %s; this library ships gfx950 (MI355X) code only", dev, prop.gcnArchName);
        return refuse();
    }
    c->num_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&c->ev0) != hipSuccess ||
        hipEventCreate(&c->ev1) != hipSuccess || hipEventCreate(&c->evm) != hipSuccess || hipEventCreate(&c->evr) != hipSuccess ||
        hipEventCreate(&c->evd) != hipSuccess || hipEventCreateWithFlags(&c->evo, hipEventDisableTiming) != hipSuccess) {
        fail(nullptr, PT_E_HIP, "stream/event creation failed");
        return refuse();
    }
    return c;
}

void pt_destroy(pt_ctx* c)
{
    if (!c) return;
    if (!c->host_only) {
        (void)wait_idle(c);
        (void)pt_comm_destroy(c);
        for (hipEvent_t e : {c->ev0, c->ev1, c->evm, c->evr, c->evd, c->evo, c->evu0, c->evu1})
            if (e) (void)hipEventDestroy(e);
        if (c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c; // frees every device buffer the context owns (DevBuf)
}

int pt_set_option(pt_ctx* c, const char* key, int64_t value)
{
    if (!c || !key) return PT_E_INVALID;
    std::string k(key);
    if (k == "spp_per_launch") c->opt.spp_per_launch = (int)(value < 0 ? 0 : value);
    else if (k == "count") c->opt.count = value ? 1 : 0;
    else if (k == "blocks_per_cu") c->opt.blocks_per_cu = (int)(value < 0 ? 0 : value);
    else if (k == "leaf_size") c->opt.leaf_size = (int)value;
    else if (k == "max_bvh_depth") c->opt.max_bvh_depth = (int)value;
    else if (k == "sticky_pct") c->opt.sticky_pct = (int)(value < 1 ? -1 : (value > 100 ? 100 : value)); // < 1: automatic
    else if (k == "cost_radius") c->opt.cost_radius = (int)(value < 0 ? 0 : (value > 8 ? 8 : value));
    else if (k == "timeline") c->opt.timeline = value != 0;
    else if (k == "latency") c->opt.latency = (int)value;
    else if (k == "census_mode") c->opt.census_mode = (int)value;
    else if (k == "schedule") c->opt.schedule = value == 0 ? 0 : 1;
    else if (k == "prepass_spp") c->opt.prepass_spp = (int)(value < 0 ? 0 : (value > 64 ? 64 : value)); // 0: automatic (8; 16 when a tier plan is prepared)
    else if (k == "chunk_tail_min") c->opt.chunk_tail_min = (int)(value < 0 ? -1 : (value > 65535 ? 65535 : value)); // -1: automatic
    else if (k == "chunk_spp") c->opt.chunk_spp = (int)(value < 1 ? 1 : (value > 65535 ? 65535 : value));
    else if (k == "slots_per_wave") c->opt.slots_per_wave = (int)(value < 0 ? 0 : value);
    else if (k == "adaptive") c->opt.tune[5] = value ? 1 : 2;
    else if (k == "bvh_builder") {
        if (value < 0 || value > 3) return fail(c, PT_E_INVALID, "bvh_builder must be 0 (host binned SAH), 1 (device LBVH), 2 (device PLOC) or 3 (by triangle count)");
        c->opt.bvh_builder = (int)value;
    }
    else if (k == "wide_leaves") c->opt.wide_leaves = value != 0; // oct nodes: subtrees of <= 7 triangles become one leaf (before pt_upload_scene)
    else if (k == "fallback") c->opt.fallback = value != 0; // force the wavefront kernel's 168-VGPR fallback instance (tests)
    else if (k == "express_permille") c->opt.express_permille = (int)(value < 0 ? -1 : (value > 500 ? 500 : value)); // -1: automatic
    else if (k == "whole") c->opt.whole = (int)(value < 0 ? -1 : (value > 1 ? 1 : value)); // whole-pixel schedule by cost class when every pixel can have a path slot: -1 the plan decides (default), 0 never, 1 always
    else if (k == "ns_express") c->opt.ns_express = (int)(value < 1 ? 1 : (value > 64 ? 64 : value));
    else if (k == "groups") c->opt.groups = (int)(value < 0 ? 0 : (value > 2 ? 2 : value)); // group walk: 0 never, 1 sparse waves (default), 2 always
    else if (k == "ploc_radius") c->opt.ploc_radius = (int)(value < 1 ? 1 : (value > 64 ? 64 : value)); // bvh_builder 2: neighbours searched on either side
    else if (k == "box_exact") c->opt.box_exact = (int)(value < 0 ? -1 : (value > 0 ? 1 : 0)); // slab test form: -1 automatic (fma unless the camera is far outside the scene), 0 fma, 1 subtracting
    else if (k == "batch_frames") c->opt.batch_frames = (int)(value < 0 ? 0 : (value > 0x7fffffff ? 0x7fffffff : value)); // pt_render_batch: most frames per launch sequence (0: what the limits allow)
    else if (k == "watertight") { // the triangle test of every walk of the wavefront render path, the ray probes and the host walk: 0 Moeller-Trumbore, 1 watertight
        if (value != 0 && value != 1) return fail(c, PT_E_INVALID, "watertight must be 0 (Moeller-Trumbore, default) or 1 (watertight edge functions)");
        if (value == 1 && c->opt.kernel != 2) return fail(c, PT_E_INVALID, "watertight = 1: the lane-per-pixel kernel (option kernel = 1) has no watertight form; set kernel = 2 first");
        c->opt.watertight = (int)value;
    }
    else if (k == "dynamic") { // next pt_upload_scene: 1 = keep what pt_update_vertices needs (vertex arrays, indices, refit schedule), on the host and in HBM
        if (value != 0 && value != 1) return fail(c, PT_E_INVALID, "dynamic must be 0 (default) or 1 (the next pt_upload_scene keeps what pt_update_vertices needs)");
        c->opt.dynamic = (int)value;
    }
    else if (k == "rays_refill") { // pt_trace_closest / pt_trace_occluded: idle lanes of a wave take new rays when at most this many lanes are still walking
        if (value < 0 || value > 63) return fail(c, PT_E_INVALID, "rays_refill must be 0 (a new batch only when the whole wave is done) .. 63 (whenever a lane is idle); default 32");
        c->opt.rays_refill = (int)value;
    }
    else if (k == "rays_grid") c->opt.rays_grid = (int)(value < 0 ? 0 : (value > 0x7fffffff ? 0x7fffffff : value)); // pt_trace_*: most workgroups of the ray launch (0: what the occupancy query says is resident)
    else if (k == "quad") c->opt.quad = value != 0; // wavefront kernel: quad nodes (two binary levels per fetch), next pt_render
    else if (k == "node_pairs") c->opt.node_pairs = value != 0;
    else if (k == "leaf_align") c->opt.leaf_align = (int)(value < 1 ? 1 : (value > 8 ? 8 : value));
    else if (k.size() == 5 && k.compare(0, 4, "tune") == 0 && k[4] >= '0' && k[4] <= '7') c->opt.tune[k[4] - '0'] = (int)value;
    else if (k == "kernel") {
        if (value != 1 && value != 2) return fail(c, PT_E_INVALID, "kernel must be 1 (lane-per-pixel) or 2 (wavefront-scheduled)");
        if (value == 1 && c->opt.watertight) return fail(c, PT_E_INVALID, "kernel = 1: the lane-per-pixel kernel has no watertight form (option watertight = 1); set watertight = 0 first");
        c->opt.kernel = (int)value;
    }
    else return fail(c, PT_E_INVALID, "unknown option '%s'", key);
    return PT_OK;
}

int pt_get_stats(pt_ctx* c, pt_stats* out)
{
    if (!c || !out) return PT_E_INVALID;
    if (!c->host_only && c->last.ev_pending) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(c->ev1));
        int wrc = check_watchdog(c);
        if (wrc) return wrc;
        float ms = 0.0f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        c->stats.kernel_ms = ms;
        c->stats.prepass_ms = 0.0;
        if (c->last.sorted) {
            HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->evm));
            c->stats.prepass_ms = ms;
        }
        c->stats.launches = c->last.launches;
        c->last.ev_pending = false;
        if (c->opt.count && c->d_counters.p) {
            PtCounters h;
            HIP_TRY(c, hipMemcpy(&h, c->d_counters.p, sizeof(h), hipMemcpyDeviceToHost));
            c->stats.samples = h.samples; c->stats.rays = h.rays; c->stats.nodes = h.nodes; c->stats.tris = h.tris;
            c->stats.scatters = h.scatters; c->stats.env_misses = h.env_misses; c->stats.nan_retries = h.nan_retries;
            for (int i = 0; i < 32; ++i) c->stats.sched[i] = h.sched[i];
            for (int i = 0; i < 8; ++i) c->stats.groups[i] = h.grp[i];
            for (int i = 0; i < 16; ++i) c->stats.lobes[i] = h.lobes[i];
            for (int i = 0; i < 4; ++i) c->stats.trav[i] = h.trav[i];
        }
    }
    c->stats.bvh_nodes = c->scene.bvh_nodes;
    c->stats.bvh_depth = c->scene.bvh_depth;
    c->stats.n_triangles = c->scene.n_triangles;
    c->stats.bvh_build_ms = c->scene.bvh_build_ms;
    *out = c->stats;
    return PT_OK;
}

int pt_set_pixel_shard(pt_ctx* c, int32_t rank, int32_t world_size, int32_t tile)
{
    if (!c) return PT_E_INVALID;
    if (world_size < 1 || rank < 0 || rank >= world_size || tile < 1) return fail(c, PT_E_INVALID, "bad shard %d/%d tile %d", rank, world_size, tile);
    if (!c->host_only && c->queue_valid && (rank != c->rank || world_size != c->world || tile != c->tile)) { // the pixel queue is another one from here on
        int rc = wait_idle(c);
        if (rc) return rc;
        c->queue_valid = false;
    }
    c->rank = rank;
    c->world = world_size;
    c->tile = tile;
    return PT_OK;
}

// Pixel ids owned by (rank, world): tile x tile tiles dealt round-robin on (tx + ty) % world; inside a tile the
// ids are emitted in 8x8 blocks so that the 64 lanes of a wave start on one compact screen patch.
int64_t pt_shard_pixels(int32_t W, int32_t H, int32_t tile, int32_t rank, int32_t world, uint32_t* ids, int64_t cap)
{
    if (W <= 0 || H <= 0 || world < 1 || rank < 0 || rank >= world) return -1;
    tile = shard_tile(tile);
    int ntx = (W + tile - 1) / tile, nty = (H + tile - 1) / tile;
    int64_t n = 0;
    for (int ty = 0; ty < nty; ++ty)
        for (int tx = 0; tx < ntx; ++tx) {
            if ((tx + ty) % world != rank) continue;
            for (int by = 0; by < tile; by += 8)
                for (int bx = 0; bx < tile; bx += 8)
                    for (int y = 0; y < 8; ++y)
                        for (int x = 0; x < 8; ++x) {
                            int px = tx * tile + bx + x, py = ty * tile + by + y;
                            if (px >= W || py >= H) continue;
                            if (ids && n < cap) ids[n] = (uint32_t)px + (uint32_t)W * (uint32_t)py;
                            ++n;
                        }
        }
    return n;
}

void pt_to_camera_data(const float look_from[3], const float look_at[3], const float look_up[3], float vfov, int32_t w, int32_t h, pt_camera* out)
{
    // camera.cpp:3-21; host code, host libm tan as in the reference.  dot/cross use the same fused forms as the device code.
    auto dot = [](const float* a, const float* b) { return std::fma(a[2], b[2], std::fma(a[1], b[1], a[0] * b[0])); };
    auto cross = [](const float* a, const float* b, float* r) {
        r[0] = std::fma(a[1], b[2], -(a[2] * b[1]));
        r[1] = std::fma(a[2], b[0], -(a[0] * b[2]));
        r[2] = std::fma(a[0], b[1], -(a[1] * b[0]));
    };
    auto normalize = [&](float* v) {
        float s = 1.0f / std::sqrt(dot(v, v));
        v[0] *= s; v[1] *= s; v[2] *= s;
    };
    const float pi = 3.14159265358979323f;
    float aspect = (float)w / (float)h;
    float theta = vfov * pi / 180.0f;
    float hh = std::tan(theta / 2);
    float vh = 2.0f * hh, vw = aspect * vh;
    float W[3] = {look_from[0] - look_at[0], look_from[1] - look_at[1], look_from[2] - look_at[2]};
    normalize(W);
    float U[3], Vv[3];
    cross(look_up, W, U);
    normalize(U);
    cross(W, U, Vv);
    normalize(Vv);
    for (int i = 0; i < 3; ++i) {
        out->origin[i] = look_from[i];
        out->horizontal[i] = vw * U[i];
        out->vertical[i] = vh * Vv[i];
        out->llc[i] = look_from[i] - out->horizontal[i] / 2.0f - out->vertical[i] / 2.0f - W[i];
    }
}

} // extern "C"
