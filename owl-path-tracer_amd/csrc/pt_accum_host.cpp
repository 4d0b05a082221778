// pt_accum_host.cpp -- the progressive accumulation (pt_accum_*; include/mi355pt.h, "progressive accumulation"): a frame that grows by
// adds.  This file owns the accumulation's state across calls (Accum, pt_internal.h), runs an add - select, the frame path of
// pt_render.cpp over the active set (pti::accum_frame), resolve - and holds the CPU twins of the two kernels of pt_accum.hip, which
// compile the very definition the kernels compile (pt_accum_math.h with PTD = static inline: pt_device_host.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

#include "pt_device_host.h"
#include "pt_accum_math.h"

#include "pt_internal.h"
#include "pt_launch.h"

using namespace pti;
using namespace ptd;

namespace pti {

int need_accum(pt_ctx* c, const char* who)
{
    if (!c->acc) return fail(c, PT_E_INVALID, "%s: the context has no accumulation (pt_accum_begin not called)", who);
    return PT_OK;
}

int refuse_comm(pt_ctx* c, const char* who)
{
    if (c->comm) return fail(c, PT_E_INVALID, "%s: a context with a communicator has no accumulation yet (render the ranks' shards with pt_set_pixel_shard and reduce them yourself)", who);
    return PT_OK;
}

} // namespace pti

namespace {

constexpr int64_t kMaxPixelSamples = 2147483648ll - 65536; // a pixel's n stays below this: n and n + n_samples are exact in int32 everywhere

// What pt_accum_add, pt_accum_add_device and the select twin refuse alike; *eff = the parameters in effect.
int check_accum_params(pt_ctx* c, const char* who, const pt_accum_params* p, pt_accum_params* eff)
{
    if (p) *eff = *p;
    else pt_accum_default_params(eff);
    if (eff->n_samples < 1 || eff->n_samples > 65535) return fail(c, PT_E_INVALID, "%s: n_samples %d outside 1..65535", who, eff->n_samples);
    if (eff->max_pixel_samples < 0) return fail(c, PT_E_INVALID, "%s: max_pixel_samples %d is negative (0 = no cap)", who, eff->max_pixel_samples);
    if (!(eff->noise_threshold >= 0.0f)) return fail(c, PT_E_INVALID, "%s: noise_threshold %g must be >= 0 (0 = uniform add)", who, (double)eff->noise_threshold);
    if (eff->reserved != 0) return fail(c, PT_E_INVALID, "%s: reserved must be 0 (is %d)", who, eff->reserved);
    return PT_OK;
}

// What an accumulation cannot be combined with, refused by name at begin and at every add.
int check_accum_context(pt_ctx* c, const char* who)
{
    if (c->opt.kernel != 2) return fail(c, PT_E_INVALID, "%s: the lane-per-pixel kernel (option kernel = 1) keeps no pixel state between launches of different calls; set kernel = 2", who);
    if (c->opt.latency) return fail(c, PT_E_INVALID, "%s: the per-pixel latency diagnostics (option latency) are per frame; switch them off for an accumulation", who);
    if (c->opt.timeline) return fail(c, PT_E_INVALID, "%s: the chunk timeline (option timeline) is per frame; switch it off for an accumulation", who);
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    return PT_OK;
}

int launch_resolve(pt_ctx* c, Accum& a, int n_samples, bool all_active, hipStream_t stream)
{
    PtAccumArgs R{};
    R.sum = (const float*)a.sum.p;
    R.seen = (float*)a.seen.p;
    R.half = (float*)a.half.p;
    R.n = (uint32_t*)a.n.p;
    R.n_half = (uint32_t*)a.n_half.p;
    R.passes = (uint32_t*)a.passes.p;
    R.noise = (float*)a.noise.p;
    R.owned = (const uint8_t*)a.owned.p;
    R.active = (const uint8_t*)a.active.p;
    R.out_rgb = (float*)a.out.p;
    R.out_rgba8 = (uint32_t*)a.out8.p;
    R.n_frame = (uint32_t)a.w * (uint32_t)a.h;
    R.width = a.w;
    R.height = a.h;
    R.n_samples = n_samples;
    R.all_active = all_active ? 1 : 0;
    HIP_TRY(c, pt_launch_accum_resolve(&R, stream));
    return PT_OK;
}

// One add on `stream`, which the caller has ordered after the context's last asynchronous call.  Other calls of the header rewrite the
// context's pixel queue and work buffers between two adds, so nothing of them is taken to have survived: the queue is put in place again
// from the accumulation's own copy (or by select), and accum_frame sizes and clears every work buffer as any frame does.
int add_device(pt_ctx* c, const pt_accum_params& prm, void* d_out_rgb, void* d_out_rgba8, hipStream_t stream)
{
    Accum& a = *c->acc;
    int rc;
    PtGeometry g{};
    const hipError_t ge = pt_accum_geometry(&g);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the accumulation kernels spills registers to scratch; such builds are refused (pt_accum.hip)");
    HIP_TRY(c, ge);
    const bool selects = prm.noise_threshold > 0.0f || prm.max_pixel_samples > 0;
    const size_t npx = (size_t)a.w * a.h;
    if ((rc = ensure(c, c->d_pixels, (size_t)a.n_owned * 4))) return rc; // (growing it first waits on the host for what is in flight)
    uint32_t n_active = a.n_owned;
    const QueueKey key{a.w, a.h, 1, a.rank, a.world, a.tile};
    if (selects && a.n_owned) {
        PtAccumSelectArgs S{};
        S.queue = (const uint32_t*)a.queue.p;
        S.noise = (const float*)a.noise.p;
        S.n = (const uint32_t*)a.n.p;
        S.active = (uint8_t*)a.active.p;
        S.ids_out = (uint32_t*)c->d_pixels.p;
        S.count = (uint32_t*)a.count.p;
        S.n_queue = a.n_owned;
        S.cap = (uint32_t)prm.max_pixel_samples;
        S.threshold = prm.noise_threshold;
        HIP_TRY(c, hipMemsetAsync(a.count.p, 0, 256, stream));
        HIP_TRY(c, hipEventRecord(c->ev0, stream)); // kernel_ms of an add that selects: from the select launch, the wait for its count included
        c->queue_valid = false; // d_pixels is the add's from here on: the next frame of another call makes its own queue again
        HIP_TRY(c, pt_launch_accum_select(&S, stream));
        // the launch cannot be planned without the size of the active set: the one host wait of an add that selects
        HIP_TRY(c, hipMemcpyAsync(&n_active, a.count.p, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(c, hipStreamSynchronize(stream));
    } else if (!(c->queue_valid && c->queue == key)) { // uniform: the shard's queue itself, as ensure_queue makes it for this key
        if (a.n_owned) HIP_TRY(c, hipMemcpyAsync(c->d_pixels.p, a.queue.p, (size_t)a.n_owned * 4, hipMemcpyDeviceToDevice, stream));
        c->queue = key;
        c->queue_valid = true;
    }
    // n_pixels describes the queue the launches run over, as after every frame (pt_debug_read_queue, pt_stats.whole_pixels); after an
    // add that selects it is the active count beside queue_valid = false, so the next frame of any call goes through ensure_queue
    c->n_pixels = n_active;
    rc = accum_frame(c, &a.cam, a.w, a.h, prm.n_samples, a.depth, a.adds == 0, (uint32_t*)a.rng.p, (float*)a.sum.p, stream, selects && a.n_owned, [&]() -> int {
        return launch_resolve(c, a, prm.n_samples, !selects, stream);
    });
    if (rc) return rc;
    // the caller's copies of the image, after kernel_ms has ended with resolve
    if (d_out_rgb) HIP_TRY(c, hipMemcpyAsync(d_out_rgb, a.out.p, npx * 12, hipMemcpyDeviceToDevice, stream));
    if (d_out_rgba8) HIP_TRY(c, hipMemcpyAsync(d_out_rgba8, a.out8.p, npx * 4, hipMemcpyDeviceToDevice, stream));
    ++a.adds;
    a.active_pixels = n_active;
    a.samples_total += (uint64_t)n_active * (uint64_t)prm.n_samples;
    a.n_upper += (uint64_t)prm.n_samples;
    return PT_OK;
}

// The accumulation still stands on the shard and the scene pt_accum_begin found.
int check_accum_unchanged(pt_ctx* c, const char* who)
{
    const Accum& a = *c->acc;
    if (a.rank != c->rank || a.world != c->world || a.tile != c->tile)
        return fail(c, PT_E_INVALID, "%s: the pixel shard changed after pt_accum_begin (%d of %d tile %d, now %d of %d tile %d); begin again", who, a.rank, a.world, a.tile, c->rank, c->world, c->tile);
    if (a.scene_epoch != c->scene_epoch) return fail(c, PT_E_INVALID, "%s: a new scene was uploaded after pt_accum_begin; begin again", who);
    return PT_OK;
}

// Everything an add refuses before it touches anything, in the order of the header; *eff = the parameters in effect.
int check_add(pt_ctx* c, const char* who, const pt_accum_params* p, pt_accum_params* eff)
{
    int rc;
    if ((rc = check_accum_params(c, who, p, eff)) || (rc = check_accum_context(c, who)) || (rc = need_accum(c, who)) || (rc = refuse_comm(c, who))) return rc;
    if ((rc = check_accum_unchanged(c, who))) return rc;
    const Accum& a = *c->acc;
    if ((int64_t)a.n_upper + eff->n_samples > kMaxPixelSamples)
        return fail(c, PT_E_INVALID, "%s: a pixel would pass %lld samples (%llu so far + %d)", who, (long long)kMaxPixelSamples, (unsigned long long)a.n_upper, eff->n_samples);
    return PT_OK;
}

// rows of a W x H image of `elem`-byte pixels, launch order <-> framebuffer order
void flip_rows(void* dst, const void* src, int W, int H, size_t elem)
{
    const size_t row = (size_t)W * elem;
    for (int y = 0; y < H; ++y) std::memcpy((char*)dst + (size_t)(H - 1 - y) * row, (const char*)src + (size_t)y * row, row);
}

// A per-pixel array of the state (launch order in HBM) to the caller in framebuffer order; dst null: none.  The context is idle.
int read_flipped(pt_ctx* c, void* dst, const DevBuf& b, int W, int H, size_t elem, const uint8_t* owned_or_null)
{
    if (!dst) return PT_OK;
    const size_t npx = (size_t)W * H;
    std::vector<char> tmp(npx * elem);
    HIP_TRY(c, hipMemcpy(tmp.data(), b.p, npx * elem, hipMemcpyDeviceToHost));
    if (owned_or_null)
        for (size_t i = 0; i < npx; ++i)
            if (!owned_or_null[i]) std::memset(tmp.data() + i * elem, 0, elem);
    flip_rows(dst, tmp.data(), W, H, elem);
    return PT_OK;
}

// ---- reprojection (pt_accum_reproject*; include/mi355pt.h, "reprojection") -------------------------------------------------------
// What the two calls and the twin refuse alike in the parameters; *eff = the parameters in effect.
int check_reproject_params(pt_ctx* c, const char* who, const pt_reproject_params* p, pt_reproject_params* eff)
{
    if (p) *eff = *p;
    else pt_accum_reproject_default_params(eff);
    if (eff->reserved != 0) return fail(c, PT_E_INVALID, "%s: reserved must be 0 (is %d)", who, eff->reserved);
    if (eff->max_history < 0 || eff->max_history == 1) return fail(c, PT_E_INVALID, "%s: max_history %d must be 0 (no cap) or >= 2", who, eff->max_history);
    if (!(eff->depth_tol >= 0.0f)) return fail(c, PT_E_INVALID, "%s: depth_tol %g must be >= 0 (+inf = test off)", who, (double)eff->depth_tol);
    if (!(eff->albedo_tol >= 0.0f)) return fail(c, PT_E_INVALID, "%s: albedo_tol %g must be >= 0 (+inf = test off)", who, (double)eff->albedo_tol);
    if (!(eff->normal_min <= 1.0f)) return fail(c, PT_E_INVALID, "%s: normal_min %g must be <= 1 (-inf = test off)", who, (double)eff->normal_min);
    return PT_OK;
}

// What pt_accum_reproject and pt_accum_reproject_device refuse before anything is touched, in the order of the header.  A host-only
// context can hold no accumulation: there the arguments alone are judged, and valid ones meet PT_E_NO_DEVICE.
int check_reproject(pt_ctx* c, const char* who, const pt_camera* new_cam, const void* aov_prev, const void* aov_cur, const pt_reproject_params* p, pt_reproject_params* eff)
{
    int rc;
    if (!c->host_only && ((rc = need_accum(c, who)) || (rc = refuse_comm(c, who)) || (rc = check_accum_unchanged(c, who)))) return rc;
    if (!new_cam || !aov_prev || !aov_cur) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !new_cam ? "new_cam" : (!aov_prev ? "aov_prev" : "aov_cur"));
    if ((rc = check_reproject_params(c, who, p, eff))) return rc;
    return need_device(c);
}

// The header's host constants, in its order, from the OLD camera; everything else of *R copied.
void reproject_constants(const pt_camera& old_cam, const pt_camera& new_cam, int W, int H, const pt_reproject_params& prm, PtAccumReproject* R)
{
    const v3 oo = V(old_cam.origin[0], old_cam.origin[1], old_cam.origin[2]), llc = V(old_cam.llc[0], old_cam.llc[1], old_cam.llc[2]);
    const v3 ho = V(old_cam.horizontal[0], old_cam.horizontal[1], old_cam.horizontal[2]), vo = V(old_cam.vertical[0], old_cam.vertical[1], old_cam.vertical[2]);
    const v3 a = llc - oo;
    const v3 N = cross(ho, vo);
    const float inn = 1.0f / dot(N, N);
    const float na = dot(N, a);
    for (int k = 0; k < 3; ++k) {
        R->o[k] = new_cam.origin[k];
        R->llc[k] = new_cam.llc[k];
        R->hor[k] = new_cam.horizontal[k];
        R->ver[k] = new_cam.vertical[k];
        R->oo[k] = old_cam.origin[k];
        R->ho[k] = old_cam.horizontal[k];
        R->vo[k] = old_cam.vertical[k];
    }
    R->a[0] = a.x; R->a[1] = a.y; R->a[2] = a.z;
    R->N[0] = N.x; R->N[1] = N.y; R->N[2] = N.z;
    R->inn = inn;
    R->na = na;
    R->depth_tol = prm.depth_tol;
    R->normal_min = prm.normal_min;
    R->albedo_tol = prm.albedo_tol;
    R->width = W;
    R->height = H;
    R->max_history = prm.max_history;
}

void swap_bufs(DevBuf& x, DevBuf& y)
{
    std::swap(x.p, y.p);
    std::swap(x.cap, y.cap);
}

// The reproject on `stream`, which the caller has ordered after the context's last asynchronous call: the second set of state buffers
// on its first use, the one kernel from the first set into the second, then - on the host, at enqueue: every later call is ordered after
// this one - the two sets swapped and the camera changed.
int reproject_device(pt_ctx* c, const pt_camera& new_cam, const pt_reproject_params& prm, const void* d_aov_prev, const void* d_aov_cur, hipStream_t stream)
{
    Accum& a = *c->acc;
    if (a.adds == 0) { // nothing to move yet: the first add starts every pixel from its seed under the new camera
        a.cam = new_cam;
        return PT_OK;
    }
    PtGeometry g{};
    int grid = 0;
    const hipError_t ge = pt_accum_reproject_geometry(a.w, a.h, &g, &grid);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the reproject kernel spills registers to scratch; such builds are refused (pt_accum_reproject.hip)");
    HIP_TRY(c, ge);
    const size_t npx = (size_t)a.w * a.h;
    int rc;
    if (!a.have_set2) {
        struct Z { DevBuf* b; size_t bytes; };
        for (const Z& z : {Z{&a.sum2, npx * 12}, Z{&a.half2, npx * 12}, Z{&a.n2, npx * 4}, Z{&a.n_half2, npx * 4}, Z{&a.passes2, npx * 4}}) {
            if ((rc = ensure(c, *z.b, z.bytes))) return rc;
            HIP_TRY(c, hipMemsetAsync(z.b->p, 0, z.bytes, stream)); // pixels outside the shard stay +0 in both sets: the kernel writes none of them
        }
        a.have_set2 = true;
    }
    PtAccumReprojectArgs A{};
    reproject_constants(a.cam, new_cam, a.w, a.h, prm, &A.R);
    A.aov_prev = (const float*)d_aov_prev;
    A.aov_cur = (const float*)d_aov_cur;
    A.owned = (const uint8_t*)a.owned.p;
    A.sum_in = (const float*)a.sum.p;
    A.half_in = (const float*)a.half.p;
    A.n_in = (const uint32_t*)a.n.p;
    A.n_half_in = (const uint32_t*)a.n_half.p;
    A.passes_in = (const uint32_t*)a.passes.p;
    A.sum_out = (float*)a.sum2.p;
    A.half_out = (float*)a.half2.p;
    A.n_out = (uint32_t*)a.n2.p;
    A.n_half_out = (uint32_t*)a.n_half2.p;
    A.passes_out = (uint32_t*)a.passes2.p;
    A.seen = (float*)a.seen.p;
    A.noise = (float*)a.noise.p;
    A.out_rgb = (float*)a.out.p;
    A.out_rgba8 = (uint32_t*)a.out8.p;
    A.n_frame = (uint32_t)npx;
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    HIP_TRY(c, pt_launch_accum_reproject(&A, stream));
    HIP_TRY(c, hipEventRecord(c->ev1, stream));
    note_pass(c, a.w, a.h, 1, grid, g, 0, false);
    swap_bufs(a.sum, a.sum2);
    swap_bufs(a.half, a.half2);
    swap_bufs(a.n, a.n2);
    swap_bufs(a.n_half, a.n_half2);
    swap_bufs(a.passes, a.passes2);
    a.cam = new_cam;
    return PT_OK;
}

} // namespace

extern "C" {

void pt_accum_default_params(pt_accum_params* p)
{
    if (!p) return;
    p->n_samples = 16;
    p->max_pixel_samples = 0;
    p->noise_threshold = 0.0f;
    p->reserved = 0;
}

int pt_accum_begin(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, int32_t max_depth)
{
    if (!c || !cam) return PT_E_INVALID;
    const char* who = "pt_accum_begin";
    int rc;
    if ((rc = check_accum_context(c, who))) return rc;
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || max_depth < 0 || max_depth > 63 || (int64_t)W * H > (int64_t)0x7fffffff)
        return fail(c, PT_E_INVALID, "%s: bad render size %dx%d depth %d (depth must be 0..63)", who, W, H, max_depth);
    if ((rc = refuse_comm(c, who)) || (rc = need_device(c))) return rc;
    const int64_t n_owned = pt_shard_pixels(W, H, c->tile, c->rank, c->world, nullptr, 0);
    if (n_owned < 0) return fail(c, PT_E_INVALID, "%s: invalid pixel shard (%d of %d)", who, c->rank, c->world);
    if ((rc = wait_idle(c))) return rc; // an earlier accumulation's buffers are freed: after whatever still reads them
    c->acc.reset();
    std::unique_ptr<Accum> acc(new Accum());
    Accum& a = *acc;
    a.cam = *cam;
    a.w = W;
    a.h = H;
    a.depth = max_depth;
    a.rank = c->rank;
    a.world = c->world;
    a.tile = c->tile;
    a.scene_epoch = c->scene_epoch;
    a.n_owned = (uint32_t)n_owned;
    const size_t npx = (size_t)W * H;
    std::vector<uint32_t> ids((size_t)n_owned);
    pt_shard_pixels(W, H, c->tile, c->rank, c->world, ids.data(), n_owned);
    std::vector<uint8_t> owned(npx, 0);
    std::vector<float> noise(npx, 0.0f);
    for (uint32_t id : ids) {
        owned[id] = 1;
        noise[id] = std::numeric_limits<float>::infinity();
    }
    struct Z { DevBuf* b; size_t bytes; };
    for (const Z& z : {Z{&a.rng, npx * 4}, Z{&a.sum, npx * 12}, Z{&a.seen, npx * 12}, Z{&a.half, npx * 12}, Z{&a.n, npx * 4}, Z{&a.n_half, npx * 4}, Z{&a.passes, npx * 4},
                       Z{&a.active, npx}, Z{&a.count, (size_t)256}, Z{&a.out, npx * 12}, Z{&a.out8, npx * 4}}) {
        if ((rc = ensure(c, *z.b, z.bytes))) return rc;
        HIP_TRY(c, hipMemsetAsync(z.b->p, 0, z.bytes, c->stream));
    }
    if ((rc = upload(c, a.noise, noise.data(), npx * 4)) || (rc = upload(c, a.owned, owned.data(), npx)) || (rc = upload(c, a.queue, ids.data(), ids.size() * 4))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (the staging vectors are locals)
    c->acc = std::move(acc);
    return PT_OK;
}

int pt_accum_add_device(pt_ctx* c, const pt_accum_params* p, void* d_out_rgb, void* d_out_rgba8, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    pt_accum_params prm;
    int rc;
    if ((rc = check_add(c, "pt_accum_add_device", p, &prm)) || (rc = need_device(c))) return rc;
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return add_device(c, prm, d_out_rgb, d_out_rgba8, stream); });
}

int pt_accum_add(pt_ctx* c, const pt_accum_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    pt_accum_params prm;
    int rc;
    if ((rc = check_add(c, "pt_accum_add", p, &prm)) || (rc = need_device(c))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->acc->w * c->acc->h;
    return blocking_call(c, [&]() -> int {
        int rc = add_device(c, prm, nullptr, nullptr, c->stream);
        if (rc) return rc;
        return drain(c, {{out_rgb, c->acc->out.p, npx * 12}, {out_rgba8, c->acc->out8.p, npx * 4}});
    });
}

int pt_accum_read(pt_ctx* c, float* out_rgb, uint32_t* out_rgba8, float* out_noise, uint32_t* out_samples)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = need_accum(c, "pt_accum_read")) || (rc = need_device(c)) || (rc = wait_idle(c))) return rc;
    const Accum& a = *c->acc;
    const size_t npx = (size_t)a.w * a.h;
    if (out_rgb) HIP_TRY(c, hipMemcpy(out_rgb, a.out.p, npx * 12, hipMemcpyDeviceToHost));
    if (out_rgba8) HIP_TRY(c, hipMemcpy(out_rgba8, a.out8.p, npx * 4, hipMemcpyDeviceToHost));
    // (noise is +0 outside the shard since pt_accum_begin, n was never written there)
    if ((rc = read_flipped(c, out_noise, a.noise, a.w, a.h, 4, nullptr)) || (rc = read_flipped(c, out_samples, a.n, a.w, a.h, 4, nullptr))) return rc;
    return check_watchdog(c);
}

int pt_accum_info_get(pt_ctx* c, pt_accum_info* out)
{
    if (!c || !out) return PT_E_INVALID;
    int rc = need_accum(c, "pt_accum_info_get");
    if (rc) return rc;
    const Accum& a = *c->acc;
    out->width = a.w;
    out->height = a.h;
    out->max_path_depth = a.depth;
    out->adds = a.adds;
    out->owned_pixels = a.n_owned;
    out->active_pixels = a.active_pixels;
    out->samples_total = a.samples_total;
    return PT_OK;
}

int pt_accum_end(pt_ctx* c)
{
    if (!c) return PT_E_INVALID;
    if (!c->acc) return PT_OK;
    int rc = wait_idle(c); // an add in flight still uses the buffers
    if (rc) return rc;
    c->acc.reset();
    return PT_OK;
}

int pt_debug_accum_state(pt_ctx* c, float* sum, float* half, uint32_t* n, uint32_t* n_half, uint32_t* passes)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = need_accum(c, "pt_debug_accum_state")) || (rc = need_device(c)) || (rc = wait_idle(c))) return rc;
    const Accum& a = *c->acc;
    std::vector<uint8_t> owned((size_t)a.w * a.h); // sum and the counters were cleared at begin and are only written inside the shard; the mask keeps that true by construction
    HIP_TRY(c, hipMemcpy(owned.data(), a.owned.p, owned.size(), hipMemcpyDeviceToHost));
    if ((rc = read_flipped(c, sum, a.sum, a.w, a.h, 12, owned.data())) || (rc = read_flipped(c, half, a.half, a.w, a.h, 12, owned.data())) ||
        (rc = read_flipped(c, n, a.n, a.w, a.h, 4, owned.data())) || (rc = read_flipped(c, n_half, a.n_half, a.w, a.h, 4, owned.data())) ||
        (rc = read_flipped(c, passes, a.passes, a.w, a.h, 4, owned.data())))
        return rc;
    return PT_OK;
}

int64_t pt_debug_accum_resolve_host(pt_ctx* c, int64_t n_pixels, const float* sum, float* seen, float* half, uint32_t* n, uint32_t* n_half, uint32_t* passes,
                                    const uint8_t* active, const uint8_t* owned, int32_t n_samples, float* out_rgb, uint32_t* out_rgba8, float* noise)
{
    if (!c) return PT_E_INVALID;
    const char* who = "pt_debug_accum_resolve_host";
    if (!sum || !seen || !half || !n || !n_half || !passes || !active || !owned || !out_rgb || !out_rgba8 || !noise) return fail(c, PT_E_INVALID, "%s: NULL array", who);
    if (n_pixels < 0 || n_pixels > 0x7fffffff) return fail(c, PT_E_INVALID, "%s: n_pixels %lld outside 0..2^31-1", who, (long long)n_pixels);
    if (n_samples < 1 || n_samples > 65535) return fail(c, PT_E_INVALID, "%s: n_samples %d outside 1..65535", who, n_samples);
    for (int64_t i = 0; i < n_pixels; ++i) {
        if (!owned[i]) {
            out_rgb[3 * i] = out_rgb[3 * i + 1] = out_rgb[3 * i + 2] = 0.0f;
            out_rgba8[i] = 0u;
            noise[i] = 0.0f;
            continue;
        }
        AccumPixel s;
        for (int k = 0; k < 3; ++k) {
            s.sum[k] = sum[3 * i + k];
            s.seen[k] = seen[3 * i + k];
            s.half[k] = half[3 * i + k];
        }
        s.n = n[i];
        s.n_half = n_half[i];
        s.passes = passes[i];
        AccumResolved o;
        accum_resolve_pixel(s, active[i] != 0, (uint32_t)n_samples, o);
        for (int k = 0; k < 3; ++k) {
            seen[3 * i + k] = s.seen[k];
            half[3 * i + k] = s.half[k];
            out_rgb[3 * i + k] = o.rgb[k];
        }
        n[i] = s.n;
        n_half[i] = s.n_half;
        passes[i] = s.passes;
        out_rgba8[i] = o.rgba8;
        noise[i] = o.noise;
    }
    return n_pixels;
}

int64_t pt_debug_accum_variance_host(pt_ctx* c, int64_t n_pixels, const float* sum, const float* half, const uint32_t* n, const uint32_t* n_half, const uint8_t* owned,
                                     float* out_rgb, float* out_var)
{
    if (!c) return PT_E_INVALID;
    const char* who = "pt_debug_accum_variance_host";
    if (!sum || !half || !n || !n_half || !owned || !out_rgb || !out_var) return fail(c, PT_E_INVALID, "%s: NULL array", who);
    if (n_pixels < 0 || n_pixels > 0x7fffffff) return fail(c, PT_E_INVALID, "%s: n_pixels %lld outside 0..2^31-1", who, (long long)n_pixels);
    for (int64_t i = 0; i < n_pixels; ++i) {
        if (!owned[i]) {
            for (int k = 0; k < 3; ++k) out_rgb[3 * i + k] = out_var[3 * i + k] = 0.0f;
            continue;
        }
        accum_variance_pixel(sum + 3 * i, half + 3 * i, n[i], n_half[i], out_rgb + 3 * i, out_var + 3 * i);
    }
    return n_pixels;
}

int64_t pt_debug_accum_select_host(pt_ctx* c, const float* noise, const uint32_t* n, const uint8_t* owned, int64_t n_pixels, const pt_accum_params* p, uint8_t* active)
{
    if (!c) return PT_E_INVALID;
    const char* who = "pt_debug_accum_select_host";
    if (!noise || !n || !owned || !active) return fail(c, PT_E_INVALID, "%s: NULL array", who);
    if (n_pixels < 0 || n_pixels > 0x7fffffff) return fail(c, PT_E_INVALID, "%s: n_pixels %lld outside 0..2^31-1", who, (long long)n_pixels);
    pt_accum_params prm;
    int rc = check_accum_params(c, who, p, &prm);
    if (rc) return rc;
    int64_t count = 0;
    for (int64_t i = 0; i < n_pixels; ++i) {
        active[i] = (owned[i] && accum_select_pixel(noise[i], n[i], (uint32_t)prm.max_pixel_samples, prm.noise_threshold)) ? 1 : 0;
        count += active[i];
    }
    return count;
}

void pt_accum_reproject_default_params(pt_reproject_params* p)
{
    if (!p) return;
    p->max_history = 0;
    p->reserved = 0;
    p->depth_tol = 0.05f;
    p->normal_min = 0.9f;
    p->albedo_tol = 0.1f;
}

int pt_accum_reproject_device(pt_ctx* c, const pt_camera* new_cam, const void* d_aov_prev, const void* d_aov_cur, const pt_reproject_params* p, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    pt_reproject_params prm;
    int rc;
    if ((rc = check_reproject(c, "pt_accum_reproject_device", new_cam, d_aov_prev, d_aov_cur, p, &prm))) return rc;
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return reproject_device(c, *new_cam, prm, d_aov_prev, d_aov_cur, stream); });
}

int pt_accum_reproject(pt_ctx* c, const pt_camera* new_cam, const float* aov_prev, const float* aov_cur, const pt_reproject_params* p)
{
    if (!c) return PT_E_INVALID;
    pt_reproject_params prm;
    int rc;
    if ((rc = check_reproject(c, "pt_accum_reproject", new_cam, aov_prev, aov_cur, p, &prm))) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->acc->adds == 0) { // only the camera changes (reproject_device): no guides to stage, no kernel to wait for
        if ((rc = wait_idle(c))) return rc;
        return reproject_device(c, *new_cam, prm, aov_prev, aov_cur, c->stream);
    }
    const size_t bytes = (size_t)c->acc->w * c->acc->h * 32;
    return blocking_call(c, [&]() -> int {
        int rc;
        // both guides staged in d_dn_aov (the denoiser's staging of guides), the new camera's first; one copy when they are one buffer
        if ((rc = ensure(c, c->d_dn_aov, 2 * bytes))) return rc;
        char* d_cur = (char*)c->d_dn_aov.p;
        char* d_prev = aov_prev == aov_cur ? d_cur : d_cur + bytes;
        HIP_TRY(c, hipMemcpyAsync(d_cur, aov_cur, bytes, hipMemcpyHostToDevice, c->stream));
        if (d_prev != d_cur) HIP_TRY(c, hipMemcpyAsync(d_prev, aov_prev, bytes, hipMemcpyHostToDevice, c->stream));
        if ((rc = reproject_device(c, *new_cam, prm, d_prev, d_cur, c->stream))) return rc;
        return drain(c, {});
    });
}

int64_t pt_debug_accum_reproject_host(pt_ctx* c, const pt_camera* old_cam, const pt_camera* new_cam, int32_t W, int32_t H, const float* aov_prev, const float* aov_cur,
                                      const uint8_t* owned, const pt_reproject_params* p, float* sum, float* half, uint32_t* n, uint32_t* n_half, uint32_t* passes,
                                      float* out_rgb, uint32_t* out_rgba8, float* out_noise)
{
    if (!c) return PT_E_INVALID;
    const char* who = "pt_debug_accum_reproject_host";
    if (!old_cam || !new_cam || !aov_prev || !aov_cur) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !old_cam ? "old_cam" : (!new_cam ? "new_cam" : (!aov_prev ? "aov_prev" : "aov_cur")));
    if (!sum || !half || !n || !n_half || !passes || !out_rgb || !out_rgba8 || !out_noise) return fail(c, PT_E_INVALID, "%s: NULL array", who);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (int64_t)W * H > (int64_t)0x7fffffff) return fail(c, PT_E_INVALID, "%s: bad frame size %dx%d", who, W, H);
    pt_reproject_params prm;
    int rc = check_reproject_params(c, who, p, &prm);
    if (rc) return rc;
    PtAccumReproject R;
    reproject_constants(*old_cam, *new_cam, W, H, prm, &R);
    // the state by launch id, as the kernel has it: the shared code indexes both alike
    const size_t npx = (size_t)W * H;
    std::vector<uint8_t> own(npx, 1);
    std::vector<float> sum_in(npx * 3), half_in(npx * 3);
    std::vector<uint32_t> n_in(npx), n_half_in(npx), passes_in(npx);
    if (owned) flip_rows(own.data(), owned, W, H, 1);
    flip_rows(sum_in.data(), sum, W, H, 12);
    flip_rows(half_in.data(), half, W, H, 12);
    flip_rows(n_in.data(), n, W, H, 4);
    flip_rows(n_half_in.data(), n_half, W, H, 4);
    flip_rows(passes_in.data(), passes, W, H, 4);
    pt_parallel_ranges((size_t)H, [&](size_t lo, size_t hi) {
        for (size_t y = lo; y < hi; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t id = (size_t)x + (size_t)W * y, ofs = (size_t)x + (size_t)W * ((size_t)H - 1 - y);
                AccumPixel s;
                for (int k = 0; k < 3; ++k) s.sum[k] = s.seen[k] = s.half[k] = 0.0f;
                s.n = s.n_half = s.passes = 0u;
                AccumResolved o;
                o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.0f;
                o.rgba8 = 0u;
                o.noise = 0.0f;
                if (own[id]) {
                    uint32_t q = 0;
                    if (accum_reproject_source(R, x, (int)y, aov_prev, aov_cur, own.data(), &q)) {
                        for (int k = 0; k < 3; ++k) {
                            s.sum[k] = sum_in[3 * (size_t)q + k];
                            s.half[k] = half_in[3 * (size_t)q + k];
                        }
                        s.n = n_in[q];
                        s.n_half = n_half_in[q];
                        s.passes = passes_in[q];
                        accum_reproject_history(s, (uint32_t)prm.max_history);
                    }
                    for (int k = 0; k < 3; ++k) s.seen[k] = s.sum[k];
                    accum_resolve_pixel(s, false, 0u, o);
                }
                for (int k = 0; k < 3; ++k) {
                    sum[3 * ofs + k] = s.sum[k];
                    half[3 * ofs + k] = s.half[k];
                    out_rgb[3 * ofs + k] = o.rgb[k];
                }
                n[ofs] = s.n;
                n_half[ofs] = s.n_half;
                passes[ofs] = s.passes;
                out_rgba8[ofs] = o.rgba8;
                out_noise[ofs] = o.noise;
            }
    });
    return (int64_t)npx;
}

} // extern "C"
