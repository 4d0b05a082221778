// pt_accum_host.cpp -- the progressive accumulation (pt_accum_*; include/mi355pt.h, "progressive accumulation"): a frame that grows by
// adds.  This file owns the accumulation's state across calls (Accum, pt_internal.h), runs an add - select, the frame path of
// pt_render.cpp over the active set (pti::accum_frame), resolve - and holds the CPU twins of the two kernels of pt_accum.hip, which
// compile the very definition the kernels compile (pt_accum_math.h with PTD = static inline, as pt_denoise_host.cpp does).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

static inline uint32_t pt_host_float_as_uint(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static inline float pt_host_uint_as_float(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
#define __float_as_uint pt_host_float_as_uint
#define __uint_as_float pt_host_uint_as_float
#define PTD static inline
#include "pt_accum_math.h"
#undef __float_as_uint
#undef __uint_as_float

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

// Everything an add refuses before it touches anything, in the order of the header; *eff = the parameters in effect.
int check_add(pt_ctx* c, const char* who, const pt_accum_params* p, pt_accum_params* eff)
{
    int rc;
    if ((rc = check_accum_params(c, who, p, eff)) || (rc = check_accum_context(c, who)) || (rc = need_accum(c, who)) || (rc = refuse_comm(c, who))) return rc;
    const Accum& a = *c->acc;
    if (a.rank != c->rank || a.world != c->world || a.tile != c->tile)
        return fail(c, PT_E_INVALID, "%s: the pixel shard changed after pt_accum_begin (%d of %d tile %d, now %d of %d tile %d); begin again", who, a.rank, a.world, a.tile, c->rank, c->world, c->tile);
    if (a.scene_epoch != c->scene_epoch) return fail(c, PT_E_INVALID, "%s: a new scene was uploaded after pt_accum_begin; begin again", who);
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
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : c->stream;
    return async_call(c, stream, [&] { return add_device(c, prm, d_out_rgb, d_out_rgba8, stream); });
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

} // extern "C"
