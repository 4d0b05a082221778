// pt_internal.h -- private to the library: the context behind the opaque pt_ctx of include/mi355pt.h and the helpers its host sources
// share: pt_api.cpp (context, options, stats), pt_scene.cpp (scene upload and clone), pt_render.cpp (frames and batches), pt_guides.cpp
// (guide pass and the device paths of the filters), pt_aov_host.cpp, pt_denoise_host.cpp and pt_upsample_host.cpp (refusals, constants
// and CPU twins of the guide pass, the two denoisers and the upsampler), pt_accum_host.cpp (progressive accumulation and its
// reprojection), pt_rays_host.cpp (ray queries), pt_points_host.cpp (point queries), pt_debug.cpp (probes and readers) and pt_comm.cpp
// (RCCL reduce, multi-GPU group). A source that runs device arithmetic on the CPU includes pt_device_host.h before its *_math.h.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mi355pt.h"
#include "pt_bvh.h"
#include "pt_launch.h"
#include "pt_types.h"

// A device allocation and its owner: freed with the object that holds it (a context, a group, a local of one call).  A buffer that was
// never allocated frees nothing, so a host-only context (device < 0) never calls into HIP.  Movable, not copyable (the move constructor
// leaves no implicit copy).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct HostTexture {
    int w = 0, h = 0;
    std::vector<uint32_t> px;
};

// What an upload with option "dynamic" = 1 keeps beside the scene so that pt_update_vertices can move its vertices (pt_scene.cpp).
struct DynScene {
    bool enabled = false;
    std::vector<float> verts, normals;                   // the meshes' arrays, concatenated; mesh m starts at vbase[m] / nbase[m] (elements of 3 floats)
    std::vector<int32_t> vbase, nbase, n_verts, n_normals; // per mesh, counts as pt_upload_scene was given them
    PtRefit refit;
    // a device context refits in HBM only: the host copies (triangle records, three hierarchies, and the shading normals when
    // stale_normals) are brought up to date by the first call that reads them (pti::sync_host_scene)
    bool host_stale = false, stale_normals = false;
    double info[8] = {};                                 // pt_debug_update_info
};

// The host copies of an uploaded scene: everything a replica of a multi-GPU group takes over from device 0 (pti::clone_scene is one
// assignment of this), and the four figures of pt_stats that describe it.
struct HostScene {
    PtBvh bvh;
    std::vector<PtNode4> nodes4; // two-level collapse of bvh.nodes for the wavefront kernel (pt_bvh_collapse4)
    int32_t root4 = -1;
    int depth4 = 0;
    std::vector<PtNode8> nodes8; // three-level collapse for the group walk of sparse waves (pt_bvh_collapse8)
    int32_t root8 = -1;
    int depth8 = 0;
    std::vector<PtShade> shade;
    std::vector<float> materials; // n * PT_MAT_STRIDE
    int n_materials = 0;
    std::vector<int32_t> material_texture;
    std::vector<HostTexture> textures;
    pt_env env{};
    HostTexture env_map;
    uint64_t bvh_nodes = 0, bvh_depth = 0, n_triangles = 0; // pt_stats
    std::vector<uint64_t> mesh_first; // global id of every mesh's first triangle, then n_triangles: the prefix sums pt_prim_to_mesh inverts
    double bvh_build_ms = 0.0;
    DynScene dyn;
};

// pt_set_option: every option with its default.
struct PtOptions {
    int spp_per_launch = 0, count = 0, blocks_per_cu = 0, leaf_size = 4, max_bvh_depth = 48, kernel = 2, slots_per_wave = 0, chunk_spp = 64, chunk_tail_min = -1, schedule = 1, prepass_spp = 0, census_mode = 0, sticky_pct = -1, latency = 0, cost_radius = 2, timeline = 0, node_pairs = 0, leaf_align = 1, bvh_builder = 3, quad = 1, groups = 1, wide_leaves = 1, fallback = 0, ploc_radius = 16, express_permille = -1, ns_express = 8, whole = -1, box_exact = -1, batch_frames = 0, watertight = 0, dynamic = 0, rays_refill = 32, rays_grid = 0;
    int tune[8] = {};
};

// What the pixel queue in d_pixels was made for (ensure_queue).
struct QueueKey {
    int w = 0, h = 0, frames = 1, rank = 0, world = 1, tile = 16;
    bool operator==(const QueueKey& o) const { return w == o.w && h == o.h && frames == o.frames && rank == o.rank && world == o.world && tile == o.tile; }
};

// What a finished frame - or launch sequence of a batch - leaves behind for pt_synchronize, pt_get_stats, the watchdog check and the
// diagnostics readers.  Written by finish_frame (pt_render.cpp) and note_pass (pt_guides.cpp) alone; the readers only take the two pending marks down, and `stream`
// belongs to the ordering helpers below (order_after_last, mark_last, wait_idle).
struct LastFrame {
    bool ev_pending = false;    // ev0 .. ev1 have not been turned into pt_stats.kernel_ms yet
    bool flag_pending = false, watchdog_fired = false; // the watchdog flag of the last render has not been looked at yet / was set
    hipStream_t stream = nullptr; // stream of the context's last asynchronous call (may be the caller's), with evo recorded at its end;
                                  // nullptr once the host has waited for it (pti::wait_idle, the end of a blocking render)
    int launches = 0;           // render-kernel launches, of all launch sequences of a batch (pt_stats.launches)
    bool sorted = false;
    int w = 0, h = 0;
    int chunks = 0;             // of the last frame that ran a kernel, with the offset of its timelines in d_laps
    size_t lap_ticks_ofs = 0;
    int seqs = 1;               // launch sequences of the last render (pt_render_batch may need several)
    bool aov_flag_pending = false; // the last call was a guide pass (pt_render_aov*) that ran a kernel: its bound flag in d_aov_ws has not been looked at yet
};

// The context's progressive accumulation (pt_accum_*; pt_accum_host.cpp): the frame that grows by adds, and the owner of its state across
// calls.  No other call of the header writes these buffers; pt_accum_variance and pt_accum_denoise (pt_guides.cpp) read them.  Everything per pixel is indexed by the launch id x + W * y except
// out / out8 (framebuffer order).
struct Accum {
    pt_camera cam{};
    int w = 0, h = 0, depth = 0;
    int rank = 0, world = 1, tile = 16; // the pixel shard as pt_accum_begin found it
    uint64_t scene_epoch = 0;           // ... and the upload it found (pt_ctx::scene_epoch)
    uint32_t n_owned = 0;
    int adds = 0;
    int64_t active_pixels = 0;          // of the last add
    uint64_t samples_total = 0;
    uint64_t n_upper = 0;               // no pixel has more samples than this: the sum of the adds' n_samples
    DevBuf rng, sum;                    // the render kernel's rng_state / accum
    DevBuf seen, half, n, n_half, passes, noise, owned, active;
    DevBuf queue;                       // the shard's pixel queue (n_owned ids), kept: other calls rewrite the context's d_pixels
    DevBuf count;                       // select's counter, 256 bytes of its own
    DevBuf out, out8;                   // resolve's image
    // pt_accum_reproject: the second set of sum / half / n / n_half / passes (36 bytes per pixel), allocated and cleared by the first
    // reproject; the kernel gathers from the first set into this one and the call swaps the two (swap_sets)
    DevBuf sum2, half2, n2, n_half2, passes2;
    bool have_set2 = false;
};

struct pt_ctx {
    int device = -1;
    bool host_only = false;
    int num_cus = 0;
    hipStream_t stream = nullptr;
    hipEvent_t evu0 = nullptr, evu1 = nullptr; // around the kernels of the last pt_update_vertices (created by the first one)
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evm = nullptr, evr = nullptr, evd = nullptr; // evm: after the cost pre-pass and the queue sort; evr / evd: after the reduce / the read-back of pt_render
    hipEvent_t evo = nullptr; // the ordering event: end of the last asynchronous call, on last.stream (no timing; never one of the events above)
    std::string err;

    HostScene scene;
    bool have_scene = false;
    uint64_t scene_epoch = 0; // counts pt_upload_scene / clone_scene: what was begun on an earlier scene notices (pt_accum_add)

    // device
    DevBuf d_nodes8, d_nodes4, d_nodes, d_tris, d_shade, d_materials, d_texdesc, d_env, d_pixels, d_heads, d_rng, d_accum, d_out, d_out8, d_counters, d_dbg_in, d_dbg_out, d_slots, d_laps, d_ring, d_params, d_cost, d_sorted, d_sort_scratch, d_dbg_start, d_bucket, d_tiers, d_batch_mats, d_batch_cams, d_seq_flags; // d_batch_*: per-frame tables of pt_render_batch; d_seq_flags: watchdog flags of its earlier launch sequences
    DevBuf d_verts, d_vnormals, d_tri_vi, d_level_nodes, d_src4, d_src8, d_refit_ws; // option "dynamic": what the refit kernels read (pt_refit.hip)
    DevBuf d_aov, d_aov_ws; // guide pass: the frame of pt_render_aov / pt_group_render_aov; bound flag (64 words) + the waves' stack overflow columns
    DevBuf d_dn_ws, d_dn_rgb, d_dn_aov, d_dn_out8; // denoiser: the filter's records (pt_denoise_workspace_bytes); pt_denoise's staging of rgb (in and out), guides and RGBA8
    DevBuf d_dn_var; // pt_denoise_var's staging of the variance map; pt_accum_variance's / pt_accum_denoise's map of the accumulation
    DevBuf d_rays_in, d_rays_out; // ray queries: the blocking forms' staging of the rays and of the results (pt_rays_host.cpp; the overflow columns and the bound flag are the guide pass's d_aov_ws)
    DevBuf d_ray_image; // ray images: the blocking form's staging of the caller's table (pt_render_rays, pt_render.cpp)
    DevBuf d_up_ws, d_up_rgb, d_up_aov; // upsampling: the low frame's records (pt_upsample_workspace_bytes); pt_upsample's staging of the low frame and its guides (the high guides and both outputs stage in d_dn_aov, d_dn_rgb, d_dn_out8)
    std::vector<DevBuf> d_textures;
    DevBuf d_cost_image; // pt_debug_set_cost_image: the caller's cost image, which run_launches copies over d_cost in launch sequences of its size
    int cost_image_w = 0, cost_image_h = 0; // 0 x 0: none set, the measured costs stand

    // pixel queue
    QueueKey queue;
    bool queue_valid = false;
    int rank = 0, world = 1, tile = 16;
    uint32_t n_pixels = 0;

    PtOptions opt;

    void* comm = nullptr;   // ncclComm_t once pt_comm_init_rank / pt_group_create attached one (pt_comm.cpp)
    int comm_rank = 0, comm_world = 1;

    pt_stats stats{}; // (its scene figures are kept in `scene`: pt_get_stats)
    LastFrame last;
    std::vector<float> batch_cams_h, batch_mats_h; // pt_render_batch: staging of the per-frame tables
    std::unique_ptr<Accum> acc; // pt_accum_begin .. pt_accum_end
};

// Helpers that more than one host source uses.  The library is built with default visibility, so the five that existed before the host
// layer was split stay among its exported names as they were; the ones the split added are PT_LOCAL and add nothing to that list.
#define PT_LOCAL __attribute__((visibility("hidden")))
namespace pti {
// pt_api.cpp
int fail(pt_ctx* c, int code, const char* fmt, ...);
int ensure(pt_ctx* c, DevBuf& b, size_t bytes);
PT_LOCAL int upload(pt_ctx* c, DevBuf& b, const void* src, size_t bytes);
PT_LOCAL int need_device(pt_ctx* c);
// A context has ONE frame's worth of work buffers, so every call that touches them is ordered after the context's last asynchronous
// call, whichever stream that call used (include/mi355pt.h, pt_render_device):
PT_LOCAL int order_after_last(pt_ctx* c, hipStream_t stream); // before a call enqueues on `stream`: a device-side wait, and only when the last call used another stream
PT_LOCAL int mark_last(pt_ctx* c, hipStream_t stream);        // after an asynchronous call has enqueued its last on `stream`
PT_LOCAL int wait_idle(pt_ctx* c);                            // the blocking calls: the host waits for last.stream (if it is not the context's), then for the context's
// pt_scene.cpp
int upload_scene_to_device(pt_ctx* c);
int clone_scene(pt_ctx* dst, const pt_ctx* src);
PT_LOCAL void sync_host_scene(pt_ctx* c); // after a pt_update_vertices on the device: the host copies refitted, if they are stale
PT_LOCAL void material_row(const pt_ctx* c, float* dst, const float* src, int i);
// pt_render.cpp
int check_watchdog(pt_ctx* c);
PT_LOCAL void fill_params(pt_ctx* c, PtKernelParams& P);
PT_LOCAL void walk_params(pt_ctx* c, const pt_camera* cam, PtKernelParams& P);
// What a one-wave quad walk (guide pass, ray queries; pt_aov_first.h, pt_aov_follow.h, pt_rays_kernels.h) needs from the host.  Its workspace
// is d_aov_ws: kWalkFlagWords words whose first is the walks' bound flag, on a line of its own, then the waves' stack overflow columns.
constexpr size_t kWalkFlagWords = 64;
PT_LOCAL bool quad_walk_available(const pt_ctx* c);            // quad nodes, or a root that is itself a leaf (walk_params asks for nodes: the wavefront kernel takes a leaf root another way)
PT_LOCAL void quad_walk_params(pt_ctx* c, PtKernelParams& P);  // P.nodes4, P.root, P.stack_entries
PT_LOCAL int check_quad_walk_size(pt_ctx* c, const char* kernel); // PT_E_LIMIT: the quad-node and leaf steps address their records with 32-bit byte offsets
PT_LOCAL int shard_tile(int tile);                             // as pt_shard_pixels rounds it: a multiple of 8, at least 8
// d_aov_ws for `grid` workgroups whose lanes may use `cap` stack levels, lds_levels of them in LDS: sized, the flag words cleared on
// `stream`, P.error_flag on the flag, *ovf on the columns ((cap - lds_levels) * 64 words per workgroup)
PT_LOCAL int walk_workspace(pt_ctx* c, int cap, int lds_levels, int grid, hipStream_t stream, PtKernelParams& P, uint32_t** ovf);
PT_LOCAL int check_render_args(pt_ctx* c, int W, int H, int max_samples, int max_depth, const int32_t* n_materials = nullptr);
// a ray image's table (pt_render_rays*, pt_render_aov_rays* and the guide twin): pointers; then communicator (comm) and, of a host table, the records
PT_LOCAL int check_ray_ptrs(pt_ctx* c, const char* who, const void* rays, const void* out, const char* out_name, bool device);
PT_LOCAL int check_ray_table(pt_ctx* c, const char* who, const void* rays, int W, int H, bool device, bool comm);
PT_LOCAL float ray_table_far_o(const pt_ray_gen* rays, size_t n); // the largest |org| component: decides the slab form as a camera's origin does
PT_LOCAL int64_t batch_max_frames(int W, int H, int max_frames);
PT_LOCAL int stage_batch_tables(pt_ctx* c, const pt_frame* frames, int n_frames, hipStream_t stream);
struct D2H { void* dst; const void* src; size_t bytes; }; // a copy to a host buffer of the caller; dst null: none
PT_LOCAL int drain(pt_ctx* c, std::initializer_list<D2H> copies);
// One add of the progressive accumulation over the pixel queue as it stands (d_pixels, n_pixels; none: no kernel runs): the frame path
// with the pixels' state in d_rng / d_sum and no framebuffer.  `resolve` enqueues what follows the launches and lies inside kernel_ms, which
// starts at ev0: recorded here before the first launch, or by the caller before its select launch (ev0_recorded).
PT_LOCAL int accum_frame(pt_ctx* c, const pt_camera* cam, int W, int H, int n_samples, int max_depth, bool first_add, uint32_t* d_rng, float* d_sum, hipStream_t stream,
                         bool ev0_recorded, const std::function<int()>& resolve);
// pt_denoise_host.cpp
PT_LOCAL int check_denoise_args(pt_ctx* c, const char* who, int W, int H, const pt_denoise_params* p, pt_denoise_params* eff,
                                void (*defaults)(pt_denoise_params*) = pt_denoise_default_params); // the refusals of pt_denoise*, pt_denoise_var* and the twins; *eff = the parameters in effect (p null: defaults)
PT_LOCAL void denoise_constants(const pt_denoise_params& p, float* kn, float* ka, float kc[8]); // the definition's host constants
// pt_upsample_host.cpp
PT_LOCAL int check_upsample_args(pt_ctx* c, const char* who, int w, int h, int W, int H, const pt_upsample_params* p, pt_upsample_params* eff); // the refusals of pt_upsample* and the twin; *eff = the parameters in effect (p null: defaults)
PT_LOCAL void upsample_constants(const pt_upsample_params& p, int w, int h, int W, int H, float* rx, float* ry, float* kn, float* ka, float* ir); // the definition's host constants
// pt_guides.cpp
// End of an auxiliary pass, after its ev1: the one place beside finish_frame (pt_render.cpp) that writes what pt_synchronize and
// pt_get_stats look at.  kernel_ms is ev0 .. ev1; g: the geometry of the pass's kernel; aov_flag: a guide pass, whose bound flag in
// d_aov_ws check_watchdog has to look at.
PT_LOCAL void note_pass(pt_ctx* c, int W, int H, int launches, int grid, const PtGeometry& g, int stack_entries, bool aov_flag);
// pt_accum_host.cpp
PT_LOCAL int need_accum(pt_ctx* c, const char* who);  // PT_E_INVALID by name without an accumulation
PT_LOCAL int refuse_comm(pt_ctx* c, const char* who); // PT_E_INVALID by name with a communicator
// pt_aov_host.cpp
PT_LOCAL int check_aov_params(pt_ctx* c, const pt_aov_params* p, const char* who, pt_aov_params* eff); // the refusals of pt_render_aov_follow* and the twin; *eff = the parameters in effect
// global triangle id -> leaf-order slot of the host scene as it stands (after sync_host_scene): the host walk reports the id, the triangle
// and shading records are in leaf order.  Built per call: nothing to invalidate where bvh.tris is rebuilt or reordered.
PT_LOCAL std::vector<int32_t> slot_of_prim(const HostScene& S);
// the surface record of pt_trace_surface at the hit (t, u, v, prim) on the triangle in leaf-order slot `slot` (< 0: the miss record), from the host
// copies of the scene with the arithmetic of pt_device.h: csrc/pt_surface.h expression for expression (pt_debug_trace_surface_host)
PT_LOCAL void surface_record_host(const HostScene& S, int32_t slot, float t, float u, float v, int32_t prim, pt_surface* out);
// one ray of pt_debug_trace_ao_host: the definition of pt_trace_ao for ray `index` through the host walk and csrc/pt_ao_math.h, the
// header the kernel compiles.  slot_of: global triangle id -> leaf-order slot; out_rays: null, or the n_rays records of this ray
PT_LOCAL void ao_ray_host(const HostScene& S, const std::vector<int32_t>& slot_of, bool wt, const pt_ray& r, uint32_t index, const pt_ao_params& prm, pt_ao_hit* out,
                          pt_ray* out_rays);
// pt_comm.cpp
PT_LOCAL int reduce_framebuffer(pt_ctx* c, void* d_rgb, void* d_rgba8, int64_t n_pixels, hipStream_t stream); // pt_reduce_framebuffer inside a call that is ordered already
PT_LOCAL int reduce_sum(pt_ctx* c, void* d_buf, size_t n_floats, hipStream_t stream); // in-place sum-reduce onto rank 0; nothing without a communicator

#define HIP_TRY(c, call)                                                                                   \
    do {                                                                                                   \
        hipError_t e__ = (call);                                                                           \
        if (e__ != hipSuccess) return pti::fail(c, PT_E_HIP, "%s failed: %s", #call, hipGetErrorString(e__)); \
    } while (0)

// An asynchronous entry point around `enqueue`: ordered after the context's last asynchronous call on the device, and itself the last
// one from here on - also when it failed half-way, for what it did enqueue.
template <class F> int async_call(pt_ctx* c, hipStream_t stream, F enqueue)
{
    int rc = order_after_last(c, stream);
    if (rc) return rc;
    rc = enqueue();
    const int rm = mark_last(c, stream);
    return rc ? rc : rm;
}

// async_call for an entry point that takes the caller's stream as void*: on the context's device and on that stream (null: the context's
// own), which `enqueue` receives.
template <class F> int async_call_on(pt_ctx* c, void* stream_v, F enqueue)
{
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t stream = stream_v ? (hipStream_t)stream_v : c->stream;
    return async_call(c, stream, [&] { return enqueue(stream); });
}

// A blocking render around `run`, which enqueues on the context's stream and drains it: ordered after the last asynchronous call like
// any other (nothing is added on an idle context or behind a call on the context's own stream).  If it fails, what it did enqueue
// may still be pending on the context's stream, which is then the last one for the next call to wait for.
template <class F> int blocking_call(pt_ctx* c, F run)
{
    int rc = order_after_last(c, c->stream);
    if (rc) return rc;
    if ((rc = run())) (void)mark_last(c, c->stream);
    return rc;
}
} // namespace pti
