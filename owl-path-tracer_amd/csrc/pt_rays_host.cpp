// pt_rays_host.cpp -- ray queries on the caller's rays (pt_trace_closest*, pt_trace_occluded*, pt_trace_surface*, pt_trace_ao*, pt_trace_hits*):
// ONE device path behind the asynchronous and blocking entry points, the CPU twins pt_debug_trace_rays_host, pt_debug_trace_surface_host,
// pt_debug_trace_ao_host and pt_debug_trace_hits_host, and pt_prim_to_mesh.
// The pass reads the scene and nothing of a frame: no pixel queue, no shard, no environment, no collective - and no materials or
// textures either, except in surface mode, which reads the hit's material row and texel (fill_params: the current table).  Its own
// buffers are d_rays_in / d_rays_out (the blocking forms' staging); the waves' stack overflow columns and the bound flag are the guide
// pass's d_aov_ws (walk_workspace, pt_internal.h) - the two passes are ordered like any two calls of a context, and check_watchdog
// looks at one flag.
#include <algorithm>
#include <cstring>

#include "pt_internal.h"
#include "pt_launch.h"

using namespace pti;

namespace {

#ifndef PT_AO_RANGES
#define PT_AO_RANGES 8 // ranges per resident wave of the ambient-occlusion launch (rays_device); 1 / 2 / 4 / 8 / 16 measured (README.md)
#endif
#ifndef PT_HITS_RANGES
#define PT_HITS_RANGES 1 // ranges per resident wave of the first-K-hits launch (rays_device); 1 / 4 measured (README.md)
#endif
constexpr float kRayTMin = 1e-3f, kRayTMax = 1e10f; // kTMin, kTMax of pt_device.h

static_assert(sizeof(pt_ray) == 32 && sizeof(pt_ray_hit) == 16, "the ray kernels read a ray as two 16-byte loads and store a hit as one");
static_assert(sizeof(pt_surface) == 80, "the surface instances store a record as five 16-byte stores");
static_assert(sizeof(pt_ao_hit) == 32 && sizeof(pt_ao_params) == 16, "the ambient-occlusion kernel stores a record as two 16-byte stores");

// What a call stores per ray: a pt_ray_hit, a byte, a pt_surface, a pt_ao_hit, or K pt_ray_hit.
enum RaysMode { kClosest = 0, kOccluded = 1, kSurface = 2, kAo = 3, kHits = 4 };
constexpr size_t kRecordBytes[5] = {sizeof(pt_ray_hit), 1, sizeof(pt_surface), sizeof(pt_ao_hit), sizeof(pt_ray_hit)}; // kHits: times K (record_bytes)
constexpr int kKernelOf[5] = {0, 0, 1, 2, 3}; // the kernel family that serves a mode: ray kernels (closest and occluded), their surface instances, ambient occlusion, first K hits
// What a mode takes beside the rays: the parameters in effect of an ambient-occlusion call, the K of a first-K-hits call.
struct RaysExtra {
    pt_ao_params ao;
    int32_t k;
};
size_t record_bytes(RaysMode mode, const RaysExtra& x) { return mode == kHits ? (size_t)x.k * kRecordBytes[kHits] : kRecordBytes[mode]; }

// The instances of the ray kernels (pt_launch.h), by [family][watertight], behind one signature: the ray and surface kernels take the
// PtRaysArgs alone, the ambient-occlusion and first-K-hits kernels have no occlusion form to select, and only the last one's geometry
// depends on the call (its LDS grows with K).
template <auto launch> hipError_t rays_only(const PtKernelParams* p, const PtRaysArgs& r, const RaysExtra&, int occluded, int grid, size_t lds_bytes, hipStream_t stream)
{
    return launch(p, &r, occluded, grid, lds_bytes, stream);
}
template <auto geometry> hipError_t rays_geometry(int occluded, int exact, int, PtGeometry* g) { return geometry(occluded, exact, g); }
template <auto launch> hipError_t ao_launch(const PtKernelParams* p, const PtRaysArgs& r, const RaysExtra& x, int, int grid, size_t lds_bytes, hipStream_t stream)
{
    PtAoArgs a{};
    a.r = r;
    a.n_rays = x.ao.n_rays;
    a.flags = x.ao.flags;
    a.thi = x.ao.radius < kRayTMax ? x.ao.radius : kRayTMax; // ao_thi of pt_ao_math.h: +inf gives the library's bound
    a.seed = x.ao.seed;
    return launch(p, &a, grid, lds_bytes, stream);
}
template <auto geometry> hipError_t ao_geometry(int, int exact, int, PtGeometry* g) { return geometry(exact, g); }
template <auto launch> hipError_t hits_launch(const PtKernelParams* p, const PtRaysArgs& r, const RaysExtra& x, int, int grid, size_t lds_bytes, hipStream_t stream)
{
    PtHitsArgs a{};
    a.r = r;
    a.k = x.k;
    return launch(p, &a, grid, lds_bytes, stream);
}
template <auto geometry> hipError_t hits_geometry(int, int exact, int k, PtGeometry* g) { return geometry(exact, k, g); }
const struct RaysInstance {
    hipError_t (*geometry)(int occluded, int exact, int k, PtGeometry* g);
    hipError_t (*launch)(const PtKernelParams* p, const PtRaysArgs& r, const RaysExtra& x, int occluded, int grid, size_t lds_bytes, hipStream_t stream);
} kRaysInstance[4][2] = {{{rays_geometry<pt_rays_geometry>, rays_only<pt_launch_rays>}, {rays_geometry<pt_rays_geometry_wt>, rays_only<pt_launch_rays_wt>}},
                         {{rays_geometry<pt_rays_surface_geometry>, rays_only<pt_launch_rays_surface>}, {rays_geometry<pt_rays_surface_geometry_wt>, rays_only<pt_launch_rays_surface_wt>}},
                         {{ao_geometry<pt_rays_ao_geometry>, ao_launch<pt_launch_rays_ao>}, {ao_geometry<pt_rays_ao_geometry_wt>, ao_launch<pt_launch_rays_ao_wt>}},
                         {{hits_geometry<pt_rays_hits_geometry>, hits_launch<pt_launch_rays_hits>}, {hits_geometry<pt_rays_hits_geometry_wt>, hits_launch<pt_launch_rays_hits_wt>}}};

// What pt_trace_ao, its device form and the twin refuse beside the ray queries' refusals; *eff = the parameters in effect.
int check_ao_params(pt_ctx* c, const char* who, const pt_ao_params* p, pt_ao_params* eff)
{
    if (p) *eff = *p;
    else pt_ao_default_params(eff);
    if (eff->n_rays < 1 || eff->n_rays > 4096) return fail(c, PT_E_INVALID, "%s: n_rays %d outside 1..4096", who, eff->n_rays);
    if (eff->flags & ~PT_AO_SHADING_NORMAL) return fail(c, PT_E_INVALID, "%s: unknown flags 0x%x (PT_AO_SHADING_NORMAL is the only one)", who, (unsigned)eff->flags);
    if (!(eff->radius > 0.0f)) return fail(c, PT_E_INVALID, "%s: radius %g must be > 0 (+inf: the library's bound)", who, (double)eff->radius);
    return PT_OK;
}

// What pt_trace_hits, its device form and the twin refuse beside the ray queries' refusals; *eff = the parameters in effect.
int check_hits_params(pt_ctx* c, const char* who, const pt_hits_params* p, pt_hits_params* eff)
{
    if (p) *eff = *p;
    else pt_hits_default_params(eff);
    if (eff->max_hits < 1 || eff->max_hits > PT_HITS_MAX) return fail(c, PT_E_INVALID, "%s: max_hits %d outside 1..%d", who, eff->max_hits, PT_HITS_MAX);
    if (eff->reserved[0] || eff->reserved[1] || eff->reserved[2]) return fail(c, PT_E_INVALID, "%s: a reserved word of pt_hits_params is not 0", who);
    return PT_OK;
}
// The parameters in effect of a call of `mode` (ao, hits: the caller's or the defaults; null for the other modes), checked.
int check_extra(pt_ctx* c, const char* who, RaysMode mode, const void* params, RaysExtra* x)
{
    *x = RaysExtra{};
    if (mode == kAo) return check_ao_params(c, who, (const pt_ao_params*)params, &x->ao);
    if (mode == kHits) {
        pt_hits_params hp{};
        const int rc = check_hits_params(c, who, (const pt_hits_params*)params, &hp);
        x->k = hp.max_hits;
        return rc;
    }
    return PT_OK;
}

// What every form refuses before anything is touched, a host-only context last (who: the entry point).
int check_rays_args(pt_ctx* c, const char* who, const void* rays, int64_t n, const void* out, bool device, RaysMode mode)
{
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(c, PT_E_INVALID, "%s: n = %lld rays (0 .. 2^31 - 1)", who, (long long)n);
    if (n > 0 && (!rays || !out)) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !rays ? (device ? "d_rays" : "rays") : (device ? "d_out" : "out"));
    if (device && n > 0 && ((uintptr_t)rays & 15u)) return fail(c, PT_E_INVALID, "%s: d_rays is not 16-byte aligned (a ray is two 16-byte loads)", who);
    if (device && mode != kOccluded && n > 0 && ((uintptr_t)out & 15u))
        return fail(c, PT_E_INVALID, "%s: d_out is not 16-byte aligned (a %s)", who, mode == kSurface ? "surface record is five 16-byte stores of its 80 bytes" : mode == kAo ? "record is two 16-byte stores" : mode == kHits ? "ray's records are K 16-byte stores" : "hit is one 16-byte store");
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    // the ray kernels walk the quad nodes - or a root that is itself a leaf - and nothing else
    if (!quad_walk_available(c))
        return fail(c, PT_E_INVALID, "%s: the ray queries need quad nodes (%s)", who, !c->opt.quad ? "option quad = 0" : "the tree is too deep for them");
    return need_device(c);
}

// One launch of the ray kernel over n >= 1 rays in HBM.  A wave owns a contiguous range of whole 64-ray blocks; the grid is what the
// occupancy query says is resident, or fewer when there are fewer blocks.
// x: the parameters in effect of an ambient-occlusion or first-K-hits call (check_extra).
int rays_device(pt_ctx* c, RaysMode mode, const void* d_rays, int64_t n, void* d_out, hipStream_t stream, const RaysExtra& x)
{
    int rc;
    if ((rc = check_quad_walk_size(c, "ray"))) return rc;
    PtKernelParams P;
    fill_params(c, P); // the scene; no camera, so no distance to judge the slab form by: the subtracting form only on request
    P.box_exact = c->opt.box_exact > 0 ? 1 : 0;
    quad_walk_params(c, P);
    const RaysInstance& inst = kRaysInstance[kKernelOf[mode]][c->opt.watertight != 0];
    const int occluded = mode == kOccluded;
    PtGeometry g{};
    const hipError_t ge = inst.geometry(occluded, P.box_exact, x.k, &g);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the ray kernel spills registers to scratch; such builds are refused (pt_kernel.hip)");
    HIP_TRY(c, ge);
    if (g.max_blocks_per_cu < 1) return fail(c, PT_E_LIMIT, "ray kernel does not fit a CU (LDS %zu bytes)", g.lds_bytes);
    const int64_t n_blocks = (n + 63) / 64;
    int64_t resident = (int64_t)c->num_cus * g.max_blocks_per_cu;
    // Ambient occlusion: a ray is 1 + K walks where it hits and one where it misses, so ranges of equal length are not equal work, and
    // with one range per resident wave the launch lasts as long as its all-hit ranges (2 M primary rays of the C4 stand-in, K = 16: 2.5
    // Grays/s).  PT_AO_RANGES times as many, shorter ranges: the hardware hands the later ones to the waves that finish early (8: 6.3
    // Grays/s, one 64-ray block per wave there; 16 is the same launch).  The price is the workspace: an overflow column per range.
    if (mode == kAo) resident *= PT_AO_RANGES;
    // First K hits: one walk per ray, longer where more surfaces lie along it; PT_HITS_RANGES = 1 and 4 measured (README.md).
    if (mode == kHits) resident *= PT_HITS_RANGES;
    if (c->opt.rays_grid > 0) resident = std::min<int64_t>(resident, c->opt.rays_grid); // option "rays_grid": fewer, longer ranges (tests, tuning)
    const int64_t blocks_per_wave = (n_blocks + resident - 1) / resident;
    const int grid = (int)((n_blocks + blocks_per_wave - 1) / blocks_per_wave);
    if (blocks_per_wave * 64 > 0x7fffffc0ll) return fail(c, PT_E_LIMIT, "ray kernel: %lld rays per wave", (long long)blocks_per_wave * 64);
    PtRaysArgs A{};
    A.cap = P.stack_entries + 3;
    if ((rc = walk_workspace(c, A.cap, g.lds_levels, grid, stream, P, &A.ovf))) return rc;
    P.lds_levels = g.lds_levels;
    A.rays = d_rays;
    A.out = d_out;
    A.n = (int32_t)n;
    A.per_wave = (int32_t)(blocks_per_wave * 64);
    A.refill = c->opt.rays_refill;
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    HIP_TRY(c, inst.launch(&P, A, x, occluded, grid, g.lds_bytes, stream));
    HIP_TRY(c, hipEventRecord(c->ev1, stream));
    note_pass(c, (int)std::min<int64_t>(n, 0x7fffffff), 1, 1, grid, g, P.stack_entries, true);
    return PT_OK;
}

int rays_async(pt_ctx* c, const char* who, RaysMode mode, const void* d_rays, int64_t n, void* d_out, void* stream_v, const void* params = nullptr)
{
    if (!c) return PT_E_INVALID;
    int rc;
    RaysExtra x;
    if ((rc = check_extra(c, who, mode, params, &x))) return rc;
    if ((rc = check_rays_args(c, who, d_rays, n, d_out, true, mode))) return rc;
    if (n == 0) return PT_OK;
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return rays_device(c, mode, d_rays, n, d_out, stream, x); });
}

// Host buffers: the rays staged in d_rays_in, the results in d_rays_out, and back.
int rays_blocking(pt_ctx* c, const char* who, RaysMode mode, const pt_ray* rays, int64_t n, void* out, const void* params = nullptr)
{
    if (!c) return PT_E_INVALID;
    int rc;
    RaysExtra x;
    if ((rc = check_extra(c, who, mode, params, &x))) return rc;
    if ((rc = check_rays_args(c, who, rays, n, out, false, mode))) return rc;
    if (n == 0) return PT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t out_bytes = (size_t)n * record_bytes(mode, x);
    return blocking_call(c, [&]() -> int {
        int rc2;
        if ((rc2 = ensure(c, c->d_rays_in, (size_t)n * sizeof(pt_ray))) || (rc2 = ensure(c, c->d_rays_out, out_bytes))) return rc2;
        HIP_TRY(c, hipMemcpyAsync(c->d_rays_in.p, rays, (size_t)n * sizeof(pt_ray), hipMemcpyHostToDevice, c->stream));
        if ((rc2 = rays_device(c, mode, c->d_rays_in.p, n, c->d_rays_out.p, c->stream, x))) return rc2;
        return drain(c, {{out, c->d_rays_out.p, out_bytes}});
    });
}

// What every CPU twin refuses, in this order, `who` by name; then the host scene is brought up to date.  *wt: the watertight option.
int twin_prologue(pt_ctx* c, const char* who, const pt_ray* rays, int64_t n, const void* out, bool* wt)
{
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(c, PT_E_INVALID, "%s: n = %lld rays (0 .. 2^31 - 1)", who, (long long)n);
    if (n > 0 && (!rays || !out)) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !rays ? "rays" : "out");
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    sync_host_scene(c);
    *wt = c->opt.watertight != 0;
    return PT_OK;
}

} // namespace

extern "C" {

int pt_trace_closest(pt_ctx* c, const pt_ray* rays, int64_t n, pt_ray_hit* out) { return rays_blocking(c, "pt_trace_closest", kClosest, rays, n, out); }
int pt_trace_occluded(pt_ctx* c, const pt_ray* rays, int64_t n, uint8_t* out) { return rays_blocking(c, "pt_trace_occluded", kOccluded, rays, n, out); }
int pt_trace_closest_device(pt_ctx* c, const void* d_rays, int64_t n, void* d_out, void* stream) { return rays_async(c, "pt_trace_closest_device", kClosest, d_rays, n, d_out, stream); }
int pt_trace_occluded_device(pt_ctx* c, const void* d_rays, int64_t n, void* d_out, void* stream) { return rays_async(c, "pt_trace_occluded_device", kOccluded, d_rays, n, d_out, stream); }
int pt_trace_surface(pt_ctx* c, const pt_ray* rays, int64_t n, pt_surface* out) { return rays_blocking(c, "pt_trace_surface", kSurface, rays, n, out); }
int pt_trace_surface_device(pt_ctx* c, const void* d_rays, int64_t n, void* d_out, void* stream) { return rays_async(c, "pt_trace_surface_device", kSurface, d_rays, n, d_out, stream); }
int pt_trace_ao(pt_ctx* c, const pt_ray* rays, int64_t n, const pt_ao_params* p, pt_ao_hit* out) { return rays_blocking(c, "pt_trace_ao", kAo, rays, n, out, p); }
int pt_trace_ao_device(pt_ctx* c, const void* d_rays, int64_t n, const pt_ao_params* p, void* d_out, void* stream) { return rays_async(c, "pt_trace_ao_device", kAo, d_rays, n, d_out, stream, p); }

int pt_trace_hits(pt_ctx* c, const pt_ray* rays, int64_t n, const pt_hits_params* p, pt_ray_hit* out) { return rays_blocking(c, "pt_trace_hits", kHits, rays, n, out, p); }
int pt_trace_hits_device(pt_ctx* c, const void* d_rays, int64_t n, const pt_hits_params* p, void* d_out, void* stream) { return rays_async(c, "pt_trace_hits_device", kHits, d_rays, n, d_out, stream, p); }

void pt_hits_default_params(pt_hits_params* p)
{
    if (!p) return;
    p->max_hits = 4;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

void pt_ao_default_params(pt_ao_params* p)
{
    if (!p) return;
    p->n_rays = 16;
    p->flags = 0;
    p->radius = __builtin_inff();
    p->seed = 0u;
}

int64_t pt_debug_trace_rays_host(pt_ctx* c, const pt_ray* rays, int64_t n, int32_t occluded, void* out)
{
    if (!c) return PT_E_INVALID;
    int rc;
    bool wt;
    if ((rc = twin_prologue(c, "pt_debug_trace_rays_host", rays, n, out, &wt))) return rc;
    pt_parallel_ranges((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const pt_ray& r = rays[i];
            const float thi = r.tmax < kRayTMax ? r.tmax : kRayTMax; // NaN and +inf: the library's own bound
            float t = 0.0f, u = 0.0f, v = 0.0f;
            int32_t prim = -1;
            const bool hit = pt_bvh_closest_hit_host(c->scene.bvh, r.org, r.dir, kRayTMin, thi, &t, &u, &v, &prim, wt);
            if (occluded) ((uint8_t*)out)[i] = hit ? 1 : 0;
            else ((pt_ray_hit*)out)[i] = hit ? pt_ray_hit{t, u, v, prim} : pt_ray_hit{0.0f, 0.0f, 0.0f, -1};
        }
    });
    return n;
}

int64_t pt_debug_trace_surface_host(pt_ctx* c, const pt_ray* rays, int64_t n, pt_surface* out)
{
    if (!c) return PT_E_INVALID;
    int rc;
    bool wt;
    if ((rc = twin_prologue(c, "pt_debug_trace_surface_host", rays, n, out, &wt))) return rc;
    const std::vector<int32_t> slot_of = slot_of_prim(c->scene);
    pt_parallel_ranges((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const pt_ray& r = rays[i];
            const float thi = r.tmax < kRayTMax ? r.tmax : kRayTMax; // NaN and +inf: the library's own bound
            float t = 0.0f, u = 0.0f, v = 0.0f;
            int32_t prim = -1;
            const bool hit = pt_bvh_closest_hit_host(c->scene.bvh, r.org, r.dir, kRayTMin, thi, &t, &u, &v, &prim, wt);
            surface_record_host(c->scene, hit ? slot_of[(size_t)prim] : -1, t, u, v, prim, &out[i]);
        }
    });
    return n;
}

int64_t pt_debug_trace_ao_host(pt_ctx* c, const pt_ray* rays, int64_t n, const pt_ao_params* p, pt_ao_hit* out, pt_ray* out_ao_rays)
{
    if (!c) return PT_E_INVALID;
    int rc;
    pt_ao_params prm{};
    if ((rc = check_ao_params(c, "pt_debug_trace_ao_host", p, &prm))) return rc;
    bool wt;
    if ((rc = twin_prologue(c, "pt_debug_trace_ao_host", rays, n, out, &wt))) return rc;
    const std::vector<int32_t> slot_of = slot_of_prim(c->scene);
    pt_parallel_ranges((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) ao_ray_host(c->scene, slot_of, wt, rays[i], (uint32_t)i, prm, &out[i], out_ao_rays ? out_ao_rays + i * (size_t)prm.n_rays : nullptr);
    });
    return n;
}

int64_t pt_debug_trace_hits_host(pt_ctx* c, const pt_ray* rays, int64_t n, const pt_hits_params* p, pt_ray_hit* out)
{
    if (!c) return PT_E_INVALID;
    int rc;
    pt_hits_params prm{};
    if ((rc = check_hits_params(c, "pt_debug_trace_hits_host", p, &prm))) return rc;
    bool wt;
    if ((rc = twin_prologue(c, "pt_debug_trace_hits_host", rays, n, out, &wt))) return rc;
    const int K = prm.max_hits;
    pt_parallel_ranges((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const pt_ray& r = rays[i];
            const float thi = r.tmax < kRayTMax ? r.tmax : kRayTMax; // NaN and +inf: the library's own bound
            float t[PT_HITS_MAX], u[PT_HITS_MAX], v[PT_HITS_MAX];
            int32_t prim[PT_HITS_MAX];
            const int found = pt_bvh_first_hits_host(c->scene.bvh, r.org, r.dir, kRayTMin, thi, K, t, u, v, prim, wt);
            for (int j = 0; j < K; ++j) out[i * (size_t)K + j] = j < found ? pt_ray_hit{t[j], u[j], v[j], prim[j]} : pt_ray_hit{0.0f, 0.0f, 0.0f, -1};
        }
    });
    return n;
}

int pt_prim_to_mesh(pt_ctx* c, int32_t prim, int32_t* mesh, int32_t* triangle)
{
    if (!c) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_prim_to_mesh: no geometries (pt_upload_scene not called)");
    const std::vector<uint64_t>& first = c->scene.mesh_first; // n_meshes + 1 prefix sums
    if (prim < 0 || first.size() < 2 || (uint64_t)prim >= first.back())
        return fail(c, PT_E_INVALID, "pt_prim_to_mesh: triangle id %d outside 0 .. %lld", prim, first.empty() ? -1ll : (long long)first.back() - 1);
    // the last mesh that starts at or before prim (meshes without triangles share their successor's start and are never the answer)
    const size_t m = (size_t)(std::upper_bound(first.begin(), first.end() - 1, (uint64_t)prim) - first.begin()) - 1;
    if (mesh) *mesh = (int32_t)m;
    if (triangle) *triangle = (int32_t)((uint64_t)prim - first[m]);
    return PT_OK;
}

} // extern "C"
