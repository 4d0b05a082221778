// pt_points_host.cpp -- nearest-surface queries for the caller's points (pt_closest_point*): ONE device path behind the asynchronous and
// the blocking entry point, and the CPU twin pt_debug_closest_point_host.
// The pass reads the triangles and the quad nodes and nothing else of the scene, and nothing of a frame: no pixel queue, no shard, no
// materials, no environment, no collective.  Its buffers are the ray queries': d_rays_in / d_rays_out stage the blocking form's points
// and records, the waves' stack overflow columns and the bound flag are the guide pass's d_aov_ws (walk_workspace, pt_internal.h) - the
// passes are ordered like any two calls of a context, and check_watchdog looks at one flag.
// The twin is the DEFINITION, not a walk: every triangle of the host copy in leaf order against every point, through pt_points_math.h,
// the header the kernel compiles.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "pt_device_host.h"
#include "pt_points_math.h"

#include "pt_internal.h"
#include "pt_launch.h"

using namespace pti;

namespace {

#ifndef PT_POINTS_RANGES
#define PT_POINTS_RANGES 4 // ranges per resident wave of the point launch (points_device); 1 / 2 / 4 / 8 measured (README.md)
#endif
static_assert(sizeof(pt_point) == 16 && sizeof(pt_point_hit) == 32, "the point kernel reads a point as one 16-byte load and stores a record as two");

// What every form refuses before anything is touched, a host-only context last (who: the entry point).
int check_points_args(pt_ctx* c, const char* who, const void* pts, int64_t n, const void* out, bool device)
{
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(c, PT_E_INVALID, "%s: n = %lld points (0 .. 2^31 - 1)", who, (long long)n);
    if (n > 0 && (!pts || !out)) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !pts ? (device ? "d_pts" : "pts") : (device ? "d_out" : "out"));
    if (device && n > 0 && ((uintptr_t)pts & 15u)) return fail(c, PT_E_INVALID, "%s: d_pts is not 16-byte aligned (a point is one 16-byte load)", who);
    if (device && n > 0 && ((uintptr_t)out & 15u)) return fail(c, PT_E_INVALID, "%s: d_out is not 16-byte aligned (a record is two 16-byte stores)", who);
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    if (!quad_walk_available(c))
        return fail(c, PT_E_INVALID, "%s: the point queries need quad nodes (%s)", who, !c->opt.quad ? "option quad = 0" : "the tree is too deep for them");
    return need_device(c);
}

// One launch of the point kernel over n >= 1 points in HBM.  A wave owns a contiguous range of whole 64-point blocks.
// A point far from every surface walks many times the nodes of a point next to one, and points that are neighbours in the caller's
// order are neighbours in space, so ranges of equal length are not equal work: with one range per resident wave, as the closest-hit
// call cuts them, 2 M lattice points over the C4 stand-in ran at 628 Mpoints/s and the same points shuffled at 1 147.  PT_POINTS_RANGES
// times as many, shorter ranges, which the hardware hands to the waves that finish early: 880 / 1 190 / 950 for 2 / 4 / 8 on the lattice
// and 1 165 / 1 423 / 2 647 on points next to the surface, against 869 / 697 / 532 shuffled (a short range has nothing to refill from).
// 4 has the least time summed over the three sets on that scene and all but the least on the other (README.md).  The price is the
// workspace: an overflow column per range.
int points_device(pt_ctx* c, const void* d_pts, int64_t n, void* d_out, hipStream_t stream)
{
    int rc;
    if ((rc = check_quad_walk_size(c, "point"))) return rc;
    PtKernelParams P;
    fill_params(c, P);
    quad_walk_params(c, P);
    PtGeometry g{};
    const hipError_t ge = pt_points_geometry(&g);
    if (ge == hipErrorInvalidConfiguration) return fail(c, PT_E_LIMIT, "this build of the point kernel spills registers to scratch; such builds are refused (pt_kernel.hip)");
    HIP_TRY(c, ge);
    if (g.max_blocks_per_cu < 1) return fail(c, PT_E_LIMIT, "point kernel does not fit a CU (LDS %zu bytes)", g.lds_bytes);
    const int64_t n_blocks = (n + 63) / 64;
    int64_t resident = (int64_t)c->num_cus * g.max_blocks_per_cu * PT_POINTS_RANGES;
    if (c->opt.rays_grid > 0) resident = std::min<int64_t>(resident, c->opt.rays_grid); // option "rays_grid": fewer, longer ranges (tests, tuning)
    const int64_t blocks_per_wave = (n_blocks + resident - 1) / resident;
    const int grid = (int)((n_blocks + blocks_per_wave - 1) / blocks_per_wave);
    if (blocks_per_wave * 64 > 0x7fffffc0ll) return fail(c, PT_E_LIMIT, "point kernel: %lld points per wave", (long long)blocks_per_wave * 64);
    PtRaysArgs A{};
    A.cap = P.stack_entries + 3; // entries; the kernel's entry is pt_points_entry_words() words, g.lds_levels of a lane's words are in LDS
    if ((rc = walk_workspace(c, A.cap * pt_points_entry_words(), g.lds_levels, grid, stream, P, &A.ovf))) return rc;
    P.lds_levels = g.lds_levels;
    A.rays = d_pts;
    A.out = d_out;
    A.n = (int32_t)n;
    A.per_wave = (int32_t)(blocks_per_wave * 64);
    A.refill = c->opt.rays_refill;
    HIP_TRY(c, hipEventRecord(c->ev0, stream));
    HIP_TRY(c, pt_launch_points(&P, &A, grid, g.lds_bytes, stream));
    HIP_TRY(c, hipEventRecord(c->ev1, stream));
    note_pass(c, (int)std::min<int64_t>(n, 0x7fffffff), 1, 1, grid, g, P.stack_entries, true);
    return PT_OK;
}

} // namespace

extern "C" {

int pt_closest_point_device(pt_ctx* c, const void* d_pts, int64_t n, void* d_out, void* stream_v)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = check_points_args(c, "pt_closest_point_device", d_pts, n, d_out, true))) return rc;
    if (n == 0) return PT_OK;
    return async_call_on(c, stream_v, [&](hipStream_t stream) { return points_device(c, d_pts, n, d_out, stream); });
}

// Host buffers: the points staged in d_rays_in, the records in d_rays_out, and back.
int pt_closest_point(pt_ctx* c, const pt_point* pts, int64_t n, pt_point_hit* out)
{
    if (!c) return PT_E_INVALID;
    int rc;
    if ((rc = check_points_args(c, "pt_closest_point", pts, n, out, false))) return rc;
    if (n == 0) return PT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t in_bytes = (size_t)n * sizeof(pt_point), out_bytes = (size_t)n * sizeof(pt_point_hit);
    return blocking_call(c, [&]() -> int {
        int rc2;
        if ((rc2 = ensure(c, c->d_rays_in, in_bytes)) || (rc2 = ensure(c, c->d_rays_out, out_bytes))) return rc2;
        HIP_TRY(c, hipMemcpyAsync(c->d_rays_in.p, pts, in_bytes, hipMemcpyHostToDevice, c->stream));
        if ((rc2 = points_device(c, c->d_rays_in.p, n, c->d_rays_out.p, c->stream))) return rc2;
        return drain(c, {{out, c->d_rays_out.p, out_bytes}});
    });
}

int64_t pt_debug_closest_point_host(pt_ctx* c, const pt_point* pts, int64_t n, pt_point_hit* out)
{
    if (!c) return PT_E_INVALID;
    const char* who = "pt_debug_closest_point_host";
    if (n < 0 || n >= ((int64_t)1 << 31)) return fail(c, PT_E_INVALID, "%s: n = %lld points (0 .. 2^31 - 1)", who, (long long)n);
    if (n > 0 && (!pts || !out)) return fail(c, PT_E_INVALID, "%s: NULL %s", who, !pts ? "pts" : "out");
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "%s: no geometries (pt_upload_scene not called)", who);
    sync_host_scene(c);
    const std::vector<PtTri>& tris = c->scene.bvh.tris; // leaf order; the slots that pad a leaf's start carry no triangle (id 0x7fffffff)
    pt_parallel_ranges((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const ptd::v3 x = ptd::V(pts[i].p[0], pts[i].p[1], pts[i].p[2]);
            const float rmax = ptd::point_rmax(pts[i].radius);
            ptd::PointBest b;
            ptd::point_reset(b, rmax * rmax);
            if (ptd::point_searches(rmax))
                for (const PtTri& t : tris)
                    if (t.id != ptd::kPointNoId)
                        ptd::point_tri(ptd::V(t.p0[0], t.p0[1], t.p0[2]), ptd::V(t.p1[0], t.p1[1], t.p1[2]), ptd::V(t.p2[0], t.p2[1], t.p2[2]), t.id, x, b);
            if (b.id != ptd::kPointNoId) out[i] = pt_point_hit{ptd::sqrt_(b.dd), b.u, b.v, b.id, {b.q.x, b.q.y, b.q.z}, b.feature};
            else out[i] = pt_point_hit{0.0f, 0.0f, 0.0f, -1, {0.0f, 0.0f, 0.0f}, 0};
        }
    });
    return n;
}

} // extern "C"
