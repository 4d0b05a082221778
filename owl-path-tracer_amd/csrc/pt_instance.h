// pt_instance.h -- what a *_geometry function asks the runtime about a kernel instance, for every .hip unit alike (host-side inline only).
// A kernel that spills registers to scratch is refused, not run: such builds of the render kernel rendered wrong pixels
// (pt_render_wave_kernel, pt_kernel.hip), and every family since is held to the same rule.  The launchers have C linkage and link
// whatever their bodies say, so the rule is spelled once; a family names its kernels and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "pt_launch.h"

// hipErrorInvalidConfiguration if one of the kernels needs scratch in this build.  For a family of several kernels: the ones beside the
// kernel whose geometry it reports - that one goes to pt_complete_geometry, which holds it to the same rule.
inline hipError_t pt_refuse_scratch(std::initializer_list<const void*> fns)
{
    for (const void* fn : fns) {
        hipFuncAttributes fa;
        const hipError_t e = hipFuncGetAttributes(&fa, fn);
        if (e != hipSuccess) return e;
        if (fa.localSizeBytes != 0) return hipErrorInvalidConfiguration;
    }
    return hipSuccess;
}

// Completes *g, whose block and lds_bytes are set, from the instance fn: registers, and the occupancy at that block and LDS size.
// allow_scratch: the instance may spill (the lane-per-pixel kernel, which was never held to the rule, and pt_kernel.hip's PT_ALLOW_SCRATCH).
inline hipError_t pt_complete_geometry(PtGeometry* g, const void* fn, bool allow_scratch = false)
{
    hipFuncAttributes fa;
    const hipError_t e = hipFuncGetAttributes(&fa, fn);
    if (e != hipSuccess) return e;
    if (fa.localSizeBytes != 0 && !allow_scratch) return hipErrorInvalidConfiguration;
    g->vgprs = fa.numRegs;
    g->max_blocks_per_cu = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&g->max_blocks_per_cu, fn, g->block, g->lds_bytes);
}

// The geometry of the one-wave-per-workgroup kernels (guide kernels, ray queries, ambient occlusion): 64 threads, a pixel or ray per lane,
// and in LDS the lds_levels lowest levels of the lanes' stacks, then park_words words per lane of parked state (the follow kernels').
inline hipError_t pt_wave_geometry(PtGeometry* g, int lds_levels, int park_words, const void* fn)
{
    g->block = 64;
    g->ns = 64;
    g->lds_levels = lds_levels;
    g->lds_bytes = (size_t)(lds_levels + park_words) * 64 * 4;
    g->state_words = 0;
    return pt_complete_geometry(g, fn);
}

// What the kernels that walk ray ranges (pt_ray_range.h) rely on: workgroup b of `grid` owns rays [b * per_wave, + per_wave) of a.n.
inline bool pt_ray_ranges_ok(int grid, const PtRaysArgs& a)
{
    if (grid < 1 || a.n < 1 || a.per_wave < 64 || (a.per_wave % 64) != 0 || a.refill < 0 || a.refill >= 64) return false;
    if ((long long)grid * a.per_wave < (long long)a.n) return false;    // the ranges cover every ray ...
    return (long long)(grid - 1) * a.per_wave < (long long)a.n;         // ... and none is empty
}
