// pt_accum_reproject.hip -- pt_accum_reproject's one kernel (include/mi355pt.h, "reprojection"), gfx950: the accumulation's state follows
// the surfaces to a new camera.  The per-pixel definition is pt_accum_math.h (accum_reproject_source, accum_reproject_history and resolve's
// accum_resolve_pixel), which the CPU twin pt_debug_accum_reproject_host compiles as well; tests/accum_reproject_ref.py restates it in
// numpy.  Arithmetic: the contract of pt_device.h (binary32, -ffp-contract=off, correctly rounded division and square root).
//
// A gather, one pixel of the NEW frame per lane in launch order (id = x + W * y, a wave on 64 consecutive pixels of a row), no LDS, no
// atomics, no scratch.  Per owned pixel: its guide record and the source's as two 16-byte loads each, the owned flag of the source, and the
// source's sum / half / n / n_half / passes as dword gathers from the state BEFORE the call - neighbouring lanes have neighbouring sources
// under any camera move, so the gathers mostly coalesce.  Written by id into the OTHER set of state buffers (the host swaps the sets):
// no lane reads what another writes.  seen, noise and the image belong to the pixel alone and are rewritten in place: about 102 B read and
// 68 B written per owned pixel.  rng is neither read nor written.
#include <hip/hip_runtime.h>

#include "../../include/mi355pt.h"
#include "pt_accum_math.h"
#include "pt_instance.h"

using namespace ptd;

namespace {

constexpr int REPROJECT_BLOCK = 256; // four waves

__global__ __launch_bounds__(REPROJECT_BLOCK) void pt_accum_reproject_kernel(PtAccumReprojectArgs A)
{
    const uint32_t id = blockIdx.x * (uint32_t)REPROJECT_BLOCK + threadIdx.x;
    if (id >= A.n_frame) return;
    if (!A.owned[id]) return; // +0 in both sets of state and in every output since pt_accum_begin; nothing writes there
    const uint32_t x = id % (uint32_t)A.R.width, y = id / (uint32_t)A.R.width;
    AccumPixel s;
    for (int k = 0; k < 3; ++k) s.sum[k] = s.half[k] = 0.0f;
    s.n = s.n_half = s.passes = 0u;
    uint32_t q = 0;
    if (accum_reproject_source(A.R, (int)x, (int)y, A.aov_prev, A.aov_cur, A.owned, &q)) {
        for (int k = 0; k < 3; ++k) {
            s.sum[k] = A.sum_in[3 * (size_t)q + k];
            s.half[k] = A.half_in[3 * (size_t)q + k];
        }
        s.n = A.n_in[q];
        s.n_half = A.n_half_in[q];
        s.passes = A.passes_in[q];
        accum_reproject_history(s, (uint32_t)A.R.max_history);
    }
    for (int k = 0; k < 3; ++k) s.seen[k] = s.sum[k];
    AccumResolved o;
    accum_resolve_pixel(s, false, 0u, o);
    for (int k = 0; k < 3; ++k) {
        A.sum_out[3 * (size_t)id + k] = s.sum[k];
        A.seen[3 * (size_t)id + k] = s.seen[k];
        A.half_out[3 * (size_t)id + k] = s.half[k];
    }
    A.n_out[id] = s.n;
    A.n_half_out[id] = s.n_half;
    A.passes_out[id] = s.passes;
    A.noise[id] = o.noise;
    const size_t ofs = (size_t)x + (size_t)A.R.width * (size_t)((uint32_t)A.R.height - 1u - y); // device.cu:251
    A.out_rgb[3 * ofs] = o.rgb[0];
    A.out_rgb[3 * ofs + 1] = o.rgb[1];
    A.out_rgb[3 * ofs + 2] = o.rgb[2];
    A.out_rgba8[ofs] = o.rgba8;
}

} // namespace

extern "C" hipError_t pt_accum_reproject_geometry(int W, int H, PtGeometry* g, int* grid)
{
    g->block = REPROJECT_BLOCK;
    g->ns = REPROJECT_BLOCK;
    g->lds_bytes = 0;
    g->lds_levels = 0;
    g->state_words = 0;
    *grid = (int)(((size_t)W * (size_t)H + REPROJECT_BLOCK - 1) / REPROJECT_BLOCK);
    return pt_complete_geometry(g, (const void*)pt_accum_reproject_kernel);
}

extern "C" hipError_t pt_launch_accum_reproject(const PtAccumReprojectArgs* a, hipStream_t stream)
{
    if (a->n_frame == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_accum_reproject_kernel, dim3((a->n_frame + REPROJECT_BLOCK - 1) / REPROJECT_BLOCK), dim3(REPROJECT_BLOCK), 0, stream, *a);
    return hipGetLastError();
}
