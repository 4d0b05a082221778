// pt_upsample.hip -- pt_upsample: joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele 2007) of a low-resolution frame with
// full-resolution guides, gfx950.  The definition is in include/mi355pt.h ("upsampling").  Its per-pixel arithmetic is pt_filter_math.h
// (filter_prepare_pixel, upsample_pixel), which the CPU twin pt_upsample_host.cpp compiles as well; the numpy restatement
// tests/upsample_ref.py states it independently, and the tests hold the three to each other bit for bit.  This unit keeps the pixel
// indexing, the guide loads, the stores to the caller's 12-byte stream, geometry and launch.
//
// Two kernels, one pixel per lane, a wave = 64 consecutive pixels of one framebuffer row, a workgroup = 4 such rows (a 64 x 4 tile,
// pt_filter_tile.h):
//   prepare    over the LOW frame: rgb (12 B) + the guide pass's 32 B per pixel -> three 16-byte records per low pixel in the context's
//              work buffer, in the layout of pt_denoise.hip's prepare: colour | normal + depth | albedo.  The three divisions of
//              PT_UPSAMPLE_DEMODULATE are done here once per low pixel, not once per tap.
//   upsample   over the HIGH frame: two float4 loads of the pixel's own guide record, then the taps x taps window fully unrolled in the
//              definition's order (j outer, i inner: the four sums are sequential chains, so the order is the result).  Each tap is three
//              16-byte loads; a wave's tap row covers about 64 * rx + 1 consecutive low pixels, so they coalesce, and the low records are
//              re-read by every high pixel above them from the cache hierarchy (no LDS, no atomics, no scratch).  The loop is written for
//              taps = 4 (j, i = -1 .. 2); taps = 2 leaves the outer ring with a wave-uniform test, which is the definition's loop
//              j, i = 0 .. 1.  out_rgb has no alignment promise: dword stores, and one dword to out_rgba8.
#include <hip/hip_runtime.h>

#include "../../include/mi355pt.h"
#include "pt_filter_math.h"
#include "pt_filter_tile.h"

using namespace ptd;

namespace {

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_upsample_prepare_kernel(PtUpsampleArgs A)
{
    int x, row;
    if (!pt_filter_pixel(A.w, A.h, x, row)) return;
    const size_t i = (size_t)row * (size_t)A.w + (size_t)x;
    const float4* g = (const float4*)A.aov_lo + 2 * i;
    filter_prepare_pixel<kFilterUpsample>(A.rgb_lo + 3 * i, nullptr, g[0], g[1], A.flags, A.sigma_depth, A.col[i], A.nz[i], A.alb[i]);
}

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_upsample_kernel(PtUpsampleArgs A)
{
    int x, row;
    if (!pt_filter_pixel(A.W, A.H, x, row)) return;
    const size_t p = (size_t)row * (size_t)A.W + (size_t)x;
    const float4* g = (const float4*)A.aov_hi + 2 * p;
    const v3 o = upsample_pixel(A, g[0], g[1], x, row);
    float* y = A.out_rgb + 3 * p;
    y[0] = o.x; y[1] = o.y; y[2] = o.z;
    if (A.out_rgba8) A.out_rgba8[p] = make_rgba(o);
}

} // namespace

extern "C" size_t pt_upsample_workspace_bytes(int w, int h) { return (size_t)w * (size_t)h * 48; } // three 16-byte records per low pixel

// Geometry of the upsample kernel for a W x H frame (block, grid = workgroups, vgprs, lds_bytes = 0); hipErrorInvalidConfiguration if
// one of the two kernels needs scratch in this build.
extern "C" hipError_t pt_upsample_geometry(int W, int H, PtGeometry* g, int* grid)
{
    const hipError_t e = pt_refuse_scratch({(const void*)pt_upsample_prepare_kernel});
    if (e != hipSuccess) return e;
    return pt_filter_geometry(W, H, 1, g, grid, (const void*)pt_upsample_kernel);
}

// prepare over the low frame, upsample over the high frame - both on `stream`.  a->ws: pt_upsample_workspace_bytes(), 16-byte aligned.
extern "C" hipError_t pt_launch_upsample(const PtUpsampleArgs* a, hipStream_t stream)
{
    PtUpsampleArgs A = *a;
    const size_t npx = (size_t)A.w * (size_t)A.h;
    float4* ws = (float4*)A.ws;
    A.col = ws;
    A.nz = ws + npx;
    A.alb = ws + 2 * npx;
    const dim3 block = pt_filter_block(), grid_lo = pt_filter_grid(A.w, A.h), grid_hi = pt_filter_grid(A.W, A.H);
    hipLaunchKernelGGL(pt_upsample_prepare_kernel, grid_lo, block, 0, stream, A);
    hipLaunchKernelGGL(pt_upsample_kernel, grid_hi, block, 0, stream, A);
    return hipGetLastError();
}
