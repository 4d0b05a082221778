// pt_denoise.hip -- pt_denoise: the guide-driven a-trous filter (Dammertz, Sewtz, Hanika, Lensch 2010) for low-sample frames, gfx950.
// The definition is in include/mi355pt.h ("denoiser").  Its per-pixel arithmetic is pt_filter_math.h, which the CPU twin
// pt_denoise_host.cpp compiles as well; the numpy restatement tests/denoise_ref.py states it independently, and the tests hold kernel,
// twin and restatement to each other bit for bit.  This unit keeps the pixel indexing, the batch frame offset, the accesses to the
// caller's 12-byte streams, geometry and launch.
//
// Three kernels, one pixel per lane, a wave = 64 consecutive pixels of one framebuffer row, a workgroup = 4 such rows (a 64 x 4 tile,
// pt_filter_tile.h):
//   prepare    rgb (12 B) + the guide pass's 32 B per pixel -> three 16-byte records per pixel in the context's work buffer:
//              colour + kz | normal + depth | albedo.  The guide records stay fixed, the colour record ping-pongs between two buffers.
//   iteration  step s = 1 << i as an argument: 25 taps x three 16-byte loads, every tap row of a wave one coalesced 1-KiB access, the
//              taps straight from the cache hierarchy (no LDS: see DESIGN.md 4, "denoiser", for what that choice rests on), one 16-byte
//              store.  The loop order (dy outer, dx inner) is the definition's: sum and wsum are sequential chains.
//   finish     colour record -> out_rgb (and out_rgba8), multiplied back by the albedo divisor with PT_DENOISE_DEMODULATE.
// The caller's rgb / out_rgb are 12 bytes per pixel with no alignment promise, so those two streams are dword accesses; every record of
// the work buffer and the guide input are 16-byte accesses.
//
// BATCH BUILD.  pt_denoise_batch.hip includes this file with PT_DENOISE_BATCH = 1: the same three kernels as pt_denoise_batch_{prepare,
// iter,finish}_kernel over K frames of one size (pt_denoise_batch), the frame in blockIdx.z.  A kernel first moves every record and
// caller pointer to its frame's own base (dn_frame); the pixel, the taps and their bounds test are then the single frame's, so no tap
// reads another frame.  With PT_DENOISE_BATCH = 0 the preprocessor removes all of it.
#include <hip/hip_runtime.h>

#include "../../include/mi355pt.h"
#include "pt_filter_math.h"
#include "pt_filter_tile.h"

using namespace ptd;

#ifndef PT_DENOISE_BATCH
#define PT_DENOISE_BATCH 0
#endif
#if PT_DENOISE_BATCH
#define pt_denoise_prepare_kernel pt_denoise_batch_prepare_kernel
#define pt_denoise_iter_kernel pt_denoise_batch_iter_kernel
#define pt_denoise_finish_kernel pt_denoise_batch_finish_kernel
#define pt_denoise_workspace_bytes pt_denoise_batch_workspace_bytes
#define pt_denoise_geometry pt_denoise_batch_geometry
#define pt_launch_denoise pt_launch_denoise_batch
#endif

namespace {

#if PT_DENOISE_BATCH
// Everything a kernel indexes by pixel, moved to frame blockIdx.z: the four record arrays are K frames long each, the caller's buffers
// are K frames back to back.  Returns the pixels a frame is apart (for the iteration kernel's src / dst).
__device__ __forceinline__ size_t dn_frame(PtDenoiseArgs& A)
{
    const size_t f = (size_t)blockIdx.z * ((size_t)A.width * (size_t)A.height);
    A.rgb += 3 * f;
    A.aov += 8 * f;
    A.out_rgb += 3 * f;
    if (A.out_rgba8) A.out_rgba8 += f;
    A.col[0] += f;
    A.col[1] += f;
    A.nz += f;
    A.alb += f;
    return f;
}
#endif

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_denoise_prepare_kernel(PtDenoiseArgs A)
{
    int x, row;
    if (!pt_filter_pixel(A.width, A.height, x, row)) return;
#if PT_DENOISE_BATCH
    dn_frame(A);
#endif
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const float4* g = (const float4*)A.aov + 2 * i;
    filter_prepare_pixel<kFilterDenoise>(A.rgb + 3 * i, nullptr, g[0], g[1], A.flags, A.sigma_depth, A.col[0][i], A.nz[i], A.alb[i]);
}

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_denoise_iter_kernel(PtDenoiseArgs A, const float4* __restrict__ src, float4* __restrict__ dst, int s, float kc)
{
    int x, row;
    if (!pt_filter_pixel(A.width, A.height, x, row)) return;
#if PT_DENOISE_BATCH
    const size_t frame_ofs = dn_frame(A);
    src += frame_ofs;
    dst += frame_ofs;
#endif
    filter_iter_pixel<false>(A, src, dst, x, row, s, kc);
}

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_denoise_finish_kernel(PtDenoiseArgs A, const float4* __restrict__ src)
{
    int x, row;
    if (!pt_filter_pixel(A.width, A.height, x, row)) return;
#if PT_DENOISE_BATCH
    src += dn_frame(A);
#endif
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const v3 o = filter_finish_pixel(src, A.alb, i, A.flags);
    float* y = A.out_rgb + 3 * i;
    y[0] = o.x; y[1] = o.y; y[2] = o.z;
    if (A.out_rgba8) A.out_rgba8[i] = make_rgba(o);
}

} // namespace

#if PT_DENOISE_BATCH
extern "C" size_t pt_denoise_workspace_bytes(int W, int H, int K) { return (size_t)K * (size_t)W * (size_t)H * 64; } // four 16-byte records per pixel of K frames
#else
extern "C" size_t pt_denoise_workspace_bytes(int W, int H) { return (size_t)W * (size_t)H * 64; } // four 16-byte records per pixel
#endif

// Geometry of the iteration kernel for a W x H frame (block, grid = workgroups, vgprs, lds_bytes = 0); hipErrorInvalidConfiguration if
// one of the three kernels needs scratch in this build.
#if PT_DENOISE_BATCH
extern "C" hipError_t pt_denoise_geometry(int W, int H, int K, PtGeometry* g, int* grid) // (K frames: grid = the workgroups of all of them)
{
#else
extern "C" hipError_t pt_denoise_geometry(int W, int H, PtGeometry* g, int* grid)
{
    const int K = 1;
#endif
    const hipError_t e = pt_refuse_scratch({(const void*)pt_denoise_finish_kernel, (const void*)pt_denoise_prepare_kernel});
    if (e != hipSuccess) return e;
    return pt_filter_geometry(W, H, K, g, grid, (const void*)pt_denoise_iter_kernel);
}

// prepare, a->iterations iteration launches, finish - all on `stream`.  a->ws: pt_denoise_workspace_bytes(), 16-byte aligned.
#if PT_DENOISE_BATCH
// (K frames, 1 <= K <= 65535: a->rgb, aov, out_rgb, out_rgba8 are those of the first; a->ws: pt_denoise_batch_workspace_bytes(W, H, K))
extern "C" hipError_t pt_launch_denoise(const PtDenoiseArgs* a, int K, hipStream_t stream)
{
    if (K < 1 || K > 65535) return hipErrorInvalidValue;
    PtDenoiseArgs A = *a;
    const size_t npx = (size_t)K * (size_t)A.width * (size_t)A.height;
#else
extern "C" hipError_t pt_launch_denoise(const PtDenoiseArgs* a, hipStream_t stream)
{
    const int K = 1;
    PtDenoiseArgs A = *a;
    const size_t npx = (size_t)A.width * (size_t)A.height;
#endif
    float4* ws = (float4*)A.ws;
    A.col[0] = ws;
    A.col[1] = ws + npx;
    A.nz = ws + 2 * npx;
    A.alb = ws + 3 * npx;
    const dim3 block = pt_filter_block(), grid = pt_filter_grid(A.width, A.height, K);
    hipLaunchKernelGGL(pt_denoise_prepare_kernel, grid, block, 0, stream, A);
    for (int i = 0; i < A.iterations; ++i)
        hipLaunchKernelGGL(pt_denoise_iter_kernel, grid, block, 0, stream, A, (const float4*)A.col[i & 1], A.col[(i + 1) & 1], 1 << i, A.kc[i]);
    hipLaunchKernelGGL(pt_denoise_finish_kernel, grid, block, 0, stream, A, (const float4*)A.col[A.iterations & 1]);
    return hipGetLastError();
}
