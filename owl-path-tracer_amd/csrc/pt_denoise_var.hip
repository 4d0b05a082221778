// pt_denoise_var.hip -- pt_denoise_var / pt_accum_denoise: the a-trous filter of pt_denoise.hip with the colour distance measured in units
// of the pixel's own estimated variance, and that variance filtered along with the colour (the spatial stage of SVGF: Schied et al.
// 2017), gfx950.  The definition is in include/mi355pt.h ("variance-guided denoise").  Its per-pixel arithmetic is pt_filter_math.h and
// pt_accum_math.h, which the CPU twins (pt_debug_denoise_var_host in pt_denoise_host.cpp, pt_debug_accum_variance_host in
// pt_accum_host.cpp) compile as well; the numpy restatement tests/denoise_var_ref.py states it independently, and the tests hold the
// three to each other bit for bit.  This unit keeps the pixel indexing, the accesses to the caller's 12-byte streams, geometry and launch.
//
// Four kernels.  The three of the filter have the shape of pt_denoise.hip - one pixel per lane, a wave = 64 consecutive pixels of one
// framebuffer row, a workgroup = a 64 x 4 tile, 16-byte records in the context's work buffer, the taps straight from the cache hierarchy:
//   variance   over an accumulation's state in launch order (id = x + W * y, as pt_accum_resolve_kernel): sum, half, n, n_half -> the
//              per-channel variance of the pixel's value in framebuffer order (pt_accum_math.h, accum_variance_pixel); dword streams.
//   prepare    rgb + var (12 B each) + the guide pass's 32 B per pixel -> three 16-byte records: colour + v | normal + depth | albedo + kz.
//              v is the sum of the three channels' variances, kVarMax where it is unknown.  The colour record ping-pongs.
//   iteration  the 25 taps of pt_denoise_iter_kernel with a per-pixel colour constant kc_p = 1 / (s2 * vb + 1e-10), vb the 3 x 3 binomial
//              mean of v around the pixel (eight more dword loads from the colour records, at distance 1 whatever the step), and a second
//              sum, of w^2 v, that becomes the next v.
//   finish     as pt_denoise_finish_kernel.
#include <hip/hip_runtime.h>

#include "../../include/mi355pt.h"
#include "pt_filter_math.h" // (and pt_accum_math.h)
#include "pt_filter_tile.h"

using namespace ptd;

namespace {

constexpr int DV_VAR_BLOCK = 256;

__global__ __launch_bounds__(DV_VAR_BLOCK) void pt_accum_variance_kernel(PtAccumVarArgs A)
{
    const uint32_t id = blockIdx.x * (uint32_t)DV_VAR_BLOCK + threadIdx.x;
    if (id >= A.n_frame) return;
    const uint32_t x = id % (uint32_t)A.width, y = id / (uint32_t)A.width;
    const size_t ofs = (size_t)x + (size_t)A.width * (size_t)((uint32_t)A.height - 1u - y); // framebuffer order, as resolve
    float rgb[3], var[3] = {0.0f, 0.0f, 0.0f}; // +0 for a pixel of another shard
    if (A.owned[id]) {
        float sum[3], half[3];
        for (int k = 0; k < 3; ++k) {
            sum[k] = A.sum[3 * (size_t)id + k];
            half[k] = A.half[3 * (size_t)id + k];
        }
        accum_variance_pixel(sum, half, A.n[id], A.n_half[id], rgb, var); // (the colour is resolve's image already)
    }
    A.out_var[3 * ofs] = var[0];
    A.out_var[3 * ofs + 1] = var[1];
    A.out_var[3 * ofs + 2] = var[2];
}

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_denoise_var_prepare_kernel(PtDenoiseVarArgs A)
{
    int x, row;
    if (!pt_filter_pixel(A.width, A.height, x, row)) return;
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const float4* g = (const float4*)A.aov + 2 * i;
    filter_prepare_pixel<kFilterDenoiseVar>(A.rgb + 3 * i, A.var + 3 * i, g[0], g[1], A.flags, A.sigma_depth, A.col[0][i], A.nz[i], A.alb[i]);
}

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_denoise_var_iter_kernel(PtDenoiseVarArgs A, const float4* __restrict__ src, float4* __restrict__ dst, int s)
{
    int x, row;
    if (!pt_filter_pixel(A.width, A.height, x, row)) return;
    filter_iter_pixel<true>(A, src, dst, x, row, s, A.s2);
}

__global__ __launch_bounds__(PT_FILTER_BLOCK) void pt_denoise_var_finish_kernel(PtDenoiseVarArgs A, const float4* __restrict__ src)
{
    int x, row;
    if (!pt_filter_pixel(A.width, A.height, x, row)) return;
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const v3 o = filter_finish_pixel(src, A.alb, i, A.flags);
    float* y = A.out_rgb + 3 * i;
    y[0] = o.x; y[1] = o.y; y[2] = o.z;
    if (A.out_rgba8) A.out_rgba8[i] = make_rgba(o);
}

} // namespace

extern "C" size_t pt_denoise_var_workspace_bytes(int W, int H) { return (size_t)W * (size_t)H * 64; } // four 16-byte records per pixel

// Geometry of the iteration kernel for a W x H frame (block, grid = workgroups, vgprs, lds_bytes = 0); hipErrorInvalidConfiguration if
// one of the four kernels needs scratch in this build.
extern "C" hipError_t pt_denoise_var_geometry(int W, int H, PtGeometry* g, int* grid)
{
    const hipError_t e = pt_refuse_scratch({(const void*)pt_accum_variance_kernel, (const void*)pt_denoise_var_finish_kernel, (const void*)pt_denoise_var_prepare_kernel});
    if (e != hipSuccess) return e;
    return pt_filter_geometry(W, H, 1, g, grid, (const void*)pt_denoise_var_iter_kernel);
}

// prepare, a->iterations iteration launches, finish - all on `stream`.  a->ws: pt_denoise_var_workspace_bytes(), 16-byte aligned.
extern "C" hipError_t pt_launch_denoise_var(const PtDenoiseVarArgs* a, hipStream_t stream)
{
    PtDenoiseVarArgs A = *a;
    const size_t npx = (size_t)A.width * (size_t)A.height;
    float4* ws = (float4*)A.ws;
    A.col[0] = ws;
    A.col[1] = ws + npx;
    A.nz = ws + 2 * npx;
    A.alb = ws + 3 * npx;
    const dim3 block = pt_filter_block(), grid = pt_filter_grid(A.width, A.height);
    hipLaunchKernelGGL(pt_denoise_var_prepare_kernel, grid, block, 0, stream, A);
    for (int i = 0; i < A.iterations; ++i)
        hipLaunchKernelGGL(pt_denoise_var_iter_kernel, grid, block, 0, stream, A, (const float4*)A.col[i & 1], A.col[(i + 1) & 1], 1 << i);
    hipLaunchKernelGGL(pt_denoise_var_finish_kernel, grid, block, 0, stream, A, (const float4*)A.col[A.iterations & 1]);
    return hipGetLastError();
}

extern "C" hipError_t pt_launch_accum_variance(const PtAccumVarArgs* a, hipStream_t stream)
{
    if (a->n_frame == 0) return hipSuccess;
    hipLaunchKernelGGL(pt_accum_variance_kernel, dim3((a->n_frame + DV_VAR_BLOCK - 1) / DV_VAR_BLOCK), dim3(DV_VAR_BLOCK), 0, stream, *a);
    return hipGetLastError();
}
