// pt_denoise_var.hip -- pt_denoise_var / pt_accum_denoise: the a-trous filter of pt_denoise.hip with the colour distance measured in units
// of the pixel's own estimated variance, and that variance filtered along with the colour (the spatial stage of SVGF: Schied et al.
// 2017), gfx950.  The definition is in include/mi355pt.h ("variance-guided denoise"); the CPU twins (pt_debug_denoise_var_host in
// pt_denoise_host.cpp, pt_debug_accum_variance_host in pt_accum_host.cpp) and the numpy restatement tests/denoise_var_ref.py implement the
// same operation sequence, and the tests hold the three to each other bit for bit.  Arithmetic: the contract of pt_device.h.
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
#include "pt_accum_math.h"
#include "pt_instance.h"

using namespace ptd;

namespace {

constexpr int DV_TILE_W = 64, DV_TILE_H = 4; // a wave per row of the tile
constexpr int DV_VAR_BLOCK = 256;

__device__ __forceinline__ bool dv_pixel(const PtDenoiseVarArgs& A, int& x, int& row)
{
    x = (int)blockIdx.x * DV_TILE_W + (int)threadIdx.x;
    row = (int)blockIdx.y * DV_TILE_H + (int)threadIdx.y;
    return x < A.width && row < A.height;
}

__device__ __forceinline__ float dv_finite_or_0(float v) { return (isinf_(v) || isnan_(v)) ? 0.0f : v; }
__device__ __forceinline__ float dv_div(float a) { return max_(a, 1e-3f); } // d_k of PT_DENOISE_DEMODULATE

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

__global__ __launch_bounds__(DV_TILE_W * DV_TILE_H) void pt_denoise_var_prepare_kernel(PtDenoiseVarArgs A)
{
    int x, row;
    if (!dv_pixel(A, x, row)) return;
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const float4* g = (const float4*)A.aov + 2 * i;
    const float4 g0 = g[0], g1 = g[1]; // albedo r g b, alpha | normal x y z, depth
    const float* c = A.rgb + 3 * i;
    const float* vr = A.var + 3 * i;
    const float r0 = dv_finite_or_0(c[0]), r1 = dv_finite_or_0(c[1]), r2 = dv_finite_or_0(c[2]);
    float v0 = vr[0], v1 = vr[1], v2 = vr[2];
    const float sd = A.sigma_depth * max_(g1.w, 1e-6f);
    const float kz = 1.0f / (sd * sd);
    A.nz[i] = g1;
    A.alb[i] = make_float4(g0.x, g0.y, g0.z, kz);
    float c0 = r0, c1 = r1, c2 = r2;
    if (A.flags & PT_DENOISE_DEMODULATE) {
        const float d0 = dv_div(g0.x), d1 = dv_div(g0.y), d2 = dv_div(g0.z);
        c0 = r0 / d0; c1 = r1 / d1; c2 = r2 / d2;
        v0 = v0 / (d0 * d0); v1 = v1 / (d1 * d1); v2 = v2 / (d2 * d2);
    }
    const float v = (v0 + v1) + v2;
    A.col[0][i] = make_float4(c0, c1, c2, (v >= 0.0f && v <= kVarMax) ? v : kVarMax);
}

__global__ __launch_bounds__(DV_TILE_W * DV_TILE_H) void pt_denoise_var_iter_kernel(PtDenoiseVarArgs A, const float4* __restrict__ src, float4* __restrict__ dst, int s)
{
    int x, row;
    if (!dv_pixel(A, x, row)) return;
    const int W = A.width, H = A.height;
    const float4* __restrict__ nzb = A.nz;
    const float4* __restrict__ alb = A.alb;
    const size_t i = (size_t)row * (size_t)W + (size_t)x;
    const float4 cp = src[i], np = nzb[i], ap = alb[i];
    const v3 c_p = V(cp.x, cp.y, cp.z), n_p = V(np.x, np.y, np.z), a_p = V(ap.x, ap.y, ap.z);
    const float kz = ap.w, kn = A.kn, ka = A.ka;
    // the variance around the pixel: 3 x 3 binomial mean over the direct neighbours
    const float m[2] = {0.5f, 0.25f};
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = row + dy;
        if (qy < 0 || qy >= H) continue; // (uniform over the wave)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const float g = m[dx < 0 ? -dx : dx] * m[dy < 0 ? -dy : dy];
            const float vq = (dx == 0 && dy == 0) ? cp.w : src[(size_t)qy * (size_t)W + (size_t)qx].w;
            gs = fma_(g, vq, gs);
            gw = gw + g;
        }
    }
    const float vb = gs / gw;
    const float kc = (A.s2 == __builtin_inff()) ? 0.0f : 1.0f / fma_(A.s2, vb, 1e-10f);
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f, vsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = row + dy * s;
        if (qy < 0 || qy >= H) continue; // (uniform over the wave)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W) continue;
            const float h = k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
            float w;
            float4 cq;
            if (dx == 0 && dy == 0) {
                w = h;
                cq = cp;
            } else {
                const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                cq = src[q];
                const float4 nq = nzb[q], aq = alb[q];
                const v3 dc = V(cq.x, cq.y, cq.z) - c_p, dn = V(nq.x, nq.y, nq.z) - n_p, da = V(aq.x, aq.y, aq.z) - a_p;
                const float ec = dot(dc, dc), en = dot(dn, dn), ea = dot(da, da);
                const float dz = nq.w - np.w;
                const float ez = dz * dz;
                const float e = fma_(ea, ka, fma_(ez, kz, fma_(en, kn, ec * kc)));
                w = h * exp_(-e);
                if (!(w > 0.0f)) continue; // NaN and non-finite guides included
            }
            sx = fma_(w, cq.x, sx);
            sy = fma_(w, cq.y, sy);
            sz = fma_(w, cq.z, sz);
            vsum = fma_(w * w, cq.w, vsum);
            wsum = wsum + w;
        }
    }
    dst[i] = make_float4(sx / wsum, sy / wsum, sz / wsum, min_(vsum / (wsum * wsum), kVarMax));
}

__global__ __launch_bounds__(DV_TILE_W * DV_TILE_H) void pt_denoise_var_finish_kernel(PtDenoiseVarArgs A, const float4* __restrict__ src)
{
    int x, row;
    if (!dv_pixel(A, x, row)) return;
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const float4 c = src[i];
    v3 o = V(c.x, c.y, c.z);
    if (A.flags & PT_DENOISE_DEMODULATE) {
        const float4 a = A.alb[i];
        o = V(o.x * dv_div(a.x), o.y * dv_div(a.y), o.z * dv_div(a.z));
    }
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
    g->block = DV_TILE_W * DV_TILE_H;
    g->ns = DV_TILE_W * DV_TILE_H;
    g->lds_bytes = 0;
    g->lds_levels = 0;
    g->state_words = 0;
    *grid = ((W + DV_TILE_W - 1) / DV_TILE_W) * ((H + DV_TILE_H - 1) / DV_TILE_H);
    return pt_complete_geometry(g, (const void*)pt_denoise_var_iter_kernel);
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
    const dim3 block(DV_TILE_W, DV_TILE_H), grid((A.width + DV_TILE_W - 1) / DV_TILE_W, (A.height + DV_TILE_H - 1) / DV_TILE_H);
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
