// pt_denoise.hip -- pt_denoise: the guide-driven a-trous filter (Dammertz, Sewtz, Hanika, Lensch 2010) for low-sample frames, gfx950.
// The definition is in include/mi355pt.h ("denoiser"); the CPU twin pt_denoise_host.cpp and the numpy restatement tests/denoise_ref.py
// implement the same operation sequence, and the tests hold the three to each other bit for bit.  Arithmetic: the contract of
// pt_device.h (binary32, -ffp-contract=off, fma only where spelled, correctly rounded division), with its exp_, dot, max_ and make_rgba.
//
// Three kernels, one pixel per lane, a wave = 64 consecutive pixels of one framebuffer row, a workgroup = 4 such rows (a 64 x 4 tile):
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
#include "pt_device.h"
#include "pt_instance.h"

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

constexpr int DN_TILE_W = 64, DN_TILE_H = 4; // a wave per row of the tile

__device__ __forceinline__ bool dn_pixel(const PtDenoiseArgs& A, int& x, int& row)
{
    x = (int)blockIdx.x * DN_TILE_W + (int)threadIdx.x;
    row = (int)blockIdx.y * DN_TILE_H + (int)threadIdx.y;
    return x < A.width && row < A.height;
}

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

__device__ __forceinline__ float dn_finite_or_0(float v) { return (isinf_(v) || isnan_(v)) ? 0.0f : v; }
__device__ __forceinline__ float dn_div(float a) { return max_(a, 1e-3f); } // d_k of PT_DENOISE_DEMODULATE

__global__ __launch_bounds__(DN_TILE_W * DN_TILE_H) void pt_denoise_prepare_kernel(PtDenoiseArgs A)
{
    int x, row;
    if (!dn_pixel(A, x, row)) return;
#if PT_DENOISE_BATCH
    dn_frame(A);
#endif
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const float4* g = (const float4*)A.aov + 2 * i;
    const float4 g0 = g[0], g1 = g[1]; // albedo r g b, alpha | normal x y z, depth
    const float* c = A.rgb + 3 * i;
    const float r0 = dn_finite_or_0(c[0]), r1 = dn_finite_or_0(c[1]), r2 = dn_finite_or_0(c[2]);
    A.nz[i] = g1;
    A.alb[i] = make_float4(g0.x, g0.y, g0.z, 0.0f);
    const float sd = A.sigma_depth * max_(g1.w, 1e-6f);
    const float kz = 1.0f / (sd * sd);
    if (A.flags & PT_DENOISE_DEMODULATE) A.col[0][i] = make_float4(r0 / dn_div(g0.x), r1 / dn_div(g0.y), r2 / dn_div(g0.z), kz);
    else A.col[0][i] = make_float4(r0, r1, r2, kz);
}

__global__ __launch_bounds__(DN_TILE_W * DN_TILE_H) void pt_denoise_iter_kernel(PtDenoiseArgs A, const float4* __restrict__ src, float4* __restrict__ dst, int s, float kc)
{
    int x, row;
    if (!dn_pixel(A, x, row)) return;
#if PT_DENOISE_BATCH
    const size_t frame_ofs = dn_frame(A);
    src += frame_ofs;
    dst += frame_ofs;
#endif
    const int W = A.width, H = A.height;
    const float4* __restrict__ nzb = A.nz;
    const float4* __restrict__ alb = A.alb;
    const size_t i = (size_t)row * (size_t)W + (size_t)x;
    const float4 cp = src[i], np = nzb[i], ap = alb[i];
    const v3 c_p = V(cp.x, cp.y, cp.z), n_p = V(np.x, np.y, np.z), a_p = V(ap.x, ap.y, ap.z);
    const float kz = cp.w, kn = A.kn, ka = A.ka;
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
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
            wsum = wsum + w;
        }
    }
    dst[i] = make_float4(sx / wsum, sy / wsum, sz / wsum, kz);
}

__global__ __launch_bounds__(DN_TILE_W * DN_TILE_H) void pt_denoise_finish_kernel(PtDenoiseArgs A, const float4* __restrict__ src)
{
    int x, row;
    if (!dn_pixel(A, x, row)) return;
#if PT_DENOISE_BATCH
    src += dn_frame(A);
#endif
    const size_t i = (size_t)row * (size_t)A.width + (size_t)x;
    const float4 c = src[i];
    v3 o = V(c.x, c.y, c.z);
    if (A.flags & PT_DENOISE_DEMODULATE) {
        const float4 a = A.alb[i];
        o = V(o.x * dn_div(a.x), o.y * dn_div(a.y), o.z * dn_div(a.z));
    }
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
#else
extern "C" hipError_t pt_denoise_geometry(int W, int H, PtGeometry* g, int* grid)
#endif
{
    const hipError_t e = pt_refuse_scratch({(const void*)pt_denoise_finish_kernel, (const void*)pt_denoise_prepare_kernel});
    if (e != hipSuccess) return e;
    g->block = DN_TILE_W * DN_TILE_H;
    g->ns = DN_TILE_W * DN_TILE_H;
    g->lds_bytes = 0;
    g->lds_levels = 0;
    g->state_words = 0;
    *grid = ((W + DN_TILE_W - 1) / DN_TILE_W) * ((H + DN_TILE_H - 1) / DN_TILE_H);
#if PT_DENOISE_BATCH
    *grid *= K;
#endif
    return pt_complete_geometry(g, (const void*)pt_denoise_iter_kernel);
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
    PtDenoiseArgs A = *a;
    const size_t npx = (size_t)A.width * (size_t)A.height;
#endif
    float4* ws = (float4*)A.ws;
    A.col[0] = ws;
    A.col[1] = ws + npx;
    A.nz = ws + 2 * npx;
    A.alb = ws + 3 * npx;
#if PT_DENOISE_BATCH
    const dim3 block(DN_TILE_W, DN_TILE_H), grid((A.width + DN_TILE_W - 1) / DN_TILE_W, (A.height + DN_TILE_H - 1) / DN_TILE_H, K);
#else
    const dim3 block(DN_TILE_W, DN_TILE_H), grid((A.width + DN_TILE_W - 1) / DN_TILE_W, (A.height + DN_TILE_H - 1) / DN_TILE_H);
#endif
    hipLaunchKernelGGL(pt_denoise_prepare_kernel, grid, block, 0, stream, A);
    for (int i = 0; i < A.iterations; ++i)
        hipLaunchKernelGGL(pt_denoise_iter_kernel, grid, block, 0, stream, A, (const float4*)A.col[i & 1], A.col[(i + 1) & 1], 1 << i, A.kc[i]);
    hipLaunchKernelGGL(pt_denoise_finish_kernel, grid, block, 0, stream, A, (const float4*)A.col[A.iterations & 1]);
    return hipGetLastError();
}
