// pt_upsample.hip -- pt_upsample: joint bilateral upsampling (Kopf, Cohen, Lischinski, Uyttendaele 2007) of a low-resolution frame with
// full-resolution guides, gfx950.  The definition is in include/mi355pt.h ("upsampling"); the CPU twin pt_upsample_host.cpp and the numpy
// restatement tests/upsample_ref.py implement the same operation sequence, and the tests hold the three to each other bit for bit.
// Arithmetic: the contract of pt_device.h (binary32, -ffp-contract=off, fma only where spelled, correctly rounded division), with its
// exp_, dot, max_, abs_ and make_rgba.
//
// Two kernels, one pixel per lane, a wave = 64 consecutive pixels of one framebuffer row, a workgroup = 4 such rows (a 64 x 4 tile):
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
#include "pt_device.h"
#include "pt_instance.h"

using namespace ptd;

namespace {

constexpr int UP_TILE_W = 64, UP_TILE_H = 4; // a wave per row of the tile

__device__ __forceinline__ float up_finite_or_0(float v) { return (isinf_(v) || isnan_(v)) ? 0.0f : v; }
__device__ __forceinline__ float up_div(float a) { return max_(a, 1e-3f); } // the divisor of PT_UPSAMPLE_DEMODULATE

__global__ __launch_bounds__(UP_TILE_W * UP_TILE_H) void pt_upsample_prepare_kernel(PtUpsampleArgs A)
{
    const int x = (int)blockIdx.x * UP_TILE_W + (int)threadIdx.x, row = (int)blockIdx.y * UP_TILE_H + (int)threadIdx.y;
    if (x >= A.w || row >= A.h) return;
    const size_t i = (size_t)row * (size_t)A.w + (size_t)x;
    const float4* g = (const float4*)A.aov_lo + 2 * i;
    const float4 g0 = g[0], g1 = g[1]; // albedo r g b, alpha | normal x y z, depth
    const float* c = A.rgb_lo + 3 * i;
    const float r0 = up_finite_or_0(c[0]), r1 = up_finite_or_0(c[1]), r2 = up_finite_or_0(c[2]);
    A.nz[i] = g1;
    A.alb[i] = make_float4(g0.x, g0.y, g0.z, 0.0f);
    if (A.flags & PT_UPSAMPLE_DEMODULATE) A.col[i] = make_float4(r0 / up_div(g0.x), r1 / up_div(g0.y), r2 / up_div(g0.z), 0.0f);
    else A.col[i] = make_float4(r0, r1, r2, 0.0f);
}

__global__ __launch_bounds__(UP_TILE_W * UP_TILE_H) void pt_upsample_kernel(PtUpsampleArgs A)
{
    const int x = (int)blockIdx.x * UP_TILE_W + (int)threadIdx.x, row = (int)blockIdx.y * UP_TILE_H + (int)threadIdx.y;
    if (x >= A.W || row >= A.H) return;
    const int w = A.w, h = A.h;
    const float4* __restrict__ col = A.col;
    const float4* __restrict__ nzb = A.nz;
    const float4* __restrict__ alb = A.alb;
    const size_t p = (size_t)row * (size_t)A.W + (size_t)x;
    const float4* g = (const float4*)A.aov_hi + 2 * p;
    const float4 g0 = g[0], g1 = g[1];
    const v3 a_p = V(g0.x, g0.y, g0.z), n_p = V(g1.x, g1.y, g1.z);
    const float z_p = g1.w, kn = A.kn, ka = A.ka, ir = A.ir;
    const float sd = A.sigma_depth * max_(z_p, 1e-6f);
    const float kz = 1.0f / (sd * sd);
    const float fx = ((float)x + 0.5f) * A.rx - 0.5f, fy = ((float)row + 0.5f) * A.ry - 0.5f;
    const int x0 = (int)__builtin_floorf(fx), y0 = (int)__builtin_floorf(fy);
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const bool ring = A.taps == 4; // (uniform) taps = 2: j, i = 0 .. 1 only
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f, wsum = 0.0f, pw = 0.0f;
#pragma unroll
    for (int j = -1; j <= 2; ++j) {
        if (!ring && (j < 0 || j > 1)) continue;
        const int qy = y0 + j;
        if (qy < 0 || qy >= h) continue;
        const float by = 1.0f - abs_((float)j - ty) * ir;
#pragma unroll
        for (int i = -1; i <= 2; ++i) {
            if (!ring && (i < 0 || i > 1)) continue;
            const int qx = x0 + i;
            if (qx < 0 || qx >= w) continue;
            const float bx = 1.0f - abs_((float)i - tx) * ir;
            if (!(bx > 0.0f && by > 0.0f)) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            const float4 cq = col[q], nq = nzb[q], aq = alb[q];
            const float b = bx * by;
            px = fma_(b, cq.x, px);
            py = fma_(b, cq.y, py);
            pz = fma_(b, cq.z, pz);
            pw = pw + b;
            const v3 dn = V(nq.x, nq.y, nq.z) - n_p, da = V(aq.x, aq.y, aq.z) - a_p;
            const float en = dot(dn, dn), ea = dot(da, da);
            const float dz = nq.w - z_p;
            const float ez = dz * dz;
            const float e = fma_(ea, ka, fma_(ez, kz, en * kn));
            const float wt = b * exp_(-e);
            if (!(wt > 0.0f)) continue; // NaN and non-finite guides included
            sx = fma_(wt, cq.x, sx);
            sy = fma_(wt, cq.y, sy);
            sz = fma_(wt, cq.z, sz);
            wsum = wsum + wt;
        }
    }
    v3 o = (wsum >= 1e-4f * pw) ? V(sx / wsum, sy / wsum, sz / wsum) : V(px / pw, py / pw, pz / pw);
    if (A.flags & PT_UPSAMPLE_DEMODULATE) o = V(o.x * up_div(a_p.x), o.y * up_div(a_p.y), o.z * up_div(a_p.z));
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
    g->block = UP_TILE_W * UP_TILE_H;
    g->ns = UP_TILE_W * UP_TILE_H;
    g->lds_bytes = 0;
    g->lds_levels = 0;
    g->state_words = 0;
    *grid = ((W + UP_TILE_W - 1) / UP_TILE_W) * ((H + UP_TILE_H - 1) / UP_TILE_H);
    return pt_complete_geometry(g, (const void*)pt_upsample_kernel);
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
    const dim3 block(UP_TILE_W, UP_TILE_H);
    const dim3 grid_lo((A.w + UP_TILE_W - 1) / UP_TILE_W, (A.h + UP_TILE_H - 1) / UP_TILE_H), grid_hi((A.W + UP_TILE_W - 1) / UP_TILE_W, (A.H + UP_TILE_H - 1) / UP_TILE_H);
    hipLaunchKernelGGL(pt_upsample_prepare_kernel, grid_lo, block, 0, stream, A);
    hipLaunchKernelGGL(pt_upsample_kernel, grid_hi, block, 0, stream, A);
    return hipGetLastError();
}
