// pt_filter_math.h -- the per-pixel definitions of the three guide-driven filters (include/mi355pt.h: "denoiser", "variance-guided
// denoise", "upsampling"), ONE copy for the kernels of pt_denoise.hip (and so pt_denoise_batch.hip), pt_denoise_var.hip and
// pt_upsample.hip and for their CPU twins in pt_denoise_host.cpp and pt_upsample_host.cpp (which include pt_device_host.h first).  The
// numpy restatements tests/denoise_ref.py, denoise_var_ref.py and upsample_ref.py are the independent statement the tests hold this to,
// bit for bit.  Arithmetic: the contract of pt_device.h - binary32, no contraction, fma only where spelled, correctly rounded division,
// its exp_, dot, max_, min_ and abs_.
// Every per-pixel record is 16 bytes and goes through float4 on both sides: colour r g b + one word | normal x y z + depth | albedo
// r g b + one word.  What the spare words carry is the filter's (FilterKind).  The record pointers are the kernels' own: a kernel passes
// its __restrict__ parameters and its argument struct on, and every record access is one 16-byte load.
#pragma once
#include "../../include/mi355pt.h" // PT_DENOISE_DEMODULATE, PT_UPSAMPLE_DEMODULATE
#include "pt_device.h"
#include "pt_accum_math.h" // kVarMax
#include "pt_launch.h"     // PtUpsampleArgs

namespace ptd {

// ---- the scalars the three filters share -------------------------------------------------------------------------------------------
PTD float filter_finite_or_0(float v) { return (isinf_(v) || isnan_(v)) ? 0.0f : v; }
PTD float filter_divisor(float a) { return max_(a, 1e-3f); } // d_k of PT_DENOISE_DEMODULATE / PT_UPSAMPLE_DEMODULATE
PTD float filter_kz(float sigma_depth, float depth)          // the depth term's constant at a pixel of this depth
{
    const float sd = sigma_depth * max_(depth, 1e-6f);
    return 1.0f / (sd * sd);
}
// A guide word from four floats: for the twins, whose callers promise no alignment (the kernels load a word as one float4).
PTD float4 filter_guide_word(const float* g) { return make_float4(g[0], g[1], g[2], g[3]); }
PTD v3 filter_remodulate(v3 o, v3 albedo) { return V(o.x * filter_divisor(albedo.x), o.y * filter_divisor(albedo.y), o.z * filter_divisor(albedo.z)); }

// ---- prepare: the three records of one pixel ---------------------------------------------------------------------------------------
// The spare words:   kFilterDenoise     colour.w = kz           albedo.w = 0
//                    kFilterDenoiseVar  colour.w = v            albedo.w = kz     (v: the summed variance, kVarMax where unknown)
//                    kFilterUpsample    colour.w = 0            albedo.w = 0      (its kz belongs to the HIGH pixel: upsample_pixel)
enum FilterKind { kFilterDenoise, kFilterDenoiseVar, kFilterUpsample };

// rgb: the pixel's three floats; var: its three variances (kFilterDenoiseVar only, else not read); g0, g1: the guide pass's two words
// {albedo r g b, alpha | normal x y z, depth}; flags: the filter's, whose one bit is the same in all three.
static_assert(PT_DENOISE_DEMODULATE == PT_UPSAMPLE_DEMODULATE, "filter_prepare_pixel and filter_finish_pixel test one bit for the three filters");
template <FilterKind K>
PTD void filter_prepare_pixel(const float* rgb, const float* var, float4 g0, float4 g1, int flags, float sigma_depth, float4& col, float4& nz, float4& alb)
{
    float c[3] = {filter_finite_or_0(rgb[0]), filter_finite_or_0(rgb[1]), filter_finite_or_0(rgb[2])};
    float v[3] = {0.0f, 0.0f, 0.0f};
    if constexpr (K == kFilterDenoiseVar) {
        v[0] = var[0]; v[1] = var[1]; v[2] = var[2];
    }
    const float kz = (K == kFilterUpsample) ? 0.0f : filter_kz(sigma_depth, g1.w);
    nz = g1;
    alb = make_float4(g0.x, g0.y, g0.z, (K == kFilterDenoiseVar) ? kz : 0.0f);
    if (flags & PT_DENOISE_DEMODULATE) {
        const float d[3] = {filter_divisor(g0.x), filter_divisor(g0.y), filter_divisor(g0.z)};
        for (int k = 0; k < 3; ++k) c[k] = c[k] / d[k];
        if constexpr (K == kFilterDenoiseVar)
            for (int k = 0; k < 3; ++k) v[k] = v[k] / (d[k] * d[k]);
    }
    float cw = kz;
    if constexpr (K == kFilterDenoiseVar) {
        const float vs = (v[0] + v[1]) + v[2];
        cw = (vs >= 0.0f && vs <= kVarMax) ? vs : kVarMax;
    }
    col = make_float4(c[0], c[1], c[2], cw);
}

// ---- one iteration pixel of the a-trous filters ------------------------------------------------------------------------------------
// The edge-stopping weight of a tap q against the pixel p, h its binomial weight.  A tap whose weight is not > 0 is skipped by the one
// loop that calls this (NaN and non-finite guides included).
PTD float filter_tap_weight(float h, float4 cq, float4 nq, float4 aq, v3 c_p, v3 n_p, v3 a_p, float z_p, float kc, float kn, float kz, float ka)
{
    const v3 dc = V(cq.x, cq.y, cq.z) - c_p, dn = V(nq.x, nq.y, nq.z) - n_p, da = V(aq.x, aq.y, aq.z) - a_p;
    const float ec = dot(dc, dc), en = dot(dn, dn), ea = dot(da, da);
    const float dz = nq.w - z_p;
    const float ez = dz * dz;
    const float e = fma_(ea, ka, fma_(ez, kz, fma_(en, kn, ec * kc)));
    return h * exp_(-e);
}

// Pixel (x, row) of the frame at step s: its new colour record, from src into dst.  A: the kernels' own arguments (PtDenoiseArgs,
// PtDenoiseVarArgs; the twin passes a record with the fields read here: width, height, nz, alb, kn, ka).  VAR = false, pt_denoise:
// colour = kc, the iteration's constant.  VAR = true, pt_denoise_var: colour = s2, and the pixel's own kc = 1 / (s2 * vb + 1e-10) with
// vb the 3 x 3 binomial mean of v over the direct neighbours (distance 1 whatever the step); a second sum, of w^2 v, becomes the next v.
// The loop order (dy outer, dx inner) is the definition's: each sum is a sequential chain over the taps, and that order is the result.
// The sums of one tap are independent of each other; they are written wsum first and sx last because that is the order in which the
// compiler schedules them as the hand-inlined kernel bodies did (make pt_denoise.s: the same instructions in the same places).
template <bool VAR, class Args>
PTD void filter_iter_pixel(const Args& A, const float4* __restrict__ src, float4* __restrict__ dst, int x, int row, int s, float colour)
{
    const int W = A.width, H = A.height;
    const float4* __restrict__ nzb = A.nz;
    const float4* __restrict__ alb = A.alb;
    const size_t i = (size_t)row * (size_t)W + (size_t)x;
    const float4 cp = src[i], np = nzb[i], ap = alb[i];
    const v3 c_p = V(cp.x, cp.y, cp.z), n_p = V(np.x, np.y, np.z), a_p = V(ap.x, ap.y, ap.z);
    const float kz = VAR ? ap.w : cp.w, kn = A.kn, ka = A.ka;
    float kc = colour;
    if constexpr (VAR) {
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
        kc = (colour == __builtin_inff()) ? 0.0f : 1.0f / fma_(colour, vb, 1e-10f);
    }
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
                w = filter_tap_weight(h, cq, nzb[q], alb[q], c_p, n_p, a_p, np.w, kc, kn, kz, ka);
                if (!(w > 0.0f)) continue; // NaN and non-finite guides included
            }
            wsum = wsum + w;
            if constexpr (VAR) vsum = fma_(w * w, cq.w, vsum);
            sz = fma_(w, cq.z, sz);
            sy = fma_(w, cq.y, sy);
            sx = fma_(w, cq.x, sx);
        }
    }
    dst[i] = make_float4(sx / wsum, sy / wsum, sz / wsum, VAR ? min_(vsum / (wsum * wsum), kVarMax) : kz);
}

// ---- finish: the pixel's three floats from its colour record, multiplied back by the albedo divisor with the flag --------------------
PTD v3 filter_finish_pixel(const float4* col, const float4* alb, size_t i, int flags)
{
    const float4 c = col[i];
    v3 o = V(c.x, c.y, c.z);
    if (flags & PT_DENOISE_DEMODULATE) {
        const float4 a = alb[i];
        o = filter_remodulate(o, V(a.x, a.y, a.z));
    }
    return o;
}

// ---- one high pixel of the upsampler -----------------------------------------------------------------------------------------------
// Pixel (x, row) of the high frame, g0 | g1 its own guide words; A: the low records and the constants.  The window is written for
// taps = 4 (j, i = -1 .. 2); taps = 2 leaves the outer ring with a uniform test, which is the definition's loop j, i = 0 .. 1.  j outer,
// i inner: the sums are sequential chains.  The edge term has no colour part and keeps its own expression, en * kn where the a-trous
// chain has fma_(en, kn, ec * kc): it does not go through filter_tap_weight.
PTD v3 upsample_pixel(const PtUpsampleArgs& A, float4 g0, float4 g1, int x, int row)
{
    const int w = A.w, h = A.h;
    const float4* __restrict__ col = A.col;
    const float4* __restrict__ nzb = A.nz;
    const float4* __restrict__ alb = A.alb;
    const v3 a_p = V(g0.x, g0.y, g0.z), n_p = V(g1.x, g1.y, g1.z);
    const float z_p = g1.w, kn = A.kn, ka = A.ka, ir = A.ir;
    const float kz = filter_kz(A.sigma_depth, z_p);
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
            wsum = wsum + wt; // (independent sums, in the order of filter_iter_pixel's)
            sz = fma_(wt, cq.z, sz);
            sy = fma_(wt, cq.y, sy);
            sx = fma_(wt, cq.x, sx);
        }
    }
    v3 o = (wsum >= 1e-4f * pw) ? V(sx / wsum, sy / wsum, sz / wsum) : V(px / pw, py / pw, pz / pw);
    if (A.flags & PT_UPSAMPLE_DEMODULATE) o = filter_remodulate(o, a_p);
    return o;
}

} // namespace ptd
