// pt_accum_math.h -- the per-pixel definition of the progressive accumulation (include/mi355pt.h, "progressive accumulation"): resolve
// and select, ONE copy for the kernels of pt_accum.hip and their CPU twins in pt_accum_host.cpp (which include pt_device.h with
// PTD = static inline first, as pt_denoise_host.cpp does).  Arithmetic: the contract of pt_device.h - binary32, no contraction, correctly
// rounded division, its sqrt_, abs_, max_ and make_rgba.
#pragma once
#include "pt_device.h"

namespace ptd {

struct AccumPixel { // the state resolve updates
    float sum[3], seen[3], half[3];
    uint32_t n, n_half, passes;
};
struct AccumResolved {
    float rgb[3];
    uint32_t rgba8;
    float noise;
};

// One owned pixel of resolve.  `active`: the pixel took n_samples more samples in this add (sum already holds them).
PTD void accum_resolve_pixel(AccumPixel& s, bool active, uint32_t n_samples, AccumResolved& o)
{
    if (active) {
        if (s.passes & 1u) { // every second pass of a pixel goes to the half buffer as well
            for (int k = 0; k < 3; ++k) s.half[k] = s.half[k] + (s.sum[k] - s.seen[k]);
            s.n_half += n_samples;
        }
        for (int k = 0; k < 3; ++k) s.seen[k] = s.sum[k];
        s.n += n_samples;
        s.passes += 1u;
    }
    o.rgb[0] = o.rgb[1] = o.rgb[2] = 0.0f;
    o.rgba8 = 0u;
    if (s.n >= 1u) {
        const float inv = 1.0f / (float)s.n; // device.cu:247 with max_samples = n
        for (int k = 0; k < 3; ++k) o.rgb[k] = s.sum[k] * inv;
        o.rgba8 = make_rgba(V(o.rgb[0], o.rgb[1], o.rgb[2]));
    }
    if (s.n_half == 0u) {
        o.noise = __builtin_inff();
        return;
    }
    const float ia = 1.0f / (float)s.n_half, ib = 1.0f / (float)(s.n - s.n_half);
    float dk[3];
    for (int k = 0; k < 3; ++k) {
        const float a = s.half[k] * ia, b = (s.sum[k] - s.half[k]) * ib;
        dk[k] = abs_(a - b);
    }
    const float d = (dk[0] + dk[1]) + dk[2];
    const float l = max_((o.rgb[0] + o.rgb[1]) + o.rgb[2], 1e-2f);
    o.noise = d / sqrt_(l);
}

// Is an owned pixel with this state part of the next add?  cap = max_pixel_samples (0: none), threshold = noise_threshold (0: uniform).
PTD bool accum_select_pixel(float noise, uint32_t n, uint32_t cap, float threshold)
{
    return (cap == 0u || n < cap) && (threshold == 0.0f || !(noise <= threshold));
}

// Variance of an owned pixel's value from the two disjoint halves of its samples (include/mi355pt.h, "variance-guided denoise"): ONE
// copy for pt_accum_variance_kernel (pt_denoise_var.hip) and pt_debug_accum_variance_host.  E[(a - b)^2] = s^2 (1 / n_half + 1 / (n -
// n_half)) and the variance of the pixel's mean is s^2 / n, hence r.  kVarMax stands for "unknown"; ia, ib and the colour are resolve's
// own expressions.
constexpr float kVarMax = 1e30f;
PTD void accum_variance_pixel(const float sum[3], const float half[3], uint32_t n, uint32_t n_half, float rgb[3], float var[3])
{
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (n >= 1u) {
        const float inv = 1.0f / (float)n;
        for (int k = 0; k < 3; ++k) rgb[k] = sum[k] * inv;
    }
    if (n_half == 0u) {
        var[0] = var[1] = var[2] = kVarMax;
        return;
    }
    const float ia = 1.0f / (float)n_half, ib = 1.0f / (float)(n - n_half);
    const float fh = (float)n_half / (float)n, r = fh * (1.0f - fh);
    for (int k = 0; k < 3; ++k) {
        const float a = half[k] * ia, b = (sum[k] - half[k]) * ib, e = a - b;
        const float v = r * (e * e);
        var[k] = (v <= kVarMax) ? v : kVarMax; // NaN and +inf included
    }
}

} // namespace ptd
