// pt_accum_math.h -- the per-pixel definition of the progressive accumulation (include/mi355pt.h, "progressive accumulation"): resolve
// and select, the variance of a pixel and its reprojection to a new camera, ONE copy for the kernels of pt_accum.hip, pt_denoise_var.hip
// and pt_accum_reproject.hip and their CPU twins in pt_accum_host.cpp (which include pt_device_host.h
// first: PTD = static inline).  Arithmetic: the contract of pt_device.h - binary32, no contraction, correctly
// rounded division, its sqrt_, abs_, max_ and make_rgba.
#pragma once
#include "pt_device.h"
#include "pt_launch.h"

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

// ---- reprojection (include/mi355pt.h, "reprojection"): ONE copy for pt_accum_reproject_kernel (pt_accum_reproject.hip) and
// pt_debug_accum_reproject_host.  Both index every per-pixel array of the state by the launch id x + W * y and the guides in framebuffer
// order x + W * (H - 1 - y).

// One guide record {albedo r g b, alpha, normal x y z, depth}: two 16-byte loads on the device (the buffers are 16-byte aligned there),
// eight floats on the host, whose callers promise no alignment.
PTD void accum_load_guide(const float* aov, size_t index, float g[8])
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 lo = reinterpret_cast<const float4*>(aov)[2 * index], hi = reinterpret_cast<const float4*>(aov)[2 * index + 1];
    g[0] = lo.x; g[1] = lo.y; g[2] = lo.z; g[3] = lo.w;
    g[4] = hi.x; g[5] = hi.y; g[6] = hi.z; g[7] = hi.w;
#else
    for (int k = 0; k < 8; ++k) g[k] = aov[8 * index + k];
#endif
}

PTD bool accum_guide_is_surface(const float g[8]) { return g[3] >= 0.5f && g[7] > 0.0f && !isinf_(g[7]); }

// Steps 1 to 5 for the owned pixel (px, py) of the new frame: has it a source in the old frame, and which (*source = its launch id)?
// owned: the shard's flags by launch id.
PTD bool accum_reproject_source(const PtAccumReproject& R, int px, int py, const float* aov_prev, const float* aov_cur, const uint8_t* owned, uint32_t* source)
{
    const float fw = (float)R.width, fh = (float)R.height;
    const size_t W = (size_t)R.width;
    // 1. the camera ray through the pixel centre (gen_camera_ray's operations)
    const float su = ((float)px + 0.5f) / fw, sv = ((float)py + 0.5f) / fh;
    const v3 org = V(R.o[0], R.o[1], R.o[2]);
    const v3 dc = normalize(((V(R.llc[0], R.llc[1], R.llc[2]) + V(R.hor[0], R.hor[1], R.hor[2]) * su) + V(R.ver[0], R.ver[1], R.ver[2]) * sv) - org);
    // 2. surface or sky
    float g[8];
    accum_load_guide(aov_cur, (size_t)px + W * (size_t)(R.height - 1 - py), g);
    const bool surface = accum_guide_is_surface(g);
    v3 r = dc;
    float ze = 0.0f;
    if (surface) {
        const v3 P = org + dc * g[7];
        r = P - V(R.oo[0], R.oo[1], R.oo[2]);
        ze = sqrt_(dot(r, r));
    }
    // 3. projection into the old camera
    const v3 N = V(R.N[0], R.N[1], R.N[2]), ho = V(R.ho[0], R.ho[1], R.ho[2]), vo = V(R.vo[0], R.vo[1], R.vo[2]);
    const float dn = dot(N, r), lam = R.na / dn;
    if (!(lam > 0.0f && !isinf_(lam))) return false;
    const v3 w = r * lam - V(R.a[0], R.a[1], R.a[2]);
    const float su_o = dot(cross(w, vo), N) * R.inn, sv_o = dot(cross(ho, w), N) * R.inn;
    const float fx = su_o * fw, fy = sv_o * fh;
    if (!(fx >= 0.0f && fx < fw && fy >= 0.0f && fy < fh)) return false; // (NaN fails)
    const int qx = (int)fx, qy = (int)fy;
    // 4. the source belongs to the context
    const size_t q = (size_t)qx + W * (size_t)qy;
    if (!owned[q]) return false;
    // 5. consistency: every comparison must be true
    float s[8];
    accum_load_guide(aov_prev, (size_t)qx + W * (size_t)(R.height - 1 - qy), s);
    if (accum_guide_is_surface(s) != surface) return false;
    if (surface) {
        if (!(abs_(s[7] - ze) <= R.depth_tol * ze)) return false;
        if (!(dot(V(g[4], g[5], g[6]), V(s[4], s[5], s[6])) >= R.normal_min)) return false;
    }
    const v3 da = V(s[0], s[1], s[2]) - V(g[0], g[1], g[2]);
    if (!(dot(da, da) <= R.albedo_tol * R.albedo_tol)) return false;
    *source = (uint32_t)q;
    return true;
}

// Step 6 on the copied state of the source: a pixel that arrives with more than max_history samples is scaled down to max_history.
PTD void accum_reproject_history(AccumPixel& s, uint32_t max_history)
{
    if (max_history == 0u || s.n <= max_history) return;
    const float f = (float)max_history / (float)s.n;
    for (int k = 0; k < 3; ++k) s.sum[k] = s.sum[k] * f;
    const uint32_t nh = (uint32_t)((uint64_t)s.n_half * (uint64_t)max_history / (uint64_t)s.n);
    const float fh = nh ? (float)nh / (float)s.n_half : 0.0f;
    for (int k = 0; k < 3; ++k) s.half[k] = nh ? s.half[k] * fh : 0.0f;
    s.n_half = nh;
    s.n = max_history;
}

} // namespace ptd
