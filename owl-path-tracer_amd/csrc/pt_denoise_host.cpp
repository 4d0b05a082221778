// pt_denoise_host.cpp -- pt_debug_denoise_host: the CPU twin of the denoiser (pt_denoise; kernels: pt_denoise.hip), and what the twin
// and the device path share on the host: the default parameters, the refusals and the host constants.  Likewise
// pt_debug_denoise_var_host, the twin of the variance-guided filter (pt_denoise_var; kernels: pt_denoise_var.hip).
// The twin runs the definition of include/mi355pt.h ("denoiser") with the arithmetic of pt_device.h itself: the header is included here
// with PTD = static inline, so exp_, dot, max_ and make_rgba are the functions the kernels compile, run by the CPU under the same contract
// (binary32, -ffp-contract=off, fma only where spelled, correctly rounded division).  Rows are spread over all host threads.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

// the bit casts pt_device.h uses are device functions of the HIP headers: host forms under the same names (as pt_aov_host.cpp)
static inline uint32_t pt_host_float_as_uint(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static inline float pt_host_uint_as_float(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
#define __float_as_uint pt_host_float_as_uint
#define __uint_as_float pt_host_uint_as_float
#define PTD static inline
#include "pt_accum_math.h" // (pt_device.h, and kVarMax)
#undef __float_as_uint
#undef __uint_as_float

#include "pt_internal.h"

using namespace pti;
using namespace ptd;

namespace pti {

// What pt_denoise, pt_denoise_device and the twin refuse alike, before anything is touched; *eff = the parameters in effect.
int check_denoise_args(pt_ctx* c, const char* who, int W, int H, const pt_denoise_params* p, pt_denoise_params* eff, void (*defaults)(pt_denoise_params*))
{
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (int64_t)W * H > (int64_t)0x7fffffff) return fail(c, PT_E_INVALID, "%s: bad frame size %dx%d", who, W, H);
    if (p) *eff = *p;
    else defaults(eff);
    if (eff->iterations < 1 || eff->iterations > 8) return fail(c, PT_E_INVALID, "%s: iterations %d outside 1..8", who, eff->iterations);
    if (eff->flags & ~PT_DENOISE_DEMODULATE) return fail(c, PT_E_INVALID, "%s: unknown flag bits 0x%x (only PT_DENOISE_DEMODULATE = 1 is defined)", who, (unsigned)(eff->flags & ~PT_DENOISE_DEMODULATE));
    const float sg[4] = {eff->sigma_color, eff->sigma_normal, eff->sigma_depth, eff->sigma_albedo};
    const char* names[4] = {"sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"};
    for (int i = 0; i < 4; ++i)
        if (!(sg[i] > 0.0f)) return fail(c, PT_E_INVALID, "%s: %s = %g must be > 0 (+infinity switches the term off)", who, names[i], (double)sg[i]);
    return PT_OK;
}

// The host constants of the definition, in float32 and in its order.
void denoise_constants(const pt_denoise_params& p, float* kn, float* ka, float kc[8])
{
    *kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    *ka = 1.0f / (p.sigma_albedo * p.sigma_albedo);
    for (int i = 0; i < 8; ++i) {
        const float sc = p.sigma_color * (1.0f / (float)(1 << i)); // x 2^-i: exact
        kc[i] = 1.0f / (sc * sc);
    }
}

} // namespace pti

namespace {

struct Rec { float x, y, z, w; };

float finite_or_0(float v) { return (isinf_(v) || isnan_(v)) ? 0.0f : v; }

// One pixel of iteration i: include/mi355pt.h, "denoiser"; the kernel's loop body (pt_denoise_iter_kernel) line for line.
Rec iter_pixel(const Rec* src, const Rec* nzb, const Rec* alb, int W, int H, int x, int row, int s, float kc, float kn, float ka)
{
    const size_t i = (size_t)row * (size_t)W + (size_t)x;
    const Rec cp = src[i], np = nzb[i], ap = alb[i];
    const v3 c_p = V(cp.x, cp.y, cp.z), n_p = V(np.x, np.y, np.z), a_p = V(ap.x, ap.y, ap.z);
    const float kz = cp.w;
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = row + dy * s;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W) continue;
            const float h = k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
            float w;
            Rec cq;
            if (dx == 0 && dy == 0) {
                w = h;
                cq = cp;
            } else {
                const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                cq = src[q];
                const Rec nq = nzb[q], aq = alb[q];
                const v3 dc = V(cq.x, cq.y, cq.z) - c_p, dn = V(nq.x, nq.y, nq.z) - n_p, da = V(aq.x, aq.y, aq.z) - a_p;
                const float ec = dot(dc, dc), en = dot(dn, dn), ea = dot(da, da);
                const float dz = nq.w - np.w;
                const float ez = dz * dz;
                const float e = fma_(ea, ka, fma_(ez, kz, fma_(en, kn, ec * kc)));
                w = h * exp_(-e);
                if (!(w > 0.0f)) continue;
            }
            sx = fma_(w, cq.x, sx);
            sy = fma_(w, cq.y, sy);
            sz = fma_(w, cq.z, sz);
            wsum = wsum + w;
        }
    }
    return Rec{sx / wsum, sy / wsum, sz / wsum, kz};
}

} // namespace

extern "C" void pt_denoise_default_params(pt_denoise_params* p)
{
    if (!p) return;
    p->iterations = 5;
    p->flags = 0;
    p->sigma_color = 4.0f;
    p->sigma_normal = 0.25f;
    p->sigma_depth = 0.1f;
    p->sigma_albedo = 0.2f;
}

extern "C" int64_t pt_debug_denoise_host(pt_ctx* c, const float* rgb, const float* aov, int32_t W, int32_t H, const pt_denoise_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    if (!rgb || !aov || !out_rgb) return fail(c, PT_E_INVALID, "pt_debug_denoise_host: NULL %s", !rgb ? "rgb" : (!aov ? "aov" : "out_rgb"));
    pt_denoise_params prm;
    int rc = check_denoise_args(c, "pt_debug_denoise_host", W, H, p, &prm);
    if (rc) return rc;
    float kn, ka, kc[8];
    denoise_constants(prm, &kn, &ka, kc);
    const bool dm = (prm.flags & PT_DENOISE_DEMODULATE) != 0;
    const size_t npx = (size_t)W * (size_t)H;
    std::vector<Rec> col[2], nzb(npx), alb(npx); // buffers of its own: out_rgb may be rgb
    col[0].resize(npx);
    col[1].resize(npx);
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // prepare
        for (size_t i = lo; i < hi; ++i) {
            const float* g = aov + 8 * i;
            const float r[3] = {finite_or_0(rgb[3 * i]), finite_or_0(rgb[3 * i + 1]), finite_or_0(rgb[3 * i + 2])};
            const float sd = prm.sigma_depth * max_(g[7], 1e-6f);
            const float kz = 1.0f / (sd * sd);
            col[0][i] = dm ? Rec{r[0] / max_(g[0], 1e-3f), r[1] / max_(g[1], 1e-3f), r[2] / max_(g[2], 1e-3f), kz} : Rec{r[0], r[1], r[2], kz};
            nzb[i] = Rec{g[4], g[5], g[6], g[7]};
            alb[i] = Rec{g[0], g[1], g[2], 0.0f};
        }
    });
    for (int it = 0; it < prm.iterations; ++it) {
        const Rec* src = col[it & 1].data();
        Rec* dst = col[(it + 1) & 1].data();
        pt_parallel_ranges((size_t)H, [&](size_t lo, size_t hi) {
            for (size_t row = lo; row < hi; ++row)
                for (int x = 0; x < W; ++x) dst[row * (size_t)W + (size_t)x] = iter_pixel(src, nzb.data(), alb.data(), W, H, x, (int)row, 1 << it, kc[it], kn, ka);
        });
    }
    const Rec* fin = col[prm.iterations & 1].data();
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // finish
        for (size_t i = lo; i < hi; ++i) {
            v3 o = V(fin[i].x, fin[i].y, fin[i].z);
            if (dm) o = V(o.x * max_(alb[i].x, 1e-3f), o.y * max_(alb[i].y, 1e-3f), o.z * max_(alb[i].z, 1e-3f));
            out_rgb[3 * i] = o.x; out_rgb[3 * i + 1] = o.y; out_rgb[3 * i + 2] = o.z;
            if (out_rgba8) out_rgba8[i] = make_rgba(o);
        }
    });
    return (int64_t)npx;
}

// ---- variance-guided filter (pt_denoise_var) -----------------------------------------------------------------------------------
namespace {

// One pixel of iteration i: include/mi355pt.h, "variance-guided denoise"; the kernel's loop body (pt_denoise_var_iter_kernel) line for
// line.  Colour records carry v in w, albedo records kz.
Rec iter_var_pixel(const Rec* src, const Rec* nzb, const Rec* alb, int W, int H, int x, int row, int s, float s2, float kn, float ka)
{
    const size_t i = (size_t)row * (size_t)W + (size_t)x;
    const Rec cp = src[i], np = nzb[i], ap = alb[i];
    const v3 c_p = V(cp.x, cp.y, cp.z), n_p = V(np.x, np.y, np.z), a_p = V(ap.x, ap.y, ap.z);
    const float kz = ap.w;
    const float m[2] = {0.5f, 0.25f};
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = row + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const float g = m[dx < 0 ? -dx : dx] * m[dy < 0 ? -dy : dy];
            gs = fma_(g, src[(size_t)qy * (size_t)W + (size_t)qx].w, gs);
            gw = gw + g;
        }
    }
    const float vb = gs / gw;
    const float kc = (s2 == __builtin_inff()) ? 0.0f : 1.0f / fma_(s2, vb, 1e-10f);
    const float k[3] = {0.375f, 0.25f, 0.0625f};
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, wsum = 0.0f, vsum = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = row + dy * s;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W) continue;
            const float h = k[dx < 0 ? -dx : dx] * k[dy < 0 ? -dy : dy];
            float w;
            Rec cq;
            if (dx == 0 && dy == 0) {
                w = h;
                cq = cp;
            } else {
                const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
                cq = src[q];
                const Rec nq = nzb[q], aq = alb[q];
                const v3 dc = V(cq.x, cq.y, cq.z) - c_p, dn = V(nq.x, nq.y, nq.z) - n_p, da = V(aq.x, aq.y, aq.z) - a_p;
                const float ec = dot(dc, dc), en = dot(dn, dn), ea = dot(da, da);
                const float dz = nq.w - np.w;
                const float ez = dz * dz;
                const float e = fma_(ea, ka, fma_(ez, kz, fma_(en, kn, ec * kc)));
                w = h * exp_(-e);
                if (!(w > 0.0f)) continue;
            }
            sx = fma_(w, cq.x, sx);
            sy = fma_(w, cq.y, sy);
            sz = fma_(w, cq.z, sz);
            vsum = fma_(w * w, cq.w, vsum);
            wsum = wsum + w;
        }
    }
    return Rec{sx / wsum, sy / wsum, sz / wsum, min_(vsum / (wsum * wsum), kVarMax)};
}

} // namespace

extern "C" void pt_denoise_var_default_params(pt_denoise_params* p)
{
    if (!p) return;
    pt_denoise_default_params(p);
    p->sigma_color = 3.0f; // standard deviations here
}

extern "C" int64_t pt_debug_denoise_var_host(pt_ctx* c, const float* rgb, const float* var, const float* aov, int32_t W, int32_t H, const pt_denoise_params* p, float* out_rgb,
                                             uint32_t* out_rgba8, float* out_var)
{
    if (!c) return PT_E_INVALID;
    if (!rgb || !var || !aov || !out_rgb) return fail(c, PT_E_INVALID, "pt_debug_denoise_var_host: NULL %s", !rgb ? "rgb" : (!var ? "var" : (!aov ? "aov" : "out_rgb")));
    pt_denoise_params prm;
    int rc = check_denoise_args(c, "pt_debug_denoise_var_host", W, H, p, &prm, pt_denoise_var_default_params);
    if (rc) return rc;
    float kn, ka, kc_unused[8];
    denoise_constants(prm, &kn, &ka, kc_unused);
    const float s2 = prm.sigma_color * prm.sigma_color;
    const bool dm = (prm.flags & PT_DENOISE_DEMODULATE) != 0;
    const size_t npx = (size_t)W * (size_t)H;
    std::vector<Rec> col[2], nzb(npx), alb(npx); // buffers of its own: out_rgb may be rgb
    col[0].resize(npx);
    col[1].resize(npx);
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // prepare
        for (size_t i = lo; i < hi; ++i) {
            const float* g = aov + 8 * i;
            float r[3] = {finite_or_0(rgb[3 * i]), finite_or_0(rgb[3 * i + 1]), finite_or_0(rgb[3 * i + 2])};
            float vk[3] = {var[3 * i], var[3 * i + 1], var[3 * i + 2]};
            const float sd = prm.sigma_depth * max_(g[7], 1e-6f);
            const float kz = 1.0f / (sd * sd);
            if (dm)
                for (int k = 0; k < 3; ++k) {
                    const float d = max_(g[k], 1e-3f);
                    r[k] = r[k] / d;
                    vk[k] = vk[k] / (d * d);
                }
            const float v = (vk[0] + vk[1]) + vk[2];
            col[0][i] = Rec{r[0], r[1], r[2], (v >= 0.0f && v <= kVarMax) ? v : kVarMax};
            nzb[i] = Rec{g[4], g[5], g[6], g[7]};
            alb[i] = Rec{g[0], g[1], g[2], kz};
        }
    });
    for (int it = 0; it < prm.iterations; ++it) {
        const Rec* src = col[it & 1].data();
        Rec* dst = col[(it + 1) & 1].data();
        pt_parallel_ranges((size_t)H, [&](size_t lo, size_t hi) {
            for (size_t row = lo; row < hi; ++row)
                for (int x = 0; x < W; ++x) dst[row * (size_t)W + (size_t)x] = iter_var_pixel(src, nzb.data(), alb.data(), W, H, x, (int)row, 1 << it, s2, kn, ka);
        });
    }
    const Rec* fin = col[prm.iterations & 1].data();
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // finish
        for (size_t i = lo; i < hi; ++i) {
            v3 o = V(fin[i].x, fin[i].y, fin[i].z);
            if (dm) o = V(o.x * max_(alb[i].x, 1e-3f), o.y * max_(alb[i].y, 1e-3f), o.z * max_(alb[i].z, 1e-3f));
            out_rgb[3 * i] = o.x; out_rgb[3 * i + 1] = o.y; out_rgb[3 * i + 2] = o.z;
            if (out_rgba8) out_rgba8[i] = make_rgba(o);
            if (out_var) out_var[i] = fin[i].w;
        }
    });
    return (int64_t)npx;
}
