// pt_upsample_host.cpp -- pt_debug_upsample_host: the CPU twin of the upsampling (pt_upsample; kernels: pt_upsample.hip), and what the
// twin and the device path share on the host: the default parameters, the refusals and the host constants.
// The twin runs the definition of include/mi355pt.h ("upsampling") with the arithmetic of pt_device.h itself: the header is included here
// with PTD = static inline, so exp_, dot, max_, abs_ and make_rgba are the functions the kernels compile, run by the CPU under the same
// contract (binary32, -ffp-contract=off, fma only where spelled, correctly rounded division).  Rows are spread over all host threads.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

// the bit casts pt_device.h uses are device functions of the HIP headers: host forms under the same names (as pt_aov_host.cpp)
static inline uint32_t pt_host_float_as_uint(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static inline float pt_host_uint_as_float(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }
#define __float_as_uint pt_host_float_as_uint
#define __uint_as_float pt_host_uint_as_float
#define PTD static inline
#include "pt_device.h"
#undef __float_as_uint
#undef __uint_as_float

#include "pt_internal.h"

using namespace pti;
using namespace ptd;

namespace pti {

// What pt_upsample, pt_upsample_device and the twin refuse alike, before anything is touched; *eff = the parameters in effect.
int check_upsample_args(pt_ctx* c, const char* who, int w, int h, int W, int H, const pt_upsample_params* p, pt_upsample_params* eff)
{
    if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return fail(c, PT_E_INVALID, "%s: bad low frame size %dx%d", who, w, h);
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (int64_t)W * H > (int64_t)0x7fffffff) return fail(c, PT_E_INVALID, "%s: bad frame size %dx%d", who, W, H);
    if (w > W || h > H) return fail(c, PT_E_INVALID, "%s: the low frame %dx%d is larger than the frame %dx%d", who, w, h, W, H);
    if (p) *eff = *p;
    else pt_upsample_default_params(eff);
    if (eff->taps != 2 && eff->taps != 4) return fail(c, PT_E_INVALID, "%s: taps %d is not 2 or 4", who, eff->taps);
    if (eff->flags & ~PT_UPSAMPLE_DEMODULATE) return fail(c, PT_E_INVALID, "%s: unknown flag bits 0x%x (only PT_UPSAMPLE_DEMODULATE = 1 is defined)", who, (unsigned)(eff->flags & ~PT_UPSAMPLE_DEMODULATE));
    const float sg[3] = {eff->sigma_normal, eff->sigma_depth, eff->sigma_albedo};
    const char* names[3] = {"sigma_normal", "sigma_depth", "sigma_albedo"};
    for (int i = 0; i < 3; ++i)
        if (!(sg[i] > 0.0f)) return fail(c, PT_E_INVALID, "%s: %s = %g must be > 0 (+infinity switches the term off)", who, names[i], (double)sg[i]);
    if (eff->reserved != 0) return fail(c, PT_E_INVALID, "%s: reserved = %d must be 0", who, eff->reserved);
    return PT_OK;
}

// The host constants of the definition, in float32 and in its order.
void upsample_constants(const pt_upsample_params& p, int w, int h, int W, int H, float* rx, float* ry, float* kn, float* ka, float* ir)
{
    *rx = (float)w / (float)W;
    *ry = (float)h / (float)H;
    *kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    *ka = 1.0f / (p.sigma_albedo * p.sigma_albedo);
    const int R = p.taps / 2;
    *ir = 1.0f / (float)R;
}

} // namespace pti

namespace {

struct Rec { float x, y, z, w; };

float finite_or_0(float v) { return (isinf_(v) || isnan_(v)) ? 0.0f : v; }
float up_div(float a) { return max_(a, 1e-3f); }

struct Consts { int w, h, W, taps, flags; float sigma_depth, rx, ry, kn, ka, ir; };

// One high pixel: include/mi355pt.h, "upsampling"; the kernel's body (pt_upsample_kernel) line for line.
v3 upsample_pixel(const Rec* col, const Rec* nzb, const Rec* alb, const float* aov_hi, const Consts& A, int x, int row)
{
    const int w = A.w, h = A.h;
    const size_t p = (size_t)row * (size_t)A.W + (size_t)x;
    const float* g = aov_hi + 8 * p;
    const v3 a_p = V(g[0], g[1], g[2]), n_p = V(g[4], g[5], g[6]);
    const float z_p = g[7], kn = A.kn, ka = A.ka, ir = A.ir;
    const float sd = A.sigma_depth * max_(z_p, 1e-6f);
    const float kz = 1.0f / (sd * sd);
    const float fx = ((float)x + 0.5f) * A.rx - 0.5f, fy = ((float)row + 0.5f) * A.ry - 0.5f;
    const int x0 = (int)__builtin_floorf(fx), y0 = (int)__builtin_floorf(fy);
    const float tx = fx - (float)x0, ty = fy - (float)y0;
    const bool ring = A.taps == 4;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f, wsum = 0.0f, pw = 0.0f;
    for (int j = -1; j <= 2; ++j) {
        if (!ring && (j < 0 || j > 1)) continue;
        const int qy = y0 + j;
        if (qy < 0 || qy >= h) continue;
        const float by = 1.0f - abs_((float)j - ty) * ir;
        for (int i = -1; i <= 2; ++i) {
            if (!ring && (i < 0 || i > 1)) continue;
            const int qx = x0 + i;
            if (qx < 0 || qx >= w) continue;
            const float bx = 1.0f - abs_((float)i - tx) * ir;
            if (!(bx > 0.0f && by > 0.0f)) continue;
            const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
            const Rec cq = col[q], nq = nzb[q], aq = alb[q];
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
            if (!(wt > 0.0f)) continue;
            sx = fma_(wt, cq.x, sx);
            sy = fma_(wt, cq.y, sy);
            sz = fma_(wt, cq.z, sz);
            wsum = wsum + wt;
        }
    }
    v3 o = (wsum >= 1e-4f * pw) ? V(sx / wsum, sy / wsum, sz / wsum) : V(px / pw, py / pw, pz / pw);
    if (A.flags & PT_UPSAMPLE_DEMODULATE) o = V(o.x * up_div(a_p.x), o.y * up_div(a_p.y), o.z * up_div(a_p.z));
    return o;
}

} // namespace

extern "C" void pt_upsample_default_params(pt_upsample_params* p)
{
    if (!p) return;
    p->taps = 4;
    p->flags = PT_UPSAMPLE_DEMODULATE;
    p->sigma_normal = 0.25f;
    p->sigma_depth = 0.1f;
    p->sigma_albedo = 0.2f;
    p->reserved = 0;
}

extern "C" int64_t pt_debug_upsample_host(pt_ctx* c, const float* rgb_lo, const float* aov_lo, int32_t w, int32_t h, const float* aov_hi, int32_t W, int32_t H,
                                          const pt_upsample_params* p, float* out_rgb, uint32_t* out_rgba8)
{
    if (!c) return PT_E_INVALID;
    if (!rgb_lo || !aov_lo || !aov_hi || !out_rgb)
        return fail(c, PT_E_INVALID, "pt_debug_upsample_host: NULL %s", !rgb_lo ? "rgb_lo" : (!aov_lo ? "aov_lo" : (!aov_hi ? "aov_hi" : "out_rgb")));
    pt_upsample_params prm;
    int rc = check_upsample_args(c, "pt_debug_upsample_host", w, h, W, H, p, &prm);
    if (rc) return rc;
    Consts A{w, h, W, prm.taps, prm.flags, prm.sigma_depth};
    upsample_constants(prm, w, h, W, H, &A.rx, &A.ry, &A.kn, &A.ka, &A.ir);
    const bool dm = (prm.flags & PT_UPSAMPLE_DEMODULATE) != 0;
    const size_t npx = (size_t)w * (size_t)h;
    std::vector<Rec> col(npx), nzb(npx), alb(npx);
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // prepare
        for (size_t i = lo; i < hi; ++i) {
            const float* g = aov_lo + 8 * i;
            const float r[3] = {finite_or_0(rgb_lo[3 * i]), finite_or_0(rgb_lo[3 * i + 1]), finite_or_0(rgb_lo[3 * i + 2])};
            col[i] = dm ? Rec{r[0] / up_div(g[0]), r[1] / up_div(g[1]), r[2] / up_div(g[2]), 0.0f} : Rec{r[0], r[1], r[2], 0.0f};
            nzb[i] = Rec{g[4], g[5], g[6], g[7]};
            alb[i] = Rec{g[0], g[1], g[2], 0.0f};
        }
    });
    pt_parallel_ranges((size_t)H, [&](size_t lo, size_t hi) {
        for (size_t row = lo; row < hi; ++row)
            for (int x = 0; x < W; ++x) {
                const v3 o = upsample_pixel(col.data(), nzb.data(), alb.data(), aov_hi, A, x, (int)row);
                const size_t i = row * (size_t)W + (size_t)x;
                out_rgb[3 * i] = o.x; out_rgb[3 * i + 1] = o.y; out_rgb[3 * i + 2] = o.z;
                if (out_rgba8) out_rgba8[i] = make_rgba(o);
            }
    });
    return (int64_t)W * (int64_t)H;
}
