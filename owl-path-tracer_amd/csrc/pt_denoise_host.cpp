// pt_denoise_host.cpp -- pt_debug_denoise_host: the CPU twin of the denoiser (pt_denoise; kernels: pt_denoise.hip), and what the twin
// and the device path share on the host: the default parameters, the refusals and the host constants.  Likewise
// pt_debug_denoise_var_host, the twin of the variance-guided filter (pt_denoise_var; kernels: pt_denoise_var.hip).
// Each twin compiles the per-pixel definition its kernels compile, pt_filter_math.h with PTD = static inline (pt_device_host.h), and
// keeps the loops around it: prepare over the pixels, the iterations over the rows, finish.  Rows are spread over all host threads.
#include "pt_device_host.h"
#include "pt_filter_math.h" // (pt_accum_math.h, and kVarMax)

#include <vector>

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

// The three passes of both filters around pt_filter_math.h: K = kFilterDenoise (colour = kc[8], the iterations' constants) or
// kFilterDenoiseVar (colour = &s2).  Returns the final colour records.  Buffers of its own: out_rgb may be rgb.
template <FilterKind K>
std::vector<float4> filter_host(const float* rgb, const float* var, const float* aov, int W, int H, const pt_denoise_params& prm, const float* colour, float kn, float ka, float* out_rgb,
                                uint32_t* out_rgba8)
{
    constexpr bool VAR = K == kFilterDenoiseVar;
    const size_t npx = (size_t)W * (size_t)H;
    std::vector<float4> col[2], nzb(npx), alb(npx);
    col[0].resize(npx);
    col[1].resize(npx);
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // prepare
        for (size_t i = lo; i < hi; ++i)
            filter_prepare_pixel<K>(rgb + 3 * i, VAR ? var + 3 * i : nullptr, filter_guide_word(aov + 8 * i), filter_guide_word(aov + 8 * i + 4), prm.flags, prm.sigma_depth, col[0][i], nzb[i], alb[i]);
    });
    const struct { int width, height; const float4 *nz, *alb; float kn, ka; } A{W, H, nzb.data(), alb.data(), kn, ka}; // what filter_iter_pixel reads of the kernels' arguments
    for (int it = 0; it < prm.iterations; ++it) {
        const float4* src = col[it & 1].data();
        float4* dst = col[(it + 1) & 1].data();
        pt_parallel_ranges((size_t)H, [&](size_t lo, size_t hi) {
            for (size_t row = lo; row < hi; ++row)
                for (int x = 0; x < W; ++x) filter_iter_pixel<VAR>(A, src, dst, x, (int)row, 1 << it, VAR ? colour[0] : colour[it]);
        });
    }
    std::vector<float4>& fin = col[prm.iterations & 1];
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // finish
        for (size_t i = lo; i < hi; ++i) {
            const v3 o = filter_finish_pixel(fin.data(), alb.data(), i, prm.flags);
            out_rgb[3 * i] = o.x; out_rgb[3 * i + 1] = o.y; out_rgb[3 * i + 2] = o.z;
            if (out_rgba8) out_rgba8[i] = make_rgba(o);
        }
    });
    return std::move(fin);
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
    filter_host<kFilterDenoise>(rgb, nullptr, aov, W, H, prm, kc, kn, ka, out_rgb, out_rgba8);
    return (int64_t)W * (int64_t)H;
}

// ---- variance-guided filter (pt_denoise_var) -----------------------------------------------------------------------------------
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
    const std::vector<float4> fin = filter_host<kFilterDenoiseVar>(rgb, var, aov, W, H, prm, &s2, kn, ka, out_rgb, out_rgba8);
    if (out_var)
        for (size_t i = 0; i < fin.size(); ++i) out_var[i] = fin[i].w;
    return (int64_t)fin.size();
}
