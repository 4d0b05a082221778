// pt_upsample_host.cpp -- pt_debug_upsample_host: the CPU twin of the upsampling (pt_upsample; kernels: pt_upsample.hip), and what the
// twin and the device path share on the host: the default parameters, the refusals and the host constants.
// The twin compiles the per-pixel definition the kernels compile, pt_filter_math.h with PTD = static inline (pt_device_host.h), and keeps
// the loops around it: prepare over the low pixels, upsample over the high rows.  Rows are spread over all host threads.
#include "pt_device_host.h"
#include "pt_filter_math.h"

#include <vector>

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
    const size_t npx = (size_t)w * (size_t)h;
    std::vector<float4> col(npx), nzb(npx), alb(npx);
    PtUpsampleArgs A{}; // the kernels' arguments, the records on the host
    A.col = col.data();
    A.nz = nzb.data();
    A.alb = alb.data();
    A.w = w; A.h = h; A.W = W; A.H = H;
    A.taps = prm.taps;
    A.flags = prm.flags;
    A.sigma_depth = prm.sigma_depth;
    upsample_constants(prm, w, h, W, H, &A.rx, &A.ry, &A.kn, &A.ka, &A.ir);
    pt_parallel_ranges(npx, [&](size_t lo, size_t hi) { // prepare
        for (size_t i = lo; i < hi; ++i)
            filter_prepare_pixel<kFilterUpsample>(rgb_lo + 3 * i, nullptr, filter_guide_word(aov_lo + 8 * i), filter_guide_word(aov_lo + 8 * i + 4), prm.flags, prm.sigma_depth, col[i], nzb[i], alb[i]);
    });
    pt_parallel_ranges((size_t)H, [&](size_t lo, size_t hi) {
        for (size_t row = lo; row < hi; ++row)
            for (int x = 0; x < W; ++x) {
                const size_t i = row * (size_t)W + (size_t)x;
                const v3 o = upsample_pixel(A, filter_guide_word(aov_hi + 8 * i), filter_guide_word(aov_hi + 8 * i + 4), x, (int)row);
                out_rgb[3 * i] = o.x; out_rgb[3 * i + 1] = o.y; out_rgb[3 * i + 2] = o.z;
                if (out_rgba8) out_rgba8[i] = make_rgba(o);
            }
    });
    return (int64_t)W * (int64_t)H;
}
