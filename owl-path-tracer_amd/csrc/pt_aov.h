// pt_aov.h -- what the guide kernels share (pt_aov_first.h: pt_render_aov; pt_aov_follow.h: pt_render_aov_follow and pt_render_aov_batch):
// their register budget, finite_ and what one first-hit sample contributes.  Units of their own beside the render kernel (whose
// instances sit at their register budgets: no room for seven more accumulators per slot), so that the render units hold the kernels
// they always held (tests/test_watertight_host.py counts them); they take the device code of pt_trace.h and nothing of pt_kernel.hip.
#pragma once
#include "pt_instance.h"
#include "pt_trace.h"
#ifndef PT_AOV_WAVES_PER_EU
#define PT_AOV_WAVES_PER_EU 4 // 128 VGPRs, 16 waves per CU at 3 KB of LDS each
#endif
namespace {
__device__ __forceinline__ bool finite_(float x) { return !(isinf_(x) || isnan_(x)); }
// What one sample contributes: tslot < 0 = miss.  The miss branch and the attribute fetch are shade_hit's, expression for expression.
__device__ __forceinline__ void aov_sample(const PtKernelParams& P, int tslot, float hu, float hv, float ht, v3 dir, v3& albedo, float& alpha, v3& normal, float& depth)
{
    if (tslot < 0) {
        v3 radiance = vs(0.0f);
        if (P.env_use_map && P.env_map.width > 0) {
            float tu, tv;
            uv_on_sphere(dir, tu, tv);
            radiance = radiance + tex_nearest(gp(P.env_map.texels), P.env_map.width, P.env_map.height, tu, tv);
        } else if (P.env_use_auto) {
            radiance = radiance + lerp3(vs(1.0f), V(0.5f, 0.7f, 1.0f), 0.5f * (dir.y + 1.0f));
        } else {
            radiance = radiance + V(P.env_color[0], P.env_color[1], P.env_color[2]);
        }
        albedo = radiance * P.env_intensity;
        alpha = 0.0f; normal = vs(0.0f); depth = 0.0f;
        return;
    }
    const f32x4 c = ldg4(P.tris, (size_t)(uint32_t)tslot * sizeof(PtTri) + 32); // {p2.z, id, material, pad}
    const size_t sb = (size_t)(uint32_t)tslot * sizeof(PtShade);
    const f32x4 s0 = ldg4(P.shade, sb), s1 = ldg4(P.shade, sb + 16), s2 = ldg4(P.shade, sb + 32), s3 = ldg4(P.shade, sb + 48);
    const int mi = __float_as_int(c.z);
    Material mat = material_default();
    int tex_slot = -1;
    if (mi >= 0) {
        const float PT_AS1* mp = gp(P.materials) + mi * PT_MAT_STRIDE;
        mat = material_load(mp);
        tex_slot = __float_as_int(mp[17]);
    }
    const float bx = hu, by = hv;
    const float bw = 1.0f - bx - by;
    const v3 v_n = normalize(interp3(bw, bx, by, V(s0.x, s0.y, s0.z), V(s0.w, s1.x, s1.y), V(s1.z, s1.w, s2.x)));
    normal = (finite_(v_n.x) && finite_(v_n.y) && finite_(v_n.z)) ? v_n : vs(0.0f); // not flipped towards the viewer; emitters have one too
    if (mat.emission > 0.0f) {
        albedo = vs(mat.emission);
    } else {
        if (tex_slot >= 0) {
            const float tu = fma_(by, s3.z, fma_(bx, s3.x, bw * s2.z));
            const float tv = fma_(by, s3.w, fma_(bx, s3.y, bw * s2.w));
            const PtTexDesc PT_AS1* tdp = gp(P.textures) + tex_slot;
            mat.base_color = tex_nearest(gp(tdp->texels), tdp->width, tdp->height, tu, tv);
        }
        albedo = mat.base_color;
    }
    alpha = 1.0f;
    depth = ht;
}
} // namespace
