// pt_aov_host.cpp -- pt_debug_aov_host: the CPU twin of the guide pass (pt_render_aov; kernel: pt_kernel.hip "guide pass"), and
// pt_debug_aov_follow_host, the twin of its follow mode (pt_render_aov_follow; "guide pass, follow mode"), with that mode's parameter checks.
// The twin runs the definition of include/mi355pt.h with the host walk of pt_debug_closest_hit_host_n over the host copies of the
// scene, and with the arithmetic of pt_device.h itself: the header is included here with PTD = static inline (pt_device_host.h), so rng_init, rng_next,
// normalize, lerp3, uv_on_sphere (the polynomial atan2 / asin), tex_nearest and the material row are the functions the kernel
// compiles, run by the CPU under the same contract (binary32, -ffp-contract=off, fma only where spelled, correctly rounded division
// and sqrt).  What is restated here is what the kernel takes from pt_trace.h, which is device code throughout: the camera ray
// (gen_camera_ray) and the miss branch / attribute fetch of shade_hit - each a few lines, once for both twin pixels, cited below.
// pt_debug_aov_rays_host, the twin of the guide pass over a ray image (pt_render_aov_rays), is the follow twin with the camera ray
// replaced by the pixel's ray record (gen_ray_from): ONE follow loop serves both.
// pti::surface_record_host, the record of pt_debug_trace_surface_host (the twin of pt_trace_surface, pt_rays_host.cpp), sits here for
// the same reason: it is pt_surface.h's function with these host forms of the device arithmetic.  So does pti::ao_ray_host, one ray
// of pt_debug_trace_ao_host (the twin of pt_trace_ao): the host walk around pt_ao_math.h, the header the kernel compiles.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "pt_device_host.h"
#include "pt_ao_math.h"

#include "pt_internal.h"

using namespace pti;
using namespace ptd;

namespace {

bool finite_(float x) { return !(isinf_(x) || isnan_(x)); }

struct AovScene {
    const HostScene* s;
    std::vector<int32_t> slot_of; // global triangle id -> leaf-order slot (the host walk reports the id, the records are in leaf order)
    v3 origin, llc, hor, ver;     // the camera
    const pt_ray_gen* rays;       // a ray image's table of W * H records instead (pt_debug_aov_rays_host); null: the camera
    int W, H, n;
    bool wt;
};

// What the two kernels take from pt_trace.h, for both twin pixels.  gen_camera_ray: the direction of the pixel's next sample.
v3 camera_dir(const AovScene& A, int px, int py, uint32_t& rng)
{
    const float rx = rng_next(rng);
    const float ry = rng_next(rng);
    const float su = ((float)px + rx) / (float)A.W;
    const float sv = ((float)py + ry) / (float)A.H;
    return normalize(((A.llc + A.hor * su) + A.ver * sv) - A.origin);
}

// gen_ray_from: the next sample's ray of pixel (px, py) from its record of the ray image - the same two draws, then the record's ray
void table_ray(const AovScene& A, int px, int py, uint32_t& rng, v3& o, v3& d)
{
    const float rx = rng_next(rng);
    const float ry = rng_next(rng);
    const pt_ray_gen& r = A.rays[(size_t)px + (size_t)A.W * (size_t)py];
    o = V(r.org[0], r.org[1], r.org[2]);
    d = normalize((V(r.dir[0], r.dir[1], r.dir[2]) + V(r.du[0], r.du[1], r.du[2]) * rx) + V(r.dv[0], r.dv[1], r.dv[2]) * ry);
}

// shade_hit's miss branch: what a ray along dir sees of the environment
v3 miss_radiance(const HostScene& S, v3 dir)
{
    v3 radiance = vs(0.0f);
    if (S.env.use_map && S.env_map.w > 0) {
        float tu, tv;
        uv_on_sphere(dir, tu, tv);
        radiance = radiance + tex_nearest(S.env_map.px.data(), S.env_map.w, S.env_map.h, tu, tv);
    } else if (S.env.use_auto) {
        radiance = radiance + lerp3(vs(1.0f), V(0.5f, 0.7f, 1.0f), 0.5f * (dir.y + 1.0f));
    } else {
        radiance = radiance + V(S.env.color[0], S.env.color[1], S.env.color[2]);
    }
    return radiance * S.env.intensity;
}

// shade_hit's attribute fetch at the hit (prim, hu, hv): the material row with its texture looked up (unless the surface emits), the
// interpolated normal and whether it is finite
struct AovHit {
    const PtTri* tr;
    Material mat;
    float bw, bx, by;
    v3 v_n;
    bool n_ok, emits;
};
AovHit fetch_hit(const AovScene& A, int32_t prim, float hu, float hv)
{
    const HostScene& S = *A.s;
    const size_t slot = (size_t)A.slot_of[(size_t)prim];
    const PtShade& sh = S.shade[slot];
    AovHit h;
    h.tr = &S.bvh.tris[slot];
    const int mi = h.tr->material;
    h.mat = material_default();
    int32_t tex_slot = -1;
    if (mi >= 0) {
        const float* mp = &S.materials[(size_t)mi * PT_MAT_STRIDE];
        h.mat = material_load(mp);
        std::memcpy(&tex_slot, mp + 17, 4);
    }
    const float bx = hu, by = hv;
    const float bw = 1.0f - bx - by;
    h.bw = bw; h.bx = bx; h.by = by;
    h.v_n = normalize(interp3(bw, bx, by, V(sh.n0[0], sh.n0[1], sh.n0[2]), V(sh.n1[0], sh.n1[1], sh.n1[2]), V(sh.n2[0], sh.n2[1], sh.n2[2])));
    h.n_ok = finite_(h.v_n.x) && finite_(h.v_n.y) && finite_(h.v_n.z);
    h.emits = h.mat.emission > 0.0f;
    if (!h.emits && tex_slot >= 0) {
        const float tu = fma_(by, sh.tc[4], fma_(bx, sh.tc[2], bw * sh.tc[0]));
        const float tv = fma_(by, sh.tc[5], fma_(bx, sh.tc[3], bw * sh.tc[1]));
        const HostTexture& tx = S.textures[(size_t)tex_slot];
        h.mat.base_color = tex_nearest(tx.px.data(), tx.w, tx.h, tu, tv);
    }
    return h;
}

// One pixel: include/mi355pt.h, "guide pass"; the kernel's loop body (pt_aov_kernel) line for line.
void aov_pixel(const AovScene& A, int px, int py, float* y)
{
    const HostScene& S = *A.s;
    uint32_t rng = rng_init((uint32_t)px, (uint32_t)py);
    v3 s_alb = vs(0.0f), s_nrm = vs(0.0f);
    float s_alpha = 0.0f, s_depth = 0.0f;
    for (int k = 0; k < A.n; ++k) {
        const v3 dir = camera_dir(A, px, py, rng);
        const float o[3] = {A.origin.x, A.origin.y, A.origin.z}, d[3] = {dir.x, dir.y, dir.z};
        float t = 0.0f, hu = 0.0f, hv = 0.0f;
        int32_t prim = -1;
        const bool hit = pt_bvh_closest_hit_host(S.bvh, o, d, kTMin, kTMax, &t, &hu, &hv, &prim, A.wt);
        v3 alb, nrm = vs(0.0f);
        float alpha = 0.0f, depth = 0.0f;
        if (!hit) {
            alb = miss_radiance(S, dir);
        } else {
            const AovHit h = fetch_hit(A, prim, hu, hv);
            if (h.n_ok) nrm = h.v_n;
            alb = h.emits ? vs(h.mat.emission) : h.mat.base_color;
            alpha = 1.0f;
            depth = t;
        }
        s_alb = s_alb + alb; s_alpha = s_alpha + alpha;
        s_nrm = s_nrm + nrm; s_depth = s_depth + depth;
    }
    const float inv_n = 1.0f / (float)A.n;
    y[0] = s_alb.x * inv_n; y[1] = s_alb.y * inv_n; y[2] = s_alb.z * inv_n; y[3] = s_alpha * inv_n;
    y[4] = s_nrm.x * inv_n; y[5] = s_nrm.y * inv_n; y[6] = s_nrm.z * inv_n; y[7] = s_depth * inv_n;
}

// Follow mode, one pixel: include/mi355pt.h, "guide pass, follow mode"; the loop of pt_aov_follow_kernel and aov_follow_surface line for line.
enum { AOV_NONE = 0, AOV_MIRROR = 1, AOV_GLASS = 2 };
int aov_classify(const Material& m, float roughness_max) // sample_disney's lobe weights
{
    const float dw = (1.0f - m.specular_transmission) * (1.0f - m.metallic);
    const float mw = m.metallic;
    const float cw = 0.25f * m.clearcoat;
    const float gw = (1.0f - m.metallic) * m.specular_transmission;
    if (mw > gw && mw > dw && mw > cw && m.roughness <= roughness_max) return AOV_MIRROR;
    if (gw > mw && gw > dw && gw > cw && m.specular_transmission_roughness <= roughness_max) return AOV_GLASS;
    return AOV_NONE;
}

void aov_follow_pixel(const AovScene& A, const pt_aov_params& prm, int px, int py, float* y)
{
    const HostScene& S = *A.s;
    uint32_t rng = rng_init((uint32_t)px, (uint32_t)py);
    v3 s_alb = vs(0.0f), s_nrm = vs(0.0f);
    float s_alpha = 0.0f, s_depth = 0.0f;
    for (int k = 0; k < A.n; ++k) {
        v3 o = A.origin, d;
        if (A.rays) table_ray(A, px, py, rng, o, d); // (pt_aov_rays_kernel: the one difference)
        else d = camera_dir(A, px, py, rng);
        v3 tint = vs(1.0f), alb = vs(0.0f), nrm = vs(0.0f);
        float dist = 0.0f, alpha = 0.0f, depth = 0.0f;
        for (int step = 0;; ++step) {
            const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
            float t = 0.0f, hu = 0.0f, hv = 0.0f;
            int32_t prim = -1;
            const bool hit = pt_bvh_closest_hit_host(S.bvh, of, df, kTMin, kTMax, &t, &hu, &hv, &prim, A.wt);
            if (step == 0) alpha = hit ? 1.0f : 0.0f; // coverage stays first-hit
            if (!hit) {
                alb = tint * miss_radiance(S, d);
                nrm = vs(0.0f);
                depth = dist;
                break;
            }
            dist = dist + t;
            const AovHit h = fetch_hit(A, prim, hu, hv);
            const Material& mat = h.mat;
            const v3 v_n = h.v_n;
            const int kind = (h.emits || step == prm.max_follow || !h.n_ok) ? (int)AOV_NONE : aov_classify(mat, prm.roughness_max);
            if (kind != AOV_NONE) {
                const v3 wo = -d;
                v3 wi = vs(0.0f), t2 = tint * mat.base_color;
                bool through = false;
                if (kind == AOV_GLASS) {
                    const float ct = dot(wo, v_n);
                    through = ct > 0.0f ? refract(wo, v_n, 1.0f / mat.ior, wi) : refract(wo, -v_n, mat.ior, wi);
                }
                if (through) t2 = tint * V(sqrt_(mat.base_color.x), sqrt_(mat.base_color.y), sqrt_(mat.base_color.z));
                else wi = reflect(wo, v_n); // a mirror, or total internal reflection
                const v3 dn = normalize(wi);
                if (finite_(dn.x) && finite_(dn.y) && finite_(dn.z)) {
                    const PtTri& tr = *h.tr;
                    o = interp3(h.bw, h.bx, h.by, V(tr.p0[0], tr.p0[1], tr.p0[2]), V(tr.p1[0], tr.p1[1], tr.p1[2]), V(tr.p2[0], tr.p2[1], tr.p2[2])); // shade_hit's v_p
                    d = dn;
                    tint = t2;
                    continue;
                }
            }
            alb = tint * (h.emits ? vs(mat.emission) : mat.base_color);
            nrm = h.n_ok ? v_n : vs(0.0f);
            depth = dist;
            break;
        }
        s_alb = s_alb + alb; s_alpha = s_alpha + alpha;
        s_nrm = s_nrm + nrm; s_depth = s_depth + depth;
    }
    const float inv_n = 1.0f / (float)A.n;
    y[0] = s_alb.x * inv_n; y[1] = s_alb.y * inv_n; y[2] = s_alb.z * inv_n; y[3] = s_alpha * inv_n;
    y[4] = s_nrm.x * inv_n; y[5] = s_nrm.y * inv_n; y[6] = s_nrm.z * inv_n; y[7] = s_depth * inv_n;
}

// What both twins take: the argument checks of pt_debug_aov_host, the scene's host copies, the slot table
int64_t aov_host(pt_ctx* c, const pt_camera* cam, const pt_ray_gen* rays, int32_t W, int32_t H, int32_t n_samples, const uint32_t* pixel_ids, int64_t n_pixels, float* out,
                 const pt_aov_params* follow, const char* who);

} // namespace

namespace pti {
// What pt_render_aov_follow, its device form and the twin refuse alike, before anything is touched; *eff = the parameters in effect.
int check_aov_params(pt_ctx* c, const pt_aov_params* p, const char* who, pt_aov_params* eff)
{
    if (p) *eff = *p;
    else pt_aov_default_params(eff);
    if (eff->n_samples < 1) return fail(c, PT_E_INVALID, "%s: n_samples %d must be >= 1", who, eff->n_samples);
    if (eff->max_follow < 0 || eff->max_follow > 8) return fail(c, PT_E_INVALID, "%s: max_follow %d outside 0..8", who, eff->max_follow);
    if (!(eff->roughness_max >= 0.0f && eff->roughness_max <= 1.0f)) return fail(c, PT_E_INVALID, "%s: roughness_max %g outside 0..1", who, (double)eff->roughness_max);
    if (eff->reserved != 0) return fail(c, PT_E_INVALID, "%s: reserved must be 0 (got %d)", who, eff->reserved);
    return PT_OK;
}
} // namespace pti

extern "C" void pt_aov_default_params(pt_aov_params* p)
{
    if (!p) return;
    p->n_samples = 1;
    p->max_follow = 4;
    p->roughness_max = 0.3f;
    p->reserved = 0;
}

extern "C" int64_t pt_debug_aov_follow_host(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, const pt_aov_params* p, const uint32_t* pixel_ids, int64_t n_pixels, float* out)
{
    if (!c || !cam || !out || n_pixels < 0 || (n_pixels > 0 && !pixel_ids)) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "no geometries (pt_upload_scene not called)");
    pt_aov_params prm;
    const int rc = check_aov_params(c, p, "pt_debug_aov_follow_host", &prm);
    if (rc) return rc;
    return aov_host(c, cam, nullptr, W, H, prm.n_samples, pixel_ids, n_pixels, out, &prm, "pt_debug_aov_follow_host");
}

extern "C" int64_t pt_debug_aov_rays_host(pt_ctx* c, const pt_ray_gen* rays, int32_t W, int32_t H, const pt_aov_params* p, const uint32_t* pixel_ids, int64_t n_pixels, float* out)
{
    if (!c) return PT_E_INVALID;
    if (n_pixels < 0 || (n_pixels > 0 && !pixel_ids)) return fail(c, PT_E_INVALID, "pt_debug_aov_rays_host: %lld pixels%s", (long long)n_pixels, pixel_ids ? "" : ", pixel_ids NULL");
    int rc;
    if ((rc = check_ray_ptrs(c, "pt_debug_aov_rays_host", rays, out, "out", false))) return rc;
    pt_aov_params prm;
    if ((rc = check_aov_params(c, p, "pt_debug_aov_rays_host", &prm))) return rc;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_debug_aov_rays_host: no geometries (pt_upload_scene not called)");
    return aov_host(c, nullptr, rays, W, H, prm.n_samples, pixel_ids, n_pixels, out, &prm, "pt_debug_aov_rays_host");
}

extern "C" int64_t pt_debug_aov_host(pt_ctx* c, const pt_camera* cam, int32_t W, int32_t H, int32_t n_samples, const uint32_t* pixel_ids, int64_t n_pixels, float* out)
{
    if (!c || !cam || !out || n_pixels < 0 || (n_pixels > 0 && !pixel_ids)) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "no geometries (pt_upload_scene not called)");
    return aov_host(c, cam, nullptr, W, H, n_samples, pixel_ids, n_pixels, out, nullptr, "pt_debug_aov_host");
}

std::vector<int32_t> pti::slot_of_prim(const HostScene& S)
{
    std::vector<int32_t> slot_of((size_t)S.n_triangles, -1);
    for (size_t s = 0; s < S.bvh.tris.size(); ++s) {
        const int32_t id = S.bvh.tris[s].id;
        if (id >= 0 && (size_t)id < slot_of.size()) slot_of[(size_t)id] = (int32_t)s; // (padding slots carry id 0x7fffffff)
    }
    return slot_of;
}

// surface_record of pt_surface.h over the host copies (pt_debug_trace_surface_host, pt_rays_host.cpp), line for line.
void pti::surface_record_host(const HostScene& S, int32_t slot, float t, float u, float v, int32_t prim, pt_surface* out)
{
    std::memset(out, 0, sizeof *out); // a miss: {+0, +0, +0, -1}, p = +0, material = -1, every remaining word +0
    out->prim = -1;
    out->material = -1;
    if (slot < 0) return;
    const PtTri& tr = S.bvh.tris[(size_t)slot];
    const PtShade& sh = S.shade[(size_t)slot];
    const int mi = tr.material;
    Material mat = material_default();
    int32_t tex_slot = -1;
    if (mi >= 0) {
        const float* mp = &S.materials[(size_t)mi * PT_MAT_STRIDE];
        mat = material_load(mp);
        std::memcpy(&tex_slot, mp + 17, 4);
    }
    const float bx = u, by = v;
    const float bw = 1.0f - bx - by;
    const v3 p0 = V(tr.p0[0], tr.p0[1], tr.p0[2]), p1 = V(tr.p1[0], tr.p1[1], tr.p1[2]), p2 = V(tr.p2[0], tr.p2[1], tr.p2[2]);
    const v3 v_p = interp3(bw, bx, by, p0, p1, p2);
    const v3 v_ns = surface_unit(interp3(bw, bx, by, V(sh.n0[0], sh.n0[1], sh.n0[2]), V(sh.n1[0], sh.n1[1], sh.n1[2]), V(sh.n2[0], sh.n2[1], sh.n2[2])));
    const v3 v_ng = surface_unit(cross(p1 - p0, p2 - p0));
    const float tu = fma_(by, sh.tc[4], fma_(bx, sh.tc[2], bw * sh.tc[0]));
    const float tv = fma_(by, sh.tc[5], fma_(bx, sh.tc[3], bw * sh.tc[1]));
    if (tex_slot >= 0) {
        const HostTexture& tx = S.textures[(size_t)tex_slot];
        mat.base_color = tex_nearest(tx.px.data(), tx.w, tx.h, tu, tv);
    }
    out->t = t; out->u = u; out->v = v; out->prim = prim;
    out->p[0] = v_p.x; out->p[1] = v_p.y; out->p[2] = v_p.z; out->material = mi;
    out->ng[0] = v_ng.x; out->ng[1] = v_ng.y; out->ng[2] = v_ng.z; out->tu = tu;
    out->ns[0] = v_ns.x; out->ns[1] = v_ns.y; out->ns[2] = v_ns.z; out->tv = tv;
    out->base[0] = mat.base_color.x; out->base[1] = mat.base_color.y; out->base[2] = mat.base_color.z; out->emission = mat.emission;
}

// One ray of pt_debug_trace_ao_host (pt_rays_host.cpp): include/mi355pt.h, "ray queries: ambient occlusion", steps 1 to 5, with every
// expression between the walks taken from pt_ao_math.h as the kernel takes it (pt_ao.h).
void pti::ao_ray_host(const HostScene& S, const std::vector<int32_t>& slot_of, bool wt, const pt_ray& r, uint32_t index, const pt_ao_params& prm, pt_ao_hit* out,
                      pt_ray* out_rays)
{
    *out = pt_ao_hit{0.0f, 0.0f, 0.0f, -1, {0.0f, 0.0f, 0.0f}, 1.0f};
    // a ray without occlusion rays: K records that nothing occludes (an empty interval), so that the count of clear records is ao * K
    for (int k = 0; out_rays && k < prm.n_rays; ++k) out_rays[k] = pt_ray{{0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 1.0f}, 0.0f};
    const float thi0 = r.tmax < kTMax ? r.tmax : kTMax; // NaN and +inf: the library's own bound
    float t = 0.0f, u = 0.0f, v = 0.0f;
    int32_t prim = -1;
    if (!pt_bvh_closest_hit_host(S.bvh, r.org, r.dir, kTMin, thi0, &t, &u, &v, &prim, wt)) return;
    const size_t slot = (size_t)slot_of[(size_t)prim];
    const PtTri& tr = S.bvh.tris[slot];
    const PtShade& sh = S.shade[slot];
    const AoSurface s = ao_surface(u, v, V(tr.p0[0], tr.p0[1], tr.p0[2]), V(tr.p1[0], tr.p1[1], tr.p1[2]), V(tr.p2[0], tr.p2[1], tr.p2[2]), V(sh.n0[0], sh.n0[1], sh.n0[2]),
                                   V(sh.n1[0], sh.n1[1], sh.n1[2]), V(sh.n2[0], sh.n2[1], sh.n2[2]), V(r.dir[0], r.dir[1], r.dir[2]), prm.flags);
    out->t = t; out->u = u; out->v = v; out->prim = prim;
    out->n[0] = s.nf.x; out->n[1] = s.nf.y; out->n[2] = s.nf.z;
    if (!s.traced) return;
    uint32_t rng = rng_init(index, prm.seed);
    const float thi = ao_thi(prm.radius);
    const float org[3] = {s.p.x, s.p.y, s.p.z};
    int clear = 0;
    for (int k = 0; k < prm.n_rays; ++k) {
        const v3 d = ao_direction(s.nf, rng);
        const float dir[3] = {d.x, d.y, d.z};
        float t2 = 0.0f, u2 = 0.0f, v2 = 0.0f;
        int32_t prim2 = -1;
        clear += pt_bvh_closest_hit_host(S.bvh, org, dir, kTMin, thi, &t2, &u2, &v2, &prim2, wt) ? 0 : 1;
        if (out_rays) out_rays[k] = pt_ray{{org[0], org[1], org[2]}, thi, {dir[0], dir[1], dir[2]}, 0.0f};
    }
    out->ao = ao_value(clear, prm.n_rays);
}

namespace {
int64_t aov_host(pt_ctx* c, const pt_camera* cam, const pt_ray_gen* rays, int32_t W, int32_t H, int32_t n_samples, const uint32_t* pixel_ids, int64_t n_pixels, float* out,
                 const pt_aov_params* follow, const char* who)
{
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || n_samples <= 0 || (int64_t)W * H > (int64_t)0x7fffffff)
        return fail(c, PT_E_INVALID, "bad guide pass size %dx%d, %d samples", W, H, n_samples);
    for (int64_t i = 0; i < n_pixels; ++i)
        if (pixel_ids[i] >= (uint32_t)W * (uint32_t)H) return fail(c, PT_E_INVALID, "%s: pixel id %u outside the %dx%d frame", who, pixel_ids[i], W, H);
    int rc;
    if (rays && (rc = check_ray_table(c, who, rays, W, H, false, false))) return rc; // the records, as the blocking form
    sync_host_scene(c);
    AovScene A;
    A.s = &c->scene;
    A.rays = rays;
    A.origin = A.llc = A.hor = A.ver = vs(0.0f);
    if (cam) {
        A.origin = V(cam->origin[0], cam->origin[1], cam->origin[2]); A.llc = V(cam->llc[0], cam->llc[1], cam->llc[2]);
        A.hor = V(cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]); A.ver = V(cam->vertical[0], cam->vertical[1], cam->vertical[2]);
    }
    A.W = W; A.H = H; A.n = n_samples;
    A.wt = c->opt.watertight != 0; // the walk follows the option as the render does
    A.slot_of = slot_of_prim(c->scene);
    pt_parallel_ranges((size_t)n_pixels, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const int px = (int)(pixel_ids[i] % (uint32_t)W), py = (int)(pixel_ids[i] / (uint32_t)W);
            if (follow) aov_follow_pixel(A, *follow, px, py, out + 8 * i);
            else aov_pixel(A, px, py, out + 8 * i);
        }
    });
    return n_pixels;
}
} // namespace
