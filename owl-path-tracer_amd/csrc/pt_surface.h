// pt_surface.h -- the surface record of pt_trace_surface (include/mi355pt.h, "ray queries: the surface at the hit"): what lies at a
// closest hit, from the records shade_hit reads and through the functions it reads them with (interp3, material_load,
// material_default, tex_nearest of pt_trace.h / pt_device.h; cross and normalize of pt_device.h).  One function, used by the surface
// instances of the ray kernels (pt_rays_kernels.h under PT_RAYS_SURFACE = 1) when a lane's walk has ended; its CPU twin is
// pti::surface_record_host (pt_aov_host.cpp), expression for expression.
// The fetch is two dependent rounds, as shade_hit's: the three 16-byte loads of PtTri and the four of PtShade (the triangle record
// repeats the material index), then the material row's five words and the texel.
// SURFACE MODE of pt_rays_kernels.h: the closest-hit walk, the lane refill, the bounds and the launcher checks as they are; a lane
// whose walk has ended stores this record - five 16-byte stores at out + ray * 80 - where the closest-hit instance stores 16 bytes.  Two
// instances per unit (EXACT 0 / 1): there is no occlusion form, and occluded = 1 answers hipErrorInvalidValue.  The names of that mode's
// kernel, launcher and geometry function are chosen here, so that pt_rays_kernels.h keeps its kernel on the source line the resource
// reports of `make asm-rays` name.
#pragma once
#include "pt_instance.h"
#include "pt_trace.h"
#if PT_WATERTIGHT
#define PT_RAYS_KERNEL pt_rays_surface_wt_kernel
#define PT_RAYS_LAUNCH pt_launch_rays_surface_wt
#define PT_RAYS_GEOMETRY pt_rays_surface_geometry_wt
#else
#define PT_RAYS_KERNEL pt_rays_surface_kernel
#define PT_RAYS_LAUNCH pt_launch_rays_surface
#define PT_RAYS_GEOMETRY pt_rays_surface_geometry
#endif
namespace {
// The 80 bytes of a pt_surface, as the five 16-byte stores they leave as.
struct SurfaceRecord {
    f32x4 hit;  // {t, u, v, prim}: pt_trace_closest's record of the ray
    f32x4 p;    // {hit point, material index}
    f32x4 ng;   // {geometric normal, texcoord u}
    f32x4 ns;   // {shading normal, texcoord v}
    f32x4 base; // {base colour after the texture lookup, emission}
};
// surface_unit(a):
//     normalize, or (0, 0, 0) where that has a component that is not finite (aov_sample's rule),
// is pt_device.h's ("the surface at a hit"), shared with ambient occlusion (pt_ao_math.h) and the
// CPU twins.  (This note takes the lines the function took: pt_rays_kernels.h, which includes
// this header in surface mode, keeps its kernel on its source line.)
// slot < 0: a miss.  (u, v, t, id) are the walk's Hit; slot is its leaf-order index, which serves PtTri and PtShade alike.
__device__ __forceinline__ SurfaceRecord surface_record(const PtKernelParams& P, int slot, float u, float v, float t, int id)
{
    SurfaceRecord r;
    r.hit = (f32x4){0.0f, 0.0f, 0.0f, __int_as_float(-1)};
    r.p = (f32x4){0.0f, 0.0f, 0.0f, __int_as_float(-1)};
    r.ng = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    r.ns = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    r.base = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    if (slot < 0) return r;
    const size_t tb = (size_t)(uint32_t)slot * sizeof(PtTri);
    const f32x4 a = ldg4(P.tris, tb), b = ldg4(P.tris, tb + 16), c = ldg4(P.tris, tb + 32); // c = {p2.z, id, material, pad}
    const size_t sb = (size_t)(uint32_t)slot * sizeof(PtShade);
    const f32x4 s0 = ldg4(P.shade, sb), s1 = ldg4(P.shade, sb + 16), s2 = ldg4(P.shade, sb + 32), s3 = ldg4(P.shade, sb + 48);
    const int mi = __float_as_int(c.z);
    Material mat = material_default();
    int tex_slot = -1;
    if (mi >= 0) {
        const float PT_AS1* mp = gp(P.materials) + mi * PT_MAT_STRIDE;
        mat = material_load(mp); // (base colour and emission are read; the other words are never loaded)
        tex_slot = __float_as_int(mp[17]);
    }
    const float bx = u, by = v;
    const float bw = 1.0f - bx - by;
    const v3 p0 = V(a.x, a.y, a.z), p1 = V(a.w, b.x, b.y), p2 = V(b.z, b.w, c.x);
    const v3 v_p = interp3(bw, bx, by, p0, p1, p2); // shade_hit's v_p: no normal offset
    const v3 v_ns = surface_unit(interp3(bw, bx, by, V(s0.x, s0.y, s0.z), V(s0.w, s1.x, s1.y), V(s1.z, s1.w, s2.x)));
    const v3 v_ng = surface_unit(cross(p1 - p0, p2 - p0)); // the index order's orientation; not flipped towards the ray
    const float tu = fma_(by, s3.z, fma_(bx, s3.x, bw * s2.z));
    const float tv = fma_(by, s3.w, fma_(bx, s3.y, bw * s2.w));
    if (tex_slot >= 0) { // whether or not the material emits
        const PtTexDesc PT_AS1* tdp = gp(P.textures) + tex_slot;
        mat.base_color = tex_nearest(gp(tdp->texels), tdp->width, tdp->height, tu, tv);
    }
    r.hit = (f32x4){t, u, v, __int_as_float(id)};
    r.p = (f32x4){v_p.x, v_p.y, v_p.z, c.z};
    r.ng = (f32x4){v_ng.x, v_ng.y, v_ng.z, tu};
    r.ns = (f32x4){v_ns.x, v_ns.y, v_ns.z, tv};
    r.base = (f32x4){mat.base_color.x, mat.base_color.y, mat.base_color.z, mat.emission};
    return r;
}
} // namespace
