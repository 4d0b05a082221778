// pt_ao_math.h -- the per-ray definition of pt_trace_ao (include/mi355pt.h, "ray queries: ambient occlusion") between the closest hit
// and the occlusion walks: the surface at the hit, the facing normal, the k-th occlusion ray and the result.  ONE copy for the kernel
// (pt_ao.h) and its CPU twin (pti::ao_ray_host, pt_aov_host.cpp, which includes pt_device.h with PTD = static inline first).  Nothing is
// restated here: interp3, surface_unit, cross, dot, onb, to_world, sample_cosine_hemisphere and the RNG are pt_device.h's, and the
// expressions of p, ng and ns are pt_trace_surface's (pt_surface.h).  Arithmetic: the contract of pt_device.h.
#pragma once
#include "pt_device.h"

namespace ptd {

constexpr int kAoShadingNormal = 1; // PT_AO_SHADING_NORMAL

struct AoSurface {
    v3 p;        // the hit point: the origin of every occlusion ray, with no offset
    v3 nf;       // the normal the hemisphere stands on, turned against the ray; (+0, +0, +0) if !traced
    bool traced; // false: the chosen normal is (0, 0, 0) - nothing is traced and ao = 1
};

// Steps 2 and 3 at the hit (u, v) of the triangle (p0, p1, p2) with vertex normals (n0, n1, n2); dir: the caller's direction, as given.
PTD AoSurface ao_surface(float u, float v, v3 p0, v3 p1, v3 p2, v3 n0, v3 n1, v3 n2, v3 dir, int flags)
{
    const float bx = u, by = v;
    const float bw = 1.0f - bx - by;
    AoSurface s;
    s.p = interp3(bw, bx, by, p0, p1, p2);
    const v3 nrm = (flags & kAoShadingNormal) ? surface_unit(interp3(bw, bx, by, n0, n1, n2)) : surface_unit(cross(p1 - p0, p2 - p0));
    s.traced = !(nrm.x == 0.0f && nrm.y == 0.0f && nrm.z == 0.0f);
    s.nf = !s.traced ? vs(0.0f) : (dot(nrm, dir) > 0.0f ? -nrm : nrm);
    return s;
}

PTD float ao_thi(float radius) { return radius < kTMax ? radius : kTMax; } // +inf: the library's bound (NaN and <= 0 never get here)

// Step 4: the next occlusion ray's direction; two draws, r1 then r2.  The frame is a function of nf alone, so forming it here, per
// ray, gives the bits of forming it once.
PTD v3 ao_direction(v3 nf, uint32_t& rng)
{
    const float r1 = rng_next(rng);
    const float r2 = rng_next(rng);
    const v3 w = sample_cosine_hemisphere(r1, r2);
    v3 t, b;
    onb(nf, t, b);
    return to_world(t, b, nf, w);
}

// Step 5
PTD float ao_value(int clear, int n_rays) { return (float)clear * (1.0f / (float)n_rays); }

} // namespace ptd
