// pt_ray_range.h -- the persistent loop of the kernels that serve a caller's rays (pt_rays_kernels.h, pt_ao.h): a wave's range of the
// rays, the refill of its idle lanes from that range, and the load of a ray.  Device code, in the anonymous namespace like pt_trace.h's;
// what the launchers check about the ranges is pt_ray_ranges_ok (pt_instance.h).
// LANE REFILL (the persistent "while-while" loop of Aila and Laine 2009, without its atomics): a wave owns the contiguous range
// [blockIdx.x * per_wave, + per_wave) of the rays - a multiple of 64, so what coherence the caller's order has stays inside a wave -
// and `next`, the first ray not handed out yet, is wave-uniform.  Every round: idle = ballot(the lane holds no ray); when at most
// `refill` lanes are still walking, every idle lane takes ray next + (its rank among the idle lanes) and next += popcount(idle).
// Nothing crosses waves.  Then every lane that holds a ray takes ONE step of its walk (quad_walk_step, pt_trace.h), and a lane whose
// ray retires stores its result at once and is idle from the next round on:
//     RayRange R = ray_range(A);
//     const auto start = [&](int i) { hit_reset(h, ray_load(A.rays, i, o, d, inv)); cur = P.root; sp = 0; steps = 0; ray = i; };
//     while (ray_range_refill(R, A.refill, ray < 0, start)) {
//         if (ray >= 0) { one step; the walk has ended: store, ray = -1 - or start the ray's next walk }
//     }
// (`start` is a callable, not a returned index: the ray load then sits inside the refill's own branch, as it did when the loop was
// written out - with the index handed back through a variable the kernels measured 1 to 2 % slower.)
// TERMINATION, read off the code: a lane that holds a ray takes a step of a walk every round, a walk is over after at most 2^20 + 1 steps
// (quad_walk_step) and a ray is a bounded number of walks; a round in which no lane holds a ray either hands out at least one
// (next < end: no lane is walking, which is <= any refill) or leaves the loop; `next` only grows.
#pragma once
#include "pt_trace.h"

namespace {

struct RayRange {
    int next, end; // wave-uniform: the first ray not handed out yet, and the end of the wave's range
};
__device__ __forceinline__ RayRange ray_range(const PtRaysArgs& A)
{
    const long long first = (long long)blockIdx.x * A.per_wave; // < n: the launcher refuses a grid with an empty range
    RayRange R;
    R.next = (int)first;
    R.end = (int)(first + A.per_wave < (long long)A.n ? first + A.per_wave : (long long)A.n);
    return R;
}

// One round's refill.  idle: the lane holds no ray.  start(i): called by every lane that starts on ray i now.  False: every ray of the
// range has been handed out and every lane is idle - the wave is finished.
template <class Start>
__device__ __forceinline__ bool ray_range_refill(RayRange& R, const int refill, const bool idle, Start start)
{
    const unsigned long long m_idle = __ballot(idle);
    const int n_idle = popc64(m_idle);
    if (R.next < R.end) {
        if (PT_WAVE - n_idle <= refill) {
            const long long i = (long long)R.next + rank_in(m_idle); // (64-bit: next may be within 63 of 2^31 - 1)
            if (idle && i < (long long)R.end) start((int)i);
            R.next = (R.end - R.next > n_idle) ? R.next + n_idle : R.end;
        }
    } else if (n_idle == PT_WAVE) {
        return false;
    }
    return true;
}

// Ray i of the caller's table as two 16-byte loads {org, tmax}, {dir, not read}.  Returns the bound of its walk: tmax, or the
// library's own bound for a tmax beyond it, NaN or +inf.
__device__ __forceinline__ float ray_load(const void* rays, int i, v3& o, v3& d, v3& inv)
{
    const f32x4 r0 = ldg4(rays, (size_t)(uint32_t)i * 32), r1 = ldg4(rays, (size_t)(uint32_t)i * 32 + 16);
    o = V(r0.x, r0.y, r0.z);
    d = V(r1.x, r1.y, r1.z);
    inv = ray_inv(d);
    return r0.w < kTMax ? r0.w : kTMax;
}

} // namespace
