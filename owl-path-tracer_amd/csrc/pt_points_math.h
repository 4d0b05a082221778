// pt_points_math.h -- the per-point definition of pt_closest_point (include/mi355pt.h, "point queries: the nearest surface"): the search
// bound, the distance from a point to a box, the closest point of a triangle and the rule by which a triangle replaces the best one.
// ONE copy for the kernel (pt_kernel_points.hip) and its CPU twin (pt_debug_closest_point_host, pt_points_host.cpp, which includes
// pt_device.h with PTD = static inline first).  Arithmetic: the contract of pt_device.h - float32, no contraction (an fma only inside
// dot), correctly rounded division and square root; dot, sqrt_ and max_ are pt_device.h's.
// WHY PRUNING BY THE BOX DISTANCE IS EXACT.  point_box_dist2 and the dd of point_tri are built from the same monotone, correctly
// rounded operations: a subtraction per axis, then dot(a, a) = fma_(a.z, a.z, fma_(a.y, a.y, a.x * a.x)), which grows with every
// |component|.  If the computed q of a triangle lies inside a box, lo <= q <= hi per axis, then fl(x - q) >= fl(x - hi) and
// fl(q - x) >= fl(lo - x), so |fl(x - q)| >= max(lo - x, x - hi, 0) per axis and dd >= dbox BIT FOR BIT.  Every ancestor's box contains
// the leaf's box (the builders pad the same way at every level), so under the PREMISE that the computed q of a triangle lies inside that
// triangle's padded leaf box, a walk that skips a box only when dbox > best (strictly) never skips the winner, nor a triangle that ties
// with it.  The pad is 1e-5 of the scene's measure; q is a vertex (exact), a point p + e * s with 0 <= s <= 1 on an edge (two roundings
// of the coordinates) or a combination (p0 + ab * v) + ac * w in the face; include/mi355pt.h states the domain on which the premise
// holds, and tests/test_closest_point_host.py asserts it on every case it uses.
#pragma once
#include "pt_device.h"

namespace ptd {

constexpr int kPointNoId = 0x7fffffff; // the id the search starts with: every real id is below it

// rmax of the definition: NaN and +inf give the library's bound.  A point with rmax < 0 finds nothing (point_searches).
PTD float point_rmax(float radius) { return radius < kTMax ? radius : kTMax; }
PTD bool point_searches(float rmax) { return !(rmax < 0.0f); }

// Squared distance from x to the box [lo, hi].  An empty slot's box {+inf, +inf} gives +inf.
PTD float point_box_dist2(v3 lo, v3 hi, v3 x)
{
    const v3 a = V(max_(max_(lo.x - x.x, x.x - hi.x), 0.0f), max_(max_(lo.y - x.y, x.y - hi.y), 0.0f), max_(max_(lo.z - x.z, x.z - hi.z), 0.0f));
    return dot(a, a);
}

// The best triangle so far: squared distance, barycentrics (u weighs p1, v weighs p2: pt_ray_hit's convention), global triangle id,
// closest point, and the feature it lies on (0 face, 1 / 2 / 3 vertex p0 / p1 / p2, 4 / 5 / 6 edge p0p1 / p1p2 / p0p2).
struct PointBest {
    float dd, u, v;
    int id;
    v3 q;
    int feature;
};
PTD void point_reset(PointBest& b, float r2) { b.dd = r2; b.u = 0.0f; b.v = 0.0f; b.id = kPointNoId; b.q = vs(0.0f); b.feature = 0; }

// One triangle against the best so far: the closest-point algorithm of the header, steps 1 to 7 in that order.  Every quantity is a
// function of the inputs alone, so all of them are formed first and the steps select: the first step whose condition holds decides,
// which is the sequential reading bit for bit (a quotient of a step that does not decide is never looked at).
PTD void point_tri(v3 p0, v3 p1, v3 p2, int id, v3 x, PointBest& b)
{
    if (p0.x == p1.x && p0.y == p1.y && p0.z == p1.z && p0.x == p2.x && p0.y == p2.y && p0.z == p2.z) return; // collapsed by the sliver rule: never a candidate
    const v3 ab = p1 - p0, ac = p2 - p0, ap = x - p0;
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    const v3 bp = x - p1;
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    const float vc = d1 * d4 - d3 * d2;
    const v3 cp = x - p2;
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    const float vb = d5 * d2 - d1 * d6;
    const float va = d3 * d6 - d5 * d4, e = d4 - d3, f = d5 - d6;
    v3 q;
    float u, v;
    int feature;
    if (d1 <= 0.0f && d2 <= 0.0f) { // 1
        q = p0; u = 0.0f; v = 0.0f; feature = 1;
    } else if (d3 >= 0.0f && d4 <= d3) { // 2
        q = p1; u = 1.0f; v = 0.0f; feature = 2;
    } else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { // 3
        const float s = d1 / (d1 - d3);
        q = p0 + ab * s; u = s; v = 0.0f; feature = 4;
    } else if (d6 >= 0.0f && d5 <= d6) { // 4
        q = p2; u = 0.0f; v = 1.0f; feature = 3;
    } else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { // 5
        const float s = d2 / (d2 - d6);
        q = p0 + ac * s; u = 0.0f; v = s; feature = 6;
    } else if (va <= 0.0f && e >= 0.0f && f >= 0.0f) { // 6
        const float s = e / (e + f);
        q = p1 + (p2 - p1) * s; u = 1.0f - s; v = s; feature = 5;
    } else { // 7
        const float k = 1.0f / ((va + vb) + vc);
        const float fv = vb * k, fw = vc * k;
        q = (p0 + ab * fv) + ac * fw; u = fv; v = fw; feature = 0;
    }
    const v3 d = x - q;
    const float dd = dot(d, d);
    if (dd < b.dd || (dd == b.dd && id < b.id)) { // a NaN dd never wins; a point at exactly dd == r2 is found; ties to the lower id
        b.dd = dd; b.u = u; b.v = v; b.id = id; b.q = q; b.feature = feature;
    }
}

} // namespace ptd
