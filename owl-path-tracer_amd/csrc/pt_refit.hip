// pt_refit.hip -- pt_update_vertices on the device: new vertices into the leaf-order records and new boxes into the three hierarchies of
// an uploaded scene, topology untouched (option "dynamic"; DESIGN.md 4 "Refit").  Four steps, plain 256-thread kernels, no atomics and
// no fences: the order between a node and its children is the order of the launches.
//   1. gather     one thread per leaf-order triangle slot: the three vertices through the retained indices, the sliver rule, p0..p2 of
//                 PtTri (and n0..n2 of PtShade when normals came with the update)
//   2. extent     two-stage min / max over the collapsed triangles -> pad = ext * 1e-5f, ext as pt_bvh_build forms it; stays in HBM
//   3. refit      one launch per height level of the binary tree, lowest first, one thread per node: a leaf child takes the bounds of its
//                 triangles -/+ pad, an internal child the union of the child node's two stored boxes
//   4. propagate  one thread per quad slot and per oct slot: the box of the binary (node, side) it is a copy of
// The host twin is pt_bvh_refit (pt_bvh.cpp) + the gather of pt_scene.cpp: the arrays must agree byte for byte (tests/test_gpu_refit.py).
#include <hip/hip_runtime.h>
#include <math.h>

#include "pt_launch.h"

#pragma clang fp contract(off) // the sliver rule is the host's expression sequence: nothing may fuse

namespace {

constexpr int kBlock = 256;

__device__ inline float rmin(float a, float b) { return b < a ? b : a; } // as pt_bvh.cpp (the vertices are finite after the sliver rule)
__device__ inline float rmax(float a, float b) { return b > a ? b : a; }
__device__ inline bool finite3(const float* q) { return fabsf(q[0]) < INFINITY && fabsf(q[1]) < INFINITY && fabsf(q[2]) < INFINITY; }

// pt_collapse_sliver of pt_scene.cpp, restated: the same double-precision expressions in the same order
__device__ inline void collapse_sliver(float* p)
{
    const double e1[3] = {(double)p[3] - (double)p[0], (double)p[4] - (double)p[1], (double)p[5] - (double)p[2]};
    const double e2[3] = {(double)p[6] - (double)p[0], (double)p[7] - (double)p[1], (double)p[8] - (double)p[2]};
    const double e3[3] = {(double)p[6] - (double)p[3], (double)p[7] - (double)p[4], (double)p[8] - (double)p[5]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double l1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], l2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2], l3 = e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2];
    const double L2 = l1 > l2 ? (l1 > l3 ? l1 : l3) : (l2 > l3 ? l2 : l3);
    if (!(n2 > 1e-10 * L2 * L2)) { // also NaN / infinite vertices: to the first finite corner, else the origin
        int f = 0;
        while (f < 3 && !finite3(p + 3 * f)) ++f;
        const float q[3] = {f < 3 ? p[3 * f] : 0.0f, f < 3 ? p[3 * f + 1] : 0.0f, f < 3 ? p[3 * f + 2] : 0.0f};
        for (int k = 0; k < 9; ++k) p[k] = q[k % 3];
    }
}

__global__ __launch_bounds__(kBlock) void refit_gather(PtTri* tris, PtShade* shade, const float* verts, const float* normals, const int32_t* tri_vi, int n_slots)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n_slots) return;
    PtTri& t = tris[i];
    if (t.id == 0x7fffffff) return; // leaf_align padding: a never-hit record, no vertices
    const int32_t* vi = tri_vi + 4 * (size_t)i;
    float p[9];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) p[3 * k + a] = verts[3 * (size_t)vi[k] + a];
    collapse_sliver(p);
    for (int a = 0; a < 3; ++a) { t.p0[a] = p[a]; t.p1[a] = p[3 + a]; t.p2[a] = p[6 + a]; }
    if (normals) {
        PtShade& s = shade[i];
        const long long nb = vi[3]; // normal base - vertex base of the slot's mesh
        for (int a = 0; a < 3; ++a) {
            s.n0[a] = normals[3 * (size_t)(vi[0] + nb) + a];
            s.n1[a] = normals[3 * (size_t)(vi[1] + nb) + a];
            s.n2[a] = normals[3 * (size_t)(vi[2] + nb) + a];
        }
    }
}

// Workspace (floats / uint32 words): [0] pad, [1] triangles that are points (collapsed slivers), then 8 words per partial of stage one:
// min xyz, max xyz, point count, unused.
struct Extent {
    float mn[3], mx[3];
    uint32_t points;
};

__device__ inline void extent_reset(Extent& e)
{
    for (int a = 0; a < 3; ++a) { e.mn[a] = INFINITY; e.mx[a] = -INFINITY; }
    e.points = 0;
}

// all threads of the block call this; thread 0 returns the block's result
__device__ inline Extent extent_block_reduce(Extent e)
{
    __shared__ float s_v[6][kBlock];
    __shared__ uint32_t s_c[kBlock];
    const int tid = (int)threadIdx.x;
    for (int a = 0; a < 3; ++a) { s_v[a][tid] = e.mn[a]; s_v[3 + a][tid] = e.mx[a]; }
    s_c[tid] = e.points;
    __syncthreads();
    for (int st = kBlock / 2; st > 0; st >>= 1) {
        if (tid < st) {
            for (int a = 0; a < 3; ++a) {
                s_v[a][tid] = rmin(s_v[a][tid], s_v[a][tid + st]);
                s_v[3 + a][tid] = rmax(s_v[3 + a][tid], s_v[3 + a][tid + st]);
            }
            s_c[tid] += s_c[tid + st];
        }
        __syncthreads();
    }
    Extent r;
    for (int a = 0; a < 3; ++a) { r.mn[a] = s_v[a][0]; r.mx[a] = s_v[3 + a][0]; }
    r.points = s_c[0];
    return r;
}

__global__ __launch_bounds__(kBlock) void refit_extent_partial(const PtTri* tris, int n_slots, float* ws)
{
    Extent e;
    extent_reset(e);
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n_slots; i += (long long)gridDim.x * kBlock) {
        const PtTri& t = tris[i];
        if (t.id == 0x7fffffff) continue;
        bool point = true;
        for (int a = 0; a < 3; ++a) {
            e.mn[a] = rmin(e.mn[a], rmin(t.p0[a], rmin(t.p1[a], t.p2[a])));
            e.mx[a] = rmax(e.mx[a], rmax(t.p0[a], rmax(t.p1[a], t.p2[a])));
            point = point && t.p0[a] == t.p1[a] && t.p0[a] == t.p2[a];
        }
        e.points += point ? 1u : 0u;
    }
    const Extent r = extent_block_reduce(e);
    if (threadIdx.x == 0) {
        float* out = ws + 8 + 8 * (size_t)blockIdx.x;
        for (int a = 0; a < 3; ++a) { out[a] = r.mn[a]; out[3 + a] = r.mx[a]; }
        out[6] = __uint_as_float(r.points);
        out[7] = 0.0f;
    }
}

__global__ __launch_bounds__(kBlock) void refit_extent_final(float* ws, int n_partials)
{
    Extent e;
    extent_reset(e);
    for (int k = (int)threadIdx.x; k < n_partials; k += kBlock) {
        const float* in = ws + 8 + 8 * (size_t)k;
        for (int a = 0; a < 3; ++a) { e.mn[a] = rmin(e.mn[a], in[a]); e.mx[a] = rmax(e.mx[a], in[3 + a]); }
        e.points += __float_as_uint(in[6]);
    }
    const Extent r = extent_block_reduce(e);
    if (threadIdx.x == 0) {
        float ext = 0.0f;
        if (r.mn[0] <= r.mx[0]) // (no live triangle: pad 0)
            for (int a = 0; a < 3; ++a) { // exactly as pt_bvh_build
                ext = rmax(ext, r.mx[a] - r.mn[a]);
                ext = rmax(ext, rmax(fabsf(r.mn[a]), fabsf(r.mx[a])));
            }
        ws[0] = ext * 1e-5f;
        ws[1] = __uint_as_float(r.points);
    }
}

__global__ __launch_bounds__(kBlock) void refit_level(PtNode* nodes, const PtTri* tris, const int32_t* list, int count, const float* ws)
{
    const int k = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (k >= count) return;
    const float pad = ws[0];
    PtNode& nd = nodes[list[k]];
    for (int side = 0; side < 2; ++side) {
        const int32_t c = side ? nd.right : nd.left;
        if (c >= 0) { // internal child (a lower level, an earlier launch): the union of its two stored boxes, no further pad
            const PtNode& cn = nodes[c];
            for (int a = 0; a < 3; ++a) { nd.lo[a][side] = rmin(cn.lo[a][0], cn.lo[a][1]); nd.hi[a][side] = rmax(cn.hi[a][0], cn.hi[a][1]); }
        } else if (c < -1) { // leaf child: the bounds of its triangles, -/+ pad
            const uint32_t code = ~(uint32_t)c, first = code >> 3, n = code & 7u;
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (uint32_t i = first; i < first + n; ++i) {
                const PtTri& t = tris[i];
                if (t.id == 0x7fffffff) continue;
                for (int a = 0; a < 3; ++a) {
                    mn[a] = rmin(mn[a], rmin(t.p0[a], rmin(t.p1[a], t.p2[a])));
                    mx[a] = rmax(mx[a], rmax(t.p0[a], rmax(t.p1[a], t.p2[a])));
                }
            }
            for (int a = 0; a < 3; ++a) { nd.lo[a][side] = mn[a] - pad; nd.hi[a][side] = mx[a] + pad; }
        }
    }
}

__global__ __launch_bounds__(kBlock) void refit_propagate4(PtNode4* nodes4, const int32_t* src, const PtNode* nodes, int n_slots4)
{
    const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (s >= n_slots4) return;
    const int32_t from = src[s];
    if (from < 0) return; // empty slot: keeps {+inf, +inf}
    const PtNode& nd = nodes[from >> 1];
    PtNode4& q = nodes4[s >> 2];
    for (int a = 0; a < 3; ++a) { q.lo[a][s & 3] = nd.lo[a][from & 1]; q.hi[a][s & 3] = nd.hi[a][from & 1]; }
}

__global__ __launch_bounds__(kBlock) void refit_propagate8(PtNode8* nodes8, const int32_t* src, const PtNode* nodes, int n_slots8)
{
    const int s = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (s >= n_slots8) return;
    const int32_t from = src[s];
    if (from < 0) return;
    const PtNode& nd = nodes[from >> 1];
    PtNode8::Child& ch = nodes8[s >> 3].c[s & 7];
    for (int a = 0; a < 3; ++a) { ch.lo[a] = nd.lo[a][from & 1]; ch.hi[a] = nd.hi[a][from & 1]; }
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

} // namespace

extern "C" {

size_t pt_refit_workspace_bytes(void) { return (8 + 8 * (size_t)PT_REFIT_PARTIALS) * sizeof(float); }

hipError_t pt_launch_refit(const PtRefitArgs* a, hipEvent_t first, hipEvent_t last, hipStream_t stream)
{
    hipError_t e;
    if ((e = hipEventRecord(first, stream)) != hipSuccess) return e;
    if (a->n_slots > 0) {
        hipLaunchKernelGGL(refit_gather, dim3(blocks_for(a->n_slots)), dim3(kBlock), 0, stream, a->tris, a->shade, a->verts, a->normals, a->tri_vi, a->n_slots);
        const int n_partials = (int)(blocks_for(a->n_slots) < (unsigned)PT_REFIT_PARTIALS ? blocks_for(a->n_slots) : (unsigned)PT_REFIT_PARTIALS);
        hipLaunchKernelGGL(refit_extent_partial, dim3((unsigned)n_partials), dim3(kBlock), 0, stream, a->tris, a->n_slots, a->ws);
        hipLaunchKernelGGL(refit_extent_final, dim3(1), dim3(kBlock), 0, stream, a->ws, n_partials);
        for (int l = 0; l < a->n_levels; ++l) {
            const int count = a->level_ofs[l + 1] - a->level_ofs[l];
            if (count > 0)
                hipLaunchKernelGGL(refit_level, dim3(blocks_for(count)), dim3(kBlock), 0, stream, a->nodes, a->tris, a->level_nodes + a->level_ofs[l], count, a->ws);
        }
        if (a->n_slots4 > 0) hipLaunchKernelGGL(refit_propagate4, dim3(blocks_for(a->n_slots4)), dim3(kBlock), 0, stream, a->nodes4, a->src4, a->nodes, a->n_slots4);
        if (a->n_slots8 > 0) hipLaunchKernelGGL(refit_propagate8, dim3(blocks_for(a->n_slots8)), dim3(kBlock), 0, stream, a->nodes8, a->src8, a->nodes, a->n_slots8);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipEventRecord(last, stream);
}

} // extern "C"
