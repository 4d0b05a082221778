// pt_scene.cpp -- the scene of a context: pt_upload_scene step by step (flatten, BVH, layout and collapses, shading records, tables,
// upload), its clone for the replicas of a multi-GPU group, materials and environment, and the host-side hooks that read the trees.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "pt_internal.h"
#include "pt_launch.h"

// Slivers are never hit (part of the closest-hit definition; the oracle applies the same rule in its own words): a triangle
// whose height over its longest edge is below 1e-5 of that edge - |e1 x e2|^2 <= 1e-10 * max|e|^4, in double - is collapsed to its first
// vertex (the first finite one) for the BVH and the triangle test (det = 0: the Moeller-Trumbore test rejects it for every ray).  Why: for such a needle the
// test's u, v, t are rounding noise and it reports "hits" far outside the triangle's bounding box, which a BVH walk does or does not see
// depending on the order in which it visits the leaves (found by tests/test_gpu_fuzz.py, seed 794689: the oracle's walk and this library's
// disagreed on one ray of 1.7e4 random scenes).  A height of < 100 ulp of the coordinates carries no geometry anyway.
static inline void pt_collapse_sliver(float* p)
{
    const double e1[3] = {(double)p[3] - (double)p[0], (double)p[4] - (double)p[1], (double)p[5] - (double)p[2]};
    const double e2[3] = {(double)p[6] - (double)p[0], (double)p[7] - (double)p[1], (double)p[8] - (double)p[2]};
    const double e3[3] = {(double)p[6] - (double)p[3], (double)p[7] - (double)p[4], (double)p[8] - (double)p[5]};
    const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const double n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
    const double l1 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], l2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2], l3 = e3[0] * e3[0] + e3[1] * e3[1] + e3[2] * e3[2];
    const double L2 = l1 > l2 ? (l1 > l3 ? l1 : l3) : (l2 > l3 ? l2 : l3);
    if (!(n2 > 1e-10 * L2 * L2)) { // also NaN / infinite vertices
        // to the first corner with finite coordinates (the origin if there is none): the leaf boxes stay finite with lo <= hi, which the
        // octant-ordered slab test of the quad-node step needs (pt_kernel.hip, node4_step).  The point is never hit wherever it lies.
        int f = 0;
        while (f < 3 && !(std::isfinite(p[3 * f]) && std::isfinite(p[3 * f + 1]) && std::isfinite(p[3 * f + 2]))) ++f;
        const float q[3] = {f < 3 ? p[3 * f] : 0.0f, f < 3 ? p[3 * f + 1] : 0.0f, f < 3 ? p[3 * f + 2] : 0.0f};
        for (int k = 0; k < 9; ++k) p[k] = q[k % 3];
    }
}
#define PT_AUTO_PLOC_TRIS 64000000 // builder 3: the device PLOC builder beyond this many triangles (see pt_upload_scene)

using namespace pti;

namespace {

HostTexture host_texture(const pt_texture& t) { return HostTexture{t.width, t.height, std::vector<uint32_t>(t.rgba8, t.rgba8 + (size_t)t.width * t.height)}; }

void copy_env(pt_ctx* c, const pt_env* env)
{
    c->scene.env = *env;
    c->scene.env_map = HostTexture{};
    if (env->map.width > 0 && env->map.height > 0 && env->map.rgba8) c->scene.env_map = host_texture(env->map);
    c->scene.env.map.rgba8 = nullptr;
}

int upload_env(pt_ctx* c)
{
    if (c->scene.env_map.w > 0) return upload(c, c->d_env, c->scene.env_map.px.data(), c->scene.env_map.px.size() * 4);
    return PT_OK;
}

int upload_materials(pt_ctx* c)
{
    return upload(c, c->d_materials, c->scene.materials.data(), c->scene.materials.size() * sizeof(float));
}

// A table of the uploaded scene replaced on the device: after the frames in flight (on a caller's stream too: wait_idle), and complete
// when the call returns.
int upload_between_frames(pt_ctx* c, int (*up)(pt_ctx*))
{
    if (c->host_only) return PT_OK;
    int rc = wait_idle(c);
    if (rc) return rc;
    if ((rc = up(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

void pack_materials(pt_ctx* c, const float* materials, int n)
{
    c->scene.n_materials = n;
    c->scene.materials.assign((size_t)n * PT_MAT_STRIDE, 0.0f);
    for (int i = 0; i < n; ++i) material_row(c, &c->scene.materials[(size_t)i * PT_MAT_STRIDE], materials + (size_t)i * PT_MAT_FLOATS, i);
}

// ---- pt_upload_scene, step by step ----

// Everything that can be checked without touching the context.
int validate_scene(pt_ctx* c, const pt_mesh* meshes, int32_t n_meshes, const float* materials, int32_t n_materials, const pt_texture* textures, int32_t n_textures,
                   const int32_t* material_texture)
{
    if (n_meshes < 0 || n_materials < 0 || n_textures < 0 || (n_meshes > 0 && !meshes) || (n_materials > 0 && !materials) ||
        (n_textures > 0 && !textures))
        return fail(c, PT_E_INVALID, "pt_upload_scene: null array with non-zero count");
    for (int i = 0; i < n_textures; ++i)
        if (textures[i].width <= 0 || textures[i].height <= 0 || !textures[i].rgba8) return fail(c, PT_E_INVALID, "texture %d is empty", i);
    if (material_texture)
        for (int i = 0; i < n_materials; ++i)
            if (material_texture[i] >= n_textures) return fail(c, PT_E_INVALID, "material %d: texture index %d out of range (%d textures)", i, material_texture[i], n_textures);
    return PT_OK;
}

// Entities flattened to nine floats per triangle, global order = entity order then face order (mesh_first: global id of a mesh's first
// triangle), and the texture slot of every material.  The only pass that looks at the positions before the BVH does: slivers collapse here.
int flatten_meshes(pt_ctx* c, const pt_mesh* meshes, int32_t n_meshes, int32_t n_materials, int32_t n_textures, const int32_t* material_texture,
                   std::vector<float>& pos, std::vector<size_t>& mesh_first)
{
    size_t n_tris = 0;
    for (int m = 0; m < n_meshes; ++m) {
        if (meshes[m].n_triangles < 0) return fail(c, PT_E_INVALID, "mesh %d: negative triangle count", m);
        n_tris += (size_t)meshes[m].n_triangles;
    }
    if (n_tris > (size_t)(1u << 28)) return fail(c, PT_E_LIMIT, "too many triangles (%zu)", n_tris);
    pos.resize(n_tris * 9);
    mesh_first.assign((size_t)n_meshes + 1, 0);
    c->scene.material_texture.assign((size_t)n_materials, -1);
    if (material_texture)
        for (int i = 0; i < n_materials; ++i) c->scene.material_texture[i] = material_texture[i];
    size_t g = 0;
    for (int m = 0; m < n_meshes; ++m) {
        const pt_mesh& ms = meshes[m];
        if (ms.n_triangles > 0 && (!ms.vertices || !ms.indices)) return fail(c, PT_E_INVALID, "mesh %d: null vertices/indices", m);
        if (ms.material_index >= n_materials) return fail(c, PT_E_INVALID, "mesh %d: material index %d out of range", m, ms.material_index);
        if (ms.texture_index >= n_textures) return fail(c, PT_E_INVALID, "mesh %d: texture index %d out of range", m, ms.texture_index);
        if (ms.texture_index >= 0 && ms.material_index >= 0 && !material_texture) c->scene.material_texture[ms.material_index] = ms.texture_index;
        const bool textured = ms.texture_index >= 0;
        // (the triangles of a large mesh are flattened by all build threads; bad: 1 = vertex index, 2 = normal, 3 = texcoord, + 4 * vertex)
        std::atomic<long long> bad{0};
        const size_t g0 = g;
        mesh_first[(size_t)m] = g0;
        pt_parallel_ranges((size_t)ms.n_triangles, [&](size_t t_lo, size_t t_hi) {
            for (size_t t = t_lo; t < t_hi; ++t) {
                for (int k = 0; k < 3; ++k) {
                    const int32_t vi = ms.indices[t * 3 + (size_t)k];
                    if (vi < 0 || vi >= ms.n_vertices) { bad.store(1 + 4ll * vi); return; }
                    // the reference traps on an out-of-bounds normal/texcoord fetch (macros.hpp:5-11)
                    if (!ms.normals || vi >= ms.n_normals) { bad.store(2 + 4ll * vi); return; }
                    if (textured && (!ms.texcoords || vi >= ms.n_texcoords)) { bad.store(3 + 4ll * vi); return; }
                    std::memcpy(&pos[(g0 + t) * 9 + (size_t)k * 3], ms.vertices + (size_t)vi * 3, 12);
                }
                pt_collapse_sliver(&pos[(g0 + t) * 9]);
            }
        });
        if (const long long b = bad.load()) {
            const int what = (int)(b & 3), vi = (int)(b >> 2);
            if (what == 1) return fail(c, PT_E_INVALID, "mesh %d: vertex index out of range", m);
            if (what == 2) return fail(c, PT_E_INVALID, "mesh %d: no normal for vertex %d", m, vi);
            return fail(c, PT_E_INVALID, "mesh %d: no texcoord for vertex %d", m, vi);
        }
        g += (size_t)ms.n_triangles;
    }
    mesh_first[(size_t)n_meshes] = g;
    return PT_OK;
}

// device PLOC (pt_lbvh.hip): the hierarchy comes down, the host lays it out (pt_bvh_from_hierarchy).  built = false: deeper than the
// stack allows, or the device ran out of its round budget (root < 0) - build_bvh then builds on the host.
int build_ploc(pt_ctx* c, const std::vector<float>& pos, int n, bool& built)
{
    std::vector<int32_t> h_child(2 * (size_t)n * 2), h_count(2 * (size_t)n);
    std::vector<float> h_box(2 * (size_t)n * 6);
    std::vector<uint32_t> h_order((size_t)n);
    int32_t root = -1, rounds = 0;
    {
        DevBuf d_pos, d_ws;
        int rc;
        if ((rc = upload(c, d_pos, pos.data(), pos.size() * sizeof(float))) || (rc = ensure(c, d_ws, pt_ploc_workspace_bytes(n)))) return rc;
        hipError_t e = pt_ploc_build_device((const float*)d_pos.p, n, c->opt.ploc_radius, d_ws.p, d_ws.cap, h_child.data(), h_box.data(), h_count.data(), h_order.data(), &root,
                                            &rounds, c->stream);
        if (e != hipSuccess) return fail(c, PT_E_HIP, "device PLOC build failed: %s", hipGetErrorString(e));
    }
    if (root < 0) return PT_OK; // out of rounds: nothing came down and scene.bvh has not been touched
    built = pt_bvh_from_hierarchy(pos.data(), n, h_child.data(), h_box.data(), h_count.data(), h_order.data(), root, c->opt.leaf_size, c->opt.max_bvh_depth, &c->scene.bvh);
    return PT_OK;
}

// device LBVH (pt_lbvh.hip): positions up, nodes + sorted order down - the host keeps its copy for the validation hooks and for the
// shading records, which follow the triangles into leaf order.  built = false: the Karras tree has no depth control (clustered or
// duplicate centroids give long chains) and this one is deeper than the stack allows.
int build_lbvh(pt_ctx* c, const std::vector<float>& pos, int n, int leaf_sz, bool& built)
{
    PtBvh& bvh = c->scene.bvh;
    int32_t root = -1, n_nodes = 0, height = 0, max_leaf = 0;
    float pad = 0.0f;
    std::vector<uint32_t> order((size_t)n);
    {
        DevBuf d_pos, d_ws, d_order;
        int rc;
        if ((rc = upload(c, d_pos, pos.data(), pos.size() * sizeof(float))) || (rc = ensure(c, d_ws, pt_lbvh_workspace_bytes(n))) ||
            (rc = ensure(c, d_order, (size_t)n * 4)) || (rc = ensure(c, c->d_nodes, (size_t)(n - 1) * sizeof(PtNode))))
            return rc;
        hipError_t e = pt_lbvh_build_device((const float*)d_pos.p, n, leaf_sz, d_ws.p, d_ws.cap, (PtNode*)c->d_nodes.p, (uint32_t*)d_order.p, &root, &n_nodes,
                                            &height, &max_leaf, &pad, c->stream);
        if (e != hipSuccess) return fail(c, PT_E_HIP, "device BVH build failed: %s", hipGetErrorString(e));
        bvh.nodes.resize((size_t)n_nodes);
        hipError_t e1 = hipMemcpy(bvh.nodes.data(), c->d_nodes.p, (size_t)n_nodes * sizeof(PtNode), hipMemcpyDeviceToHost);
        hipError_t e2 = hipMemcpy(order.data(), d_order.p, (size_t)n * 4, hipMemcpyDeviceToHost);
        if (e1 != hipSuccess || e2 != hipSuccess) return fail(c, PT_E_HIP, "device BVH read-back failed");
    }
    if (height > std::min(c->opt.max_bvh_depth, (int)PT_MAX_STACK)) return PT_OK;
    bvh.root = root;
    bvh.depth = height;
    bvh.max_leaf = max_leaf;
    bvh.pad = pad;
    bvh.tris.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        PtTri& t = bvh.tris[(size_t)i];
        std::memcpy(t.p0, &pos[(size_t)order[(size_t)i] * 9], 36);
        t.id = (int32_t)order[(size_t)i];
        t.material = -1;
        t.pad = 0;
    }
    built = true;
    return PT_OK;
}

// The binary BVH over `pos` (replaces owlGroupBuildAccel, application.cpp:135-139) by the builder the options choose.
int build_bvh(pt_ctx* c, const std::vector<float>& pos, size_t n_tris)
{
    const int leaf_sz = std::max(1, std::min(7, c->opt.leaf_size));
    // builder 3 = automatic: the host SAH tree walks fastest (C4: 478 ms against 606 for PLOC and 697 for the Karras tree) and, since the
    // builder runs on all host threads (round 4), is built as fast as the device PLOC tree comes down and is laid out: 0.9 M triangles 58-83 ms
    // against 88, 4 M triangles 350 against 360 ms (and walks 4 % faster there) - PLOC only takes over where the host builder's memory would
    // become the limit (PT_AUTO_PLOC_TRIS)
    const int builder = c->opt.bvh_builder == 3 ? (n_tris > (size_t)PT_AUTO_PLOC_TRIS ? 2 : 0) : c->opt.bvh_builder;
    bool built = false;
    if (builder != 0 && !c->host_only && n_tris > (size_t)leaf_sz) {
        const int rc = builder == 2 ? build_ploc(c, pos, (int)n_tris, built) : build_lbvh(c, pos, (int)n_tris, leaf_sz, built);
        if (rc) return rc;
    }
    // the host builder: the default, and - because it caps the depth - what takes over from a device builder instead of failing the upload
    // (a tree deeper than max_bvh_depth, PLOC out of rounds).  pt_bvh_build resets every field of scene.bvh first: nothing of the nodes
    // build_lbvh read back or of the partial layout of pt_bvh_from_hierarchy survives, and upload_scene_to_device rewrites d_nodes.
    if (!built) pt_bvh_build(pos.data(), (int32_t)n_tris, c->opt.leaf_size, c->opt.max_bvh_depth, &c->scene.bvh);
    return PT_OK;
}

// Leaf layout of the binary tree, then its quad and oct collapses.
void layout_and_collapse(pt_ctx* c)
{
    HostScene& s = c->scene;
    pt_bvh_layout(&s.bvh, c->opt.node_pairs, c->opt.leaf_align);
    s.bvh_nodes = s.bvh.nodes.size();
    std::vector<int32_t>* src4 = s.dyn.enabled ? &s.dyn.refit.src4 : nullptr; // option "dynamic": which binary box every slot copies
    std::vector<int32_t>* src8 = s.dyn.enabled ? &s.dyn.refit.src8 : nullptr;
    { // the two collapses only read the binary tree: side by side
        std::thread oct([&] { pt_bvh_collapse8(s.bvh, c->opt.wide_leaves, &s.nodes8, &s.root8, &s.depth8, src8); });
        pt_bvh_collapse4(s.bvh, &s.nodes4, &s.root4, &s.depth4, src4);
        oct.join();
    }
    if (3 * s.depth4 + 1 > PT_MAX_STACK) { s.nodes4.clear(); s.dyn.refit.src4.clear(); } // the quad walk could need more stack than the kernel has: binary walk instead
    if (7 * s.depth8 + 1 > PT_GROUP_STACK) { s.nodes8.clear(); s.dyn.refit.src8.clear(); } // a group's stack (eight LDS stack columns) could overflow: no group walk
}

// shading records in leaf order (padding slots included), gathered from the caller's arrays: the three vertex normals and
// texcoords of triangle `id` (device.cu:63-94) and its material, which the triangle record carries as well
void shading_records(pt_ctx* c, const pt_mesh* meshes, const std::vector<size_t>& mesh_first)
{
    HostScene& s = c->scene;
    const size_t n_slots = s.bvh.tris.size();
    s.shade.resize(n_slots);
    pt_parallel_ranges(n_slots, [&](size_t lo, size_t hi) {
        int m = 0;
        for (size_t i = lo; i < hi; ++i) {
            PtShade& sh = s.shade[i];
            std::memset(&sh, 0, sizeof(sh));
            const int32_t id = s.bvh.tris[i].id;
            if (id == 0x7fffffff) { sh.material = -1; continue; }
            if (!((size_t)id >= mesh_first[(size_t)m] && (size_t)id < mesh_first[(size_t)m + 1]))
                m = (int)(std::upper_bound(mesh_first.begin(), mesh_first.end(), (size_t)id) - mesh_first.begin()) - 1;
            const pt_mesh& ms = meshes[m];
            const size_t t = (size_t)id - mesh_first[(size_t)m];
            sh.material = ms.material_index;
            s.bvh.tris[i].material = ms.material_index;
            for (int k = 0; k < 3; ++k) {
                const int32_t vi = ms.indices[t * 3 + (size_t)k]; // validated by flatten_meshes
                float* nd = k == 0 ? sh.n0 : (k == 1 ? sh.n1 : sh.n2);
                std::memcpy(nd, ms.normals + (size_t)vi * 3, 12);
                if (ms.texcoords && vi < ms.n_texcoords) std::memcpy(&sh.tc[k * 2], ms.texcoords + (size_t)vi * 2, 8);
            }
        }
    });
}

// Option "dynamic" = 1: what pt_update_vertices needs beside the scene - the meshes' vertex and normal arrays, concatenated, with
// per-mesh bases; per leaf-order slot its three vertex indices with the base folded in; the refit schedule of the binary tree.  (The
// collapses have already noted which binary box every quad / oct slot copies: layout_and_collapse.)
int retain_dynamic(pt_ctx* c, const pt_mesh* meshes, int32_t n_meshes, const std::vector<size_t>& mesh_first)
{
    HostScene& s = c->scene;
    DynScene& d = s.dyn;
    if (!d.enabled) return PT_OK;
    size_t nv = 0, nn = 0;
    for (int m = 0; m < n_meshes; ++m) {
        d.vbase.push_back((int32_t)nv);
        d.nbase.push_back((int32_t)nn);
        d.n_verts.push_back(meshes[m].n_vertices);
        d.n_normals.push_back(meshes[m].n_normals);
        nv += (size_t)std::max(0, meshes[m].n_vertices);
        nn += (size_t)std::max(0, meshes[m].n_normals);
        if (nv > 0x7fffffffull || nn > 0x7fffffffull) return fail(c, PT_E_LIMIT, "option \"dynamic\": more than 2^31 vertices or normals");
    }
    d.verts.assign(nv * 3, 0.0f);
    d.normals.assign(nn * 3, 0.0f);
    for (int m = 0; m < n_meshes; ++m) {
        if (meshes[m].vertices && meshes[m].n_vertices > 0) std::memcpy(&d.verts[(size_t)d.vbase[(size_t)m] * 3], meshes[m].vertices, (size_t)meshes[m].n_vertices * 12);
        if (meshes[m].normals && meshes[m].n_normals > 0) std::memcpy(&d.normals[(size_t)d.nbase[(size_t)m] * 3], meshes[m].normals, (size_t)meshes[m].n_normals * 12);
    }
    const size_t n_slots = s.bvh.tris.size();
    d.refit.tri_vi.assign(n_slots * 4, -1);
    pt_parallel_ranges(n_slots, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            const int32_t id = s.bvh.tris[i].id;
            if (id == 0x7fffffff) continue;
            const int m = (int)(std::upper_bound(mesh_first.begin(), mesh_first.end(), (size_t)id) - mesh_first.begin()) - 1;
            const size_t t = (size_t)id - mesh_first[(size_t)m];
            for (int k = 0; k < 3; ++k) d.refit.tri_vi[i * 4 + (size_t)k] = d.vbase[(size_t)m] + meshes[m].indices[t * 3 + (size_t)k]; // validated by flatten_meshes
            d.refit.tri_vi[i * 4 + 3] = d.nbase[(size_t)m] - d.vbase[(size_t)m];
        }
    });
    pt_bvh_refit_schedule(s.bvh, &d.refit);
    return PT_OK;
}

// Step 1 of an update on the host copies: every live slot's vertices through the retained indices, the sliver rule, p0..p2 of its
// PtTri - and n0..n2 of its PtShade with `normals`.  Returns the number of triangles that are points afterwards (collapsed slivers).
size_t gather_host(pt_ctx* c, bool normals)
{
    HostScene& s = c->scene;
    const DynScene& d = s.dyn;
    std::atomic<size_t> points{0};
    pt_parallel_ranges(s.bvh.tris.size(), [&](size_t lo, size_t hi) {
        size_t n_points = 0;
        for (size_t i = lo; i < hi; ++i) {
            PtTri& tr = s.bvh.tris[i];
            if (tr.id == 0x7fffffff) continue;
            const int32_t* vi = &d.refit.tri_vi[i * 4];
            float p[9];
            for (int k = 0; k < 3; ++k) std::memcpy(p + 3 * k, &d.verts[(size_t)vi[k] * 3], 12);
            pt_collapse_sliver(p);
            std::memcpy(tr.p0, p, 36);
            n_points += (p[0] == p[3] && p[0] == p[6] && p[1] == p[4] && p[1] == p[7] && p[2] == p[5] && p[2] == p[8]) ? 1 : 0;
            if (normals) {
                PtShade& sh = s.shade[i];
                for (int k = 0; k < 3; ++k) std::memcpy(k == 0 ? sh.n0 : (k == 1 ? sh.n1 : sh.n2), &d.normals[(size_t)((long long)vi[k] + vi[3]) * 3], 12);
            }
        }
        points += n_points;
    });
    return points.load();
}

// Host copies of the textures, the material table and the environment.
void copy_tables(pt_ctx* c, const float* materials, int32_t n_materials, const pt_texture* textures, int32_t n_textures, const pt_env* env)
{
    c->scene.textures.clear();
    for (int i = 0; i < n_textures; ++i) c->scene.textures.push_back(host_texture(textures[i]));
    pack_materials(c, materials, n_materials);
    pt_env def{};
    copy_env(c, env ? env : &def);
}

} // namespace

extern "C" int pt_upload_scene(pt_ctx* c, const pt_mesh* meshes, int32_t n_meshes, const float* materials, int32_t n_materials,
                    const pt_texture* textures, int32_t n_textures, const int32_t* material_texture, const pt_env* env)
{
    if (!c) return PT_E_INVALID;
    int rc = validate_scene(c, meshes, n_meshes, materials, n_materials, textures, n_textures, material_texture);
    if (rc) return rc;
    // from here on the context has NO scene until the upload has succeeded (a failure half way must not leave the previous scene's flag
    // over new host arrays)
    c->have_scene = false;
    ++c->scene_epoch;
    c->scene.dyn = DynScene{};
    c->scene.dyn.enabled = c->opt.dynamic != 0;
    // every device buffer of the scene is reused in place where its capacity suffices (ensure), and a device builder writes d_nodes
    // directly: after the frames in flight
    if (!c->host_only && (rc = wait_idle(c))) return rc;
    // PT_UPLOAD_TRACE=1: phase times of this call on stderr
    const bool trace = getenv("PT_UPLOAD_TRACE") && getenv("PT_UPLOAD_TRACE")[0] == '1';
    auto t_phase = std::chrono::steady_clock::now();
    auto phase = [&](const char* what) {
        const auto now = std::chrono::steady_clock::now();
        if (trace) fprintf(stderr, "pt_upload_scene: %-28s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_phase).count());
        t_phase = now;
    };

    std::vector<float> pos;
    std::vector<size_t> mesh_first;
    if ((rc = flatten_meshes(c, meshes, n_meshes, n_materials, n_textures, material_texture, pos, mesh_first))) return rc;
    const size_t n_tris = pos.size() / 9;
    phase("flatten entities");
    auto t0 = std::chrono::steady_clock::now();
    if ((rc = build_bvh(c, pos, n_tris))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    c->scene.bvh_build_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    c->scene.bvh_nodes = c->scene.bvh.nodes.size();
    c->scene.bvh_depth = (uint64_t)c->scene.bvh.depth;
    c->scene.n_triangles = n_tris;
    c->scene.mesh_first.assign(mesh_first.begin(), mesh_first.end()); // pt_prim_to_mesh
    if (c->scene.bvh.depth > PT_MAX_STACK) return fail(c, PT_E_LIMIT, "BVH depth %d exceeds %d", c->scene.bvh.depth, PT_MAX_STACK);
    phase("BVH build");
    layout_and_collapse(c);
    phase("quad + oct nodes");
    shading_records(c, meshes, mesh_first);
    phase("shading records");
    if ((rc = retain_dynamic(c, meshes, n_meshes, mesh_first))) return rc;
    copy_tables(c, materials, n_materials, textures, n_textures, env);
    if (!c->host_only && (rc = upload_scene_to_device(c))) return rc;
    phase("textures, upload to HBM");
    c->have_scene = true;
    return PT_OK;
}

namespace pti {

// One row of the device material table: the PT_MAT_FLOATS floats of the caller's row i, then the context's texture slot of material i.
void material_row(const pt_ctx* c, float* dst, const float* src, int i)
{
    std::memcpy(dst, src, PT_MAT_FLOATS * sizeof(float));
    const int32_t slot = i < (int)c->scene.material_texture.size() ? c->scene.material_texture[i] : -1;
    std::memcpy(dst + 17, &slot, 4);
}

// Host copies of the scene (BVH, quad nodes, triangles, shading records, textures, materials, environment) -> this context's GPU.
int upload_scene_to_device(pt_ctx* c)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const int n_textures = (int)c->scene.textures.size();
    int rc;
    if ((rc = upload(c, c->d_nodes, c->scene.bvh.nodes.data(), c->scene.bvh.nodes.size() * sizeof(PtNode)))) return rc;
    if ((rc = upload(c, c->d_nodes4, c->scene.nodes4.data(), c->scene.nodes4.size() * sizeof(PtNode4)))) return rc;
    if ((rc = upload(c, c->d_nodes8, c->scene.nodes8.data(), c->scene.nodes8.size() * sizeof(PtNode8)))) return rc;
    if ((rc = upload(c, c->d_tris, c->scene.bvh.tris.data(), c->scene.bvh.tris.size() * sizeof(PtTri)))) return rc;
    if ((rc = upload(c, c->d_shade, c->scene.shade.data(), c->scene.shade.size() * sizeof(PtShade)))) return rc;
    if (const DynScene& d = c->scene.dyn; d.enabled) { // what the refit kernels read (pt_refit.hip)
        if ((rc = upload(c, c->d_verts, d.verts.data(), d.verts.size() * sizeof(float)))) return rc;
        if ((rc = upload(c, c->d_vnormals, d.normals.data(), d.normals.size() * sizeof(float)))) return rc;
        if ((rc = upload(c, c->d_tri_vi, d.refit.tri_vi.data(), d.refit.tri_vi.size() * 4))) return rc;
        if ((rc = upload(c, c->d_level_nodes, d.refit.level_nodes.data(), d.refit.level_nodes.size() * 4))) return rc;
        if ((rc = upload(c, c->d_src4, d.refit.src4.data(), d.refit.src4.size() * 4))) return rc;
        if ((rc = upload(c, c->d_src8, d.refit.src8.data(), d.refit.src8.size() * 4))) return rc;
        if ((rc = ensure(c, c->d_refit_ws, pt_refit_workspace_bytes()))) return rc;
    }
    c->d_textures.clear();
    std::vector<PtTexDesc> descs((size_t)n_textures);
    for (int i = 0; i < n_textures; ++i) {
        c->d_textures.emplace_back();
        if ((rc = upload(c, c->d_textures.back(), c->scene.textures[i].px.data(), c->scene.textures[i].px.size() * 4))) return rc;
        descs[i].texels = (const uint32_t*)c->d_textures.back().p;
        descs[i].width = c->scene.textures[i].w;
        descs[i].height = c->scene.textures[i].h;
    }
    if ((rc = upload(c, c->d_texdesc, descs.data(), descs.size() * sizeof(PtTexDesc)))) return rc;
    if ((rc = upload_materials(c))) return rc;
    if ((rc = upload_env(c))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PT_OK;
}

// The scene of `src` (built once: BVH, leaf-order records, quad nodes) copied into `dst` and uploaded to dst's GPU: the replicas
// of a multi-GPU group (pt_group_upload_scene) do not each rebuild the BVH on the host.
int clone_scene(pt_ctx* dst, const pt_ctx* src)
{
    if (!src->have_scene) return fail(dst, PT_E_NO_SCENE, "clone_scene: the source context has no scene");
    sync_host_scene(const_cast<pt_ctx*>(src)); // (the host copies are a cache of what the source's device holds after an update)
    dst->scene = src->scene;
    dst->have_scene = true;
    ++dst->scene_epoch;
    dst->queue_valid = false;
    if (dst->host_only) return PT_OK;
    return upload_scene_to_device(dst);
}

// After pt_update_vertices on a device context only HBM holds the moved scene: the host twin of the refit runs when somebody reads the
// host copies (the product path never does).
void sync_host_scene(pt_ctx* c)
{
    DynScene& d = c->scene.dyn;
    if (!d.enabled || !d.host_stale) return;
    (void)gather_host(c, d.stale_normals);
    pt_bvh_refit(&c->scene.bvh, d.refit, &c->scene.nodes4, &c->scene.nodes8);
    d.host_stale = d.stale_normals = false;
}

} // namespace pti

extern "C" {

int pt_update_vertices(pt_ctx* c, const pt_mesh* meshes, int32_t n_meshes)
{
    if (!c) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_update_vertices before pt_upload_scene");
    HostScene& s = c->scene;
    DynScene& d = s.dyn;
    // everything is checked before anything is touched
    if (!d.enabled) return fail(c, PT_E_INVALID, "pt_update_vertices: the scene was not uploaded with option \"dynamic\" = 1");
    if (n_meshes != (int32_t)d.vbase.size()) return fail(c, PT_E_INVALID, "pt_update_vertices: %d meshes, the scene was uploaded with %zu", n_meshes, d.vbase.size());
    if (n_meshes > 0 && !meshes) return fail(c, PT_E_INVALID, "pt_update_vertices: null mesh array with non-zero count");
    for (int m = 0; m < n_meshes; ++m)
        if (meshes[m].n_vertices != d.n_verts[(size_t)m] || meshes[m].n_normals != d.n_normals[(size_t)m])
            return fail(c, PT_E_INVALID, "pt_update_vertices: mesh %d has %d vertices / %d normals, the scene was uploaded with %d / %d", m, meshes[m].n_vertices,
                        meshes[m].n_normals, d.n_verts[(size_t)m], d.n_normals[(size_t)m]);
    if (!c->host_only) { // after the frames in flight, as upload_between_frames
        if (int rc = wait_idle(c)) return rc;
        if (!c->evu0) HIP_TRY(c, hipEventCreate(&c->evu0));
        if (!c->evu1) HIP_TRY(c, hipEventCreate(&c->evu1));
    }
    // the host keeps the new arrays (the caller owns its input); the device gets the ranges that changed
    bool any_normals = false;
    double h2d = 0.0;
    for (int m = 0; m < n_meshes; ++m) {
        const pt_mesh& ms = meshes[m];
        if (ms.vertices && ms.n_vertices > 0) {
            float* dst = &d.verts[(size_t)d.vbase[(size_t)m] * 3];
            const size_t bytes = (size_t)ms.n_vertices * 12;
            std::memcpy(dst, ms.vertices, bytes);
            if (!c->host_only) {
                HIP_TRY(c, hipMemcpyAsync((char*)c->d_verts.p + (size_t)d.vbase[(size_t)m] * 12, dst, bytes, hipMemcpyHostToDevice, c->stream));
                h2d += (double)bytes;
            }
        }
        if (ms.normals && ms.n_normals > 0) {
            float* dst = &d.normals[(size_t)d.nbase[(size_t)m] * 3];
            const size_t bytes = (size_t)ms.n_normals * 12;
            std::memcpy(dst, ms.normals, bytes);
            any_normals = true;
            if (!c->host_only) {
                HIP_TRY(c, hipMemcpyAsync((char*)c->d_vnormals.p + (size_t)d.nbase[(size_t)m] * 12, dst, bytes, hipMemcpyHostToDevice, c->stream));
                h2d += (double)bytes;
            }
        }
    }
    const int levels = d.refit.level_ofs.empty() ? 0 : (int)d.refit.level_ofs.size() - 1;
    double ms_dev = 0.0, slivers = 0.0;
    if (c->host_only) { // the host twin is the update
        slivers = (double)gather_host(c, any_normals);
        pt_bvh_refit(&s.bvh, d.refit, &s.nodes4, &s.nodes8);
    } else {
        PtRefitArgs a{};
        a.nodes = (PtNode*)c->d_nodes.p; a.nodes4 = (PtNode4*)c->d_nodes4.p; a.nodes8 = (PtNode8*)c->d_nodes8.p;
        a.tris = (PtTri*)c->d_tris.p; a.shade = (PtShade*)c->d_shade.p;
        a.verts = (const float*)c->d_verts.p; a.normals = any_normals ? (const float*)c->d_vnormals.p : nullptr;
        a.tri_vi = (const int32_t*)c->d_tri_vi.p; a.level_nodes = (const int32_t*)c->d_level_nodes.p;
        a.src4 = (const int32_t*)c->d_src4.p; a.src8 = (const int32_t*)c->d_src8.p;
        a.ws = (float*)c->d_refit_ws.p;
        a.level_ofs = d.refit.level_ofs.data();
        a.n_slots = (int32_t)s.bvh.tris.size(); a.n_levels = levels;
        a.n_slots4 = (int32_t)std::min(s.nodes4.size() * 4, d.refit.src4.size()); a.n_slots8 = (int32_t)std::min(s.nodes8.size() * 8, d.refit.src8.size());
        hipError_t e = pt_launch_refit(&a, c->evu0, c->evu1, c->stream);
        if (e != hipSuccess) return fail(c, PT_E_HIP, "pt_update_vertices: refit launch failed: %s", hipGetErrorString(e));
        uint32_t down[2] = {0, 0}; // pad (float bits), collapsed slivers
        if (a.n_slots > 0) HIP_TRY(c, hipMemcpyAsync(down, c->d_refit_ws.p, sizeof(down), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->evu0, c->evu1));
        ms_dev = ms;
        std::memcpy(&s.bvh.pad, &down[0], 4); // walk_params and the automatic box_exact decision read the host's pad
        slivers = (double)down[1];
        d.host_stale = true;
        d.stale_normals = d.stale_normals || any_normals;
    }
    c->queue_valid = false; // whatever is cached per geometry
    const double info[8] = {ms_dev, h2d, slivers, (double)s.bvh.pad, (double)levels, 0.0, 0.0, 0.0};
    std::memcpy(d.info, info, sizeof(info));
    return PT_OK;
}

int pt_debug_update_info(pt_ctx* c, double out[8])
{
    if (!c || !out) return PT_E_INVALID;
    std::memcpy(out, c->scene.dyn.info, sizeof(c->scene.dyn.info));
    return PT_OK;
}

int pt_set_materials(pt_ctx* c, const float* materials, int32_t n_materials)
{
    if (!c || !materials || n_materials < 0) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_set_materials before pt_upload_scene");
    if (n_materials != c->scene.n_materials) return fail(c, PT_E_INVALID, "material count changed (%d -> %d); re-upload the scene", c->scene.n_materials, n_materials);
    pack_materials(c, materials, n_materials);
    return upload_between_frames(c, upload_materials);
}

int pt_set_environment(pt_ctx* c, const pt_env* env)
{
    if (!c || !env) return PT_E_INVALID;
    copy_env(c, env);
    return upload_between_frames(c, upload_env);
}

int pt_debug_closest_hit_host(pt_ctx* c, const float org[3], const float dir[3], float tmin, float tmax, float* t, float* u, float* v, int32_t* prim)
{
    if (!c || !c->have_scene) return PT_E_NO_SCENE;
    sync_host_scene(c);
    return pt_bvh_closest_hit_host(c->scene.bvh, org, dir, tmin, tmax, t, u, v, prim, c->opt.watertight != 0) ? 1 : 0;
}

int64_t pt_debug_closest_hit_host_n(pt_ctx* c, const float* rays, int64_t n, float tmin, float tmax, float* out)
{
    if (!c || !rays || !out || n < 0) return PT_E_INVALID;
    if (!c->have_scene) return PT_E_NO_SCENE;
    sync_host_scene(c);
    const bool wt = c->opt.watertight != 0; // the walk follows the option as the render does
    pt_parallel_ranges((size_t)n, [&](size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i) {
            float t = 0.0f, u = 0.0f, v = 0.0f;
            int32_t prim = -1;
            const bool hit = pt_bvh_closest_hit_host(c->scene.bvh, rays + 6 * i, rays + 6 * i + 3, tmin, tmax, &t, &u, &v, &prim, wt);
            float* y = out + 5 * i;
            y[0] = hit ? 1.0f : 0.0f; y[1] = t; y[2] = u; y[3] = v;
            const int32_t id = hit ? prim : -1;
            std::memcpy(y + 4, &id, 4);
        }
    });
    return n;
}

int64_t pt_debug_export_tree(pt_ctx* c, int32_t which, void* out, int64_t cap)
{
    if (!c || cap < 0) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_debug_export_tree before pt_upload_scene");
    const bool from_device = (which & PT_TREE_DEVICE) != 0; // the named array as HBM holds it (what the refit kernels wrote)
    which &= ~PT_TREE_DEVICE;
    if (from_device && c->host_only) return fail(c, PT_E_INVALID, "pt_debug_export_tree: PT_TREE_DEVICE on a host-only context");
    if (!from_device) sync_host_scene(c);
    int64_t info[8] = {c->scene.bvh.root, c->scene.root4, c->scene.root8, c->scene.bvh.depth, c->scene.depth4, c->scene.depth8, 0, c->scene.bvh.max_leaf};
    std::memcpy(&info[6], &c->scene.bvh.pad, sizeof(float));
    const void* src = nullptr;
    size_t bytes = 0;
    const void* d_src = nullptr; // (the sizes are the host arrays': an update changes no count)
    switch (which) {
    case PT_TREE_BINARY: src = c->scene.bvh.nodes.data(); bytes = c->scene.bvh.nodes.size() * sizeof(PtNode); d_src = c->d_nodes.p; break;
    case PT_TREE_QUAD: src = c->scene.nodes4.data(); bytes = c->scene.nodes4.size() * sizeof(PtNode4); d_src = c->d_nodes4.p; break;
    case PT_TREE_OCT: src = c->scene.nodes8.data(); bytes = c->scene.nodes8.size() * sizeof(PtNode8); d_src = c->d_nodes8.p; break;
    case PT_TREE_TRIS: src = c->scene.bvh.tris.data(); bytes = c->scene.bvh.tris.size() * sizeof(PtTri); d_src = c->d_tris.p; break;
    case PT_TREE_INFO: src = info; bytes = sizeof(info); break;
    default: return fail(c, PT_E_INVALID, "pt_debug_export_tree: unknown array %d", which);
    }
    if (!out) return (int64_t)bytes; // size query
    if ((size_t)cap < bytes) return fail(c, PT_E_INVALID, "pt_debug_export_tree: %zu bytes needed, %lld given", bytes, (long long)cap);
    if (bytes && from_device && which != PT_TREE_INFO) {
        if (int rc = wait_idle(c)) return rc;
        HIP_TRY(c, hipMemcpy(out, d_src, bytes, hipMemcpyDeviceToHost));
    } else if (bytes) std::memcpy(out, src, bytes);
    return (int64_t)bytes;
}

int pt_debug_clone_scene(pt_ctx* dst, const pt_ctx* src)
{
    if (!dst || !src || dst == src) return PT_E_INVALID;
    return pti::clone_scene(dst, src);
}

int pt_debug_quad_info(pt_ctx* c, int64_t out[8])
{
    if (!c || !out) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_debug_quad_info before pt_upload_scene");
    sync_host_scene(c);
    // {quad nodes, depth, leaf slots, triangles in leaf slots, empty slots, internal slots, binary nodes, binary leaf references}
    int64_t leaf_slots = 0, tris = 0, empty = 0, internal = 0, bin_leaves = 0;
    for (const PtNode4& q : c->scene.nodes4) {
        for (int k = 0; k < 4; ++k) {
            const int32_t r = q.child[k];
            if (r == -1) {
                ++empty;
                for (int a = 0; a < 3; ++a)
                    if (!(q.lo[a][k] == INFINITY && q.hi[a][k] == INFINITY)) return fail(c, PT_E_LIMIT, "quad node: empty slot with a finite box");
                continue;
            }
            if (r >= 0) ++internal;
            else {
                ++leaf_slots;
                tris += (int64_t)(~(uint32_t)r & 7u);
            }
            // the octant-ordered slab test (node4_step) takes the lo row as the entry plane for inv > 0 and the hi row for inv < 0: exact
            // only for finite lo <= hi
            for (int a = 0; a < 3; ++a)
                if (!(std::isfinite(q.lo[a][k]) && std::isfinite(q.hi[a][k]) && q.lo[a][k] <= q.hi[a][k]))
                    return fail(c, PT_E_LIMIT, "quad node: slot %d has a box that is not finite with lo <= hi on axis %d", k, a);
        }
    }
    for (const PtNode& nd : c->scene.bvh.nodes) {
        if (nd.left < -1) ++bin_leaves;
        if (nd.right < -1) ++bin_leaves;
    }
    out[0] = (int64_t)c->scene.nodes4.size(); out[1] = c->scene.depth4; out[2] = leaf_slots; out[3] = tris; out[4] = empty; out[5] = internal;
    out[6] = (int64_t)c->scene.bvh.nodes.size(); out[7] = bin_leaves;
    return PT_OK;
}

int pt_debug_oct_info(pt_ctx* c, int64_t out[8])
{
    if (!c || !out) return PT_E_INVALID;
    if (!c->have_scene) return fail(c, PT_E_NO_SCENE, "pt_debug_oct_info before pt_upload_scene");
    sync_host_scene(c);
    // {oct nodes, depth, leaf slots, triangles in leaf slots, empty slots, internal slots, largest leaf, triangle slots of the scene}
    int64_t leaf_slots = 0, tris = 0, empty = 0, internal = 0, max_leaf = 0;
    std::vector<uint8_t> seen(c->scene.bvh.tris.size(), 0);
    std::vector<uint8_t> referenced(c->scene.nodes8.size(), 0);
    for (const PtNode8& q : c->scene.nodes8) {
        for (int k = 0; k < 8; ++k) {
            const int32_t r = q.c[k].ref;
            if (r >= 0) {
                if ((size_t)r >= c->scene.nodes8.size() || referenced[(size_t)r]++) return fail(c, PT_E_LIMIT, "oct node: child %d out of range or referenced twice", r);
                ++internal;
            } else if (r == -1) {
                ++empty;
                for (int a = 0; a < 3; ++a)
                    if (!(q.c[k].lo[a] == INFINITY && q.c[k].hi[a] == INFINITY)) return fail(c, PT_E_LIMIT, "oct node: empty slot with a finite box");
            } else {
                const uint32_t code = ~(uint32_t)r, first = code >> 3, count = code & 7u;
                ++leaf_slots;
                tris += count;
                max_leaf = std::max<int64_t>(max_leaf, count);
                for (uint32_t t = first; t < first + count; ++t) {
                    if (t >= seen.size() || seen[t]++) return fail(c, PT_E_LIMIT, "oct node: triangle slot %u out of range or in two leaves", t);
                    // the leaf's box must hold its triangles (wide leaves take the box of the subtree they replace)
                    const PtTri& tr = c->scene.bvh.tris[t];
                    if (tr.id == 0x7fffffff) continue; // leaf_align padding
                    for (int a = 0; a < 3; ++a) {
                        const float lo = std::min(tr.p0[a], std::min(tr.p1[a], tr.p2[a])), hi = std::max(tr.p0[a], std::max(tr.p1[a], tr.p2[a]));
                        if (lo < q.c[k].lo[a] || hi > q.c[k].hi[a]) return fail(c, PT_E_LIMIT, "oct node: triangle slot %u sticks out of its leaf box", t);
                    }
                }
            }
        }
    }
    out[0] = (int64_t)c->scene.nodes8.size(); out[1] = c->scene.depth8; out[2] = leaf_slots; out[3] = tris; out[4] = empty; out[5] = internal;
    out[6] = max_leaf; out[7] = (int64_t)c->scene.bvh.tris.size();
    return PT_OK;
}

} // extern "C"
