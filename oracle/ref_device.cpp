/*
 * ref_device.cpp -- the reference's own device code, compiled for the CPU.  TEST INFRASTRUCTURE ONLY.
 *
 * oracle/Makefile (target `ref`) compiles this file against a reference checkout (REF_DIR) with the stand-in headers
 * in oracle/ref_shim and writes oracle/_ref/libref_device.so; nothing compiled from the reference is kept in the
 * repository.  The reference's random.hpp, math.hpp, sample_methods.hpp, the disney/ headers and device.cu (trace_path,
 * ray_gen, triangle_hit, miss) run as written.  The code below only marshals plain C arrays in and out and sets up
 * what OWL and OptiX would: launch parameters, per-mesh buffers, program data and hit state.  Its C ABI mirrors the
 * oracle's (pt_oracle.h), so that oracle/reference.py can put the two side by side.
 */
#include "device/device.cu"

thread_local ref_shim_state g_ref_shim;

namespace {

/* A scene: the oracle's triangle soup (for the closest-hit query) plus the reference's per-mesh buffers.
   Consecutive triangles with the same material and texture form one mesh, i.e. one OWL geometry with its entity_data,
   so primitive indices are mesh-local as under OptiX. */
struct ref_scene {
    orc_scene* soup;
    int32_t n_tris, n_meshes, n_materials, n_textures;
    int32_t* mesh_of;  /* per triangle */
    int32_t* first;    /* per mesh: first global triangle */
    entity_data* entities;
    vec3* vertices;    /* 3 per triangle, global order */
    vec3* normals;
    vec2* texcoords;   /* 3 per triangle, or null */
    ivec3* indices;    /* per triangle, into its mesh's vertices */
    Buffer *vbuf, *nbuf, *tbuf, *ibuf; /* per mesh */
    material_data* materials;
    orc_texture* textures;
};

/* traceRay calls left before the driver stops a launch: the reference retries a NaN/inf BSDF sample without limit
   (device.cu:196-201); past the budget every trace misses, so the loop ends, and the call reports the overflow. */
thread_local int64_t g_trace_budget = 0;
thread_local int g_trace_overflow = 0;

material_data mat_load(const float* p)
{
    material_data m{};
    m.base_color = vec3{p[0], p[1], p[2]};
    m.subsurface = p[3]; m.metallic = p[4]; m.specular = p[5]; m.specular_tint = p[6]; m.roughness = p[7];
    m.anisotropic = p[8]; m.sheen = p[9]; m.sheen_tint = p[10]; m.clearcoat = p[11]; m.clearcoat_gloss = p[12];
    m.ior = p[13]; m.specular_transmission = p[14]; m.specular_transmission_roughness = p[15]; m.emission = p[16];
    return m;
}
vec3 ld(const float* p) { return vec3{p[0], p[1], p[2]}; }
void st(float* p, const vec3& v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

void set_launch(const ref_scene* s, const orc_env* env, int max_samples, int max_depth)
{
    launch_params_data& lp = optixLaunchParams;
    lp.max_path_depth = max_depth;
    lp.max_samples = max_samples;
    lp.material_buffer = Buffer{(size_t)s->n_materials, s->materials};
    lp.vertices_buffer = Buffer{(size_t)s->n_meshes, s->vbuf};
    lp.indices_buffer = Buffer{(size_t)s->n_meshes, s->ibuf};
    lp.normals_buffer = Buffer{(size_t)s->n_meshes, s->nbuf};
    lp.texcoords_buffer = Buffer{(size_t)s->n_meshes, s->tbuf};
    lp.world = (OptixTraversableHandle)s;
    lp.environment_map = env->map.width > 0 ? (cudaTextureObject_t)&env->map : 0;
    lp.environment_use = env->use_map != 0;
    lp.environment_auto = env->use_auto != 0;
    lp.environment_color = vec3{env->color[0], env->color[1], env->color[2]};
    lp.environment_intensity = env->intensity;
}

camera_data camera_load(const orc_camera* c)
{
    camera_data d;
    d.origin = ld(c->origin);
    d.llc = ld(c->llc);
    d.horizontal = ld(c->horizontal);
    d.vertical = ld(c->vertical);
    return d;
}

} // namespace

void ref_shim_trace(OptixTraversableHandle world, int ray_type, const vec3& org, const vec3& dir, float tmin, float tmax, void* prd)
{
    const ref_scene* s = (const ref_scene*)world;
    const float o[3] = {org.x, org.y, org.z}, d[3] = {dir.x, dir.y, dir.z};
    float t = 0.0f, u = 0.0f, v = 0.0f;
    int32_t prim = -1;
    int hit = orc_intersect(s->soup, o, d, tmin, tmax, 1, &t, &u, &v, &prim);
    if (--g_trace_budget < 0) {
        g_trace_overflow = 1;
        hit = 0;
    }
    ref_shim_state saved = g_ref_shim;
    g_ref_shim.prd = prd;
    if (ray_type == 0) {
        if (hit) {
            int32_t mesh = s->mesh_of[prim];
            g_ref_shim.program_data = &s->entities[mesh];
            g_ref_shim.bary = float2{u, v};
            g_ref_shim.t = t;
            g_ref_shim.direction = float3{dir.x, dir.y, dir.z};
            g_ref_shim.primitive = (unsigned)(prim - s->first[mesh]);
            ref_closest_hit_triangle_hit();
        } else {
            ref_miss_miss();
        }
    } else if (!hit) {
        ref_miss_miss_shadow();
    }
    saved.last_rgba_color = g_ref_shim.last_rgba_color;
    g_ref_shim = saved;
}

float4 ref_shim_tex2d(cudaTextureObject_t tex, float u, float v)
{
    float rgb[3];
    orc_tex_nearest((const orc_texture*)tex, u, v, rgb);
    return float4{rgb[0], rgb[1], rgb[2], 1.0f}; /* alpha is never read (vec3{texColor}) */
}

extern "C" {

/* ---- unit hooks: the same signatures as the oracle's orc_* hooks ---- */
uint32_t ref_rng_init(uint32_t seed_u, uint32_t seed_v) { return random{seed_u, seed_v}.state; }
float ref_rng_next(uint32_t* state)
{
    random r;
    r.state = *state;
    float f = r();
    *state = r.state;
    return f;
}

void ref_sample_disney(const float mat[ORC_MAT_FLOATS], const float wo[3], uint32_t* rng_state, int32_t* sampled_lobe, float f[3],
                       float wi[3], float* pdf)
{
    material_data m = mat_load(mat);
    random r;
    r.state = *rng_state;
    vec3 lwi{};      /* device.cu:181 local_wi{} */
    float lpdf{};    /* device.cu:183 */
    int lobe = *sampled_lobe;
    vec3 res = sample_disney(m, ld(wo), r, lwi, lpdf, lobe);
    *rng_state = r.state;
    *sampled_lobe = lobe;
    st(f, res);
    st(wi, lwi);
    *pdf = lpdf;
}

void ref_eval_lobe(int lobe, const float mat[ORC_MAT_FLOATS], const float wo[3], const float wh[3], const float wi[3], float f[3], float* pdf)
{
    material_data m = mat_load(mat);
    vec3 r{0.0f};
    float p = 0.0f;
    switch (lobe) {
    case DISNEY_SAMPLED_LOBE_DIFFUSE: r = eval_disney_diffuse(m, ld(wo), ld(wh), ld(wi), p); break;
    case DISNEY_SAMPLED_LOBE_CLEARCOAT: r = eval_disney_clearcoat(m, ld(wo), ld(wh), ld(wi), p); break;
    case DISNEY_SAMPLED_LOBE_METALLIC: r = eval_disney_specular_brdf(m, ld(wo), ld(wh), ld(wi), p); break;
    case DISNEY_SAMPLED_LOBE_GLASS: r = eval_disney_specular_bsdf(m, ld(wo), ld(wh), ld(wi), p); break;
    default: break;
    }
    st(f, r);
    *pdf = p;
}

void ref_eval_sheen(const float mat[ORC_MAT_FLOATS], const float wo[3], const float wi[3], float f[3])
{
    st(f, eval_disney_sheen(mat_load(mat), ld(wo), ld(wi)));
}

void ref_onb(const float n[3], float t[3], float b[3])
{
    vec3 tt, bb;
    onb(ld(n), tt, bb);
    st(t, tt);
    st(b, bb);
}
void ref_to_local(const float t[3], const float b[3], const float n[3], const float w[3], float out[3]) { st(out, to_local(ld(t), ld(b), ld(n), ld(w))); }
void ref_to_world(const float t[3], const float b[3], const float n[3], const float w[3], float out[3]) { st(out, to_world(ld(t), ld(b), ld(n), ld(w))); }
void ref_sample_cosine_hemisphere(float u0, float u1, float out[3]) { st(out, sample_cosine_hemisphere(vec2{u0, u1})); }
int ref_refract(const float w[3], const float n[3], float eta, float wi[3])
{
    vec3 r{0.0f};
    bool ok = refract(ld(w), ld(n), eta, r);
    st(wi, r);
    return ok ? 1 : 0;
}
float ref_fresnel_equation(const float i[3], const float m[3], float eta_i, float eta_t) { return fresnel_equation(ld(i), ld(m), eta_i, eta_t); }
float ref_d_gtr1(const float wh[3], float alpha) { return d_gtr1(ld(wh), alpha); }
float ref_d_gtr2(const float wm[3], float ax, float ay) { return d_gtr_2(ld(wm), ax, ay); }
float ref_lambda(const float w[3], float ax, float ay) { return lambda(ld(w), ax, ay); }
void ref_uv_on_sphere(const float n[3], float uv[2])
{
    vec2 r = uv_on_sphere(ld(n));
    uv[0] = r.x;
    uv[1] = r.y;
}

/* ---- scenes and launches ---- */
void* ref_scene_create(const orc_scene_desc* d)
{
    ref_scene* s = new ref_scene{};
    const int32_t n = d->n_tris;
    s->soup = orc_scene_create(d, 4);
    s->n_tris = n;
    s->mesh_of = new int32_t[n > 0 ? n : 1];
    s->first = new int32_t[n > 0 ? n : 1];
    s->entities = new entity_data[n > 0 ? n : 1];
    s->vertices = new vec3[(size_t)n * 3 + 1];
    s->normals = new vec3[(size_t)n * 3 + 1];
    s->texcoords = d->texcoords ? new vec2[(size_t)n * 3 + 1] : nullptr;
    s->indices = new ivec3[n > 0 ? n : 1];
    s->n_textures = d->n_textures;
    s->textures = new orc_texture[d->n_textures > 0 ? d->n_textures : 1];
    for (int32_t i = 0; i < d->n_textures; ++i) {
        const orc_texture& t = d->textures[i];
        uint32_t* px = new uint32_t[(size_t)t.width * t.height + 1];
        for (size_t k = 0; k < (size_t)t.width * t.height; ++k) px[k] = t.rgba8[k];
        s->textures[i] = orc_texture{t.width, t.height, px};
    }
    s->n_materials = d->n_materials;
    s->materials = d->n_materials > 0 ? new material_data[d->n_materials] : nullptr;
    for (int32_t i = 0; i < d->n_materials; ++i) s->materials[i] = mat_load(d->materials + (size_t)i * ORC_MAT_FLOATS);

    int32_t mesh = -1, local = 0, mesh_mi = 0, mesh_ti = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t mi = d->material_index[i];
        const int32_t ti = (d->texcoords && d->texture_index[i] >= 0) ? d->texture_index[i] : -1;
        if (mesh < 0 || mi != mesh_mi || ti != mesh_ti) {
            ++mesh;
            mesh_mi = mi;
            mesh_ti = ti;
            local = 0;
            s->first[mesh] = i;
            entity_data e{};
            e.mesh_index = mesh;
            e.material_index = mi;
            e.has_texture = ti >= 0;
            e.texture = ti >= 0 ? (cudaTextureObject_t)&s->textures[ti] : 0;
            s->entities[mesh] = e;
        }
        s->mesh_of[i] = mesh;
        for (int k = 0; k < 3; ++k) {
            s->vertices[(size_t)i * 3 + k] = ld(d->positions + (size_t)i * 9 + k * 3);
            s->normals[(size_t)i * 3 + k] = ld(d->normals + (size_t)i * 9 + k * 3);
            if (s->texcoords) s->texcoords[(size_t)i * 3 + k] = vec2{d->texcoords[(size_t)i * 6 + k * 2], d->texcoords[(size_t)i * 6 + k * 2 + 1]};
        }
        s->indices[i] = ivec3{3 * local, 3 * local + 1, 3 * local + 2};
        ++local;
    }
    s->n_meshes = mesh + 1;
    const int32_t nm = s->n_meshes > 0 ? s->n_meshes : 1;
    s->vbuf = new Buffer[nm];
    s->nbuf = new Buffer[nm];
    s->tbuf = new Buffer[nm];
    s->ibuf = new Buffer[nm];
    for (int32_t m = 0; m < s->n_meshes; ++m) {
        const int32_t f = s->first[m];
        const size_t cnt = (size_t)((m + 1 < s->n_meshes ? s->first[m + 1] : n) - f);
        s->vbuf[m] = Buffer{cnt * 3, s->vertices + (size_t)f * 3};
        s->nbuf[m] = Buffer{cnt * 3, s->normals + (size_t)f * 3};
        s->tbuf[m] = Buffer{s->texcoords ? cnt * 3 : 0, s->texcoords ? (void*)(s->texcoords + (size_t)f * 3) : nullptr};
        s->ibuf[m] = Buffer{cnt, s->indices + f};
    }
    return s;
}

void ref_scene_destroy(void* p)
{
    ref_scene* s = (ref_scene*)p;
    if (!s) return;
    orc_scene_destroy(s->soup);
    for (int32_t i = 0; i < s->n_textures; ++i) delete[] s->textures[i].rgba8;
    delete[] s->textures;
    delete[] s->mesh_of; delete[] s->first; delete[] s->entities;
    delete[] s->vertices; delete[] s->normals; delete[] s->texcoords; delete[] s->indices;
    delete[] s->vbuf; delete[] s->nbuf; delete[] s->tbuf; delete[] s->ibuf;
    delete[] s->materials;
    delete s;
}

int ref_scene_meshes(const void* p) { return ((const ref_scene*)p)->n_meshes; }

/* ray_gen (device.cu:220-254) for every pixel, one launch index at a time.  out_rgb: W*H*3 floats at the framebuffer
   offset ray_gen writes (the float colour handed to make_rgba); out_rgba8: W*H, written by ray_gen itself.
   Returns 0, or 1 if a pixel ran out of its trace budget. */
int ref_render(const void* scene, const orc_camera* cam, const orc_env* env, int W, int H, int max_samples, int max_depth, float* out_rgb,
               uint32_t* out_rgba8)
{
    const ref_scene* s = (const ref_scene*)scene;
    set_launch(s, env, max_samples, max_depth);
    ray_gen_data rg;
    rg.fb_ptr = out_rgba8;
    rg.fb_size = ivec2{W, H};
    rg.camera = camera_load(cam);
    int overflow = 0;
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            g_ref_shim.program_data = &rg;
            g_ref_shim.launch_index = ivec2{px, py};
            g_trace_budget = (int64_t)max_samples * (max_depth + 1) * 65;
            g_trace_overflow = 0;
            ref_raygen_ray_gen();
            overflow |= g_trace_overflow;
            st(out_rgb + ((size_t)px + (size_t)W * (size_t)(H - 1 - py)) * 3, g_ref_shim.last_rgba_color);
        }
    return overflow;
}

/* Per-sample radiance and rng state of one pixel: the sample loop of ray_gen (device.cu:226-243) around the
   reference's trace_path.  Returns 0, or 1 on trace budget overflow. */
int ref_trace_pixel(const void* scene, const orc_camera* cam, const orc_env* env, int W, int H, int px, int py, int max_samples, int max_depth,
                    float* per_sample_rgb, uint32_t* per_sample_state)
{
    const ref_scene* s = (const ref_scene*)scene;
    set_launch(s, env, max_samples, max_depth);
    const camera_data c = camera_load(cam);
    const ivec2 pixelId{px, py}, fb_size{W, H};
    random pxRand{(uint32_t)pixelId.x, (uint32_t)pixelId.y};
    g_trace_budget = (int64_t)max_samples * (max_depth + 1) * 65;
    g_trace_overflow = 0;
    for (int32_t smp = 0; smp < max_samples; ++smp) {
        vec2 const rand{pxRand(), pxRand()};
        vec2 const screen{(vec2{pixelId} + rand) / vec2{fb_size}};
        radiance_ray ray{c.origin, normalize(c.llc + screen.u * c.horizontal + screen.v * c.vertical - c.origin), t_min, t_max};
        int32_t sample = smp;
        st(per_sample_rgb + (size_t)smp * 3, trace_path(ray, pxRand, sample));
        per_sample_state[smp] = pxRand.state;
    }
    return g_trace_overflow;
}

} /* extern "C" */
