// main.cpp -- host entry point with the reference's file-level behaviour (path_tracer/Main.cpp:13-31,
// path_tracer/src/application.cpp:143-181,297-371, application.hpp:89-108): read CWD/assets/settings.json, <scene>.json,
// <scene>.obj.scene (+ environment.hdr, textures), then run the material sweep ("test_loop") and write one PNG per step as
// <scene>_<test.name>_<attribute_name>(<value>).png in the CWD.  The render itself goes through the C-ABI (mi355pt.h).
//
// Optional flags (defaults reproduce the reference, which has no CLI): --assets DIR, --out DIR, --settings FILE, --device N
// (-1: load + build only, no render), --gpus N (devices --device .. --device + N - 1 of this node, default 0..N-1: pixel tiles sharded over them, one RCCL reduce of the
// float3 framebuffer onto device 0 - pt_group_* in mi355pt.h; the image is bit-identical to --gpus 1), --devices a,b,c (the same
// group path on exactly these devices, the reduce onto the first; with --gpus the counts must agree, with --device it is an error;
// a device named twice is refused by the real RCCL), --dump-scene FILE (binary dump of the ingested scene for the loader tests),
// --batch K (K >= 1: test_loop collects K sweep steps and renders them with ONE pt_render_batch - one launch sequence for K frames -
// instead of K x pt_set_materials + pt_render; the PNGs are byte for byte the same; not together with --gpus / --devices),
// --watertight (option "watertight" = 1 on every context: the watertight triangle test, mi355pt.h; not together with --batch).
// --aov N (N >= 1: after every frame the guide pass with N samples per pixel - pt_render_aov / pt_group_render_aov, mi355pt.h - and three
// more files next to <name>.png: <name>_albedo.png = make_rgba of the albedo, <name>_normal.png = make_rgba of 0.5 * n + 0.5,
// <name>_depth.png = grey, depth / the frame's largest depth; works with --gpus / --devices and --watertight, not with --batch).
// --follow K [--follow-roughness R] (needs --aov N: the guide pass in follow mode - pt_render_aov_follow / pt_group_render_aov_follow with
// max_follow = K in 0..8 and roughness_max = R in 0..1, default 0.3 - the same three files, and what --denoise consumes).
// --denoise (needs --aov N, so not with --batch either: after every frame and its guides pt_denoise with the default parameters - mi355pt.h,
// "denoiser" - and one more file, <name>_denoised.png = the filter's RGBA8 image; with --gpus / --devices the filter runs on the first
// device's context, which holds the reduced frame).
// --adds K (1 <= K <= max_samples: every frame is a progressive accumulation - pt_accum_begin, K uniform pt_accum_add of max_samples / K
// samples, the remainder with the last, pt_accum_end; mi355pt.h, "progressive accumulation" - and the files are byte for byte those
// without the flag; works with --watertight, --aov and --denoise, not with --gpus / --devices or --batch).
// --denoise-variance (needs --adds K with K >= 2 and --aov N, not with --denoise: after every frame and its guides pt_accum_denoise with the
// default parameters - mi355pt.h, "variance-guided denoise" - on the frame's accumulation; <name>_denoised.png = its RGBA8 image).
// --upsample K (K in 2..8; needs --aov N, not with --batch, --adds, --denoise-variance or --gpus / --devices: every frame is rendered at
// ceil(W / K) x ceil(H / K), the guide pass runs at both sizes, --denoise filters the low frame, and pt_upsample with the default
// parameters - mi355pt.h, "upsampling" - lifts it to W x H; <name>.png is that image and the only file of the frame).
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mi355pt.h"
#include "image_io.h"
#include "scene_loader.h"

namespace {

bool file_exists(const std::string& p)
{
    struct stat st;
    return ::stat(p.c_str(), &st) == 0;
}

void dump_scene(const std::string& path, const host::Scene& s)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + path);
    auto w32 = [&](int32_t v) { std::fwrite(&v, 4, 1, f); };
    auto wstr = [&](const std::string& t) { w32((int32_t)t.size()); std::fwrite(t.data(), 1, t.size(), f); };
    std::fwrite("PTSC", 1, 4, f);
    std::fwrite(&s.camera, sizeof(float), 10, f);
    w32((int32_t)s.materials.size());
    for (auto const& m : s.materials) { wstr(m.name); std::fwrite(m.data.data(), 4, host::kMatFloats, f); wstr(m.texture_file); }
    w32((int32_t)s.meshes.size());
    for (auto const& m : s.meshes) {
        wstr(m.name);
        w32((int32_t)(m.vertices.size() / 3)); w32((int32_t)(m.normals.size() / 3)); w32((int32_t)(m.texcoords.size() / 2)); w32((int32_t)(m.indices.size() / 3));
        std::fwrite(m.vertices.data(), 4, m.vertices.size(), f);
        std::fwrite(m.normals.data(), 4, m.normals.size(), f);
        std::fwrite(m.texcoords.data(), 4, m.texcoords.size(), f);
        std::fwrite(m.indices.data(), 4, m.indices.size(), f);
    }
    w32((int32_t)s.entities.size());
    for (auto const& e : s.entities) { w32(e.mesh); w32(e.material); }
    std::fclose(f);
}

// --devices a,b,c: non-negative integers, at least one
std::vector<int32_t> parse_devices(const std::string& list)
{
    std::vector<int32_t> devs;
    size_t p = 0;
    for (;;) {
        const size_t q = list.find(',', p);
        const std::string tok = list.substr(p, q == std::string::npos ? std::string::npos : q - p);
        if (tok.empty() || tok.size() > 6 || tok.find_first_not_of("0123456789") != std::string::npos)
            throw std::runtime_error("--devices needs a comma-separated list of non-negative device numbers, got '" + list + "'");
        devs.push_back((int32_t)std::atoi(tok.c_str()));
        if (q == std::string::npos) break;
        p = q + 1;
    }
    return devs;
}

std::string fmt1(float v)
{
    char b[64];
    std::snprintf(b, sizeof(b), "%.1f", v); // fmt "{:.1f}" (application.hpp:101-105)
    return b;
}

struct App {
    host::Settings settings;
    host::Scene scene;
    std::vector<float> materials; // n * 17
    pt_ctx* ctx = nullptr;     // device 0's context (all of them for --gpus 1)
    pt_group* group = nullptr; // --gpus N: N contexts + the library's RCCL communicator
    pt_camera cam{};
    std::string out_dir;
    int batch = 0; // --batch K: sweep steps per pt_render_batch (0: one pt_render per step)
    int aov = 0;   // --aov N: samples per pixel of the guide pass after every frame (0: none)
    int follow = -1;               // --follow K: the guide pass in follow mode, max_follow = K (-1: first hit, pt_render_aov)
    float follow_roughness = -1.0f; // --follow-roughness R: roughness_max (< 0: the default of pt_aov_default_params)
    bool denoise = false; // --denoise: pt_denoise of every frame with its guides
    int adds = 0;  // --adds K: every frame in K uniform adds of a progressive accumulation (0: one pt_render)
    bool denoise_variance = false; // --denoise-variance: pt_accum_denoise of every frame's accumulation with its guides
    int upsample = 0; // --upsample K: render at 1/K of the size in each direction, pt_upsample to the full size (0: render at full size)
};

void check(App& a, int rc, const char* what)
{
    if (rc < 0) throw std::runtime_error(std::string(what) + ": " + (a.group ? pt_group_last_error(a.group) : pt_last_error(a.ctx)));
}

// owl::make_rgba as csrc/pt_device.h has it: min(255, max(0, int(f * 256))) per channel, alpha 255
uint32_t make_8bit(float f)
{
    const float s = f * 256.0f;
    int v = (s != s) ? 0 : (s >= 2147483520.0f ? 2147483647 : (s <= -2147483520.0f ? -2147483647 : (int)s));
    v = v < 0 ? 0 : v;
    return (uint32_t)(v > 255 ? 255 : v);
}
uint32_t make_rgba(float r, float g, float b) { return make_8bit(r) | (make_8bit(g) << 8) | (make_8bit(b) << 16) | (0xffu << 24); }

// the guide pass of --aov (first hit, or --follow) at W x H into g
void render_guides(App& a, int W, int H, std::vector<float>& g)
{
    g.resize((size_t)W * H * 8);
    if (a.follow >= 0) {
        pt_aov_params prm;
        pt_aov_default_params(&prm);
        prm.n_samples = a.aov;
        prm.max_follow = a.follow;
        if (a.follow_roughness >= 0.0f) prm.roughness_max = a.follow_roughness;
        if (a.group) check(a, pt_group_render_aov_follow(a.group, &a.cam, W, H, &prm, g.data()), "pt_group_render_aov_follow");
        else check(a, pt_render_aov_follow(a.ctx, &a.cam, W, H, &prm, g.data()), "pt_render_aov_follow");
    } else if (a.group) check(a, pt_group_render_aov(a.group, &a.cam, W, H, a.aov, g.data()), "pt_group_render_aov");
    else check(a, pt_render_aov(a.ctx, &a.cam, W, H, a.aov, g.data()), "pt_render_aov");
}

// --aov: the guide buffers of the frame just rendered, as three PNGs next to it (base = the frame's path without ".png");
// --denoise: the frame (rgb) filtered with them, as a fourth
void write_guides(App& a, const std::string& base, const std::vector<float>& rgb)
{
    const int W = a.settings.buffer_size[0], H = a.settings.buffer_size[1];
    const size_t npx = (size_t)W * H;
    std::vector<float> g;
    render_guides(a, W, H, g);
    float far = 0.0f;
    for (size_t i = 0; i < npx; ++i) far = g[8 * i + 7] > far ? g[8 * i + 7] : far;
    std::vector<uint32_t> albedo(npx), normal(npx), depth(npx);
    for (size_t i = 0; i < npx; ++i) {
        const float* p = &g[8 * i];
        albedo[i] = make_rgba(p[0], p[1], p[2]);
        normal[i] = make_rgba(0.5f * p[4] + 0.5f, 0.5f * p[5] + 0.5f, 0.5f * p[6] + 0.5f);
        const float d = far > 0.0f ? p[7] / far : 0.0f;
        depth[i] = make_rgba(d, d, d);
    }
    const char* names[3] = {"_albedo.png", "_normal.png", "_depth.png"};
    const std::vector<uint32_t>* img[3] = {&albedo, &normal, &depth};
    for (int k = 0; k < 3; ++k) {
        imgio::write_png_rgba8(base + names[k], W, H, img[k]->data());
        std::printf("Image written to %s\n", (base + names[k]).c_str());
    }
    if (!a.denoise && !a.denoise_variance) return;
    std::vector<float> out(npx * 3);
    std::vector<uint32_t> out8(npx);
    if (a.denoise_variance) { // the frame's accumulation is still open (render_frame): filtered where it lies, with its own variance estimate
        if (pt_accum_denoise(a.ctx, g.data(), nullptr, out.data(), out8.data()) < 0) throw std::runtime_error(std::string("pt_accum_denoise: ") + pt_last_error(a.ctx));
    } else if (pt_denoise(a.ctx, rgb.data(), g.data(), W, H, nullptr, out.data(), out8.data()) < 0) throw std::runtime_error(std::string("pt_denoise: ") + pt_last_error(a.ctx));
    imgio::write_png_rgba8(base + "_denoised.png", W, H, out8.data());
    std::printf("Image written to %s\n", (base + "_denoised.png").c_str());
}

// --upsample K: the frame at ceil(W / K) x ceil(H / K) under the SAME camera (pt_camera is resolution-independent), guides at both sizes,
// --denoise at the low size, pt_upsample to W x H
void render_frame_upsampled(App& a, const std::string& values)
{
    std::fprintf(stderr, "TRACING\n");
    const int W = a.settings.buffer_size[0], H = a.settings.buffer_size[1];
    const int w = (W + a.upsample - 1) / a.upsample, h = (H + a.upsample - 1) / a.upsample;
    std::vector<float> lo((size_t)w * h * 3), g_lo, g_hi, out((size_t)W * H * 3);
    std::vector<uint32_t> rgba((size_t)W * H);
    check(a, pt_render(a.ctx, &a.cam, w, h, a.settings.max_samples, a.settings.max_path_depth, lo.data(), nullptr), "pt_render");
    pt_stats st;
    pt_get_stats(a.ctx, &st);
    render_guides(a, w, h, g_lo);
    if (a.denoise) check(a, pt_denoise(a.ctx, lo.data(), g_lo.data(), w, h, nullptr, lo.data(), nullptr), "pt_denoise");
    render_guides(a, W, H, g_hi);
    check(a, pt_upsample(a.ctx, lo.data(), g_lo.data(), w, h, g_hi.data(), W, H, nullptr, out.data(), rgba.data()), "pt_upsample");
    pt_stats su;
    pt_get_stats(a.ctx, &su);
    std::string path = a.out_dir + "/" + a.settings.scene + "_" + a.settings.test.name + "_" + a.settings.test.attribute_name + "(" + values + ").png";
    imgio::write_png_rgba8(path, W, H, rgba.data());
    std::printf("Image written to %s\n", path.c_str());
    std::fprintf(stderr, "  %.1f ms render kernel at %dx%d, %.3f ms upsample to %dx%d\n", st.kernel_ms, w, h, su.kernel_ms, W, H);
}

// render_frame, application.cpp:363-371
void render_frame(App& a, const std::string& values)
{
    if (a.upsample > 0) return render_frame_upsampled(a, values);
    std::fprintf(stderr, "TRACING\n");
    const int W = a.settings.buffer_size[0], H = a.settings.buffer_size[1];
    std::vector<float> rgb((size_t)W * H * 3);
    std::vector<uint32_t> rgba((size_t)W * H);
    double adds_ms = 0.0;
    if (a.adds > 0) { // the frame grows by a.adds uniform adds; only the last add's image is kept
        check(a, pt_accum_begin(a.ctx, &a.cam, W, H, a.settings.max_path_depth), "pt_accum_begin");
        pt_accum_params prm;
        pt_accum_default_params(&prm);
        const int each = a.settings.max_samples / a.adds;
        for (int k = 0; k < a.adds; ++k) {
            const bool last = k + 1 == a.adds;
            prm.n_samples = last ? a.settings.max_samples - each * (a.adds - 1) : each;
            check(a, pt_accum_add(a.ctx, &prm, last ? rgb.data() : nullptr, last ? rgba.data() : nullptr), "pt_accum_add");
            pt_stats sk;
            if (pt_get_stats(a.ctx, &sk) == PT_OK) adds_ms += sk.kernel_ms;
        }
        // (the accumulation stays open for --denoise-variance: ended below, after the guides)
    } else if (a.group) check(a, pt_group_render(a.group, &a.cam, W, H, a.settings.max_samples, a.settings.max_path_depth, rgb.data(), rgba.data()), "pt_group_render");
    else check(a, pt_render(a.ctx, &a.cam, W, H, a.settings.max_samples, a.settings.max_path_depth, rgb.data(), rgba.data()), "pt_render");
    pt_stats st;
    pt_get_stats(a.ctx, &st);
    if (a.adds > 0) st.kernel_ms = adds_ms; // the kernels of all adds
    for (int32_t i = 1; i < pt_group_size(a.group); ++i) { // the frame takes as long as its slowest rank
        pt_stats si;
        if (pt_get_stats(pt_group_ctx(a.group, i), &si) == PT_OK && si.kernel_ms > st.kernel_ms) st.kernel_ms = si.kernel_ms;
    }
    std::string name = a.settings.scene + "_" + a.settings.test.name + "_" + a.settings.test.attribute_name + "(" + values + ").png";
    std::string path = a.out_dir + "/" + name;
    imgio::write_png_rgba8(path, W, H, rgba.data());
    std::printf("Image written to %s\n", path.c_str());
    std::fprintf(stderr, "  %.1f ms kernel, %.1f Msamples/s\n", st.kernel_ms, (double)W * H * a.settings.max_samples / (st.kernel_ms * 1e3));
    if (a.aov > 0) write_guides(a, path.substr(0, path.size() - 4), rgb);
    if (a.adds > 0) check(a, pt_accum_end(a.ctx), "pt_accum_end");
}

// --batch: the collected sweep steps (material table and value string each) as one pt_render_batch; one PNG per step as render_frame writes it
void render_batch(App& a, const std::vector<std::vector<float>>& tables, const std::vector<std::string>& values)
{
    std::fprintf(stderr, "TRACING (batch of %zu)\n", tables.size());
    const int W = a.settings.buffer_size[0], H = a.settings.buffer_size[1];
    const size_t K = tables.size(), npx = (size_t)W * H;
    std::vector<pt_frame> frames(K);
    for (size_t f = 0; f < K; ++f) {
        frames[f].camera = a.cam;
        frames[f].materials = tables[f].data();
    }
    std::vector<float> rgb(K * npx * 3);
    std::vector<uint32_t> rgba(K * npx);
    check(a, pt_render_batch(a.ctx, frames.data(), (int32_t)K, (int32_t)a.scene.materials.size(), W, H, a.settings.max_samples, a.settings.max_path_depth, rgb.data(),
                             rgba.data()), "pt_render_batch");
    pt_stats st;
    pt_get_stats(a.ctx, &st);
    for (size_t f = 0; f < K; ++f) {
        std::string name = a.settings.scene + "_" + a.settings.test.name + "_" + a.settings.test.attribute_name + "(" + values[f] + ").png";
        std::string path = a.out_dir + "/" + name;
        imgio::write_png_rgba8(path, W, H, rgba.data() + f * npx);
        std::printf("Image written to %s\n", path.c_str());
    }
    std::fprintf(stderr, "  %.1f ms kernel for %zu frames (%d launches), %.1f Msamples/s\n", st.kernel_ms, K, st.launches,
                 (double)K * W * H * a.settings.max_samples / (st.kernel_ms * 1e3));
}

float* find_material(App& a)
{ // get_material, application.cpp:307-317 (the reference dereferences end() when the name is unknown; we report it)
    for (size_t i = 0; i < a.scene.materials.size(); ++i)
        if (a.scene.materials[i].name == a.settings.test.material_name) return &a.materials[i * host::kMatFloats];
    throw std::runtime_error("test.material_name '" + a.settings.test.material_name + "' is not a material of the scene");
}

// test_loop<T>, application.hpp:89-108
void test_loop(App& a)
{
    const host::TestData& t = a.settings.test;
    const int vstep = (int)(t.step_size * 100);
    if (vstep <= 0) throw std::runtime_error("test.step_size * 100 < 1: the reference would loop forever (application.hpp:94-95)");
    const bool vec = !t.vec_values.empty(); // Main.cpp:25-28
    if (vec ? t.vec_values.size() < 2 : t.flt_values.size() < 2) throw std::runtime_error("test.values needs two entries");
    float* mat = find_material(a);
    const int attr = host::attribute_index(t.attribute_name);
    std::vector<std::vector<float>> tables; // --batch: the steps collected so far
    std::vector<std::string> names;
    for (int i = 0; i <= 100; i += vstep) {
        const float c = i / 100.0f;
        std::string values;
        if (vec) { // modify_sbt(vec3): base_color (application.cpp:320-326)
            for (int k = 0; k < 3; ++k) {
                float v = t.vec_values[0][k] + (t.vec_values[1][k] - t.vec_values[0][k]) * c;
                mat[k] = v;
                values += (k ? "," : "") + fmt1(v);
            }
        } else { // modify_sbt(float): one named attribute; unknown names change nothing (application.cpp:329-360)
            float v = t.flt_values[0] + (t.flt_values[1] - t.flt_values[0]) * c;
            if (attr >= 0) mat[attr] = v;
            values = fmt1(v);
        }
        if (a.batch > 0) { // the step's table goes into the batch; the context's own table is not touched
            tables.push_back(a.materials);
            names.push_back(values);
            if ((int)tables.size() == a.batch || i + vstep > 100) {
                render_batch(a, tables, names);
                tables.clear();
                names.clear();
            }
            continue;
        }
        if (a.group) check(a, pt_group_set_materials(a.group, a.materials.data(), (int32_t)a.scene.materials.size()), "pt_group_set_materials");
        else check(a, pt_set_materials(a.ctx, a.materials.data(), (int32_t)a.scene.materials.size()), "pt_set_materials"); // reset_field
        render_frame(a, values);
    }
}

} // namespace

int main(int argc, char** argv)
{
    try {
        App a;
        char cwd[4096];
        if (!getcwd(cwd, sizeof(cwd))) throw std::runtime_error("getcwd failed");
        std::string assets = std::string(cwd) + "/assets"; // Main.cpp:17
        std::string settings_path, dump;
        a.out_dir = cwd;
        int device = 0, gpus = 0; // gpus 0: flag not given, single context as in the reference
        bool have_upsample = false;
        bool have_device = false, have_devices = false, have_batch = false, have_adds = false, have_aov = false, have_follow = false, have_follow_roughness = false, watertight = false;
        std::vector<int32_t> devs; // --devices
        for (int i = 1; i < argc; ++i) {
            std::string k = argv[i];
            auto next = [&]() { if (i + 1 >= argc) throw std::runtime_error("missing value for " + k); return std::string(argv[++i]); };
            if (k == "--assets") assets = next();
            else if (k == "--out") a.out_dir = next();
            else if (k == "--settings") settings_path = next();
            else if (k == "--device") { device = std::atoi(next().c_str()); have_device = true; }
            else if (k == "--devices") { devs = parse_devices(next()); have_devices = true; }
            else if (k == "--gpus") gpus = std::atoi(next().c_str());
            else if (k == "--dump-scene") dump = next();
            else if (k == "--batch") { a.batch = std::atoi(next().c_str()); have_batch = true; }
            else if (k == "--aov") { a.aov = std::atoi(next().c_str()); have_aov = true; }
            else if (k == "--follow") { a.follow = std::atoi(next().c_str()); have_follow = true; }
            else if (k == "--follow-roughness") { a.follow_roughness = (float)std::atof(next().c_str()); have_follow_roughness = true; }
            else if (k == "--watertight") watertight = true;
            else if (k == "--denoise") a.denoise = true;
            else if (k == "--denoise-variance") a.denoise_variance = true;
            else if (k == "--adds") { a.adds = std::atoi(next().c_str()); have_adds = true; }
            else if (k == "--upsample") { a.upsample = std::atoi(next().c_str()); have_upsample = true; }
            else if (k == "--convert-png" || k == "--convert-hdr") { // codec self-test hooks: decode with our reader, re-encode with our writer
                std::string in = next(), out = next();
                imgio::Image img = k == "--convert-png" ? imgio::load_png_rgba8(in) : imgio::load_hdr_as_ldr_rgba8(in);
                imgio::write_png_rgba8(out, img.width, img.height, img.rgba.data());
                return 0;
            }
            else throw std::runtime_error("unknown option " + k);
        }
        if (gpus < 0) throw std::runtime_error("--gpus needs a positive count");
        if (have_adds && a.adds < 1) throw std::runtime_error("--adds needs a positive number of adds per frame");
        if (have_adds && (gpus > 0 || have_devices)) throw std::runtime_error("--adds cannot be combined with --gpus / --devices (pt_accum_* has no group form)");
        if (have_adds && have_batch) throw std::runtime_error("--adds cannot be combined with --batch (there are no batches of accumulations)");
        if (have_batch && a.batch < 1) throw std::runtime_error("--batch needs a positive number of frames per batch");
        if (have_batch && (gpus > 0 || have_devices)) throw std::runtime_error("--batch cannot be combined with --gpus / --devices yet (pt_group_* has no batch call)");
        if (have_devices) {
            if (have_device) throw std::runtime_error("--devices and --device exclude each other (--devices lists every device)");
            if (gpus > 0 && gpus != (int)devs.size())
                throw std::runtime_error("--devices names " + std::to_string(devs.size()) + " device(s) but --gpus says " + std::to_string(gpus));
            gpus = (int)devs.size();
        }
        if (a.denoise && have_batch) throw std::runtime_error("--denoise cannot be combined with --batch (it needs the guides of --aov, which has no batch form)");
        if (a.denoise && !have_aov) throw std::runtime_error("--denoise needs --aov N (the filter is driven by the guide buffers)");
        if (a.denoise_variance && a.denoise) throw std::runtime_error("--denoise-variance cannot be combined with --denoise (both write <name>_denoised.png)");
        if (a.denoise_variance && (!have_adds || a.adds < 2))
            throw std::runtime_error("--denoise-variance needs --adds K with K >= 2 (the variance estimate comes from the two halves of an accumulation's samples)");
        if (a.denoise_variance && !have_aov) throw std::runtime_error("--denoise-variance needs --aov N (the filter is driven by the guide buffers)");
        if (have_upsample && have_batch) throw std::runtime_error("--upsample cannot be combined with --batch (pt_upsample has no batch form)");
        if (have_upsample && !have_aov) throw std::runtime_error("--upsample needs --aov N (the upsampling is driven by the guide buffers at both sizes)");
        if (have_upsample && (a.upsample < 2 || a.upsample > 8)) throw std::runtime_error("--upsample needs a factor 2..8");
        if (have_upsample && (have_adds || a.denoise_variance)) throw std::runtime_error("--upsample cannot be combined with --adds / --denoise-variance (it renders the low frame with one pt_render)");
        if (have_upsample && (gpus > 0 || have_devices)) throw std::runtime_error("--upsample cannot be combined with --gpus / --devices (pt_upsample has no group form)");
        if (have_follow && !have_aov) throw std::runtime_error("--follow needs --aov N (it is a mode of the guide pass)");
        if (have_follow && (a.follow < 0 || a.follow > 8)) throw std::runtime_error("--follow needs a number of surfaces 0..8");
        if (have_follow_roughness && !have_follow) throw std::runtime_error("--follow-roughness needs --follow K");
        if (have_follow_roughness && !(a.follow_roughness >= 0.0f && a.follow_roughness <= 1.0f)) throw std::runtime_error("--follow-roughness needs a value 0..1");
        if (have_aov && a.aov < 1) throw std::runtime_error("--aov needs a positive number of samples per pixel");
        if (have_aov && have_batch) throw std::runtime_error("--aov cannot be combined with --batch (the guide pass has no batch form)");
        if (have_batch && watertight) throw std::runtime_error("--batch cannot be combined with --watertight (pt_render_batch has no watertight instances)");
        if (settings_path.empty()) settings_path = assets + "/settings.json"; // application.cpp:145

        std::fprintf(stderr, "Parsing settings\n");
        a.settings = host::parse_settings(settings_path);
        if (have_adds && a.adds > a.settings.max_samples)
            throw std::runtime_error("--adds " + std::to_string(a.adds) + " exceeds max_samples = " + std::to_string(a.settings.max_samples) + " (every add needs at least one sample)");
        std::fprintf(stderr, "Parsing camera\nParsing materials\n");
        a.scene = host::load_scene(assets, a.settings.scene);
        for (auto const& m : a.scene.materials) std::fprintf(stderr, " - %s\n", m.name.c_str());
        if (!dump.empty()) dump_scene(dump, a.scene);

        // environment map (application.cpp:160; image_buffer.cpp:36-58)
        imgio::Image env_img;
        const std::string env_path = assets + "/environment.hdr";
        if (file_exists(env_path)) {
            env_img = imgio::load_hdr_as_ldr_rgba8(env_path);
            imgio::flip_vertical(env_img);
        } else {
            std::fprintf(stderr, "Image file %s does not exist. Continue with empty.\n", env_path.c_str());
        }

        // entities -> pt_mesh (application.cpp:186-247)
        std::vector<pt_mesh> meshes;
        std::vector<imgio::Image> tex_images;
        std::vector<int> tex_of_material(a.scene.materials.size(), -1);
        for (auto const& e : a.scene.entities) {
            const host::Mesh& m = a.scene.meshes[e.mesh];
            pt_mesh pm{};
            pm.vertices = m.vertices.data(); pm.n_vertices = (int32_t)(m.vertices.size() / 3);
            pm.normals = m.normals.empty() ? nullptr : m.normals.data(); pm.n_normals = (int32_t)(m.normals.size() / 3);
            pm.texcoords = m.texcoords.empty() ? nullptr : m.texcoords.data(); pm.n_texcoords = (int32_t)(m.texcoords.size() / 2);
            pm.indices = m.indices.data(); pm.n_triangles = (int32_t)(m.indices.size() / 3);
            pm.material_index = e.material;
            pm.texture_index = -1;
            const std::string& tf = a.scene.materials[e.material].texture_file;
            if (!tf.empty()) {
                if (tex_of_material[e.material] < 0) {
                    const std::string tp = assets + "/" + tf;
                    if (file_exists(tp)) {
                        imgio::Image img = imgio::load_png_rgba8(tp);
                        imgio::flip_vertical(img); // application.cpp:229-234
                        tex_of_material[e.material] = (int)tex_images.size();
                        tex_images.push_back(std::move(img));
                    } else {
                        // The reference prints this warning and RETURNS from bind_sbt_data, leaving the pipeline unbuilt
                        // (application.cpp:219-223, a bug).  Documented divergence: render the entity untextured.
                        std::fprintf(stderr, "Image file %s does not exist. Continue with empty.\n", tp.c_str());
                    }
                }
                pm.texture_index = tex_of_material[e.material];
            }
            meshes.push_back(pm);
        }
        std::vector<pt_texture> textures;
        for (auto const& img : tex_images) textures.push_back({img.width, img.height, img.rgba.data()});
        for (auto const& m : a.scene.materials) a.materials.insert(a.materials.end(), m.data.begin(), m.data.end());

        pt_env env{};
        env.use_map = a.settings.environment_use;
        env.use_auto = a.settings.environment_auto;
        for (int i = 0; i < 3; ++i) env.color[i] = a.settings.environment_color[i];
        env.intensity = a.settings.environment_intensity;
        env.map = {env_img.width, env_img.height, env_img.rgba.empty() ? nullptr : env_img.rgba.data()};

        if (meshes.empty()) throw std::runtime_error("no geometries"); // application.cpp:133
        if (gpus >= 1 && device >= 0) { // devices device..device+gpus-1: a scene replica on each, the library's communicator across them
            if (!have_devices)
                for (int i = 0; i < gpus; ++i) devs.push_back(device + i);
            a.group = pt_group_create(devs.data(), gpus);
            if (!a.group) throw std::runtime_error(std::string("pt_group_create: ") + pt_last_error(nullptr));
            a.ctx = pt_group_ctx(a.group, 0);
            check(a, pt_group_upload_scene(a.group, meshes.data(), (int32_t)meshes.size(), a.materials.data(), (int32_t)a.scene.materials.size(),
                                           textures.data(), (int32_t)textures.size(), nullptr, &env), "pt_group_upload_scene");
        } else {
            pt_config cfg{device, 0};
            a.ctx = pt_create(&cfg);
            if (!a.ctx) throw std::runtime_error(std::string("pt_create: ") + pt_last_error(nullptr));
            check(a, pt_upload_scene(a.ctx, meshes.data(), (int32_t)meshes.size(), a.materials.data(), (int32_t)a.scene.materials.size(),
                                     textures.data(), (int32_t)textures.size(), nullptr, &env), "pt_upload_scene");
        }
        if (watertight) {
            if (a.group) check(a, pt_group_set_option(a.group, "watertight", 1), "pt_group_set_option");
            else check(a, pt_set_option(a.ctx, "watertight", 1), "pt_set_option");
        }
        pt_to_camera_data(a.scene.camera.look_from, a.scene.camera.look_at, a.scene.camera.look_up, a.scene.camera.vertical_fov,
                          a.settings.buffer_size[0], a.settings.buffer_size[1], &a.cam); // parse_camera -> to_camera_data
        pt_stats st;
        pt_get_stats(a.ctx, &st);
        std::fprintf(stderr, "scene '%s': %llu triangles in %zu entities, BVH %llu nodes depth %llu (%.1f ms)\n", a.settings.scene.c_str(),
                     (unsigned long long)st.n_triangles, meshes.size(), (unsigned long long)st.bvh_nodes, (unsigned long long)st.bvh_depth, st.bvh_build_ms);
        if (device >= 0) test_loop(a);
        else std::fprintf(stderr, "--device -1: scene loaded and BVH built, no render\n");
        if (a.group) pt_group_destroy(a.group);
        else pt_destroy(a.ctx); // Main.cpp:30
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
