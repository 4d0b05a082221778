/*
 * mi355pt.h -- C-ABI of the MI355X-native path-tracing render loop (libmi355pt.so).
 *
 * Drop-in boundary for the hot path of jctemp/owl-path-tracer: everything between
 * `owlLaunch2D(ray_gen, W, H, lp)` (path_tracer/src/application.cpp:366) and the framebuffer being
 * readable, i.e. ray_gen / trace_path / triangle_hit / miss (path_tracer/src/device/device.cu:113-293),
 * the OptiX traversal they call, and the host->device contract that application.cpp fills in
 * (launch_params_data, ray_gen_data, entity_data: path_tracer/src/device/device_global.hpp:38-74).
 * The reference has no FFI of its own; each entry point below names the reference call(s) it replaces.
 *
 * Plain C, POD structs, plain pointers and sizes; no C++/torch types cross this boundary.  Every call
 * returns 0 on success or a negative PT_E_* code (no exception crosses the ABI; message via
 * pt_last_error).  A context is bound to one GPU and is not thread-safe (same as the reference: single
 * host thread, application.cpp).  Caller owns every input array (copied during the call) and every
 * output array; the library owns device memory, the BVH and its stream.
 */
#ifndef MI355PT_H
#define MI355PT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_ABI_VERSION 5
#define PT_MAT_FLOATS 17 /* material_data: device_global.hpp:19-36, 68 bytes, field order kept */

enum {
    PT_OK = 0,
    PT_E_INVALID = -1,   /* bad argument (the reference would throw std::runtime_error / trap) */
    PT_E_NO_DEVICE = -2, /* no usable gfx950 device / HIP runtime failure at create */
    PT_E_HIP = -3,       /* a HIP call failed (message has the HIP error string) */
    PT_E_NO_SCENE = -4,  /* render before upload ("no geometries", application.cpp:133) */
    PT_E_LIMIT = -5      /* scene exceeds an internal limit (BVH depth / index range) */
};

typedef struct pt_ctx pt_ctx;

typedef struct pt_config {
    int32_t device;   /* HIP device ordinal (reference: create_context(nullptr, 1), application.cpp:62) */
    int32_t reserved; /* must be 0 */
} pt_config;

/* One entity = one OBJ object that matched a material (application.cpp:166-179, :186-247).
 * Arrays as produced by create_mesh (utils/mesh_loader.cpp:9-83). */
typedef struct pt_mesh {
    const float* vertices;   /* n_vertices * 3   (vertex_buffer, application.cpp:197) */
    const float* normals;    /* n_normals * 3    (normal_buffer, :198) -- must cover every vertex index */
    const float* texcoords;  /* n_texcoords * 2  (texcoords_buffer, :200) or NULL */
    const int32_t* indices;  /* n_triangles * 3  (index_buffer, :199) */
    int32_t n_vertices, n_normals, n_texcoords, n_triangles;
    int32_t material_index;  /* entity_data.material_index (:212); <0 => material_data{} defaults (device.cu:150-154) */
    int32_t texture_index;   /* index into textures[] or <0 (entity_data.has_texture/texture, :236-243) */
} pt_mesh;

/* RGBA8 image, row 0 = v = 0, i.e. AFTER the vertical flip the reference applies at load
 * (application.cpp:229-234, utils/image_buffer.cpp:50-55); sampled nearest / clamp / normalised
 * coordinates (owl.hpp:248-257). */
typedef struct pt_texture {
    int32_t width, height;
    const uint32_t* rgba8;
} pt_texture;

/* launch_params_data environment fields (device_global.hpp:59-63, application.cpp:285-289) */
typedef struct pt_env {
    int32_t use_map;    /* environment_use  (only effective with a non-empty map, device.cu:138) */
    int32_t use_auto;   /* environment_auto */
    float color[3];     /* environment_color */
    float intensity;    /* environment_intensity */
    pt_texture map;     /* environment_map; width == 0 => none */
} pt_env;

/* camera_data (camera.hpp:14-20), 48 bytes, produced by to_camera_data (camera.cpp:3-21) */
typedef struct pt_camera {
    float origin[3], llc[3], horizontal[3], vertical[3];
} pt_camera;

/* Work counters of the last counted render (pt_set_option "count" = 1). One sample = one camera path. */
typedef struct pt_stats {
    double kernel_ms;       /* first launch to last kernel end of the last pt_render*, HIP events on the launch stream */
    int32_t launches;       /* render-kernel launches in the last pt_render* */
    int32_t vgprs, sgprs, lds_bytes, block, grid, stack_entries; /* launch geometry of the render kernel */
    uint64_t samples, rays, nodes, tris, scatters, env_misses, nan_retries; /* valid when counted */
    uint64_t bvh_nodes, bvh_depth, n_triangles;
    double bvh_build_ms;
    /* counted renders, wavefront kernel: {node steps, lanes in them, triangle steps, lanes, retire passes, lanes retired,
     * hit-shading passes, items, miss-shading passes, items, traversal phases, parked lanes,
     * scheduler iterations, sum of idle lanes, sum of finished lanes awaiting retirement, sum of node+leaf lanes} */
    uint64_t sched[32];
    double prepass_ms;      /* part of kernel_ms spent in the cost pre-pass launch + queue sort (0 when the schedule has none) */
    /* counted renders, group walk of sparse waves (eight lanes per ray): {phases, iterations, sum of busy groups, of groups at a
     * node, of groups at a leaf, rays traced, shader-clock cycles, 0} */
    uint64_t groups[8];
    /* last pt_render (not pt_render_device): time on the stream between the end of the render kernels and the end of the RCCL reduce
     * (0 without a communicator; includes waiting for the slowest rank), and of the read-back into the caller's buffers (root) */
    double reduce_ms, d2h_ms;
    int32_t kernel_variant; /* 1 lane per pixel, 2 wavefront kernel, 3 its fallback instance with the larger register budget (chosen when
                             * the 128-VGPR instance of this build would need scratch, or by option "fallback") */
    int32_t express_pixels; /* pixels of the last cost-ordered launch that were rendered as express pixels (waves of their own) */
    int32_t whole_pixels;   /* other pixels of that launch that kept their path slot for all samples (whole-pixel schedule: every pixel had a slot from the start); 0: ring schedule */
    int32_t prepass_spp;    /* samples per pixel of the cost pre-pass launch of the last render (0: the render did not sort) */
    /* counted renders, hit-shading passes by sampled lobe (disney.cuh:9-13: 0 diffuse, 1 clearcoat, 2 metallic, 3 glass; 4 = emitter hit,
     * 5 = NaN retry): [0..5] items, [7] always 0 (it counted the passes of an experiment that is gone), [8..13] passes in which at least one
     * item took that branch, [14] passes that ran two or more BSDF bodies, [15] passes whose items all took the same branch */
    uint64_t lobes[16];
    /* counted renders, traversal (lane-steps): [0] quad-node steps that enter no child, [1] of those: the node lies beyond the best hit
     * found so far, [2] option "watertight" = 1: (ray, triangle) pairs whose edge functions were recomputed from float64 products (else 0),
     * [3] leaf steps that do not improve the hit */
    uint64_t trav[4];
} pt_stats;

/* ---- lifecycle (replaces init_owl_data/destroy_context: application.cpp:59-128, Main.cpp:30) ---- */
pt_ctx* pt_create(const pt_config* cfg);          /* NULL on failure; pt_last_error(NULL) has the reason */
void pt_destroy(pt_ctx* ctx);
const char* pt_last_error(const pt_ctx* ctx);     /* ctx may be NULL (creation errors) */
int pt_abi_version(void);

/* ---- scene (replaces bind_sbt_data + init_owl_world: application.cpp:184-294, :131-140) ----
 * Copies the meshes, builds the BVH2 on the host and uploads everything to HBM.
 * Closest hit = the minimum over all triangles of the Moeller-Trumbore t (ties: lower global triangle index), independent of the hierarchy;
 * sliver triangles - height below 1e-5 of the longest edge, i.e. below ~100 ulp of their coordinates - are never hit (their test result
 * would be rounding noise).  OptiX's watertight test gives such triangles a vanishing cross-section as well. */
int pt_upload_scene(pt_ctx* ctx, const pt_mesh* meshes, int32_t n_meshes, const float* materials, int32_t n_materials,
                    const pt_texture* textures, int32_t n_textures, const int32_t* material_texture, const pt_env* env);
/* material_texture: optional n_materials ints (texture index per material or <0).  NULL => derived from
 * pt_mesh.texture_index of the entities using the material (the reference ties the texture to the
 * material's filename, parser.cpp:32-35 / application.cpp:214-243). */

/* replaces reset_field (application.cpp:297-304): re-upload the material table, BVH untouched */
int pt_set_materials(pt_ctx* ctx, const float* materials, int32_t n_materials);
int pt_set_environment(pt_ctx* ctx, const pt_env* env);

/* ---- moving geometry: new vertices for the uploaded scene, the hierarchies refitted on the device, nothing rebuilt (no reference
 * counterpart: the reference rebuilds its acceleration structure, application.cpp:131-140) ----
 * Needs a scene uploaded with option "dynamic" = 1.  Reads ONLY these fields of each mesh: vertices (NULL = this mesh is unchanged),
 * normals (NULL = keep the normals the library holds), n_vertices and n_normals; n_meshes and these counts must equal the upload's,
 * everything else in pt_mesh is ignored (indices may be NULL).  Blocking; waits for the frames in flight, on a caller's stream too
 * (pt_render_device).  Every argument is checked before anything is touched: a refused call (PT_E_NO_SCENE: no scene; PT_E_INVALID:
 * scene not uploaded with "dynamic" = 1, a count that differs, a NULL array with a non-zero count) leaves the scene exactly as it was.
 * The topology of the three hierarchies stays; triangle records, sliver collapse, padding and every box become bit for bit what a fresh
 * pt_upload_scene of the moved meshes would store for that topology, so - the closest hit being independent of the hierarchy - every
 * frame, probe and counter after the call equals the one after a fresh upload.  What does not follow the geometry is the QUALITY of the
 * tree: it was built for the uploaded positions and walks slower the further the scene deforms (DESIGN.md 4 "Refit" has figures); the
 * remedy is a fresh pt_upload_scene. */
int pt_update_vertices(pt_ctx* ctx, const pt_mesh* meshes, int32_t n_meshes);

/* ---- pixel ownership (multi-GPU sharding; no reference counterpart: the reference is single-GPU) ----
 * Default: this context renders every pixel.  Launch-index pixel id = x + W*y (ray_gen's pixelId). */
int pt_set_pixel_shard(pt_ctx* ctx, int32_t rank, int32_t world_size, int32_t tile);
/* Host-only helper (no GPU needed): ids owned by `rank` when tile x tile pixel tiles are dealt along the
 * anti-diagonals: tile (tx, ty), counted from pixel (0, 0), belongs to rank (tx + ty) % world_size.  `tile` is
 * first rounded up to a multiple of 8, at least 8 (so tiles 1, 4 and 8 deal alike, and 9 deals as 16): the
 * kernels work in 8 x 8 pixel blocks and a block has one owner.  Returns the count (writes at most cap ids,
 * tile by tile, inside a tile in 8 x 8 blocks); <0 on error. */
int64_t pt_shard_pixels(int32_t width, int32_t height, int32_t tile, int32_t rank, int32_t world_size, uint32_t* ids, int64_t cap);

/* ---- render (replaces owlLaunch2D + framebuffer read-back: application.cpp:363-369) ----
 * Blocking.  out_rgb: W*H*3 floats, linear, averaged over max_samples, stored at
 * x + W*(H-1-y) like the reference framebuffer (device.cu:251); pixels not owned by this context
 * are 0.  out_rgba8 (optional): owl::make_rgba of the same values (device.cu:252-253). */
int pt_render(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, int32_t max_samples, int32_t max_path_depth,
              float* out_rgb, uint32_t* out_rgba8);
/* Same render, asynchronous on `stream` (a hipStream_t; NULL = the context's own stream), result left
 * in HBM at d_out_rgb (device pointer, W*H*3 floats) for the caller's RCCL reduce.  d_out_rgba8 optional.
 *
 * STREAMS AND WHAT MAY BE CALLED WHILE A FRAME IS IN FLIGHT.  A context has ONE frame's worth of work buffers (pixel queue, rings,
 * cost image, sort, tier plan, kernel parameters, RNG and accumulation state, counters), one copy of the scene in HBM and one set of
 * timing events.  The context's own stream is non-blocking: HIP orders nothing between it and a caller's stream.  THE LIBRARY does:
 * every call that touches what a frame in flight uses is ordered after the context's LAST ASYNCHRONOUS CALL, whichever stream that
 * call was given.  So any call of this header may follow a pt_*_device call at once, with no pt_synchronize between them.
 *   - The asynchronous calls (pt_render_device, pt_render_batch_device, pt_render_aov_device, pt_render_aov_follow_device, pt_render_aov_batch_device, pt_denoise_device,
 *     pt_denoise_batch_device, pt_denoise_var_device, pt_accum_add_device, pt_accum_denoise_device, pt_accum_reproject_device, pt_upsample_device, pt_trace_closest_device, pt_trace_occluded_device, pt_trace_surface_device, pt_trace_ao_device, pt_trace_hits_device, pt_closest_point_device, pt_render_rays_device, pt_render_aov_rays_device, pt_reduce_framebuffer) wait ON THE
 *     DEVICE: the stream they are given waits for an event recorded at the end of the previous asynchronous call - only if that call
 *     used another stream; on the same stream the stream's own order suffices and nothing is added.  The host returns at once, with
 *     two exceptions that existed before: a frame of another size, shard or batch length rewrites the pixel queue and a frame that
 *     needs larger work buffers reallocates them (pt_denoise_device: its filter records, when the frame is larger than any it filtered
 *     before) - both first wait on the host for the frame in flight; pt_render_batch_device and pt_render_aov_batch_device
 *     return when their per-frame tables have reached HBM, i.e. after whatever precedes them on `stream`; and a pt_accum_add_device that
 *     selects its pixels returns when the count of its active set has reached the host (see there).
 *   - The blocking renders (pt_render, pt_render_batch, pt_render_aov, pt_render_aov_follow, pt_render_aov_batch, pt_accum_add), pt_denoise, pt_denoise_batch, pt_denoise_var, pt_accum_denoise, pt_accum_reproject, pt_upsample, pt_trace_closest, pt_trace_occluded, pt_trace_hits, pt_closest_point, pt_trace_surface, pt_trace_ao, pt_render_rays and pt_render_aov_rays run on the context's stream behind the same device-side wait
 *     and return with the context idle.  After a blocking call, or on the context's own stream, they add no wait at all.
 *   - The calls that change or read what a frame uses WAIT ON THE HOST for the last asynchronous call's stream (if it is not the
 *     context's) and then for the context's: pt_set_materials, pt_set_environment, pt_update_vertices, pt_upload_scene,
 *     pt_set_pixel_shard when it changes the shard of a queue in use, pt_accum_begin, pt_accum_read, pt_accum_variance, pt_accum_end, pt_comm_destroy, pt_destroy, pt_debug_eval and the pt_debug_*
 *     readers of device state - and pt_synchronize, which is that wait plus the watchdog check.  A frame enqueued before such a call
 *     renders the state before it, a frame enqueued after it the state after it.
 *   - pt_get_stats waits for the end of the last frame's kernels (an event), not for the stream.
 * WHAT STAYS THE CALLER'S BUSINESS: the output buffers - the library does not know who reads d_out_rgb, so a second frame into the
 * same buffer, or a read of it, is ordered by the caller (same stream, an event of its own, or pt_synchronize); the stream - it must
 * live until a pt_synchronize (or another of the host-waiting calls above) that follows the last call on it has returned; after
 * that the library does not look at it again.  One thread at a time per context, as everywhere in this header. */
int pt_render_device(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, int32_t max_samples, int32_t max_path_depth,
                     void* d_out_rgb, void* d_out_rgba8, void* stream);
/* Waits on the host for the context's last asynchronous call - pt_render_device, pt_render_batch_device, pt_render_aov_device,
 * pt_render_aov_follow_device, pt_render_aov_batch_device, pt_denoise_device, pt_denoise_batch_device, pt_denoise_var_device, pt_accum_add_device, pt_accum_denoise_device, pt_accum_reproject_device, pt_upsample_device, pt_trace_closest_device, pt_trace_occluded_device, pt_trace_surface_device, pt_trace_ao_device, pt_trace_hits_device, pt_closest_point_device, pt_render_rays_device, pt_render_aov_rays_device or pt_reduce_framebuffer, on the stream it was given - and for the context's own stream.  Every earlier asynchronous call of the context
 * is complete then as well, whatever stream it used: each was ordered before the next (see pt_render_device).  Returns PT_E_HIP if a
 * wave's watchdog fired during the last frame (the image is then incomplete); pt_get_stats reports the same.  PT_OK at once on an idle
 * or host-only context.  A caller's stream may be destroyed once this has returned. */
int pt_synchronize(pt_ctx* ctx);

/* ---- batch render: K frames of the uploaded scene in one launch sequence (no reference counterpart: the reference's test_loop,
 * host/main.cpp, renders its material sweep one owlLaunch2D per value) ----
 * Every frame has its own camera and its own material table; size, samples, depth and environment are shared.  Frame f is stored at
 * out + f * W*H*3 (out_rgba8 + f * W*H) in the framebuffer order of pt_render, and is bit for bit what pt_set_materials(frame f's table)
 * + pt_render(frame f's camera) gives: the frames are stacked into one virtual image of W x (K*H) whose pixels - own RNG stream each,
 * seeded by the position inside the frame - share one pixel queue, one cost pre-pass, one sort and one main launch.
 *   n_materials must equal the scene's; a row's texture slot stays the one pt_upload_scene derived; the context's own table
 *   (pt_set_materials) is neither used (unless materials == NULL) nor changed.
 *   Any n_frames >= 1: a batch that exceeds what one launch sequence can hold (K*H <= 65535 rows, K*W*H < 2^24 pixels, option
 *   "batch_frames") is cut into several by the library (pt_debug_plan_batch shows how); a single frame beyond them is PT_E_LIMIT.
 *   The pixel shard applies per frame (a rank owns the same tiles in every frame); with a communicator pt_render_batch issues ONE
 *   reduce per launch sequence over all of its frames and rank 0 receives them.
 *   Refused with PT_E_INVALID and a message, never rendered frame by frame: option "kernel" = 1, "latency", "timeline".
 *   pt_get_stats afterwards covers the whole batch: kernel_ms from the first launch to the last kernel end, launches = render-kernel
 *   launches of all launch sequences, counted renders sum over the frames; prepass_ms is the first launch sequence's, the geometry
 *   fields the last one's.  The readers below (pt_debug_read_queue / _tiers / _laps) then describe the LAST launch sequence, pixel ids
 *   being those of its virtual image: x + W * (f*H + y), f counted from the sequence's first frame. */
typedef struct pt_frame {
    pt_camera camera;
    const float* materials; /* n_materials * PT_MAT_FLOATS of this frame; NULL = the context's current table */
} pt_frame;
int pt_render_batch(pt_ctx* ctx, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t width, int32_t height,
                    int32_t max_samples, int32_t max_path_depth, float* out_rgb, uint32_t* out_rgba8);
/* The same, asynchronous on `stream` (NULL = the context's), frames left in HBM (n_frames * W*H*3 floats; d_out_rgba8 optional); no reduce. */
int pt_render_batch_device(pt_ctx* ctx, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t width, int32_t height,
                           int32_t max_samples, int32_t max_path_depth, void* d_out_rgb, void* d_out_rgba8, void* stream);
/* Host only, no GPU needed: how a batch of n_frames is cut into launch sequences.  out[i] = frames of sequence i (at most cap are
 * written); max_frames = option "batch_frames" (0: what the limits allow).  Returns the number of sequences, PT_E_LIMIT if one frame
 * is already too large, PT_E_INVALID for bad arguments. */
int64_t pt_debug_plan_batch(int32_t width, int32_t height, int32_t n_frames, int32_t max_frames, int32_t* out, int64_t cap);

/* ---- guide pass: first-hit albedo, shading normal, depth and coverage (no reference counterpart; the guides pt_denoise below - or a denoiser behind
 * the library - wants for its low-sample frames, and a coverage channel for compositing) ----
 * A pass of its own beside the render: one launch of a guide kernel that walks camera rays to their closest hit and stops there.
 * DEFINITION, for pixel (px, py) of a W x H frame and n_samples >= 1 (the kernel, the CPU twin pt_debug_aov_host and the numpy
 * restatement tests/aov_ref.py implement exactly this):
 *   rng = rng_init(px, py); for k = 0 .. n_samples-1: rx = rng_next, then ry = rng_next, and the ray is gen_camera_ray's, operation
 *   for operation: su = (px + rx) / W, sv = (py + ry) / H, dir = normalize(((llc + horizontal*su) + vertical*sv) - origin), from origin.
 *   Nothing else draws from the stream: SAMPLE 0 IS THE BEAUTY FRAME'S FIRST CAMERA RAY OF THAT PIXEL; THE LATER SAMPLES ARE THE GUIDE
 *   PASS'S OWN JITTER (the beauty frame's stream goes on into its bounces, so its second camera ray is another one).
 *   Closest hit as everywhere in this library: t > 1e-3, minimum t, ties to the lower triangle id, slivers never hit; option
 *   "watertight" selects the triangle test.  Each sample contributes 8 floats:
 *     miss: albedo = what the miss shader returns (environment map texel, or the automatic gradient, or the environment colour, times
 *           the environment intensity); alpha, normal and depth 0;
 *     hit:  alpha 1; depth = the hit's t; normal = the interpolated shading normal exactly as the hit shader forms it (the fma chain
 *           over the three vertex normals, then normalize) - NOT flipped towards the viewer, computed for emitters too, (0,0,0) if a
 *           component is not finite; albedo = (emission, emission, emission) if the material's emission > 0, else its base colour
 *           after the hit shader's texture lookup (material defaults for material_index < 0).
 *   The contributions are summed in float32 in sample order from 0, and the stored value is sum * (1.0f / (float)n_samples).
 * LAYOUT: 8 consecutive floats per pixel, {albedo r, g, b, alpha, normal x, y, z, depth}, at pixel offset x + W*(H-1-y) like out_rgb;
 * pixels the context does not own (pt_set_pixel_shard) are all 0.
 * LIMITS: first hit only - a window shows the window, a mirror the mirror; pt_render_aov_follow below lets the guide ray pass such
 * surfaces.  Batch form: pt_render_aov_batch below with max_follow = 0.
 * pt_render_aov: blocking.  Honours the pixel shard, the current material table and environment, "watertight", "box_exact", "quad", and
 * a scene moved by pt_update_vertices.  With a communicator: ONE sum-reduce of the W*H*8 floats onto rank 0 (one non-zero contributor
 * per pixel: bit-identical to the one-GPU buffers); the other ranks may pass NULL.  pt_get_stats afterwards: kernel_ms and launches (1)
 * are the guide launch's, and so are vgprs, lds_bytes, block, grid, stack_entries.  The pass keeps no state: a pt_render after it is bit
 * for bit the pt_render before it.  Sizes as pt_render (PT_E_INVALID beyond 65535 x 65535 or for n_samples < 1); PT_E_NO_SCENE
 * without a scene; every argument is checked before anything is touched.  Without quad nodes (option "quad" = 0, or a tree too deep for
 * them) the pass runs the binary walk, which has no watertight test: together with "watertight" = 1 that is refused with PT_E_INVALID. */
int pt_render_aov(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, int32_t n_samples, float* out_aov);
/* The same, asynchronous on `stream` (NULL = the context's), no reduce, the W*H*8 floats left in HBM at d_out_aov (16-byte aligned);
 * conventions of pt_render_device.  pt_synchronize waits for it and returns PT_E_HIP if a walk ran out of its step or stack bound. */
int pt_render_aov_device(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, int32_t n_samples, void* d_out_aov, void* stream);

/* ---- guide pass, follow mode: the guide ray passes mirrors and glass to the surface seen in them or through them ----
 * The guide pass above with a loop around its walk; kernels of their own (csrc/pt_kernel_aov_follow.hip), the CPU twin
 * pt_debug_aov_follow_host and the numpy restatement tests/aov_follow_ref.py implement exactly this.
 * DEFINITION, per sample.  The camera ray, the RNG draws and the closest-hit rule are exactly those of pt_render_aov; the follow loop
 * draws nothing from the stream.  Arithmetic: the contract of csrc/pt_device.h, and its reflect, refract, dot, normalize, sqrt_; interp3
 * of csrc/pt_trace.h.
 *   tint = (1,1,1); dist = 0; o = camera origin; d = camera ray direction
 *   for step = 0, 1, ...:
 *     closest hit of (o, d) under the library's rule (t > 1e-3, minimum t, lower id, slivers never; "watertight" selects the test)
 *     step 0 decides alpha: 1 on a hit, 0 on a miss                    (coverage stays first-hit: it is for compositing)
 *     miss:  albedo = tint * (what the miss shader returns for d); normal = 0; depth = dist; stop
 *     dist = dist + t                                                   (float32, in step order)
 *     material row, texture slot, bw = 1 - u - v, bx = u, by = v, v_n = normalize(interp3 of the vertex normals), base colour after the
 *       texture lookup: the expressions of pt_render_aov's hit, i.e. of the hit shader, unchanged
 *     kind = NONE if emission > 0, or step == max_follow, or a component of v_n is not finite; else classify(material)
 *     kind NONE:  albedo = tint * (emission > 0 ? (e,e,e) : base colour); normal = v_n if finite else 0; depth = dist; stop
 *     wo = -d;  v_p = interp3(bw, bx, by, p0, p1, p2)                   (the hit shader's hit point, no normal offset)
 *     MIRROR: wi = reflect(wo, v_n);                       tint' = tint * base colour
 *     GLASS:  c = dot(wo, v_n);  c > 0 ? (n' = v_n, eta = 1.0f / ior) : (n' = -v_n, eta = ior)
 *             refract(wo, n', eta, wi) succeeds:           tint' = tint * (sqrt_(base.x), sqrt_(base.y), sqrt_(base.z))
 *             else (total internal reflection):            wi = reflect(wo, v_n); tint' = tint * base colour
 *     d' = normalize(wi); a component of d' not finite: this surface is kind NONE after all (its albedo under the tint that reached it), stop
 *     o = v_p; d = d'; tint = tint'
 *   classify: with the lobe weights of the BSDF sampler, mw = metallic, gw = (1 - metallic) * specular_transmission,
 *     dw = (1 - specular_transmission) * (1 - metallic), cw = 0.25f * clearcoat:
 *     MIRROR if mw > gw && mw > dw && mw > cw && roughness <= roughness_max;
 *     else GLASS if gw > mw && gw > dw && gw > cw && specular_transmission_roughness <= roughness_max;  else NONE (NaN fields land here).
 *   Accumulation, the 1.0f / n_samples scale, the 8-float layout, the framebuffer order and the pixel shard are those of pt_render_aov.
 * CONSEQUENCES: max_follow = 0 is bit for bit pt_render_aov (1.0f * x and 0 + t are exact); for any max_follow a sample whose first hit
 * is not followed contributes exactly what it contributes to pt_render_aov.
 * LIMITS: the normal of a followed sample is the last surface's normal in world space, not mirrored into the virtual image; depth is
 * the path length; at glass only the transmitted ray is followed, except on total internal reflection - the Fresnel reflection on a
 * window is not guided; the tint ignores Fresnel and the specular tint.  Batch form: pt_render_aov_batch below.
 * pt_render_aov_follow (blocking) and pt_render_aov_follow_device (asynchronous; joins the asynchronous calls of the streams contract at
 * pt_render_device: ordered after the context's last asynchronous call and itself the last one afterwards) behave like pt_render_aov and
 * pt_render_aov_device in everything those list: arguments checked before anything is touched, PT_E_NO_SCENE, PT_E_INVALID - also for
 * max_follow outside 0..8, roughness_max outside [0, 1] or NaN, reserved != 0 -, the refusal of "watertight" = 1 on the binary walk, one
 * sum-reduce with a communicator, the pt_get_stats fields, no render state kept. */
typedef struct pt_aov_params {
    int32_t n_samples;    /* >= 1 */
    int32_t max_follow;   /* 0..8 specular surfaces a guide ray may pass; 0 = first hit */
    float roughness_max;  /* 0..1: a surface rougher than this is not followed */
    int32_t reserved;     /* must be 0 */
} pt_aov_params;
void pt_aov_default_params(pt_aov_params* p);   /* 1, 4, 0.3f, 0 */
int pt_render_aov_follow(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, const pt_aov_params* p /* NULL = defaults */, float* out_aov);
int pt_render_aov_follow_device(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, const pt_aov_params* p, void* d_out_aov, void* stream);
/* The guide buffers of a batch: the frames of pt_render_batch (own camera and material table each) through the follow kernels, ONE
 * launch per launch sequence (batch instances: csrc/pt_kernel_aov_follow_batch.hip).  DEFINED BY THE SINGLE-FRAME CALL: frame f is stored
 * at out_aov + f * W*H*8 and is bit for bit what pt_set_materials(frame f's table) + pt_render_aov_follow(frame f's camera, p) stores
 * for that frame alone; a materials == NULL frame uses the context's current table.  max_follow = 0 therefore gives the first-hit guides
 * of pt_render_aov (CONSEQUENCES above).  Frames and tables as pt_render_batch: n_materials must equal the scene's; a row's texture slot
 * stays the one the upload derived; the context's own table is neither used (unless a frame's is NULL) nor changed; the pixel shard
 * applies per frame and pixels not owned are +0.  The batch is cut into launch sequences exactly as pt_render_batch cuts it
 * (pt_debug_plan_batch, option "batch_frames"; a single frame beyond a sequence is PT_E_LIMIT) and the result does not depend on the cut.
 * REFUSED before anything is touched or enqueued, with a message that names the call: everything pt_render_aov_follow refuses,
 * n_frames < 1 or frames == NULL, a wrong n_materials, and option "watertight" = 1 (batches have no watertight instances).  On a
 * host-only context valid arguments give PT_E_NO_DEVICE, invalid ones PT_E_INVALID.
 * pt_render_aov_batch: blocking, like pt_render_aov_follow; with a communicator ONE sum-reduce per launch sequence over all of its frames
 * onto rank 0 (the other ranks may pass NULL).  pt_render_aov_batch_device: asynchronous on `stream` (NULL = the context's), no reduce,
 * n_frames * W*H*8 floats left in HBM at d_out_aov (16-byte aligned); joins the asynchronous calls of the streams contract at
 * pt_render_device and, like pt_render_batch_device, returns when its per-frame tables have reached HBM.  pt_get_stats afterwards:
 * kernel_ms from the first to the last kernel of the call, launches = launch sequences, the geometry fields of the guide kernel (grid: the
 * longest sequence's).  No render state is kept: a pt_render after it is bit for bit the pt_render before it. */
int pt_render_aov_batch(pt_ctx* ctx, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t width, int32_t height,
                        const pt_aov_params* p /* NULL = defaults */, float* out_aov);
int pt_render_aov_batch_device(pt_ctx* ctx, const pt_frame* frames, int32_t n_frames, int32_t n_materials, int32_t width, int32_t height,
                               const pt_aov_params* p, void* d_out_aov, void* stream);

/* ---- denoiser: guide-driven a-trous filter for low-sample frames (no reference counterpart; the reference binds no denoiser) ----
 * An edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010): L iterations of a 5 x 5 B3-spline kernel whose tap
 * distance doubles each iteration, every tap weighted by how far it differs from the centre pixel in colour, shading normal, relative
 * depth and albedo; optionally on colour / albedo (PT_DENOISE_DEMODULATE).  It consumes a frame of pt_render and the guide buffers of
 * pt_render_aov, needs the WHOLE frame and no scene: with N GPUs call it on rank 0 (or pt_group_ctx(g, 0)) after the reduce.  It issues
 * no collective and has no group form; pt_denoise_batch below filters the frames of a batch.
 * BUFFERS: rgb and out_rgb are W*H*3 floats, aov the W*H*8 floats of pt_render_aov, all in the framebuffer order those calls produce
 * (the kernel is symmetric, so the filter works in framebuffer rows and columns as they lie in memory: row = index / W, x = index % W).
 * out_rgb may equal rgb (d_out_rgb may equal d_rgb): the filter works on buffers of its own.  out_rgba8 is optional.
 * DEFINITION (the kernels of csrc/pt_denoise.hip, the CPU twin pt_debug_denoise_host and the numpy restatement tests/denoise_ref.py
 * implement exactly this).  Arithmetic: the contract of csrc/pt_device.h - float32, no contraction, fma_ only where written, correctly
 * rounded "/", dot(a, b) = fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)), and its exp_, max_, make_rgba.
 *   Per pixel p, from aov: a = floats 0..2 (albedo), n = floats 4..6 (normal), z = float 7 (depth).
 *   Prepare:  rgb_k that is not finite is taken as 0;  d_k = max_(a_k, 1e-3f) with the flag, else 1;  c0_k = rgb_k / d_k with the flag,
 *             else rgb_k itself;  kz_p = 1.0f / (sd * sd) with sd = sigma_depth * max_(z_p, 1e-6f).
 *   Host constants, once, in float32 and in this order:  kn = 1.0f / (sigma_normal * sigma_normal);  ka likewise from sigma_albedo;  per
 *             iteration i: sc = sigma_color * 2^-i (exact), kc_i = 1.0f / (sc * sc).
 *   Iteration i = 0 .. L-1, s = 1 << i:  sum = (0, 0, 0), wsum = 0, then for dy = -2..2 (outer loop) and dx = -2..2 (inner loop):
 *             q = (x + dx*s, row + dy*s); a tap outside the frame is skipped (no clamp, no mirror);
 *             h = k[|dx|] * k[|dy|] with k = {3/8, 1/4, 1/16} (the products are exact);
 *             centre tap: w = h, nothing else computed;
 *             any other tap:  ec = dot(c_i(q) - c_i(p), same);  en = dot(n(q) - n(p), same);  dz = z(q) - z(p), ez = dz * dz;
 *                             ea = dot(a(q) - a(p), same);  e = fma_(ea, ka, fma_(ez, kz_p, fma_(en, kn, ec * kc_i)));
 *                             w = h * exp_(-e);  if !(w > 0) the tap is skipped (NaN and non-finite guides included);
 *             sum_k = fma_(w, c_i(q)_k, sum_k), wsum = wsum + w.
 *             After the 25 taps: c_{i+1}(p)_k = sum_k / wsum (wsum >= 9/64 always: the centre tap).
 *   Finish:   out_k = c_L_k * d_k with the flag, else c_L_k;  out_rgba8 = make_rgba(out).
 * LIMITS: relative depth under-filters surfaces seen at grazing angles; with the guides of pt_render_aov glass and mirrors are filtered by
 * their own surface, not by what shows in them (pt_render_aov_follow supplies guides that follow them); the colour sigma halves each iteration, as in the paper.
 * REFUSED with PT_E_INVALID and a message, before anything is touched: a NULL pointer (p and out_rgba8 excepted), W or H outside
 * 1..65535 or W*H >= 2^31, iterations outside 1..8, a flag bit other than PT_DENOISE_DEMODULATE, a sigma that is not > 0 (NaN included;
 * +infinity is allowed and switches the term off).  A host-only context answers pt_denoise and pt_denoise_device with PT_E_NO_DEVICE.
 * pt_denoise: blocking (H2D of both inputs, the filter, D2H; the context is idle on return).  pt_denoise_device: asynchronous on `stream`
 * (NULL = the context's), device pointers, d_aov 16-byte aligned; conventions of pt_render_device - ordered after the context's last
 * asynchronous call and itself the last one afterwards; pt_synchronize waits for it.  pt_get_stats afterwards: kernel_ms from the first
 * to the last filter kernel, launches = the filter's (L + 2), block, grid, vgprs, lds_bytes those of the iteration kernel.  The filter
 * keeps no render state: a pt_render after it is bit for bit the pt_render before it. */
#define PT_DENOISE_DEMODULATE 1
typedef struct pt_denoise_params {
    int32_t iterations;   /* L, 1..8: steps 1, 2, 4, ... 2^(L-1) */
    int32_t flags;        /* bit 0 (PT_DENOISE_DEMODULATE): filter colour / albedo, multiply back at the end; other bits must be 0 */
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo; /* each > 0; +infinity switches the term off */
} pt_denoise_params;
void pt_denoise_default_params(pt_denoise_params* p);   /* 5, 0, 4.0f, 0.25f, 0.1f, 0.2f */
int pt_denoise(pt_ctx* ctx, const float* rgb, const float* aov, int32_t width, int32_t height, const pt_denoise_params* p /* NULL = defaults */,
               float* out_rgb, uint32_t* out_rgba8 /* optional */);
int pt_denoise_device(pt_ctx* ctx, const void* d_rgb, const void* d_aov, int32_t width, int32_t height, const pt_denoise_params* p,
                      void* d_out_rgb, void* d_out_rgba8, void* stream);
/* The filter over the frames of a batch (csrc/pt_denoise_batch.hip): n_frames frames of one size, W*H*3 floats apart in rgb and out_rgb,
 * W*H*8 in aov, W*H in out_rgba8 - the layouts pt_render_batch and pt_render_aov_batch produce - with shared parameters.  DEFINED BY THE
 * SINGLE-FRAME CALL: frame f is bit for bit pt_denoise of frame f of rgb and frame f of aov; no tap ever reads another frame.  out_rgb may
 * equal rgb (d_out_rgb may equal d_rgb); out_rgba8 is optional; no scene is needed.  The batch is cut into launch sequences as
 * pt_render_batch cuts it (pt_debug_plan_batch, option "batch_frames"; a single frame beyond a sequence is PT_E_LIMIT): a sequence is
 * L + 2 launches over one set of filter records for its frames (64 bytes per pixel of the sequence), and the result does not depend on
 * the cut.  REFUSED before anything is touched, with a message that names the call: everything pt_denoise refuses, and n_frames < 1; on a
 * host-only context valid arguments give PT_E_NO_DEVICE, invalid ones PT_E_INVALID.  pt_denoise_batch is blocking like pt_denoise,
 * pt_denoise_batch_device asynchronous like pt_denoise_device (same streams contract).  pt_get_stats afterwards: kernel_ms from the first
 * to the last kernel of the call, launches = sequences * (L + 2), block, grid (the longest sequence's), vgprs, lds_bytes those of the
 * iteration kernel.  No render state is kept. */
int pt_denoise_batch(pt_ctx* ctx, const float* rgb, const float* aov, int32_t n_frames, int32_t width, int32_t height,
                     const pt_denoise_params* p /* NULL = defaults */, float* out_rgb, uint32_t* out_rgba8 /* optional */);
int pt_denoise_batch_device(pt_ctx* ctx, const void* d_rgb, const void* d_aov, int32_t n_frames, int32_t width, int32_t height,
                            const pt_denoise_params* p, void* d_out_rgb, void* d_out_rgba8, void* stream);
/* The CPU twin of the filter: the definition above on all host threads; works on a host-only context; returns width * height. */
int64_t pt_debug_denoise_host(pt_ctx* ctx, const float* rgb, const float* aov, int32_t width, int32_t height, const pt_denoise_params* p,
                              float* out_rgb, uint32_t* out_rgba8);

/* ---- progressive accumulation: a frame that grows by "adds", with a per-pixel noise estimate and adaptive adds (no reference
 * counterpart: the reference restarts every frame at sample 0) ----
 * A context holds at most ONE accumulation.  It owns its device buffers (62 bytes per pixel of the frame beside the 16 of the image); no other
 * call of this header writes them (pt_accum_variance and pt_accum_denoise, further down, read them; pt_accum_reproject, further down still, moves them to a new camera).  pt_accum_begin fixes camera, size, depth and the pixel shard as they are at that moment;
 * every pt_accum_add gives the pixels of its ACTIVE SET n_samples more samples of their own RNG streams and returns the image so far.
 * STATE per pixel: rng and sum[3] - the render kernel's own rng_state / accum at the launch id x + W*y - and seen[3], half[3], n, n_half,
 * passes, noise.  pt_accum_begin sets noise = +inf and everything else 0.
 * AN ADD: (1) select the active set; (2) run the render path (the wavefront kernel, its schedules, option "watertight") over exactly
 * those pixels for n_samples more samples of each pixel's stream - a pixel's first add starts from the seed of pt_render, later ones from
 * the stored state; the render kernel writes no framebuffer; (3) resolve.
 * DEFINITION (the kernels of csrc/pt_accum.hip, the CPU twins pt_debug_accum_resolve_host / pt_debug_accum_select_host - one source,
 * csrc/pt_accum_math.h - and the numpy restatement tests/accum_ref.py implement exactly this).  Arithmetic: the contract of
 * csrc/pt_device.h - float32, no contraction, correctly rounded "/", its sqrt_, max_, make_rgba; |v| clears the sign bit.
 *   Resolve, for every owned pixel:
 *     if the pixel was active in this add:  if passes is odd: half_k = half_k + (sum_k - seen_k), n_half += n_samples;
 *                                           then seen = sum, n += n_samples, passes += 1.
 *     n >= 1:  out_k = sum_k * (1.0f / (float)n) - pt_render's own expression with max_samples = n - and rgba8 = make_rgba(out);
 *     n == 0:  out = +0, rgba8 = 0.
 *     noise = +inf while n_half == 0; else a_k = half_k * (1.0f / (float)n_half), b_k = (sum_k - half_k) * (1.0f / (float)(n - n_half)),
 *             d = (|a_0 - b_0| + |a_1 - b_1|) + |a_2 - b_2|,  l = max_((out_0 + out_1) + out_2, 1e-2f),  noise = d / sqrt_(l).
 *     This is the half-buffer error estimate of production adaptive samplers: two disjoint sample sets of the same pixel (the samples
 *     of the pixel's even and of its odd passes), normalised by brightness.
 *   Pixels the context does not own are +0 in every output.
 *   Select, for the next add: an owned pixel is active iff (max_pixel_samples == 0 || n < max_pixel_samples) and
 *     (noise_threshold == 0 || !(noise <= noise_threshold)).  NaN and +inf are active, so every pixel takes part in a frame's first two
 *     adds whatever the threshold.  The order of the compacted id list is not part of the contract; the image does not depend on it.  An
 *     empty active set is not an error: no render kernel is launched, resolve still rewrites the outputs, active_pixels = 0.
 * CONSEQUENCES.  A pixel with n samples is bit for bit that pixel of pt_render at max_samples = n (same camera, size, depth, scene
 * state, "watertight"), however the n were split into adds: uniform adds totalling N give the whole frame of pt_render(N), rgba8
 * included.  Samples see the materials, environment and vertices current at their add.  Changing the pixel shard or uploading a new
 * scene after pt_accum_begin makes the next add PT_E_INVALID until a new begin.  The accumulation itself stays as it was and stays
 * readable: pt_accum_read, pt_accum_info_get, pt_debug_accum_state, pt_accum_variance, pt_accum_denoise (which judges the shard the
 * accumulation was begun with) and pt_accum_end go on working on it; with the shard it was begun with set again, adds go on too.
 * LAYOUTS: out_rgb (W*H*3 floats), out_rgba8, out_noise and out_samples (W*H each) are in framebuffer order x + W*(H-1-y), like out_rgb
 * of pt_render.
 * ORDERING: pt_accum_add_device joins the asynchronous calls of the streams contract at pt_render_device: ordered after the context's
 * last asynchronous call and itself the last one afterwards.  pt_accum_add is a blocking render (context's stream, idle on return);
 * pt_accum_begin, pt_accum_read, pt_accum_end and pt_debug_accum_state wait on the host like pt_set_materials.  A uniform add without a
 * cap returns at once on the host (the exceptions of pt_render_device apply: a work buffer that has to grow).  An add that SELECTS
 * (threshold > 0 or a cap) waits on the host for the 4-byte count of its active set - i.e. for everything before it on its stream -
 * because the launch cannot be planned without it.  Any other call of the header may come between two adds (a pt_render of another size,
 * guide passes, the denoiser, batches): it leaves the accumulation untouched and is itself unchanged by it.
 * COMMUNICATOR: not built yet - pt_accum_begin, pt_accum_add and pt_accum_add_device on a context with a communicator are PT_E_INVALID
 * by name (an accumulation begun before the communicator was attached can still be read and ended).  There is no pt_group_*
 * form.  A pixel shard set with pt_set_pixel_shard works: noise and sample maps are per shard.
 * REFUSED with PT_E_INVALID and a message that names the call, before anything is touched: n_samples outside 1..65535, a negative cap,
 * a threshold that is negative or NaN, reserved != 0; options "kernel" = 1, "latency", "timeline"; add / read / info without a begin;
 * sizes pt_render refuses; a pixel's n about to pass 2^31 - 65536 (judged by the sum of the adds' n_samples).  PT_E_NO_SCENE without a
 * scene.  On a host-only context valid arguments give PT_E_NO_DEVICE at pt_accum_begin, so no accumulation exists there.
 * pt_get_stats after an add: kernel_ms from the first launch - of an add that selects, the select kernel's, so the wait for the count lies
 * inside - to the end of resolve, launches = the render-kernel launches (0 for an empty active set), the geometry fields the render
 * kernel's (after an empty active set: those of the last frame that ran one). */
typedef struct pt_accum_params {
    int32_t n_samples;          /* 1..65535: samples this add gives every ACTIVE pixel */
    int32_t max_pixel_samples;  /* 0 = no cap; else a pixel with n >= this is never active again (n may overshoot by < n_samples) */
    float   noise_threshold;    /* 0 = uniform add (every owned pixel under the cap); > 0 = only pixels with !(noise <= threshold) */
    int32_t reserved;           /* must be 0 */
} pt_accum_params;
void pt_accum_default_params(pt_accum_params* p);            /* 16, 0, 0.0f, 0 */
typedef struct pt_accum_info {
    int32_t  width, height, max_path_depth, adds;            /* adds so far */
    int64_t  owned_pixels, active_pixels;                    /* active: of the last add */
    uint64_t samples_total;                                  /* sum over the adds of active_pixels * n_samples */
} pt_accum_info;
int pt_accum_begin(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, int32_t max_path_depth); /* replaces an accumulation the context has */
int pt_accum_add(pt_ctx* ctx, const pt_accum_params* p /* NULL = defaults */, float* out_rgb /* may be NULL */, uint32_t* out_rgba8 /* may be NULL */);
int pt_accum_add_device(pt_ctx* ctx, const pt_accum_params* p, void* d_out_rgb /* may be NULL */, void* d_out_rgba8 /* may be NULL */, void* stream);
int pt_accum_read(pt_ctx* ctx, float* out_rgb, uint32_t* out_rgba8, float* out_noise, uint32_t* out_samples); /* any pointer may be NULL */
int pt_accum_info_get(pt_ctx* ctx, pt_accum_info* out);
int pt_accum_end(pt_ctx* ctx);                               /* frees the buffers; PT_OK when there is none */
/* Validation hooks.  The two twins work on a host-only context and on flat arrays of n_pixels pixels (no row order is implied).
 * resolve: sum[3n], seen[3n], half[3n], n, n_half, passes, active and owned flags (bytes, 0 / not 0), n_samples 1..65535 -> seen, half, n,
 * n_half, passes updated in place, out_rgb[3n], out_rgba8[n], noise[n]; returns n_pixels.  select: -> active flags (0 / 1); returns the
 * number of active pixels; refuses the parameters an add refuses.  state: the raw state of the context's accumulation in framebuffer
 * order (sum and half W*H*3 floats, the others W*H; any pointer may be NULL), +0 outside the shard; waits on the host. */
int64_t pt_debug_accum_resolve_host(pt_ctx* ctx, int64_t n_pixels, const float* sum, float* seen, float* half, uint32_t* n, uint32_t* n_half, uint32_t* passes,
                                    const uint8_t* active, const uint8_t* owned, int32_t n_samples, float* out_rgb, uint32_t* out_rgba8, float* noise);
int64_t pt_debug_accum_select_host(pt_ctx* ctx, const float* noise, const uint32_t* n, const uint8_t* owned, int64_t n_pixels, const pt_accum_params* p, uint8_t* active);
int pt_debug_accum_state(pt_ctx* ctx, float* sum, float* half, uint32_t* n, uint32_t* n_half, uint32_t* passes);

/* ---- variance-guided denoise of a growing frame (no reference counterpart) ----
 * pt_denoise's colour sigma is a constant in absolute units, right for one noise level only: as an accumulation gathers samples the
 * filtered frame stops improving.  This filter is the spatial stage of SVGF (Schied et al. 2017): the same a-trous kernel, but the
 * colour distance is measured in units of the pixel's own estimated VARIANCE, and that variance is filtered along with the colour, so
 * the filter narrows by itself as the frame converges.  The accumulation already stores what the estimate needs (half, n_half).  For a
 * first preview of a few samples pt_denoise stays the better call: one difference of two halves is a noisy variance estimate.
 * No batch form and no group form: like pt_denoise it needs the whole frame (with N GPUs: on rank 0 after the reduce).
 *
 * 1. VARIANCE OF AN ACCUMULATION'S PIXELS (csrc/pt_accum_math.h accum_variance_pixel, ONE copy for the kernel and its CPU twin), with
 *    VMAX = 1e30f, per owned pixel from sum, half, n, n_half:
 *      n_half == 0:  var_k = VMAX, k = 0..2 (unknown).
 *      otherwise:    ia = 1.0f / (float)n_half, ib = 1.0f / (float)(n - n_half) (resolve's own expressions);
 *                    fh = (float)n_half / (float)n, r = fh * (1.0f - fh);
 *                    a_k = half_k * ia, b_k = (sum_k - half_k) * ib, e_k = a_k - b_k;  var_k = r * (e_k * e_k);
 *                    if !(var_k <= VMAX) var_k = VMAX (NaN and +inf included).
 *      colour:       n >= 1: sum_k * (1.0f / (float)n) (resolve's expression), else +0.
 *    Pixels that are not owned are +0 in both outputs.  Why r: E[(a - b)^2] = s^2 (1/n_half + 1/(n - n_half)), and the variance of the
 *    pixel's mean is s^2 / n.
 *    pt_accum_variance writes the W*H*3 floats of the map in framebuffer order; it waits on the host like pt_accum_read.
 *    pt_debug_accum_variance_host: the twin on flat arrays of n_pixels pixels, like the other accumulation twins; returns n_pixels.
 * 2. THE FILTER.  pt_denoise_var(rgb, var, aov): var is W*H*3 floats laid out like rgb, the per-channel variance of the pixel value;
 *    every other buffer, the order and out_rgb == rgb are as for pt_denoise.  It reuses pt_denoise_params; HERE sigma_color COUNTS
 *    STANDARD DEVIATIONS (default 3).  DEFINITION: that of pt_denoise, same arithmetic contract, fma_ only where written, except:
 *      Prepare:  rgb, d_k, c0 and kz as in pt_denoise;  v_k = var_k without the flag, v_k = var_k / (d_k * d_k) with it;
 *                v = (v_0 + v_1) + v_2,  v0(p) = (v >= 0.0f && v <= VMAX) ? v : VMAX.
 *      Host constants:  kn, ka as before;  s2 = sigma_color * sigma_color.  No per-iteration halving: the filtered variance narrows
 *                the colour term by itself.
 *      Iteration i, s = 1 << i, at pixel p:
 *        (1) the variance around p, over the 3 x 3 DIRECT neighbours (distance 1, not s):  gs = 0, gw = 0;  for dy = -1..1 (outer), dx =
 *            -1..1 (inner), taps outside the frame skipped:  g = m[|dx|] * m[|dy|] with m = {1/2, 1/4};  gs = fma_(g, v_i(q), gs),
 *            gw = gw + g;  vb = gs / gw.
 *        (2) kc_p = 0 if s2 is +infinity (no colour term), else kc_p = 1.0f / fma_(s2, vb, 1e-10f).
 *        (3) the 25 taps of pt_denoise in its order with kc_p in the place of kc_i; every tap that is taken also does
 *            vs = fma_(w * w, v_i(q), vs) (centre tap: w = h).  c_{i+1} = sum / wsum,  v_{i+1} = min_(vs / (wsum * wsum), VMAX).
 *      Finish:   that of pt_denoise.
 *    CONSEQUENCES: a pixel whose variance is unknown is filtered by its guides alone; a variance map of 0 leaves every pixel that
 *    differs from its neighbours as it is.
 *    REFUSED: everything pt_denoise refuses, and NULL var; on a host-only context valid arguments give PT_E_NO_DEVICE, invalid ones
 *    PT_E_INVALID.  pt_denoise_var is blocking like pt_denoise; pt_denoise_var_device is asynchronous like pt_denoise_device (d_aov
 *    16-byte aligned) and joins the asynchronous calls of the streams contract.  pt_get_stats afterwards: kernel_ms from the first to the
 *    last kernel, launches = L + 2, block, grid, vgprs, lds_bytes those of the iteration kernel.
 *    pt_debug_denoise_var_host: the CPU twin, works on a host-only context; out_var (optional, W*H floats) receives v_L; returns W*H.
 * 3. ON THE ACCUMULATION, WITHOUT A HOST ROUND TRIP.  pt_accum_denoise / pt_accum_denoise_device run the variance kernel over the
 *    accumulation's state and then the filter on resolve's image; W and H are the accumulation's.  They read the state and change none of
 *    it: the next add, pt_accum_read and a pt_render afterwards are bit for bit what they are without the call, and the result is bit for
 *    bit pt_denoise_var(pt_accum_read's rgb, pt_accum_variance's map, aov).  The blocking form behaves like pt_denoise; the device form is
 *    asynchronous and ordered like pt_accum_add_device.  REFUSED by name before anything is touched: no accumulation; a pixel shard that
 *    does not own the whole frame (the filter needs every pixel); a communicator (as pt_accum_add); NULL aov or out_rgb; the parameter
 *    refusals of pt_denoise.  pt_get_stats afterwards: as pt_denoise_var with launches = L + 3.
 * The four kernels are csrc/pt_denoise_var.hip; the numpy restatement is tests/denoise_var_ref.py. */
void pt_denoise_var_default_params(pt_denoise_params* p);   /* 5, 0, 3.0f, 0.25f, 0.1f, 0.2f */
int pt_denoise_var(pt_ctx* ctx, const float* rgb, const float* var, const float* aov, int32_t width, int32_t height,
                   const pt_denoise_params* p /* NULL = defaults */, float* out_rgb, uint32_t* out_rgba8 /* optional */);
int pt_denoise_var_device(pt_ctx* ctx, const void* d_rgb, const void* d_var, const void* d_aov, int32_t width, int32_t height, const pt_denoise_params* p,
                          void* d_out_rgb, void* d_out_rgba8, void* stream);
int64_t pt_debug_denoise_var_host(pt_ctx* ctx, const float* rgb, const float* var, const float* aov, int32_t width, int32_t height, const pt_denoise_params* p,
                                  float* out_rgb, uint32_t* out_rgba8, float* out_var /* optional: v_L, W*H floats */);
int pt_accum_variance(pt_ctx* ctx, float* out_var);
int64_t pt_debug_accum_variance_host(pt_ctx* ctx, int64_t n_pixels, const float* sum, const float* half, const uint32_t* n, const uint32_t* n_half,
                                     const uint8_t* owned, float* out_rgb, float* out_var);
int pt_accum_denoise(pt_ctx* ctx, const float* aov, const pt_denoise_params* p /* NULL = defaults */, float* out_rgb, uint32_t* out_rgba8 /* optional */);
int pt_accum_denoise_device(pt_ctx* ctx, const void* d_aov, const pt_denoise_params* p, void* d_out_rgb, void* d_out_rgba8 /* optional */, void* stream);

/* ---- reprojection: move an accumulation to a new camera (no reference counterpart) ----
 * When the camera moves, a new pt_accum_begin throws every sample away.  pt_accum_reproject keeps them: the accumulation's own state
 * follows the surfaces to the new camera, every pixel keeps its RNG stream, and pixels that come into view (or fail a consistency test)
 * restart with n = 0 and noise = +inf, which is what an add's select already takes for "needs samples".  pt_accum_read,
 * pt_accum_variance, pt_accum_denoise and the next pt_accum_add work on the result unchanged; the render kernel is not involved.
 * aov_prev holds the guides (W*H*8 floats, as pt_render_aov produces them) under the accumulation's CURRENT camera, aov_cur the guides
 * under new_cam; W and H are the accumulation's; the device pointers are 16-byte aligned; the two may be the same buffer.
 * DEFINITION (the kernel of csrc/pt_accum_reproject.hip and the CPU twin pt_debug_accum_reproject_host - one source,
 * csrc/pt_accum_math.h accum_reproject_source / accum_reproject_history - and the numpy restatement tests/accum_reproject_ref.py
 * implement exactly this).  Arithmetic is the contract of csrc/pt_device.h: its dot, cross, normalize, sqrt_, abs_, isinf_, unfused
 * + - *, correctly rounded /.
 *   Host constants, computed once per call, in this order, from the OLD camera (o', llc', h', v'):
 *     a = llc' - o',  N = cross(h', v'),  inn = 1.0f / dot(N, N),  na = dot(N, a).
 *   Per owned pixel (px, py) of the new frame, with g its record of aov_cur at framebuffer index px + W*(H-1-py):
 *   1. Camera ray through the pixel centre.  su = ((float)px + 0.5f) / (float)W, sv likewise with H;
 *      dc = normalize(((llc + horizontal*su) + vertical*sv) - origin), which are gen_camera_ray's operations on the new camera.
 *   2. Surface or sky.  The pixel is a surface if g.alpha >= 0.5f && g.depth > 0.0f && !isinf_(g.depth), else sky (a point at infinity).
 *      Surface: P = origin + dc * g.depth, r = P - o', ze = sqrt_(dot(r, r)).   Sky: r = dc.
 *   3. Projection into the old camera.  dn = dot(N, r), lam = na / dn.  No history unless lam > 0.0f && !isinf_(lam).
 *      w = r * lam - a;  su' = dot(cross(w, v'), N) * inn,  sv' = dot(cross(h', w), N) * inn;  fx = su' * (float)W, fy = sv' * (float)H.
 *      No history unless fx >= 0 && fx < W && fy >= 0 && fy < H (NaN fails).  qx = (int)fx, qy = (int)fy.
 *      The SOURCE is the one old pixel that contains the point: one tap, no interpolation, so n, n_half and passes stay integers.
 *   4. No history if the source is not owned by the context.
 *   5. Consistency, with s the record of aov_prev at qx + W*(H-1-qy), classified as in step 2.  Every comparison must be TRUE, so NaN
 *      guides fail:  same class;  surface: abs_(s.depth - ze) <= depth_tol * ze and dot(g.normal, s.normal) >= normal_min;
 *      both classes: da = s.albedo - g.albedo, dot(da, da) <= albedo_tol * albedo_tol.
 *   6. History.  Copy sum, half, n, n_half, passes of launch id qx + W*qy.  Then, if max_history != 0 && n > max_history:
 *        f = (float)max_history / (float)n,  sum_k = sum_k * f;
 *        nh = (uint32_t)((uint64_t)n_half * max_history / n);
 *        half_k = nh ? half_k * ((float)nh / (float)n_half) : +0;
 *        n_half = nh,  n = max_history.
 *      No history: all of these are +0 / 0.
 *   7. Resolve.  seen = sum.  Then accum_resolve_pixel(state, active = false, ...) of pt_accum_math.h gives out_rgb, out_rgba8 and
 *      noise: resolve's own expressions, one copy.
 *   Pixels that are not owned stay +0 everywhere.  rng is not read and not written: every pixel goes on with its own stream.
 * After the call the accumulation's camera is new_cam: pt_accum_read, pt_accum_variance, pt_accum_denoise and the next pt_accum_add see
 * the moved state.  A pixel without history has n = 0 and noise = +inf, so it is active in any selecting add.  adds, samples_total,
 * owned_pixels and the bound on a pixel's n (the sum of the adds' n_samples) are unchanged.
 * CONSEQUENCES AND LIMITS.
 *   - After a reproject, "a pixel with n samples is bit for bit pt_render at n" no longer holds for this accumulation.  It holds again
 *     after pt_accum_begin.
 *   - Static scenes only: samples taken before pt_update_vertices, pt_set_materials or pt_set_environment are carried along.  The albedo
 *     test catches part of a material change, nothing more.
 *   - One tap misplaces history by up to half a pixel per call.  max_history bounds how long that is kept.
 *   - View-dependent shading (mirrors, glass) is reprojected by its surface, not by what shows in it.
 *   - Before the first add (adds == 0) the call only changes the camera.
 *   - A second set of state buffers (36 bytes per pixel) is allocated at the first reproject and swapped with the first set by the call.
 * The three default tolerances are starting values chosen from the filter's sigmas, not measured optima.
 * ORDERING: pt_accum_reproject_device joins the asynchronous calls of the streams contract at pt_render_device and the list at
 * pt_synchronize.  The blocking form belongs with pt_accum_denoise: context's stream, idle on return; it uploads both guides.  The
 * host-side pointer swap and camera change happen at enqueue, which is safe because every later call is ordered after it.
 * REFUSED with PT_E_INVALID by name, before anything is touched: no accumulation; a communicator (as pt_accum_add); a shard changed or
 * a scene uploaded since begin (as pt_accum_add); NULL camera or guides; reserved != 0; max_history of 1 or negative; a tolerance that is
 * negative or NaN; normal_min that is NaN or > 1.  A host-only context - which can hold no accumulation - judges the arguments alone and
 * answers PT_E_NO_DEVICE to valid ones.  The twin works there: old_cam is the camera the state was gathered under, owned the shard's
 * flags (W*H bytes, framebuffer order; NULL = all); sum, half, n, n_half, passes are updated in place, in framebuffer order as
 * pt_debug_accum_state gives them; it refuses what the call refuses of its arguments, NULL arrays and sizes pt_render refuses; returns W*H.
 * pt_get_stats afterwards: kernel_ms of the one kernel, launches = 1, block, grid, vgprs, lds_bytes the reproject kernel's. */
typedef struct pt_reproject_params {
    int32_t max_history;  /* 0 = no cap; else >= 2: a pixel that arrives with n > max_history is scaled down to it */
    int32_t reserved;     /* must be 0 */
    float depth_tol;      /* >= 0: |z_source - z_expected| <= depth_tol * z_expected;  +inf = test off */
    float normal_min;     /* -1..1 or -inf: dot(n_cur, n_source) >= normal_min;          -inf = test off */
    float albedo_tol;     /* >= 0: |a_source - a_cur|^2 <= albedo_tol^2;                 +inf = test off */
} pt_reproject_params;
void pt_accum_reproject_default_params(pt_reproject_params* p);   /* 0, 0, 0.05f, 0.9f, 0.1f */
int pt_accum_reproject(pt_ctx* ctx, const pt_camera* new_cam, const float* aov_prev, const float* aov_cur, const pt_reproject_params* p /* NULL = defaults */);
int pt_accum_reproject_device(pt_ctx* ctx, const pt_camera* new_cam, const void* d_aov_prev, const void* d_aov_cur, const pt_reproject_params* p, void* stream);
int64_t pt_debug_accum_reproject_host(pt_ctx* ctx, const pt_camera* old_cam, const pt_camera* new_cam, int32_t width, int32_t height,
                                      const float* aov_prev, const float* aov_cur, const uint8_t* owned /* W*H, framebuffer order; NULL = all */, const pt_reproject_params* p,
                                      float* sum, float* half, uint32_t* n, uint32_t* n_half, uint32_t* passes, /* in/out, framebuffer order, as pt_debug_accum_state gives them */
                                      float* out_rgb, uint32_t* out_rgba8, float* out_noise);                   /* framebuffer order; returns W*H */

/* ---- upsampling: lift a low-resolution frame to full resolution with full-resolution guides (no reference counterpart) ----
 * The render is the one cost of a frame that grows with the pixel count; the guide pass is cheap at any size and pt_camera is
 * resolution-independent (su = (px + rx) / W: ONE camera struct serves both sizes).  Irradiance is smooth where albedo and geometry
 * are not, so a frame rendered (and filtered) at w x h is lifted to W x H by joint bilateral upsampling (Kopf, Cohen, Lischinski,
 * Uyttendaele 2007): a tent filter over taps x taps low-resolution pixels, every tap weighted by how far its low-resolution guides
 * differ from the high-resolution pixel's in shading normal, relative depth and albedo; optionally on colour / albedo
 * (PT_UPSAMPLE_DEMODULATE).  It needs no scene and keeps no render state; it needs WHOLE frames: with N GPUs call it on rank 0 after
 * the reduce.  No batch form, no group form, no collective.
 * BUFFERS: rgb_lo is w*h*3 floats, aov_lo w*h*8 floats, aov_hi W*H*8 floats, out_rgb W*H*3 floats, all in the framebuffer order that
 * pt_render and pt_render_aov produce; like pt_denoise the filter works in rows as they lie in memory (row = index / width; the mapping
 * below is symmetric under the row flip).  Device guide pointers are 16-byte aligned.  Outputs must not overlap inputs.  out_rgba8 is
 * optional.
 * DEFINITION (the kernels of csrc/pt_upsample.hip, the CPU twin pt_debug_upsample_host and the numpy restatement tests/upsample_ref.py
 * implement exactly this).  Arithmetic: the contract of csrc/pt_device.h - float32, no contraction, fma_ only where written, correctly
 * rounded "/", its dot, exp_, max_, abs_, make_rgba; floorf is exact.
 *   Host constants, once, in this order:  rx = (float)w / (float)W, ry = (float)h / (float)H;  kn = 1.0f / (sigma_normal * sigma_normal),
 *             ka likewise from sigma_albedo;  R = taps / 2, ir = 1.0f / (float)R.
 *   Prepare, per low pixel q, from aov_lo: a = floats 0..2, n = floats 4..6, z = float 7.  An rgb_k that is not finite is taken as 0;
 *             c(q)_k = rgb_k / max_(a_k, 1e-3f) with the flag, else rgb_k.
 *   Per high pixel p = (x, row), with a_p, n_p, z_p from its aov_hi record:
 *     1. sd = sigma_depth * max_(z_p, 1e-6f), kz = 1.0f / (sd * sd).
 *     2. fx = ((float)x + 0.5f) * rx - 0.5f, x0 = (int)floorf(fx), tx = fx - (float)x0.  The same gives fy, y0, ty from row and ry.
 *     3. sum = psum = (0, 0, 0), wsum = pw = 0.
 *     4. For j = 1-R .. R (outer) and i = 1-R .. R (inner), q = (x0 + i, y0 + j):
 *          a tap outside the low frame is skipped (no clamp, no mirror);
 *          bx = 1.0f - abs_((float)i - tx) * ir, by likewise from j and ty, and the tap is skipped unless bx > 0 && by > 0;
 *          b = bx * by;  psum_k = fma_(b, c(q)_k, psum_k);  pw = pw + b;
 *          en = dot(n(q) - n_p, same);  dz = z(q) - z_p, ez = dz * dz;  ea = dot(a(q) - a_p, same);
 *          e = fma_(ea, ka, fma_(ez, kz, en * kn));  wt = b * exp_(-e);
 *          if !(wt > 0) the tap adds nothing more (NaN and non-finite guides included);
 *          sum_k = fma_(wt, c(q)_k, sum_k);  wsum = wsum + wt.
 *     5. v = (wsum >= 1e-4f * pw) ? sum / wsum : psum / pw.  When no low-resolution neighbour matches, the pixel is a feature thinner
 *        than a low pixel and gets the plain tent filter.  pw > 0 always, because the tap at x0 or at x0 + 1 lies in the frame with
 *        positive bx (and likewise in y).
 *     6. out_k = v_k * max_(a_p_k, 1e-3f) with the flag, else v_k;  out_rgba8 = make_rgba(out).
 * CONSEQUENCES: every sigma at +infinity, flag 0, taps 2 and finite guides give bilinear interpolation.  Equal sizes, identical finite
 * guides, flag 0 and taps 2 give the sanitised input bit for bit: there is then one tap with b = 1, and exp_(-0.0f) is exactly 1.0f by
 * the code of pt_device.h (a -0.0f comes back as +0.0f: fma_(1, c, +0); with taps 4 the tent has radius 2 and reaches the neighbours).
 * LIMITS: first-hit guides blur what shows in mirrors and glass; pt_render_aov_follow guides at both sizes help.  Shadow and
 * indirect-light edges have no guide: they are interpolated at low-resolution sharpness.
 * REFUSED with PT_E_INVALID, by name, before anything is touched: a NULL pointer (p and out_rgba8 excepted); w, h, W or H outside
 * 1..65535, or W*H >= 2^31; w > W or h > H; taps not 2 or 4; an unknown flag bit; a sigma that is not > 0 (NaN included; +infinity is
 * allowed and switches the term off); reserved != 0.  A host-only context answers valid arguments with PT_E_NO_DEVICE and invalid ones
 * with PT_E_INVALID; the twin works there.
 * ORDERING: pt_upsample_device joins the asynchronous calls of the streams contract at pt_render_device and the list at pt_synchronize
 * (its records, 48 bytes per low pixel, live in a work buffer of the context that grows like pt_denoise_device's).  pt_upsample is
 * blocking like pt_denoise: it stages its three inputs and reads back.  pt_get_stats afterwards: kernel_ms from the first to the last
 * kernel, launches = 2, block, grid, vgprs, lds_bytes those of the upsample kernel. */
#define PT_UPSAMPLE_DEMODULATE 1
typedef struct pt_upsample_params {
    int32_t taps;       /* 2 or 4: the low-resolution window is taps x taps */
    int32_t flags;      /* bit 0 PT_UPSAMPLE_DEMODULATE; other bits must be 0 */
    float sigma_normal, sigma_depth, sigma_albedo;   /* each > 0; +infinity switches the term off */
    int32_t reserved;   /* must be 0 */
} pt_upsample_params;                                 /* 24 bytes */
void pt_upsample_default_params(pt_upsample_params* p);   /* 4, PT_UPSAMPLE_DEMODULATE, 0.25f, 0.1f, 0.2f, 0 */
int pt_upsample(pt_ctx* ctx, const float* rgb_lo, const float* aov_lo, int32_t w, int32_t h, const float* aov_hi, int32_t W, int32_t H,
                const pt_upsample_params* p /* NULL = defaults */, float* out_rgb, uint32_t* out_rgba8 /* optional */);
int pt_upsample_device(pt_ctx* ctx, const void* d_rgb_lo, const void* d_aov_lo, int32_t w, int32_t h, const void* d_aov_hi, int32_t W, int32_t H,
                       const pt_upsample_params* p, void* d_out_rgb, void* d_out_rgba8, void* stream);
/* The CPU twin: the definition above on all host threads; works on a host-only context; returns W * H. */
int64_t pt_debug_upsample_host(pt_ctx* ctx, const float* rgb_lo, const float* aov_lo, int32_t w, int32_t h, const float* aov_hi, int32_t W, int32_t H,
                               const pt_upsample_params* p, float* out_rgb, uint32_t* out_rgba8);

/* ---- ray queries: closest hit and occlusion for the CALLER'S rays (no reference counterpart: the reference traces only the rays its
 * own ray_gen makes, and shoots no shadow rays) ----
 * pt_trace_closest answers "what does this ray hit", pt_trace_occluded "does this ray hit anything before tmax" - picking, line of
 * sight, ambient-occlusion and visibility guides, light baking, motion vectors.  Kernels of their own (csrc/pt_kernel_rays.hip,
 * csrc/pt_kernel_rays_wt.hip) around the device functions of the render kernel; the CPU twin is pt_debug_trace_rays_host.
 * DEFINITION, per ray (a pt_ray: 32 bytes; the kernel reads it as two 16-byte loads).
 *   thi = tmax < 1e10f ? tmax : 1e10f: NaN and +infinity give the library's own bound.  The lower bound is the library's fixed 1e-3, as
 *   everywhere.  Float 7 of the record (`unused`) is NOT READ: it leaves room for a per-ray lower bound later.  dir need not be
 *   normalised, and t is in units of |dir|.  org and dir must be finite and dir non-zero (the domain of the probes below); the hit
 *   domain is the one stated at "validation hooks": origins within 10 extents, no coplanar or grazing rays.
 *   CLOSEST: over all triangles the active test accepts with 1e-3 < t <= thi, the one with minimum t, ties to the lower global
 *   triangle id, slivers never; the active test is Moeller-Trumbore, or the watertight test under option "watertight" = 1.  This is
 *   exactly pt_debug_closest_hit_host(org, dir, 1e-3, thi): that walk starts at t = thi, id = 0x7fffffff, so a hit at exactly thi is
 *   taken.  out = {t, u, v, prim}, prim the global triangle id (entity order, then face order; pt_prim_to_mesh inverts it); a miss is
 *   {+0, +0, +0, -1}.
 *   OCCLUDED: out = 1 iff the closest set above is not empty, else 0 - a property of the scene, not of the walk, which stops at the first
 *   triangle it accepts.
 * The calls honour "watertight", "box_exact" (1: the subtracting slab form; 0 and the default -1: the fma form - there is no camera to
 * measure, and the hit domain keeps origins within 10 extents, inside that form's reach of 42) and a scene moved by pt_update_vertices.
 * They ignore the pixel shard, materials and environment.  With a communicator they issue no collective: every context traces its own
 * rays.  They need quad nodes: a scene loaded with option "quad" = 0, or one whose tree is too deep for them, is refused with
 * PT_E_INVALID by name.  They keep no render state: a pt_render after them is bit for bit the one before.  n == 0 is PT_OK with no launch.
 * REFUSED with PT_E_INVALID, by name, before anything is touched: NULL rays or out with n > 0; n < 0 or n >= 2^31; a d_rays that is
 * not 16-byte aligned (nor a d_out of pt_trace_closest_device: a hit is one 16-byte store).  PT_E_NO_SCENE without a scene.  On a
 * host-only context valid arguments give PT_E_NO_DEVICE and invalid ones PT_E_INVALID; the twin works there.
 * ORDERING: the _device forms (device pointers, `stream` NULL = the context's) join the asynchronous calls of the streams contract at
 * pt_render_device and the list at pt_synchronize.  The blocking forms stage the rays, run on the context's stream behind the same
 * device-side wait, and read back; the context is idle on return.
 * THE WALK: a wave owns a contiguous range of rays (a multiple of 64: the caller's coherence stays inside a wave) and refills its idle
 * lanes from it when no more than "rays_refill" lanes are still walking (pt_set_option); every walk is bounded like the probes', and
 * pt_synchronize returns PT_E_HIP if one ran out of its step or stack bound (that ray is reported as a miss), as for the guide pass.
 * pt_get_stats afterwards: kernel_ms and launches (1) are the ray launch's, and so are block, grid, vgprs, lds_bytes, stack_entries.
 * NOT BUILT: no pt_main flag, no pt_group_* form, no batch form. */
typedef struct pt_ray     { float org[3]; float tmax; float dir[3]; float unused; } pt_ray;     /* 32 bytes */
typedef struct pt_ray_hit { float t, u, v; int32_t prim; } pt_ray_hit;                          /* 16 bytes */
int pt_trace_closest        (pt_ctx* ctx, const pt_ray* rays, int64_t n, pt_ray_hit* out);
int pt_trace_closest_device (pt_ctx* ctx, const void* d_rays, int64_t n, void* d_out /* n pt_ray_hit */, void* stream);
int pt_trace_occluded       (pt_ctx* ctx, const pt_ray* rays, int64_t n, uint8_t* out);
int pt_trace_occluded_device(pt_ctx* ctx, const void* d_rays, int64_t n, void* d_out /* n bytes */, void* stream);
/* The CPU twin: the definition above run by the host walk of pt_debug_closest_hit_host_n on all host threads; works on a host-only
 * context, follows "watertight" and pt_update_vertices.  occluded = 0: out is n pt_ray_hit; else n bytes.  Returns n. */
int64_t pt_debug_trace_rays_host(pt_ctx* ctx, const pt_ray* rays, int64_t n, int32_t occluded, void* out);
/* Host only: the mesh (entity of the upload) and the triangle inside it of a global triangle id, through the prefix sums of n_triangles
 * of the upload.  PT_E_INVALID outside 0 .. n_triangles-1, PT_E_NO_SCENE without a scene. */
int pt_prim_to_mesh(pt_ctx* ctx, int32_t prim, int32_t* mesh, int32_t* triangle);

/* ---- ray queries: the surface at the hit (no reference counterpart) ----
 * pt_trace_surface is pt_trace_closest with WHAT IS THERE stored beside the hit: the hit point, the geometric and the shading normal,
 * the texcoord, the material index, the base colour after the texture lookup and the emission - what picking, ambient occlusion and
 * baking need next, from the records the library keeps in HBM in leaf order beside the triangle the walk just tested.  A caller takes
 * p and ng / ns from this call, makes rays of their own and sends them to pt_trace_occluded_device on the same stream; for cosine-weighted
 * ambient occlusion that composition is built in as ONE kernel: pt_trace_ao, below.
 * Kernels of their own (csrc/pt_kernel_rays_surface.hip, csrc/pt_kernel_rays_surface_wt.hip: the closest-hit walk of the ray kernels,
 * whose lanes retire through csrc/pt_surface.h); the CPU twin is pt_debug_trace_surface_host.
 * DEFINITION, per ray (a pt_ray as above; out: a pt_surface, 80 bytes, stored as five 16-byte stores).  Arithmetic under the contract
 * of csrc/pt_device.h: binary32, no contraction, fma only where written (fma_).
 *   The first 16 bytes {t, u, v, prim} are bit for bit what pt_trace_closest stores for that ray: thi, the tie-break, slivers never,
 *   option "watertight".
 *   A MISS is {+0, +0, +0, -1}, then p = +0, material = -1, and every remaining word +0.  All 80 bytes are written for every ray.
 *   A HIT, with bx = u, by = v, bw = 1.0f - bx - by, (p0, p1, p2) the triangle's vertices, (n0, n1, n2) its vertex normals and
 *   (tc0, tc1, tc2) its texcoords as the render's shade_hit reads them (csrc/pt_trace.h), and
 *   interp3(bw, bx, by, a, b, c) = fma_(by, c, fma_(bx, b, bw * a)) per component:
 *     p        = interp3(bw, bx, by, p0, p1, p2) - the render's hit point, with no normal offset; NOT org + t * dir.
 *     ns       = normalize(interp3(bw, bx, by, n0, n1, n2)), or (0, 0, 0) if a component of that is not finite; NOT flipped towards
 *                the ray (the normal of the guide pass).
 *     ng       = normalize(cross(p1 - p0, p2 - p0)) with cross(a, b).x = fma_(a.y, b.z, -(a.z * b.y)) (cyclic) and
 *                normalize(a) = a * (1.0f / sqrt(dot(a, a))); (0, 0, 0) by the same rule; NOT flipped: its orientation is that of the
 *                mesh's index order.
 *     tu, tv   = fma_(by, tc2.x, fma_(bx, tc1.x, bw * tc0.x)) and likewise in y; always computed (a mesh without texcoords: zeros).
 *     material = the mesh's material_index as uploaded (may be < 0).
 *     The ROW is the default material for material < 0 (base colour 0.8, emission 0), else row `material` of the current table
 *     (pt_set_materials) with its texture slot.
 *     base     = the row's base colour, or the nearest texel at (tu, tv) of the row's texture if it has one (the render's lookup:
 *                RGBA8, clamp, normalised coordinates) - taken whether or not the material emits (the render and the guide pass
 *                skip the lookup on an emitter).
 *     emission = the row's emission.
 * The call honours "watertight", "box_exact" (as pt_trace_*: only 1 selects the subtracting form), "rays_refill", "rays_grid",
 * pt_set_materials and pt_update_vertices (the records are the leaf-order ones a refit rewrites).  It ignores the pixel shard and the
 * environment, issues no collective and keeps no render state: a pt_render after it is bit for bit the one before.  It needs quad nodes.
 * REFUSALS, ORDERING, n == 0, pt_get_stats, the bound flag behind pt_synchronize (a walk that ran out of its step or stack bound
 * retires as a miss) and HOST-ONLY CONTEXTS are those of pt_trace_closest / pt_trace_closest_device, word for word, with pt_surface in
 * place of pt_ray_hit: in particular d_out must be 16-byte aligned (a record is five 16-byte stores), and pt_trace_surface_device joins
 * the asynchronous calls at pt_render_device and the list at pt_synchronize.
 * NOT BUILT: a lookup from a caller's (prim, u, v) without a ray - the records are in leaf order and the scene keeps no table from a
 * triangle id to its slot on the device; a mesh index in the record (pt_prim_to_mesh stays the way); no pt_main flag, no pt_group_*
 * form, no batch form. */
typedef struct pt_surface {          /* 80 bytes */
    float t, u, v; int32_t prim;     /* bit for bit pt_trace_closest's record of this ray */
    float p[3];    int32_t material; /* hit point; the mesh's material_index (may be < 0) */
    float ng[3];   float tu;         /* geometric normal; interpolated texcoord u */
    float ns[3];   float tv;         /* shading normal;   interpolated texcoord v */
    float base[3]; float emission;   /* base colour after the texture lookup; material emission */
} pt_surface;
int pt_trace_surface       (pt_ctx* ctx, const pt_ray* rays, int64_t n, pt_surface* out);
int pt_trace_surface_device(pt_ctx* ctx, const void* d_rays, int64_t n, void* d_out /* n pt_surface, 16-byte aligned */, void* stream);
/* The CPU twin: pt_debug_trace_rays_host's walk, then the record above from the host copies of the scene (triangles, shading
 * records, material table, textures); works on a host-only context, follows "watertight", pt_set_materials and pt_update_vertices.
 * Returns n. */
int64_t pt_debug_trace_surface_host(pt_ctx* ctx, const pt_ray* rays, int64_t n, pt_surface* out);

/* ---- ray queries: ambient occlusion (no reference counterpart: the reference shoots no shadow rays) ----
 * pt_trace_ao is pt_trace_closest with the AMBIENT OCCLUSION at the hit stored beside it: the fraction of K cosine-distributed rays
 * from the hit point that reach `radius` unoccluded.  It is the composition pt_trace_surface -> K hemisphere rays per hit ->
 * pt_trace_occluded in ONE kernel (csrc/pt_kernel_rays_ao.hip, csrc/pt_kernel_rays_ao_wt.hip; csrc/pt_ao.h): a lane walks its primary
 * ray and then its own K occlusion rays without leaving the wave, and no occlusion ray is ever stored to HBM.  The CPU twin is
 * pt_debug_trace_ao_host; kernel and twin compile the arithmetic between the walks from one header, csrc/pt_ao_math.h.
 * DEFINITION, per ray i - its index in the caller's array (a pt_ray as above; out: a pt_ao_hit, 32 bytes, stored as two 16-byte
 * stores).  Arithmetic under the contract of csrc/pt_device.h: binary32, no contraction, fma only where written.
 *   1. CLOSEST HIT: exactly pt_trace_closest's - thi, the tie-break, slivers never, option "watertight".  A miss stores
 *      {+0, +0, +0, -1}, then {+0, +0, +0, 1.0f}.
 *   2. SURFACE: p, ng and ns are exactly pt_trace_surface's expressions.  nrm = ns under PT_AO_SHADING_NORMAL, else ng.  If nrm is
 *      (0, 0, 0) the second half is {+0, +0, +0, 1.0f} and nothing is traced.  No material row and no texel is read.
 *   3. FACING: nf = dot(nrm, dir) > 0.0f ? -nrm : nrm, with dir the caller's direction as given (not normalised) and dot of
 *      pt_device.h: dot(a, b) = fma_(a.z, b.z, fma_(a.y, b.y, a.x * b.x)).
 *   4. OCCLUSION RAYS: rng = rng_init((uint32_t)i, seed) and onb(nf, T, B), once per ray.  For k = 0 .. K-1: r1 = rng_next(rng), then
 *      r2 = rng_next(rng); w = sample_cosine_hemisphere(r1, r2); d_k = to_world(T, B, nf, w) (all of pt_device.h).  Ray k starts at p
 *      with NO offset - the library's fixed 1e-3 lower bound does that work, as in the render - has direction d_k and the bound
 *      thi = radius < 1e10f ? radius : 1e10f.  It is occluded iff pt_trace_occluded of {p, thi, d_k} would store 1: a property of the
 *      scene, not of the walk.  clear = the number of rays that are not occluded.
 *   5. RESULT: ao = (float)clear * (1.0f / (float)K), and n = nf.
 * CONSEQUENCES.  The first 16 bytes are pt_trace_closest's record of the ray.  With out_ao_rays from the twin, clear of ray i equals
 * the number of zeros pt_trace_occluded returns for records i*K .. i*K+K-1 (a ray that traces nothing - a miss, a zero normal - gets K
 * records with the empty interval tmax = +0, which nothing occludes: K zeros, ao = 1).  The stream depends on (i, seed) only, so the
 * result does not depend on "rays_refill", "rays_grid", the grid or the slab form.  The occlusion rays of a surface point leave the
 * hit domain stated at "validation hooks" now and then (a direction that grazes an edge below 1e-2 rad); there kernel and twin are
 * both valid walks and may disagree on a ray, as everywhere.
 * The call honours "watertight", "box_exact" (as pt_trace_*: only 1 selects the subtracting form), "rays_refill", "rays_grid" and
 * pt_update_vertices.  It ignores the pixel shard, the materials and the environment, issues no collective and keeps no render state.
 * It needs quad nodes.  The step and stack bounds of the walk apply PER WALK; a ray one of whose walks runs out is reported as a miss
 * with ao = 1, and pt_synchronize returns PT_E_HIP.
 * THE WALK is that of pt_trace_closest with one difference in the launch: a ray is 1 + K walks where it hits and one where it misses,
 * so the call cuts eight times as many, shorter ranges as the other ray queries (never shorter than 64 rays; "rays_grid" caps their
 * number as it does there) and lets the hardware balance them; the stack-overflow workspace of the context grows with the ranges.
 * REFUSALS, ORDERING, n == 0, pt_get_stats, the bound flag behind pt_synchronize and HOST-ONLY CONTEXTS are those of pt_trace_closest /
 * pt_trace_closest_device, word for word, with pt_ao_hit in place of pt_ray_hit (d_out 16-byte aligned).  ADDITIONALLY REFUSED with
 * PT_E_INVALID, by name, before anything else: n_rays outside 1..4096, a flag bit other than PT_AO_SHADING_NORMAL, a radius that is not
 * > 0 (NaN included).  pt_trace_ao_device joins the asynchronous calls at pt_render_device and the list at pt_synchronize; pt_trace_ao
 * joins the blocking calls.
 * NOT BUILT: a camera or ray-image form; pt_group_*, batch and communicator forms; a pt_main flag; a per-ray lower bound (the origin
 * offset stays the library's 1e-3); stratified or low-discrepancy sampling (K independent draws of the per-ray stream). */
#define PT_AO_SHADING_NORMAL 1
typedef struct pt_ao_params {   /* 16 bytes */
    int32_t  n_rays;   /* K, 1..4096 occlusion rays per hit */
    int32_t  flags;    /* bit 0 PT_AO_SHADING_NORMAL: hemisphere about ns; 0: about ng.  Other bits must be 0 */
    float    radius;   /* > 0: tmax of the occlusion rays in world units; +inf = the library's bound.  NaN, <= 0 refused */
    uint32_t seed;     /* second word of the per-ray stream */
} pt_ao_params;
void pt_ao_default_params(pt_ao_params* p);      /* 16, 0, +inf, 0 */
typedef struct pt_ao_hit {      /* 32 bytes, two 16-byte stores */
    float t, u, v; int32_t prim;   /* bit for bit pt_trace_closest's record of this ray */
    float n[3];    float ao;       /* the facing normal used; fraction of occlusion rays that were NOT occluded */
} pt_ao_hit;
int pt_trace_ao        (pt_ctx* ctx, const pt_ray* rays, int64_t n, const pt_ao_params* p /* NULL = defaults */, pt_ao_hit* out);
int pt_trace_ao_device (pt_ctx* ctx, const void* d_rays, int64_t n, const pt_ao_params* p, void* d_out /* n pt_ao_hit, 16-byte aligned */, void* stream);
/* The CPU twin: the definition above through the host walk on all host threads and csrc/pt_ao_math.h; works on a host-only context,
 * follows "watertight" and pt_update_vertices.  out_ao_rays: NULL, or n * K pt_ray records - the occlusion rays of ray i at
 * i*K .. i*K+K-1, as pt_trace_occluded takes them.  Returns n. */
int64_t pt_debug_trace_ao_host(pt_ctx* ctx, const pt_ray* rays, int64_t n, const pt_ao_params* p, pt_ao_hit* out, pt_ray* out_ao_rays);

/* ---- ray queries: the first K hits (no reference counterpart: the reference stops every ray at its first surface) ----
 * pt_trace_hits answers "what lies along this ray, in order": the first K triangles it crosses, not only the first - layered
 * transparency and X-ray views, wall thickness (second hit minus first), peeling away a cover, counting the surfaces between two
 * points, picking through a window.  Re-shooting from each hit with an epsilon loses coplanar surfaces, accumulates error and costs a
 * launch per layer; this is ONE walk per ray.  Kernels of their own (csrc/pt_kernel_rays_hits.hip, csrc/pt_kernel_rays_hits_wt.hip;
 * csrc/pt_hits.h): the walk of the ray kernels, whose leaf step offers every triangle it accepts to a per-lane sorted list in LDS
 * instead of keeping the best one.  The CPU twin is pt_debug_trace_hits_host.
 * DEFINITION, per ray i (a pt_ray as above; out: K = max_hits records of pt_ray_hit at out[i*K .. i*K+K-1], K 16-byte stores).
 *   thi, the fixed lower bound 1e-3, the ray domain and the unread float 7 are exactly those of pt_trace_closest.
 *   S = the set of triangles the active test accepts with 1e-3 < t <= thi; the active test is Moeller-Trumbore, or the watertight
 *   test under option "watertight" = 1.  Slivers are never in S.
 *   S is ordered by (t as a float32 value, global triangle id), ascending.
 *   out[i*K + j] for j < min(K, |S|) is {t, u, v, prim} of the j-th element; the bits of t, u and v are what the triangle test computes
 *   for that triangle - what pt_trace_closest would store if that triangle were the closest.
 *   Every entry j >= |S| is the miss record {+0, +0, +0, -1}.
 *   All K * 16 bytes of every ray are written; nothing behind n * K * 16 is touched.
 * CONSEQUENCES.  K = 1 is bit for bit pt_trace_closest.  Entry 0 for any K is pt_trace_closest's record of the ray.  The list for K is
 * the prefix of the list for any K' > K.  The result is a property of the scene, not of the walk: it does not depend on the hierarchy,
 * "rays_grid", "rays_refill", the slab form or a refit against a fresh upload.  Two triangles with bit-equal t (a surface stored
 * twice) both appear, the lower id first.
 * A walk that runs out of its step or stack bound retires its ray with K miss records and raises the flag behind pt_synchronize
 * (PT_E_HIP), like the other ray kernels.
 * The call honours "watertight", "box_exact" (as pt_trace_*: only 1 selects the subtracting form), "rays_refill", "rays_grid" and
 * pt_update_vertices.  It ignores the pixel shard, the materials and the environment, issues no collective, keeps no render state (a
 * pt_render after it is bit for bit the one before) and needs quad nodes.  n == 0 is PT_OK with no launch.
 * THE WALK is that of pt_trace_closest - a wave owns a contiguous range of rays and refills its idle lanes from it, one range per
 * resident wave - with the node step culling against thi until a lane's list is full and against its K-th entry from then on; boxes
 * whose entry distance ties with that entry are still visited.  The list is in LDS behind the lane's stack, (12 + 4 K) * 256 bytes per
 * wave, so the waves resident on a CU shrink as K grows (pt_get_stats: lds_bytes).
 * REFUSALS, ORDERING, pt_get_stats (the hits kernel's launch: launches 1, block, grid, vgprs, lds_bytes, stack_entries) and HOST-ONLY
 * CONTEXTS are those of pt_trace_closest / pt_trace_closest_device, word for word, by name, before anything is touched (d_out 16-byte
 * aligned); on a host-only context valid arguments give PT_E_NO_DEVICE, invalid ones PT_E_INVALID, and the twin works there.
 * ADDITIONALLY REFUSED with PT_E_INVALID, by name, before anything else: max_hits outside 1..PT_HITS_MAX, a reserved word that is not 0.
 * pt_trace_hits_device joins the asynchronous calls at pt_render_device and the list at pt_synchronize; pt_trace_hits joins the
 * blocking calls.
 * NOT BUILT: a per-ray lower bound or (t, id) floor to continue past the K-th hit (float 7 of pt_ray stays unread); a count of all
 * hits; surface records per entry; a pt_group_* form; a batch form; a pt_main flag. */
#define PT_HITS_MAX 16
typedef struct pt_hits_params {   /* 16 bytes */
    int32_t max_hits;      /* K, 1..PT_HITS_MAX records per ray */
    int32_t reserved[3];   /* must be 0 */
} pt_hits_params;
void pt_hits_default_params(pt_hits_params* p);   /* 4, 0, 0, 0 */
int pt_trace_hits        (pt_ctx* ctx, const pt_ray* rays, int64_t n, const pt_hits_params* p /* NULL = defaults */, pt_ray_hit* out /* n * K */);
int pt_trace_hits_device (pt_ctx* ctx, const void* d_rays, int64_t n, const pt_hits_params* p, void* d_out /* n * K pt_ray_hit, 16-byte aligned */, void* stream);
/* The CPU twin: the definition above by the HOST WALK of pt_debug_trace_rays_host (not a brute force) with a sorted K-list in place of
 * the best hit, on all host threads.  Its slab tests cull against thi alone, never against the list, so the triangles it offers to the
 * list do not depend on K and its lists are prefixes of each other on every ray.  Works on a host-only context, follows "watertight"
 * and pt_update_vertices.  Returns n. */
int64_t pt_debug_trace_hits_host(pt_ctx* ctx, const pt_ray* rays, int64_t n, const pt_hits_params* p, pt_ray_hit* out);

/* ---- point queries: the nearest surface to the CALLER'S points (no reference counterpart: the reference answers questions about its
 * own rays only) ----
 * pt_closest_point answers "how far is this point from the scene, and where is the nearest surface" - distance fields for collision
 * and contact, proximity shading, snapping bake samples and particles to a surface, distance supervision for implicit models - on the
 * hierarchy that is in HBM already and that pt_update_vertices refits.  A kernel of its own (csrc/pt_kernel_points.hip): NOT a variant
 * of the ray walk but a nearest-first, distance-pruned descent of the quad tree, with point-to-box distances where the rays have slab
 * tests and a point-to-triangle kernel where they have a ray-triangle test.  The CPU twin is pt_debug_closest_point_host; kernel and
 * twin compile the per-triangle code and the box distance from one header, csrc/pt_points_math.h.
 * DEFINITION, per point (a pt_point: 16 bytes, one 16-byte load; out: a pt_point_hit, 32 bytes, two 16-byte stores).  Arithmetic under
 * the contract of csrc/pt_device.h: binary32, no contraction, correctly rounded / and sqrt, and its dot(a, b) = fma_(a.z, b.z,
 * fma_(a.y, b.y, a.x * b.x)), sqrt_ and max_.  v3 * scalar and v3 +- v3 are per component.
 *   SEARCH BOUND.  rmax = radius < 1e10f ? radius : 1e10f: NaN and +infinity give the library's own bound.  r2 = rmax * rmax.  A
 *   negative radius (rmax < 0) finds nothing, whatever r2 is.
 *   PER TRIANGLE (p0, p1, p2) with global id `id`, and x = p.  A triangle that the sliver rule collapsed (p0 == p1 == p2) is never a
 *   candidate.  Otherwise, in exactly this order (Ericson, "Real-Time Collision Detection", 5.1.5):
 *     1. ab = p1 - p0, ac = p2 - p0, ap = x - p0, d1 = dot(ab, ap), d2 = dot(ac, ap).
 *        If d1 <= 0 && d2 <= 0: q = p0, (u, v) = (0, 0), feature 1.
 *     2. bp = x - p1, d3 = dot(ab, bp), d4 = dot(ac, bp).  If d3 >= 0 && d4 <= d3: q = p1, (1, 0), feature 2.
 *     3. vc = d1*d4 - d3*d2.  If vc <= 0 && d1 >= 0 && d3 <= 0: s = d1 / (d1 - d3), q = p0 + ab*s, (s, 0), feature 4.
 *     4. cp = x - p2, d5 = dot(ab, cp), d6 = dot(ac, cp).  If d6 >= 0 && d5 <= d6: q = p2, (0, 1), feature 3.
 *     5. vb = d5*d2 - d1*d6.  If vb <= 0 && d2 >= 0 && d6 <= 0: s = d2 / (d2 - d6), q = p0 + ac*s, (0, s), feature 6.
 *     6. va = d3*d6 - d5*d4, e = d4 - d3, f = d5 - d6.  If va <= 0 && e >= 0 && f >= 0: s = e / (e + f), q = p1 + (p2 - p1)*s,
 *        (1 - s, s), feature 5.
 *     7. Else: k = 1.0f / ((va + vb) + vc), v = vb*k, w = vc*k, q = (p0 + ab*v) + ac*w, (v, w), feature 0.
 *   Then e = x - q per component and dd = dot(e, e).  u weighs p1 and v weighs p2: the convention of pt_ray_hit.  feature: 0 the face,
 *   1 / 2 / 3 the vertex p0 / p1 / p2, 4 / 5 / 6 the edge p0p1 / p1p2 / p0p2.
 *   WINNER.  The search starts at best = r2, best_id = 0x7fffffff; a triangle replaces the best iff dd < best || (dd == best && id <
 *   best_id).  So a NaN dd never wins, a point at exactly dd == r2 is found, and ties - a point nearest to a shared vertex or edge, a
 *   mesh uploaded twice - go to the lower global triangle id.
 *   RECORD.  out = {sqrt_(dd), u, v, prim, q, feature}, prim the global triangle id (pt_prim_to_mesh inverts it); nothing found is
 *   prim = -1 and every other word +0.  All 32 bytes are written for every point.
 * The result is a property of the scene and the point: it does not depend on the hierarchy, the visiting order, the grid or the refill
 * setting.  WHY: the walk skips a box only when dbox > best (strictly), with dbox = dot(a, a), a = max_(max_(lo - x, x - hi), 0) per
 * axis.  dbox and dd are built from the same monotone, correctly rounded operations, so if the computed q of a triangle lies inside a
 * box, lo <= q <= hi per axis, then |fl(x - q)| >= a per axis and dd >= dbox bit for bit; every ancestor's box contains the leaf's box
 * with the builders' pad.  THE PREMISE is therefore that the computed q of the winning triangle lies inside that triangle's padded leaf
 * box.  The pad is 1e-5 of E = max(scene extent, largest |coordinate| of the scene), 2^-16.6 E.  A vertex q is exact.  An edge q =
 * p + e*s has 0 <= s <= 1 - s is a non-negative number over its sum with another - and two roundings, under 2^-22 E.  Step 7 is reached
 * with va, vb, vc > 0 wherever the conditions of the earlier steps agree with each other, and then v, w and 1 - v - w lie in (0, 1)
 * WHATEVER cancellation did to their values: q is a convex combination of the vertices up to four roundings.  So the distance of the
 * point decides how well q is PLACED on the triangle (v and w are differences of products that cancel: their relative error grows
 * with the square of distance over edge length), not whether q lies on it, and the premise asks only the latter.  What remains is
 * step 7 reached with a weight <= 0, where rounding made steps 3, 5 and 6 contradict one another; q then leaves the triangle by
 * |weight| times an edge.
 *   DOMAIN: finite points whose largest |coordinate| is within 10 E - the ray queries' "within 10 extents" - on scenes of finite
 *   triangles.  tests/test_closest_point_host.py asserts the premise on every case it uses, for the winner of every point and for
 *   every triangle on a subsample, out to 10 E.  Outside the domain every form is still a valid evaluation of the steps above on the
 *   triangles it visits, and two forms may then report different triangles.
 * The call honours pt_update_vertices, "rays_refill" and "rays_grid" (the lane refill and the ranges of pt_trace_closest).  It ignores
 * the pixel shard, materials, environment, "watertight" and "box_exact".  With a communicator it issues no collective.  It needs quad
 * nodes: a scene loaded with option "quad" = 0, or one whose tree is too deep for them, is refused with PT_E_INVALID by name.  It keeps
 * no render state: a pt_render after it is bit for bit the one before.  n == 0 is PT_OK with no launch.
 * REFUSED with PT_E_INVALID, by name, before anything is touched: NULL pts or out with n > 0; n < 0 or n >= 2^31; a d_pts or a d_out
 * that is not 16-byte aligned.  PT_E_NO_SCENE without a scene.  On a host-only context valid arguments give PT_E_NO_DEVICE and invalid
 * ones PT_E_INVALID; the twin works there.
 * ORDERING: pt_closest_point_device (device pointers, `stream` NULL = the context's) joins the asynchronous calls of the streams
 * contract at pt_render_device and the list at pt_synchronize.  The blocking form stages the points, runs on the context's stream
 * behind the same device-side wait, and reads back; the context is idle on return.
 * THE WALK: a wave owns a contiguous range of points (a multiple of 64) and refills its idle lanes from it when no more than
 * "rays_refill" lanes are still walking; the call cuts four times as many, shorter ranges as pt_trace_closest (never shorter than 64
 * points; "rays_grid" caps their number as it does there), because points far from every surface cost many times the steps of points
 * next to one.  A lane's stack is in LDS with the deeper levels in the wave's HBM column; an entry is the child's reference alone, and
 * one that the best distance has overtaken costs a step that enters nothing (the form that keeps the box distance beside the reference
 * measured slower).  Every walk is bounded in steps and stack; pt_synchronize returns PT_E_HIP if one ran out of a bound (that point is
 * reported as not found), as for the ray queries.  pt_get_stats afterwards: kernel_ms and launches (1) are the point launch's, and so
 * are block, grid, vgprs, lds_bytes, stack_entries.
 * NOT BUILT: a sign (inside or outside); the k nearest triangles; pt_group_*, batch and pt_main forms. */
typedef struct pt_point     { float p[3]; float radius; } pt_point;                                          /* 16 bytes, one 16-byte load */
typedef struct pt_point_hit { float dist, u, v; int32_t prim; float q[3]; int32_t feature; } pt_point_hit;   /* 32 bytes, two 16-byte stores */
int pt_closest_point        (pt_ctx* ctx, const pt_point* pts, int64_t n, pt_point_hit* out);
int pt_closest_point_device (pt_ctx* ctx, const void* d_pts, int64_t n, void* d_out /* n pt_point_hit, 16-byte aligned */, void* stream);
/* The CPU twin: the definition above by brute force over the host copy of the triangles in leaf order, on all host threads - the
 * definition, not a walk; works on a host-only context, follows pt_update_vertices.  Returns n. */
int64_t pt_debug_closest_point_host(pt_ctx* ctx, const pt_point* pts, int64_t n, pt_point_hit* out);

/* ---- ray images: path-traced radiance along the CALLER'S rays (no reference counterpart: the reference starts every path at its one
 * pinhole camera, device.cu:231-241) ----
 * pt_render_rays is pt_render with the camera replaced by a ray image: one pt_ray_gen record per pixel - an equirectangular or fisheye
 * panorama, a cube-map light probe, an irradiance or lightmap bake from surface points, a lens model with an aperture.  Everything
 * behind the camera ray is the render kernel itself: the instances of csrc/pt_kernel_rayimage.hip are csrc/pt_kernel.hip compiled with
 * another ray generator (gen_ray_from, csrc/pt_trace.h).
 * DEFINITION.  `rays` is a ray image of width x height records (a pt_ray_gen: 64 bytes; the kernel reads it as four 16-byte loads, once
 * per sample); the record of pixel (x, y) is at launch index x + W*y.  Pixel (x, y) is pt_render's pixel in everything except the camera
 * ray: the stream rng_init(x, y), rx = rng_next then ry = rng_next per sample, trace_path with its bounce loop, Russian roulette and NaN
 * retries, the sum over max_samples, out = sum * (1 / max_samples) and make_rgba, stored at x + W*(H-1-y).  The camera ray of a sample
 * starts at org and has the direction
 *     dir_s = normalize((dir + du * rx) + dv * ry)
 * in the arithmetic contract of csrc/pt_device.h: float32, no contraction, v3 * scalar per component, the same normalize
 * (v * (1 / sqrt(dot(v, v)))).  Both draws are made even when du = dv = 0, so the stream is pt_render's.  The four reserved floats are
 * NOT READ.  Two consequences:
 *   - with du = dv = 0 the pixel is bit for bit pixel (x, y) of pt_render at the same W, H, max_samples and depth with the camera
 *     {origin = org, llc = L, horizontal = 0, vertical = 0}, whenever fl(L - org) == dir;
 *   - at W = H = 1 with org = 0 the pixel is bit for bit pt_render's with the camera {0, dir, du, dv}: su = (0 + rx) / 1 = rx, and
 *     x - 0 = x.
 * The call honours the material table, the environment, pt_update_vertices, the schedules and their knobs, "count" and a pixel shard set
 * with pt_set_pixel_shard (pixels not owned are +0); the pt_get_stats fields are those of a pt_render.  "box_exact": 1 the subtracting
 * slab form, 0 the fma form; the default -1 judges the blocking form's table as walk_params judges a camera (the largest |org| component
 * against 42 scene extents) and gives the device form, whose records the host cannot see, the subtracting form - the image is the same
 * under both.  It keeps no state: a pt_render after it is bit for bit the one before it, and an accumulation on the context is untouched.
 * REFUSED with PT_E_INVALID, by name, before anything is touched: NULL rays / d_rays or out_rgb / d_out_rgb; the sizes and depths pt_render
 * refuses; a d_rays that is not 16-byte aligned; in the blocking form (the host reads the table) a record whose org, dir, du or dv is not
 * finite or whose dir is 0; option "watertight" = 1 (there are no watertight instances, as with batches), "kernel" = 1, "latency",
 * "timeline"; a context with a communicator.  PT_E_NO_SCENE without a scene.  On a host-only context valid arguments give PT_E_NO_DEVICE
 * and invalid ones PT_E_INVALID.  The device form cannot check the records: a record that the blocking form would refuse gives an
 * undefined pixel, inside the walk's usual bounds (steps, stack, watchdog).
 * ORDERING: pt_render_rays_device joins the asynchronous calls of the streams contract at pt_render_device and the list at
 * pt_synchronize; d_rays stays the caller's buffer and must stay valid and unchanged until the work has completed on `stream`.  The
 * blocking form stages the table in a buffer of the context's, runs on the context's stream behind the same device-side wait, and reads
 * back; the context is idle on return.
 * NOT BUILT: no pt_main flag, no pt_group_* form, no batch form, no watertight instances, no communicator, no accumulation over a ray
 * image.  The guide pass over a ray image is pt_render_aov_rays below. */
typedef struct pt_ray_gen {      /* 64 bytes, read as four 16-byte loads */
    float org[3]; float reserved0;   /* reserved floats are NOT READ */
    float dir[3]; float reserved1;
    float du[3];  float reserved2;   /* jitter: dir + du*rx + dv*ry, rx, ry in [0,1) */
    float dv[3];  float reserved3;
} pt_ray_gen;
int pt_render_rays(pt_ctx* ctx, const pt_ray_gen* rays, int32_t width, int32_t height, int32_t max_samples, int32_t max_path_depth,
                   float* out_rgb, uint32_t* out_rgba8);
int pt_render_rays_device(pt_ctx* ctx, const void* d_rays, int32_t width, int32_t height, int32_t max_samples, int32_t max_path_depth,
                          void* d_out_rgb, void* d_out_rgba8, void* stream);
/* The guide pass over a ray image: the 8-float guide record of pt_render_aov / pt_render_aov_follow - what pt_denoise, pt_denoise_batch,
 * pt_denoise_var and pt_upsample filter under - for a frame rendered with pt_render_rays.  The instances of csrc/pt_kernel_aov_rays.hip
 * and csrc/pt_kernel_aov_rays_wt.hip are the follow kernels (csrc/pt_aov_follow.h) compiled with the ray generator of the ray image
 * (gen_ray_from, csrc/pt_trace.h): quad walk only, both slab forms, both triangle tests.
 * DEFINITION: that of pt_render_aov_follow, word for word, with ONE substitution - the camera ray.  The camera ray of sample k of pixel
 * (px, py) is the ray of pt_render_rays: the stream is rng_init(px, py); each sample draws rx = rng_next, then ry = rng_next (both draws
 * are made even when du = dv = 0); the record is read at launch index px + W*py; the ray starts at org and has the direction
 *     dir_s = normalize((dir + du * rx) + dv * ry)
 * in the arithmetic contract of csrc/pt_device.h; the four reserved floats are NOT READ.  Everything after the camera ray is
 * pt_render_aov_follow's, unchanged: the closest-hit rule (option "watertight" selects the triangle test), the follow loop with o = org,
 * classify, the tint and the path length, coverage from step 0, the float32 sum in sample order times 1.0f / n_samples, the 8-float
 * layout at x + W*(H-1-y), +0 for pixels the context does not own.  max_follow = 0 gives first-hit guides (the CONSEQUENCES at
 * pt_render_aov_follow): there is no separate first-hit entry point.
 * CONSEQUENCES:
 *   (a) with du = dv = 0, pixel (x, y) is bit for bit pixel (x, y) of pt_render_aov_follow at the same W, H and params under the camera
 *       {origin = org, llc = L, horizontal = 0, vertical = 0}, whenever fl(L - org) == dir;
 *   (b) at W = H = 1 with org = 0 the pixel is bit for bit pt_render_aov_follow's under the camera {0, dir, du, dv}: su = (0 + rx) / 1 = rx,
 *       and x - 0 = x;
 *   (c) sample 0 of a pixel is the first camera ray of that pixel in pt_render_rays of the same table: where the pixel's coverage at
 *       n_samples = 1 says hit, its first surface is that path's first hit.
 * The call honours the material table, the environment, pt_update_vertices, a pixel shard set with pt_set_pixel_shard and "watertight".
 * "box_exact" as pt_render_rays: the default -1 judges the blocking form's origins and gives the device form the subtracting form - the
 * buffer is the same under both.  It keeps no render state: a pt_render, an accumulation or a pt_render_rays around it is unchanged.
 * pt_get_stats afterwards reads as after pt_render_aov: launches = 1, the guide kernel's geometry fields, kernel_ms.  pt_synchronize
 * returns PT_E_HIP if a walk ran out of its step or stack bound.
 * REFUSED with PT_E_INVALID, by name, before anything is touched: NULL rays / d_rays or out_aov / d_out_aov; a d_rays or d_out_aov that
 * is not 16-byte aligned; the sizes pt_render_aov refuses; what pt_render_aov_follow refuses in p; in the blocking form and the twin
 * (the host reads the table) a record whose org, dir, du or dv is not finite or whose dir is 0; a scene without quad nodes - option
 * "quad" = 0 or a tree too deep for them (as pt_trace_*: there are no binary-walk instances); a context with a communicator (as
 * pt_render_rays).  PT_E_NO_SCENE without a scene.  On a host-only context valid arguments give PT_E_NO_DEVICE and invalid ones
 * PT_E_INVALID.  The device form cannot check the records: a record that the blocking form would refuse gives an undefined pixel, inside
 * the walk's usual bounds.
 * ORDERING: pt_render_aov_rays_device (W*H*8 floats left in HBM at d_out_aov) joins the asynchronous calls of the streams contract at
 * pt_render_device and the list at pt_synchronize; d_rays stays the caller's buffer and must stay valid and unchanged until the work
 * has completed on `stream`.  The blocking form stages the table in the buffer pt_render_rays stages it in, runs on the context's stream
 * behind the same device-side wait, and reads back; the context is idle on return.
 * LIMITS: those of pt_render_aov_follow.  pt_denoise does not wrap around the seam of an equirectangular panorama: its taps outside
 * the frame are skipped, so the two columns at the seam are filtered as frame edges.
 * NOT BUILT: no pt_main flag, no pt_group_* form, no batch form. */
int pt_render_aov_rays(pt_ctx* ctx, const pt_ray_gen* rays, int32_t width, int32_t height, const pt_aov_params* p /* NULL = defaults */,
                       float* out_aov);
int pt_render_aov_rays_device(pt_ctx* ctx, const void* d_rays, int32_t width, int32_t height, const pt_aov_params* p, void* d_out_aov,
                              void* stream);

/* ---- N GPUs: pixel tiles sharded over ranks + ONE RCCL sum-reduce of the float3 framebuffer onto rank 0 (pt_comm.cpp) ----
 * No reference counterpart (the reference is single-GPU: create_context(nullptr, 1), application.cpp:62); for N > 1 these
 * replace the render + read-back of application.cpp:363-369.  Every pixel has exactly one non-zero contributor, so the
 * N-GPU frame is bit-identical to the 1-GPU frame.  The library owns the communicator (librccl.so.1, resolved on first use).
 *
 * (a) One process per GPU.  Rank 0 calls pt_comm_get_unique_id; the 128 bytes reach the other ranks by the launcher's
 *     means; every rank calls pt_comm_init_rank (collective; also sets the rank's pixel shard, tile 16).  From then on
 *     pt_render renders the shard, reduces, and fills out_rgb / out_rgba8 on rank 0 only (other ranks may pass NULL). */
#define PT_COMM_ID_BYTES 128
int pt_comm_get_unique_id(uint8_t id[PT_COMM_ID_BYTES]);
int pt_comm_init_rank(pt_ctx* ctx, const uint8_t id[PT_COMM_ID_BYTES], int32_t rank, int32_t world_size);
int pt_comm_destroy(pt_ctx* ctx);
/* The reduce by itself, asynchronous on `stream` (NULL = the context's stream), in place on the device buffer pt_render_device
 * filled (n_pixels*3 floats): exactly ONE collective on every rank, whatever else is passed.  d_rgba8 (optional, n_pixels uint32)
 * is an OUTPUT on rank 0 - owl::make_rgba of the reduced frame, bit for bit what the owning ranks would have stored (one non-zero
 * contributor per pixel) - and ignored on the other ranks.  A no-op without a communicator.
 * Environment: PT_RCCL_PATH = the RCCL library to load (default librccl.so.1 by the usual search). */
int pt_reduce_framebuffer(pt_ctx* ctx, void* d_rgb, void* d_rgba8, int64_t n_pixels, void* stream);
/* Pinned host memory for the frame, like the reference's framebuffer (owlBufferGetPointer, owl.hpp:108-111). */
void* pt_host_alloc(size_t bytes);
void pt_host_free(void* p);

/* (b) One process, N GPUs (`pt_main --gpus N` / `pt_main --devices a,b,c`): N contexts + ncclCommInitAll; scene calls fan out to
 *     every device (full replica each), pt_group_render = shards + one reduce + read-back from devices[0].  devices NULL = 0..n-1;
 *     otherwise any n device numbers in any order (n <= 64).  A device named twice is refused by the real RCCL (ncclCommInitAll fails,
 *     pt_group_create returns NULL); the stub collective of the test suite (tests/stub/fake_rccl.cpp) accepts it, which is how the
 *     tests run N contexts on one card.  After pt_group_render returned PT_E_HIP from the reduce, destroy the group. */
typedef struct pt_group pt_group;
pt_group* pt_group_create(const int32_t* devices, int32_t n);   /* NULL on failure; pt_last_error(NULL) has the reason */
void pt_group_destroy(pt_group* g);
int32_t pt_group_size(const pt_group* g);
pt_ctx* pt_group_ctx(pt_group* g, int32_t i);
const char* pt_group_last_error(const pt_group* g);
int pt_group_upload_scene(pt_group* g, const pt_mesh* meshes, int32_t n_meshes, const float* materials, int32_t n_materials,
                          const pt_texture* textures, int32_t n_textures, const int32_t* material_texture, const pt_env* env);
int pt_group_set_materials(pt_group* g, const float* materials, int32_t n_materials);
int pt_group_set_option(pt_group* g, const char* key, int64_t value);
int pt_group_update_vertices(pt_group* g, const pt_mesh* meshes, int32_t n_meshes); /* every device refits its own replica */
int pt_group_render(pt_group* g, const pt_camera* cam, int32_t width, int32_t height, int32_t max_samples, int32_t max_path_depth,
                    float* out_rgb, uint32_t* out_rgba8);
/* pt_render_aov over the group: every device's own tiles, one reduce of the W*H*8 floats onto devices[0], read-back from there */
int pt_group_render_aov(pt_group* g, const pt_camera* cam, int32_t width, int32_t height, int32_t n_samples, float* out_aov);
/* pt_render_aov_follow over the group, the same way */
int pt_group_render_aov_follow(pt_group* g, const pt_camera* cam, int32_t width, int32_t height, const pt_aov_params* p /* NULL = defaults */, float* out_aov);

/* Tuning / test options (all have working defaults; none changes an image, except "watertight"):
 *   "kernel" 2 (default, wavefront-scheduled) | 1 (lane per pixel);  "count" 0/1: instrumented kernel that fills pt_stats;
 *   "leaf_size", "max_bvh_depth": BVH builder, next pt_upload_scene;  "bvh_builder" 3 (default: by triangle count - 0 up to 64 M
 *   triangles, 2 beyond) | 0 (binned SAH on all host threads: the tree that walks fastest, 0.9 M triangles in 58-83 ms) | 1 (linear BVH built on
 *   the device, csrc/pt_lbvh.hip: 50 ms, 1.4x slower to walk) | 2 (PLOC on the device: 88 ms, 1.04-1.25x slower to walk; "ploc_radius" 16);  1 and 2
 *   hand over to 0, and the upload succeeds, where the device tree is deeper than max_bvh_depth, where PLOC has not finished after 4096
 *   rounds, on a host-only context and for no more than leaf_size triangles;  "blocks_per_cu", "slots_per_wave": launch geometry;
 *   "schedule" 1 (default: cost pre-pass + cost-ordered queue, from 4 x prepass_spp samples per pixel) | 0 (chunks only);
 *   "prepass_spp" (0 = automatic: 8, or 16 when a tier plan is prepared), "cost_radius" (2: the cost of a pixel - the time its pre-pass
 *   samples took - is de-noised by the mean over the look-alike pixels of its (2r+1)^2 neighbourhood), "whole" -1 (default: a launch
 *   whose pixels can all have a path slot from the start hands out whole pixels by cost class if a plan made on the device says so)
 *   | 0 (never: ring schedule) | 1 (always), "sticky_pct" (automatic: min(80, 50 + 6 x pixels per path slot) %: share of the
 *   remaining samples a pixel gets in its first chunk), "chunk_spp" (64, schedule 0), "chunk_tail_min" (-1 = automatic: an eighth of the
 *   samples after the pre-pass, at least 16: smallest of the halving tail chunks; 0 = no tail), "spp_per_launch" (kernel 1: samples per launch; kernel 2: forces schedule 0 with this
 *   chunk size - the resumability tests use it);  "census_mode", "latency": diagnostics of the instrumented build;
 *   "groups" 1 (default: a wave with few rays to trace walks them eight lanes per ray over oct nodes) | 0 (never) | 2 (always: tests),
 *   "wide_leaves" 1 (oct nodes: subtrees of <= 7 triangles are one leaf step; next pt_upload_scene), "tune6" / "tune7" (16 / 24: ray-queue
 *   level and running pixels up to which a wave counts as sparse);  "tune0" (8: a shading pass with idle lanes also takes the entries of the other
 *   queue when that holds at least this many; > 64 = never; off by itself when an environment map is bound);
 *   "quad" 1 (default: two binary levels per 128-byte record) | 0;  "box_exact" -1 (default: slab distances by one fma per plane, the
 *   subtracting form when the camera is more than 42 scene extents from the origin) | 0 | 1;  "fallback" 1: use the wavefront kernel's 168-VGPR instance (what
 *   the library does by itself when the 128-VGPR instance of a build needs scratch);
 *   "batch_frames" 0 (default: as many as the limits allow) | n: most frames per launch sequence of pt_render_batch;
 *   "watertight" 0 (default: Moeller-Trumbore, bit for bit the images of every earlier version) | 1: every triangle test of the wavefront
 *   render path (pt_render, pt_render_device, the communicator path, pt_group_render), of the ray probes 30..35 and of
 *   pt_debug_closest_hit_host / _n is the watertight test of Woop, Benthin and Wald in the float32 sequence of DESIGN.md 2.1: no ray
 *   passes between two triangles that share an edge or a vertex (OptiX, which the reference traces with, lets none through either).
 *   THE ONE OPTION THAT CHANGES AN IMAGE: t, u, v of a hit come from another operation sequence, and rays that Moeller-Trumbore lets
 *   through a seam (10-16 % of the rays aimed at shared edges or vertices, ~1e-6 of random ones) now hit.  Everything else of the
 *   closest-hit definition stays: two-sided, t > 1e-3, minimum t, ties to the lower triangle id, slivers collapsed at upload (so a
 *   needle inside a closed mesh still opens a gap of under 1e-5 of its edge).  Switchable between renders of one context, no new
 *   pt_upload_scene.  With "watertight" = 1 these are refused with PT_E_INVALID and a message, never rendered with the other test:
 *   option "kernel" = 1 (either order of the two pt_set_option calls), pt_debug_eval's closest-hit op 21, pt_render_batch(_device).
 *   "dynamic" 0 (default: pt_upload_scene keeps and allocates exactly what it always did) | 1: the NEXT pt_upload_scene also keeps, on
 *   the host and in HBM, what pt_update_vertices needs - the meshes' vertex and normal arrays, three vertex indices per triangle slot,
 *   the binary nodes sorted by height, and for every quad / oct slot the binary box it is a copy of.
 *   "rays_refill" 0..63 (default 32, a starting value nobody had measured when it was chosen; README "Ray queries" has the figures): a wave
 *   of pt_trace_closest / pt_trace_occluded gives its idle lanes new rays of its range when at most this many lanes are still walking -
 *   0: a new batch only when the whole wave is done, 63: whenever a lane is idle.  Like the others it changes no result.
 *   "rays_grid" 0 (default: as many waves as the occupancy query says are resident, or one per 64 rays if that is fewer) | n: at most n
 *   waves, each with a longer range - the tests use it to give a wave many 64-ray blocks to refill from; it changes no result. */
int pt_set_option(pt_ctx* ctx, const char* key, int64_t value);
int pt_get_stats(pt_ctx* ctx, pt_stats* out);

/* ---- host utilities ---- */
/* to_camera_data (camera.cpp:3-21) */
void pt_to_camera_data(const float look_from[3], const float look_at[3], const float look_up[3], float vertical_fov_deg,
                       int32_t width, int32_t height, pt_camera* out);

/* ---- validation hooks (used by tests/ only; never on the render path) ----
 * Closest hit = minimum over all triangles of the Moeller-Trumbore t (option "watertight" = 1: of the watertight test's t, for the host
 * walk and the ray probes 30..35; op 21 is refused then) (ties: lower global triangle id), slivers never hit.  Every walk
 * (lane per pixel, quad, group, host) computes exactly that, whatever the hierarchy, for ray origins whose largest |coordinate| is
 * within 10 x max(scene extent, largest |coordinate| of the scene) and rays that do not lie in a non-axis-aligned triangle's plane up
 * to rounding, nor graze one at its edge at less than 1e-2 rad.  Farther out the triangle test places hits outside the padded boxes (1 of 300 000 rays from 41 extents, 7e-4 of the
 * rays from 3 000: brute force and any hierarchy, the oracle's too, then disagree); DESIGN.md 2.1. */
/* Closest hit through the PRODUCT BVH walked on the host: validates the host builder without a GPU. */
int pt_debug_closest_hit_host(pt_ctx* ctx, const float org[3], const float dir[3], float tmin, float tmax,
                              float* t, float* u, float* v, int32_t* prim);
/* The same for n rays at once (rays: o[3], d[3] each; out: hit, t, u, v, id bits - 5 floats each), on all host threads.  Returns n. */
int64_t pt_debug_closest_hit_host_n(pt_ctx* ctx, const float* rays, int64_t n, float tmin, float tmax, float* out);
/* The CPU twin of the guide pass (pt_render_aov): its definition run by the host walk of pt_debug_closest_hit_host_n over the host
 * copies of the scene, on all host threads; works on a host-only context (device = -1), follows "watertight", the current materials and
 * environment, and pt_update_vertices.  pixel_ids: launch-index ids x + W*y (any, whatever the pixel shard); out: 8 floats per listed
 * pixel, in list order.  Returns n_pixels; PT_E_NO_SCENE / PT_E_INVALID as pt_render_aov, and PT_E_INVALID for an id outside the frame. */
int64_t pt_debug_aov_host(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, int32_t n_samples, const uint32_t* pixel_ids,
                          int64_t n_pixels, float* out);
/* The CPU twin of the follow mode (pt_render_aov_follow), the same way; p NULL = the defaults; PT_E_INVALID also for what that call refuses in p. */
int64_t pt_debug_aov_follow_host(pt_ctx* ctx, const pt_camera* cam, int32_t width, int32_t height, const pt_aov_params* p, const uint32_t* pixel_ids,
                                 int64_t n_pixels, float* out);
/* The CPU twin of the guide pass over a ray image (pt_render_aov_rays), the same way: the follow twin with the camera ray replaced by the
 * pixel's record of `rays` (width x height records).  PT_E_INVALID also for what the blocking form refuses in the table and in p; it
 * walks the host's binary tree, so it works whatever "quad" says, and on a host-only context. */
int64_t pt_debug_aov_rays_host(pt_ctx* ctx, const pt_ray_gen* rays, int32_t width, int32_t height, const pt_aov_params* p,
                               const uint32_t* pixel_ids, int64_t n_pixels, float* out);
/* Batched device-side evaluation of the kernel's building blocks on the GPU (op codes in pt_kernel_aux.hip):
 * lets the parity tests compare them bit-for-bit with the oracle.  in/out are host arrays.
 * Ops 30..35 are RAY PROBES: in = o[3], d[3] per ray, out = {hit, t, u, v, id bits, aux} (6 floats), through the device functions of
 * the render kernel itself (not copies of them):
 *   30 / 31  quad walk, whole stack in LDS: ray_inv -> node4_step<.., all in LDS> -> leaf_test; slab form fma (30) / subtracting (31);
 *   32 / 33  quad walk with the short LDS stack and the HBM overflow column (node4_step<.., PT_LDS_STACK>); fma / subtracting;
 *            aux of 30..33 = deepest stack level the ray's walk reached (entries; > PT_LDS_STACK = 12: pushes went to HBM);
 *   34 / 35  group walk: traverse_groups over the oct nodes, eight lanes per ray, 100 rays per wave in 24 path slots, shading batches of
 *            8 so that groups are parked and resumed; fma / subtracting; t is not carried by that walk (0); aux = group phases of the ray's
 *            wave that had ended with parked groups when the ray was written out.
 * A scene whose quad / oct nodes do not exist (tree too deep) is an error, not another walk.  The caller's rays must be finite. */
int pt_debug_eval(pt_ctx* ctx, int32_t op, const float* in, int32_t in_stride, float* out, int32_t out_stride, int64_t n);

/* Read-back of the hierarchy a context holds after pt_upload_scene (host copies; works on a host-only context and after a device
 * build): raw records as csrc/pt_types.h lays them out.  out NULL: returns the bytes needed; else copies and returns the bytes
 * written (cap too small: PT_E_INVALID).  PT_TREE_INFO: int64[8] = {root, root4, root8, depth, depth4, depth8, pad (float bits in
 * the low word), largest leaf}; roots are node indices or leaf codes; the quad / oct arrays are empty when the tree is too deep for them.
 * which | PT_TREE_DEVICE: the named array read back from HBM (a hipMemcpy) instead of the host copy - what the kernels of
 * pt_update_vertices wrote; PT_E_INVALID on a host-only context; PT_TREE_INFO is the host's either way.  After pt_update_vertices on a
 * device context the host copies are refitted by the first call that reads them (this one without the flag, pt_debug_closest_hit_host /
 * _n, pt_debug_quad_info / _oct_info, pt_debug_clone_scene): the render path never pays for a host refit. */
enum { PT_TREE_BINARY = 0, PT_TREE_QUAD = 1, PT_TREE_OCT = 2, PT_TREE_TRIS = 3, PT_TREE_INFO = 4, PT_TREE_DEVICE = 16 };
int64_t pt_debug_export_tree(pt_ctx* ctx, int32_t which, void* out, int64_t cap);

/* The last pt_update_vertices of this context: out = {device milliseconds from the first kernel to the last (HIP events; 0 on a host-only
 * context), bytes copied host to device, triangles the sliver rule collapsed to points, the padding of the boxes, height levels of the
 * binary tree (= refit launches), 0, 0, 0}; all 0 before the first update. */
int pt_debug_update_info(pt_ctx* ctx, double out[8]);

/* What pt_group_upload_scene does for devices 1..n-1: the scene `src` holds (BVH built once) copied into `dst` and uploaded to
 * dst's GPU.  Exposed so that a one-GPU box can test it with two contexts on the same device. */
int pt_debug_clone_scene(pt_ctx* dst, const pt_ctx* src);

/* Structure of the quad nodes the wavefront kernel walks (host side, no GPU needed): out = {quad nodes, depth, leaf slots,
 * triangles in leaf slots, empty slots, internal slots, binary nodes, binary leaf references}.  Every leaf of the binary tree
 * must appear in exactly one quad slot; an empty slot must carry the never-hit box. */
int pt_debug_quad_info(pt_ctx* ctx, int64_t out[8]);

/* The same for the oct nodes of the group walk (PtNode8): out = {oct nodes, depth, leaf slots, triangles in leaf slots, empty slots,
 * internal slots, largest leaf, triangle slots of the scene}.  Fails (PT_E_LIMIT) if a triangle slot is in no or in two leaves, a
 * triangle sticks out of its leaf's box, a node is referenced twice or an empty slot has a finite box. */
int pt_debug_oct_info(pt_ctx* ctx, int64_t out[8]);

/* The pixel queue of the last pt_render* call with the cost-ordered schedule: queue_ids[i] = pixel id (x + width * y) of
 * entry i of the cost-ordered queue, input_ids[i] / cost[i] = entry i of the shard's input queue and its cost class: 16 log2 of
 * the microseconds its first prepass_spp samples took (1..255).  Any pointer may be NULL.  Returns the number of entries (0: the last
 * render did not sort), or a negative error. */
int64_t pt_debug_read_queue(pt_ctx* ctx, uint32_t* queue_ids, uint32_t* input_ids, uint8_t* cost, int64_t cap);

/* For tests of the queue sort and the tier plan: a cost image of the caller's in place of the measured one.  img: width * height
 * cost classes, index x + width * y; the context keeps a device copy (uploaded here, after waiting for the context's last call like
 * the readers above; freed by pt_destroy).  While an image is set, every launch sequence with the cost-ordered schedule whose launch image
 * is exactly width x height - for pt_render_batch the virtual image W x (K * H) of a sequence of K frames - runs its cost pre-pass as
 * always and then copies the image over the measured costs (device to device, on the launch's stream, before the counting sort): the
 * queue, the tier plan and what pt_debug_read_queue returns as cost are those of the image, the frame is the same bit for bit.  A launch
 * sequence of another size ignores the image.  The bytes are taken as given: the sort reads 0 as "not this rank's pixel", so a caller who
 * wants the semantics of a shard writes 0 at the pixels the rank does not own.  img NULL: back to the measured costs (width and height
 * are not looked at).  PT_E_NO_DEVICE on a host-only context, PT_E_INVALID for a size pt_render refuses. */
int pt_debug_set_cost_image(pt_ctx* ctx, const uint8_t* img, int32_t width, int32_t height);

/* Timeline of the last wavefront launch, three arrays of n_chunks + 1 values: ticks[0] = constant 100 MHz clock (s_memrealtime)
 * at kernel entry, ticks[1 + c] = when the last pixel finished chunk c; then [0] unused, [1 + c] = when the last work item of
 * chunk c started; then [0] unused, [1 + c] = queue entry that finished chunk c last.  Returns the number of values written. */
int64_t pt_debug_read_laps(pt_ctx* ctx, uint64_t* ticks, int64_t cap);

/* With option "latency" = 1: per pixel (index x + width * y), ticks of the 100 MHz clock from the entry of the last cost-ordered main
 * launch to the moment the pixel's last sample was stored (0 for pixels outside this rank's shard); then, if cap allows, a second
 * array of the same size: rays traced per pixel in that launch (option "count" = 1, else zeros).  Returns the number of values
 * written, 0 if the last render was not such a launch. */
int64_t pt_debug_read_finish(pt_ctx* ctx, uint32_t* ticks, int64_t cap);

/* Tier table of the last launch with the whole-pixel schedule (pt_stats.whole_pixels != 0): words[0] = number of tiers, then 8 words
 * per tier: first queue entry, entries, pixels per wave, first workgroup, workgroups, cost class, 2 unused.  Returns the number of
 * words written (at most 257), 0 if the last render used the ring schedule. */
int64_t pt_debug_read_tiers(pt_ctx* ctx, uint32_t* words, int64_t cap);

/* The tier plan for a launch whose cost-ordered queue holds bucket_pixels[b] pixels in cost bucket b (32 buckets, 0 = most expensive,
 * each 19 % cheaper than the one before), with `capacity` resident workgroups and `ns` path slots per wave: exactly what the device
 * computes after the counting sort, run on the host (no GPU needed).  force = 1: plan even when the cost distribution has no tail.
 * Same output as pt_debug_read_tiers (words[0] = 0: the plan declines and the launch runs the ring schedule); cap >= 257. */
int64_t pt_debug_plan_tiers(const uint32_t* bucket_pixels, int32_t capacity, int32_t ns, int32_t force, uint32_t* words, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MI355PT_H */
