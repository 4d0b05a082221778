"""ctypes binding of the C-ABI in include/mi355pt.h (libmi355pt.so) for tests and bench.py.

There is NO fallback: if the shared object is missing, or a render is requested without a gfx950 GPU, this
raises.  Nothing here imports or calls the CPU oracle.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("PT_LIB_PATH") or os.path.join(_PKG, "libmi355pt.so")  # PT_LIB_PATH: A/B builds (tools/ab_bench.py)
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "mi355pt.h")

PT_MAT_FLOATS = 17
OPS = {"sin": 0, "cos": 1, "tan": 2, "atan": 3, "atan2": 4, "asin": 5, "log": 6, "exp": 7, "pow": 8, "sqrt": 9, "div": 10,
       "sample_disney": 20, "closest_hit": 21, "frame": 22, "rng": 23,
       # ray probes through the render kernel's own walks (include/mi355pt.h): quad walk with the whole stack in LDS / with the HBM overflow
       # column, group walk; "_exact" = the subtracting slab form.  6 floats out: hit, t, u, v, id bits, aux
       "quad": 30, "quad_exact": 31, "quad_ovf": 32, "quad_ovf_exact": 33, "group": 34, "group_exact": 35}
PROBE_OPS = ("quad", "quad_exact", "quad_ovf", "quad_ovf_exact", "group", "group_exact")
PT_LDS_STACK = 12  # csrc/pt_trace.h: stack levels of the quad walk kept in LDS

# csrc/pt_types.h, for Context.export_trees
NODE_DTYPE = np.dtype([("lo", "<f4", (3, 2)), ("hi", "<f4", (3, 2)), ("left", "<i4"), ("right", "<i4"), ("pad", "<u4", (2,))])
NODE4_DTYPE = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("child", "<i4", (4,)), ("pad", "<u4", (4,))])
NODE8_DTYPE = np.dtype([("c", [("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("ref", "<i4"), ("pad", "<u4")], (8,))])
TRI_DTYPE = np.dtype([("p0", "<f4", (3,)), ("p1", "<f4", (3,)), ("p2", "<f4", (3,)), ("id", "<i4"), ("material", "<i4"), ("pad", "<u4")])
assert (NODE_DTYPE.itemsize, NODE4_DTYPE.itemsize, NODE8_DTYPE.itemsize, TRI_DTYPE.itemsize) == (64, 128, 256, 48)


class PtError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("reserved", C.c_int32)]


class Mesh(C.Structure):
    _fields_ = [("vertices", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)), ("texcoords", C.POINTER(C.c_float)),
                ("indices", C.POINTER(C.c_int32)), ("n_vertices", C.c_int32), ("n_normals", C.c_int32), ("n_texcoords", C.c_int32),
                ("n_triangles", C.c_int32), ("material_index", C.c_int32), ("texture_index", C.c_int32)]


class Texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgba8", C.POINTER(C.c_uint32))]


class Env(C.Structure):
    _fields_ = [("use_map", C.c_int32), ("use_auto", C.c_int32), ("color", C.c_float * 3), ("intensity", C.c_float), ("map", Texture)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("llc", C.c_float * 3), ("horizontal", C.c_float * 3), ("vertical", C.c_float * 3)]

    def as_array(self):
        return np.array(list(self.origin) + list(self.llc) + list(self.horizontal) + list(self.vertical), np.float32)


class Frame(C.Structure):
    """pt_frame: one frame of a batch - its camera and its material table (NULL: the context's current one)."""
    _fields_ = [("camera", Camera), ("materials", C.POINTER(C.c_float))]


class DenoiseParams(C.Structure):
    """pt_denoise_params: iterations L (1..8), flags (PT_DENOISE_DEMODULATE), the four sigmas (> 0; +inf switches a term off)."""
    _fields_ = [("iterations", C.c_int32), ("flags", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("sigma_albedo", C.c_float)]


class AovParams(C.Structure):
    """pt_aov_params: n_samples (>= 1), max_follow (0..8 specular surfaces a guide ray may pass), roughness_max (0..1), reserved (0)."""
    _fields_ = [("n_samples", C.c_int32), ("max_follow", C.c_int32), ("roughness_max", C.c_float), ("reserved", C.c_int32)]


class AoParams(C.Structure):
    """pt_ao_params: n_rays (K, 1..4096 occlusion rays per hit), flags (PT_AO_SHADING_NORMAL), radius (> 0; +inf: the library's bound), seed."""
    _fields_ = [("n_rays", C.c_int32), ("flags", C.c_int32), ("radius", C.c_float), ("seed", C.c_uint32)]


class HitsParams(C.Structure):
    """pt_hits_params: max_hits (K, 1..PT_HITS_MAX records per ray), three reserved words (0)."""
    _fields_ = [("max_hits", C.c_int32), ("reserved", C.c_int32 * 3)]


class AccumParams(C.Structure):
    """pt_accum_params: n_samples (1..65535) for every active pixel, max_pixel_samples (0: no cap), noise_threshold (0: uniform add), reserved (0)."""
    _fields_ = [("n_samples", C.c_int32), ("max_pixel_samples", C.c_int32), ("noise_threshold", C.c_float), ("reserved", C.c_int32)]


class ReprojectParams(C.Structure):
    """pt_reproject_params: max_history (0: no cap, else >= 2), reserved (0), depth_tol (>= 0), normal_min (<= 1), albedo_tol (>= 0); +inf / -inf switch a test off."""
    _fields_ = [("max_history", C.c_int32), ("reserved", C.c_int32), ("depth_tol", C.c_float), ("normal_min", C.c_float), ("albedo_tol", C.c_float)]


pt_reproject_params = ReprojectParams


class UpsampleParams(C.Structure):
    """pt_upsample_params: taps (2 or 4), flags (PT_UPSAMPLE_DEMODULATE), three sigmas (> 0; +inf switches a term off), reserved (0)."""
    _fields_ = [("taps", C.c_int32), ("flags", C.c_int32), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float),
                ("reserved", C.c_int32)]


class AccumInfo(C.Structure):
    """pt_accum_info."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("max_path_depth", C.c_int32), ("adds", C.c_int32), ("owned_pixels", C.c_int64),
                ("active_pixels", C.c_int64), ("samples_total", C.c_uint64)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("launches", C.c_int32), ("vgprs", C.c_int32), ("sgprs", C.c_int32), ("lds_bytes", C.c_int32),
                ("block", C.c_int32), ("grid", C.c_int32), ("stack_entries", C.c_int32),
                ("samples", C.c_uint64), ("rays", C.c_uint64), ("nodes", C.c_uint64), ("tris", C.c_uint64), ("scatters", C.c_uint64),
                ("env_misses", C.c_uint64), ("nan_retries", C.c_uint64), ("bvh_nodes", C.c_uint64), ("bvh_depth", C.c_uint64),
                ("n_triangles", C.c_uint64), ("bvh_build_ms", C.c_double), ("sched", C.c_uint64 * 32), ("prepass_ms", C.c_double), ("groups", C.c_uint64 * 8), ("reduce_ms", C.c_double), ("d2h_ms", C.c_double), ("kernel_variant", C.c_int32), ("express_pixels", C.c_int32), ("whole_pixels", C.c_int32), ("prepass_spp", C.c_int32), ("lobes", C.c_uint64 * 16), ("trav", C.c_uint64 * 4)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["sched"] = list(self.sched)
        d["groups"] = list(self.groups)
        d["lobes"] = list(self.lobes)
        d["trav"] = list(self.trav)
        return d


EXPORTS = ["pt_create", "pt_destroy", "pt_last_error", "pt_abi_version", "pt_upload_scene", "pt_set_materials", "pt_set_environment",
           "pt_set_pixel_shard", "pt_shard_pixels", "pt_render", "pt_render_device", "pt_synchronize", "pt_set_option", "pt_get_stats",
           "pt_to_camera_data", "pt_debug_closest_hit_host", "pt_debug_closest_hit_host_n", "pt_debug_export_tree", "pt_debug_eval", "pt_debug_read_queue", "pt_debug_read_laps", "pt_debug_read_finish", "pt_debug_read_tiers", "pt_debug_plan_tiers", "pt_debug_set_cost_image",
           "pt_comm_get_unique_id", "pt_comm_init_rank", "pt_comm_destroy", "pt_reduce_framebuffer", "pt_host_alloc", "pt_host_free",
           "pt_group_create", "pt_group_destroy", "pt_group_size", "pt_group_ctx", "pt_group_last_error", "pt_group_upload_scene",
           "pt_group_set_materials", "pt_group_set_option", "pt_group_render", "pt_debug_quad_info", "pt_debug_oct_info", "pt_debug_clone_scene",
           "pt_render_batch", "pt_render_batch_device", "pt_debug_plan_batch", "pt_update_vertices", "pt_group_update_vertices", "pt_debug_update_info",
           "pt_render_aov", "pt_render_aov_device", "pt_group_render_aov", "pt_debug_aov_host",
           "pt_denoise_default_params", "pt_denoise", "pt_denoise_device", "pt_debug_denoise_host",
           "pt_aov_default_params", "pt_render_aov_follow", "pt_render_aov_follow_device", "pt_group_render_aov_follow", "pt_debug_aov_follow_host",
           "pt_render_aov_batch", "pt_render_aov_batch_device", "pt_denoise_batch", "pt_denoise_batch_device",
           "pt_accum_default_params", "pt_accum_begin", "pt_accum_add", "pt_accum_add_device", "pt_accum_read", "pt_accum_info_get", "pt_accum_end",
           "pt_debug_accum_resolve_host", "pt_debug_accum_select_host", "pt_debug_accum_state",
           "pt_denoise_var_default_params", "pt_denoise_var", "pt_denoise_var_device", "pt_debug_denoise_var_host",
           "pt_accum_variance", "pt_debug_accum_variance_host", "pt_accum_denoise", "pt_accum_denoise_device",
           "pt_accum_reproject_default_params", "pt_accum_reproject", "pt_accum_reproject_device", "pt_debug_accum_reproject_host",
           "pt_upsample_default_params", "pt_upsample", "pt_upsample_device", "pt_debug_upsample_host",
           "pt_trace_closest", "pt_trace_closest_device", "pt_trace_occluded", "pt_trace_occluded_device", "pt_debug_trace_rays_host", "pt_prim_to_mesh", "pt_trace_surface", "pt_trace_surface_device", "pt_debug_trace_surface_host",
           "pt_ao_default_params", "pt_trace_ao", "pt_trace_ao_device", "pt_debug_trace_ao_host",
           "pt_hits_default_params", "pt_trace_hits", "pt_trace_hits_device", "pt_debug_trace_hits_host",
           "pt_closest_point", "pt_closest_point_device", "pt_debug_closest_point_host",
           "pt_render_rays", "pt_render_rays_device", "pt_render_aov_rays", "pt_render_aov_rays_device", "pt_debug_aov_rays_host"]
# pt_ray / pt_ray_hit (include/mi355pt.h "ray queries"): 32 and 16 bytes
RAY_DTYPE = np.dtype([("org", "<f4", (3,)), ("tmax", "<f4"), ("dir", "<f4", (3,)), ("unused", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 16
# pt_surface (include/mi355pt.h "ray queries: the surface at the hit"): pt_trace_closest's record, then what lies at the hit
SURFACE_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("p", "<f4", (3,)), ("material", "<i4"), ("ng", "<f4", (3,)), ("tu", "<f4"),
                          ("ns", "<f4", (3,)), ("tv", "<f4"), ("base", "<f4", (3,)), ("emission", "<f4")])
assert SURFACE_DTYPE.itemsize == 80
# pt_ao_hit (include/mi355pt.h "ray queries: ambient occlusion"): pt_trace_closest's record, then the facing normal and the occlusion
AO_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("n", "<f4", (3,)), ("ao", "<f4")])
assert AO_DTYPE.itemsize == 32 and C.sizeof(AoParams) == 16
PT_AO_SHADING_NORMAL = 1
PT_HITS_MAX = 16  # pt_trace_hits: the largest K
assert C.sizeof(HitsParams) == 16
# pt_point / pt_point_hit (include/mi355pt.h "point queries: the nearest surface"): 16 and 32 bytes
POINT_DTYPE = np.dtype([("p", "<f4", (3,)), ("radius", "<f4")])
POINT_HIT_DTYPE = np.dtype([("dist", "<f4"), ("u", "<f4"), ("v", "<f4"), ("prim", "<i4"), ("q", "<f4", (3,)), ("feature", "<i4")])
assert POINT_DTYPE.itemsize == 16 and POINT_HIT_DTYPE.itemsize == 32
# pt_ray_gen (include/mi355pt.h "ray images"): 64 bytes; pyhost/ray_image.py builds tables of these
RAY_GEN_DTYPE = np.dtype([("org", "<f4", (3,)), ("reserved0", "<f4"), ("dir", "<f4", (3,)), ("reserved1", "<f4"),
                          ("du", "<f4", (3,)), ("reserved2", "<f4"), ("dv", "<f4", (3,)), ("reserved3", "<f4")])
assert RAY_GEN_DTYPE.itemsize == 64
PT_DENOISE_DEMODULATE = 1
PT_UPSAMPLE_DEMODULATE = 1
PT_TREE_DEVICE = 16  # pt_debug_export_tree: ORed into `which`, the array as HBM holds it
PT_COMM_ID_BYTES = 128

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PtError("libmi355pt.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    L = C.CDLL(LIB_PATH)
    fp = C.POINTER(C.c_float)
    L.pt_create.restype = C.c_void_p
    L.pt_create.argtypes = [C.POINTER(Config)]
    L.pt_destroy.restype = None
    L.pt_destroy.argtypes = [C.c_void_p]
    L.pt_last_error.restype = C.c_char_p
    L.pt_last_error.argtypes = [C.c_void_p]
    L.pt_abi_version.restype = C.c_int
    L.pt_upload_scene.argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_int32, fp, C.c_int32, C.POINTER(Texture), C.c_int32,
                                  C.POINTER(C.c_int32), C.POINTER(Env)]
    L.pt_set_materials.argtypes = [C.c_void_p, fp, C.c_int32]
    L.pt_set_environment.argtypes = [C.c_void_p, C.POINTER(Env)]
    L.pt_set_pixel_shard.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.pt_shard_pixels.restype = C.c_int64
    L.pt_shard_pixels.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int64]
    L.pt_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, C.POINTER(C.c_uint32)]
    L.pt_render_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_synchronize.argtypes = [C.c_void_p]
    L.pt_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.pt_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.pt_to_camera_data.restype = None
    L.pt_to_camera_data.argtypes = [fp, fp, fp, C.c_float, C.c_int32, C.c_int32, C.POINTER(Camera)]
    L.pt_debug_closest_hit_host.argtypes = [C.c_void_p, fp, fp, C.c_float, C.c_float, fp, fp, fp, C.POINTER(C.c_int32)]
    L.pt_debug_closest_hit_host_n.argtypes = [C.c_void_p, fp, C.c_int64, C.c_float, C.c_float, fp]
    L.pt_debug_closest_hit_host_n.restype = C.c_int64
    L.pt_debug_export_tree.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    L.pt_debug_export_tree.restype = C.c_int64
    L.pt_debug_eval.argtypes = [C.c_void_p, C.c_int32, fp, C.c_int32, fp, C.c_int32, C.c_int64]
    L.pt_debug_read_queue.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.c_int64]
    L.pt_debug_read_queue.restype = C.c_int64
    L.pt_debug_read_laps.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_int64]
    L.pt_debug_read_laps.restype = C.c_int64
    L.pt_debug_read_finish.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64]
    L.pt_debug_read_finish.restype = C.c_int64
    L.pt_debug_read_tiers.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_int64]
    L.pt_debug_read_tiers.restype = C.c_int64
    L.pt_debug_plan_tiers.argtypes = [C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int64]
    L.pt_debug_plan_tiers.restype = C.c_int64
    L.pt_debug_set_cost_image.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]
    u8p = C.POINTER(C.c_uint8)
    L.pt_comm_get_unique_id.argtypes = [u8p]
    L.pt_comm_init_rank.argtypes = [C.c_void_p, u8p, C.c_int32, C.c_int32]
    L.pt_comm_destroy.argtypes = [C.c_void_p]
    L.pt_reduce_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_host_alloc.restype = C.c_void_p
    L.pt_host_alloc.argtypes = [C.c_size_t]
    L.pt_host_free.restype = None
    L.pt_host_free.argtypes = [C.c_void_p]
    L.pt_group_create.restype = C.c_void_p
    L.pt_group_create.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    L.pt_group_destroy.restype = None
    L.pt_group_destroy.argtypes = [C.c_void_p]
    L.pt_group_size.argtypes = [C.c_void_p]
    L.pt_group_ctx.restype = C.c_void_p
    L.pt_group_ctx.argtypes = [C.c_void_p, C.c_int32]
    L.pt_group_last_error.restype = C.c_char_p
    L.pt_group_last_error.argtypes = [C.c_void_p]
    L.pt_group_upload_scene.argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_int32, fp, C.c_int32, C.POINTER(Texture), C.c_int32,
                                        C.POINTER(C.c_int32), C.POINTER(Env)]
    L.pt_group_set_materials.argtypes = [C.c_void_p, fp, C.c_int32]
    L.pt_group_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.pt_debug_quad_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.pt_debug_oct_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.pt_debug_clone_scene.argtypes = [C.c_void_p, C.c_void_p]
    L.pt_group_render.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, C.POINTER(C.c_uint32)]
    L.pt_render_batch.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, C.POINTER(C.c_uint32)]
    L.pt_render_batch_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_debug_plan_batch.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int64]
    L.pt_debug_plan_batch.restype = C.c_int64
    L.pt_update_vertices.argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_int32]
    L.pt_group_update_vertices.argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_int32]
    L.pt_debug_update_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.pt_render_aov.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, fp]
    L.pt_render_aov_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.pt_group_render_aov.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, fp]
    L.pt_debug_aov_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int64, fp]
    L.pt_debug_aov_host.restype = C.c_int64
    L.pt_aov_default_params.restype = None
    L.pt_aov_default_params.argtypes = [C.POINTER(AovParams)]
    L.pt_render_aov_follow.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(AovParams), fp]
    L.pt_render_aov_follow_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(AovParams), C.c_void_p, C.c_void_p]
    L.pt_group_render_aov_follow.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(AovParams), fp]
    L.pt_debug_aov_follow_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.POINTER(AovParams), C.POINTER(C.c_uint32), C.c_int64, fp]
    L.pt_debug_aov_follow_host.restype = C.c_int64
    L.pt_denoise_default_params.restype = None
    L.pt_denoise_default_params.argtypes = [C.POINTER(DenoiseParams)]
    L.pt_denoise.argtypes = [C.c_void_p, fp, fp, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), fp, C.POINTER(C.c_uint32)]
    L.pt_denoise_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_debug_denoise_host.argtypes = [C.c_void_p, fp, fp, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), fp, C.POINTER(C.c_uint32)]
    L.pt_debug_denoise_host.restype = C.c_int64
    L.pt_render_aov_batch.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AovParams), fp]
    L.pt_render_aov_batch_device.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AovParams), C.c_void_p, C.c_void_p]
    L.pt_denoise_batch.argtypes = [C.c_void_p, fp, fp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), fp, C.POINTER(C.c_uint32)]
    L.pt_denoise_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
    u32p = C.POINTER(C.c_uint32)
    L.pt_accum_default_params.restype = None
    L.pt_accum_default_params.argtypes = [C.POINTER(AccumParams)]
    L.pt_accum_begin.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_int32, C.c_int32, C.c_int32]
    L.pt_accum_add.argtypes = [C.c_void_p, C.POINTER(AccumParams), fp, u32p]
    L.pt_accum_add_device.argtypes = [C.c_void_p, C.POINTER(AccumParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_accum_read.argtypes = [C.c_void_p, fp, u32p, fp, u32p]
    L.pt_accum_info_get.argtypes = [C.c_void_p, C.POINTER(AccumInfo)]
    L.pt_accum_end.argtypes = [C.c_void_p]
    L.pt_debug_accum_resolve_host.argtypes = [C.c_void_p, C.c_int64, fp, fp, fp, u32p, u32p, u32p, u8p, u8p, C.c_int32, fp, u32p, fp]
    L.pt_debug_accum_resolve_host.restype = C.c_int64
    L.pt_debug_accum_select_host.argtypes = [C.c_void_p, fp, u32p, u8p, C.c_int64, C.POINTER(AccumParams), u8p]
    L.pt_debug_accum_select_host.restype = C.c_int64
    L.pt_debug_accum_state.argtypes = [C.c_void_p, fp, fp, u32p, u32p, u32p]
    L.pt_denoise_var_default_params.restype = None
    L.pt_denoise_var_default_params.argtypes = [C.POINTER(DenoiseParams)]
    L.pt_denoise_var.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), fp, u32p]
    L.pt_denoise_var_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_debug_denoise_var_host.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32, C.c_int32, C.POINTER(DenoiseParams), fp, u32p, fp]
    L.pt_debug_denoise_var_host.restype = C.c_int64
    L.pt_accum_variance.argtypes = [C.c_void_p, fp]
    L.pt_debug_accum_variance_host.argtypes = [C.c_void_p, C.c_int64, fp, fp, u32p, u32p, u8p, fp, fp]
    L.pt_debug_accum_variance_host.restype = C.c_int64
    L.pt_accum_denoise.argtypes = [C.c_void_p, fp, C.POINTER(DenoiseParams), fp, u32p]
    L.pt_accum_denoise_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_accum_reproject_default_params.restype = None
    L.pt_accum_reproject_default_params.argtypes = [C.POINTER(ReprojectParams)]
    L.pt_accum_reproject.argtypes = [C.c_void_p, C.POINTER(Camera), fp, fp, C.POINTER(ReprojectParams)]
    L.pt_accum_reproject_device.argtypes = [C.c_void_p, C.POINTER(Camera), C.c_void_p, C.c_void_p, C.POINTER(ReprojectParams), C.c_void_p]
    L.pt_debug_accum_reproject_host.argtypes = [C.c_void_p, C.POINTER(Camera), C.POINTER(Camera), C.c_int32, C.c_int32, fp, fp, u8p, C.POINTER(ReprojectParams),
                                                fp, fp, u32p, u32p, u32p, fp, u32p, fp]
    L.pt_debug_accum_reproject_host.restype = C.c_int64
    L.pt_upsample_default_params.restype = None
    L.pt_upsample_default_params.argtypes = [C.POINTER(UpsampleParams)]
    L.pt_upsample.argtypes = [C.c_void_p, fp, fp, C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32, C.POINTER(UpsampleParams), fp, u32p]
    L.pt_upsample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(UpsampleParams), C.c_void_p, C.c_void_p,
                                     C.c_void_p]
    L.pt_debug_upsample_host.argtypes = [C.c_void_p, fp, fp, C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32, C.POINTER(UpsampleParams), fp, u32p]
    L.pt_debug_upsample_host.restype = C.c_int64
    L.pt_trace_closest.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_trace_closest_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.pt_trace_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_trace_occluded_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.pt_debug_trace_rays_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
    L.pt_debug_trace_rays_host.restype = C.c_int64
    L.pt_prim_to_mesh.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.pt_trace_surface.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_trace_surface_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.pt_debug_trace_surface_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_debug_trace_surface_host.restype = C.c_int64
    L.pt_ao_default_params.argtypes = [C.POINTER(AoParams)]
    L.pt_ao_default_params.restype = None
    L.pt_trace_ao.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AoParams), C.c_void_p]
    L.pt_trace_ao_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AoParams), C.c_void_p, C.c_void_p]
    L.pt_debug_trace_ao_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AoParams), C.c_void_p, C.c_void_p]
    L.pt_debug_trace_ao_host.restype = C.c_int64
    L.pt_hits_default_params.argtypes = [C.POINTER(HitsParams)]
    L.pt_hits_default_params.restype = None
    L.pt_trace_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(HitsParams), C.c_void_p]
    L.pt_trace_hits_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(HitsParams), C.c_void_p, C.c_void_p]
    L.pt_debug_trace_hits_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(HitsParams), C.c_void_p]
    L.pt_debug_trace_hits_host.restype = C.c_int64
    L.pt_closest_point.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_closest_point_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.pt_debug_closest_point_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pt_debug_closest_point_host.restype = C.c_int64
    L.pt_render_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, fp, C.POINTER(C.c_uint32)]
    L.pt_render_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pt_render_aov_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(AovParams), fp]
    L.pt_render_aov_rays_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(AovParams), C.c_void_p, C.c_void_p]
    L.pt_debug_aov_rays_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(AovParams), C.POINTER(C.c_uint32), C.c_int64, fp]
    L.pt_debug_aov_rays_host.restype = C.c_int64
    _lib = L
    return L


def comm_unique_id():
    """128 opaque bytes from rank 0 (ncclGetUniqueId inside the library) for pt_comm_init_rank on every rank."""
    buf = (C.c_uint8 * PT_COMM_ID_BYTES)()
    rc = lib().pt_comm_get_unique_id(buf)
    if rc < 0:
        raise PtError("pt_comm_get_unique_id failed (%d): %s" % (rc, lib().pt_last_error(None).decode()))
    return bytes(buf)


class PinnedFrame:
    """W x H x 3 float32 (and optionally W x H uint32) in pinned host memory from pt_host_alloc, viewed as numpy arrays."""

    def __init__(self, W, H, want_rgba8=False):
        self._p = lib().pt_host_alloc(W * H * 12)
        self._p8 = lib().pt_host_alloc(W * H * 4) if want_rgba8 else None
        if not self._p or (want_rgba8 and not self._p8):
            raise PtError("pt_host_alloc failed")
        self.rgb = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_float)), shape=(H, W, 3))
        self.rgba8 = np.ctypeslib.as_array(C.cast(self._p8, C.POINTER(C.c_uint32)), shape=(H, W)) if want_rgba8 else None

    def free(self):
        if getattr(self, "_p", None):
            self.rgb = None
            lib().pt_host_free(self._p)
            self._p = None
        if getattr(self, "_p8", None):
            self.rgba8 = None
            lib().pt_host_free(self._p8)
            self._p8 = None


def _vec3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def to_camera_data(look_from, look_at, look_up, vfov, w, h):
    cam = Camera()
    lib().pt_to_camera_data(_vec3(look_from), _vec3(look_at), _vec3(look_up), float(vfov), int(w), int(h), C.byref(cam))
    return cam


def shard_pixels(w, h, tile, rank, world):
    n = lib().pt_shard_pixels(w, h, tile, rank, world, None, 0)
    if n < 0:
        raise PtError("pt_shard_pixels: invalid arguments")
    ids = np.empty(int(n), np.uint32)
    lib().pt_shard_pixels(w, h, tile, rank, world, ids.ctypes.data_as(C.POINTER(C.c_uint32)), n)
    return ids


def _texture(arr):
    t = Texture()
    if arr is None:
        t.width = t.height = 0
        t.rgba8 = None
        return t, None
    a = np.ascontiguousarray(arr, np.uint32)
    t.width, t.height = a.shape[1], a.shape[0]
    t.rgba8 = a.ctypes.data_as(C.POINTER(C.c_uint32))
    return t, a


def make_env(use_map=False, use_auto=False, color=(0, 0, 0), intensity=0.0, env_map=None):
    e = Env()
    e.use_map = int(bool(use_map))
    e.use_auto = int(bool(use_auto))
    for i in range(3):
        e.color[i] = float(color[i])
    e.intensity = float(intensity)
    e.map, e._keep = _texture(env_map)
    return e


def make_rays(rays, tmax=np.inf):
    """(n, 6) float32 origins and directions -> n pt_ray records (RAY_DTYPE) with the given bound(s): a scalar or n values.  The
    float that the library does not read is set to NaN."""
    r = np.asarray(rays, np.float32).reshape(-1, 6)
    out = np.zeros(r.shape[0], RAY_DTYPE)
    out["org"], out["dir"] = r[:, :3], r[:, 3:]
    out["tmax"] = np.asarray(tmax, np.float32)
    out["unused"] = np.float32(np.nan)
    return out


def _rays(rays):
    """pt_ray records as a contiguous RAY_DTYPE array (an (n, 6) float array gets tmax = +inf)."""
    a = np.asarray(rays)
    return np.ascontiguousarray(a) if a.dtype == RAY_DTYPE else make_rays(a)


def make_points(points, radius=np.inf):
    """(n, 3) float32 positions -> n pt_point records (POINT_DTYPE) with the given radius or radii: a scalar or n values."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.zeros(p.shape[0], POINT_DTYPE)
    out["p"] = p
    out["radius"] = np.asarray(radius, np.float32)
    return out


def _points(points):
    """pt_point records as a contiguous POINT_DTYPE array (an (n, 3) float array gets radius = +inf)."""
    a = np.asarray(points)
    return np.ascontiguousarray(a) if a.dtype == POINT_DTYPE else make_points(a)


def denoise_default_params(**changes):
    """pt_denoise_default_params (5 iterations, no flag, sigmas 4, 0.25, 0.1, 0.2), with the given fields changed."""
    p = DenoiseParams()
    lib().pt_denoise_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(DenoiseParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def denoise_var_default_params(**changes):
    """pt_denoise_var_default_params (as denoise_default_params, sigma_color 3 - standard deviations), with the given fields changed."""
    p = DenoiseParams()
    lib().pt_denoise_var_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(DenoiseParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def upsample_default_params(**changes):
    """pt_upsample_default_params (taps 4, PT_UPSAMPLE_DEMODULATE, sigmas 0.25, 0.1, 0.2), with the given fields changed."""
    p = UpsampleParams()
    lib().pt_upsample_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(UpsampleParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def aov_default_params(**changes):
    """pt_aov_default_params (1 sample, max_follow 4, roughness_max 0.3), with the given fields changed."""
    p = AovParams()
    lib().pt_aov_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(AovParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def hits_params(k=None):
    """The pt_hits_params of a call: k None = pt_hits_default_params (K = 4), an int = that K, a HitsParams = itself."""
    if isinstance(k, HitsParams):
        return k
    p = HitsParams()
    lib().pt_hits_default_params(C.byref(p))
    if k is not None:
        p.max_hits = int(k)
    return p


def ao_default_params(**changes):
    """pt_ao_default_params (16 rays, hemisphere about the geometric normal, radius +inf, seed 0), with the given fields changed."""
    p = AoParams()
    lib().pt_ao_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(AoParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def accum_default_params(**changes):
    """pt_accum_default_params (16 samples, no cap, threshold 0 = uniform), with the given fields changed."""
    p = AccumParams()
    lib().pt_accum_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(AccumParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def reproject_default_params(**changes):
    """pt_accum_reproject_default_params (no cap, depth_tol 0.05, normal_min 0.9, albedo_tol 0.1), with the given fields changed."""
    p = ReprojectParams()
    lib().pt_accum_reproject_default_params(C.byref(p))
    for k, v in changes.items():
        if k not in dict(ReprojectParams._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def plan_tiers(bucket_pixels, capacity, ns=96, force=False):
    """The device's tier plan (pt_tiers.h) for a cost histogram of 32 buckets, run on the host: list of dicts as Context.read_tiers()."""
    h = np.ascontiguousarray(bucket_pixels, np.uint32)
    assert h.size == 32
    t = np.zeros(257, np.uint32)
    n = lib().pt_debug_plan_tiers(h.ctypes.data_as(C.POINTER(C.c_uint32)), int(capacity), int(ns), int(bool(force)), t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size)
    if n < 0:
        raise RuntimeError("pt_debug_plan_tiers: %d" % n)
    return [dict(zip(("q0", "pixels", "per_wave", "wave0", "waves", "cost_class"), (int(x) for x in t[1 + 8 * i:7 + 8 * i]))) for i in range(int(t[0]))]


def plan_batch(W, H, n_frames, max_frames=0):
    """How pt_render_batch cuts n_frames frames of W x H into launch sequences (host only): frames per sequence.  max_frames = option
    "batch_frames".  Raises PtError when one frame is already beyond a launch sequence, or for bad arguments."""
    n = lib().pt_debug_plan_batch(int(W), int(H), int(n_frames), int(max_frames), None, 0)
    if n < 0:
        raise PtError("pt_debug_plan_batch failed (%d): %s" % (n, "one frame exceeds a launch sequence" if n == -5 else "invalid arguments"))
    out = (C.c_int32 * int(n))()
    lib().pt_debug_plan_batch(int(W), int(H), int(n_frames), int(max_frames), out, int(n))
    return [int(x) for x in out]


def _marshal_frames(frames):
    """frames: list of (Camera, materials or None), materials (n, 17) float32.  Returns (Frame array, materials per frame, keep-alive)."""
    arr = (Frame * max(1, len(frames)))()
    keep, n_mat = [], 0
    for i, (cam, mats) in enumerate(frames):
        C.memmove(C.byref(arr[i].camera), C.byref(cam), C.sizeof(Camera))
        if mats is None:
            arr[i].materials = None
        else:
            m = np.ascontiguousarray(np.asarray(mats, np.float32).reshape(-1, PT_MAT_FLOATS))
            keep.append(m)
            n_mat = m.shape[0]
            arr[i].materials = m.ctypes.data_as(C.POINTER(C.c_float))
    return arr, n_mat, keep


def _marshal_scene(entities, materials, textures=None, mesh_textures=None, env=None):
    """The argument list of pt_upload_scene / pt_group_upload_scene after the handle, and the arrays it points into (keep them
    alive until the call returned).  entities: list of (mesh dict, material index); materials: (n,17) float32; textures: list of
    (H,W) uint32 arrays; mesh_textures: per-entity texture index (or None)."""
    textures = textures or []
    keep = []
    arr = (Mesh * max(1, len(entities)))()
    for i, (m, mat_id) in enumerate(entities):
        v = np.ascontiguousarray(m["vertices"], np.float32)
        n = np.ascontiguousarray(m["normals"], np.float32)
        tc = np.ascontiguousarray(m["texcoords"], np.float32)
        idx = np.ascontiguousarray(m["indices"], np.int32)
        keep += [v, n, tc, idx]
        e = arr[i]
        e.vertices = v.ctypes.data_as(C.POINTER(C.c_float))
        e.normals = n.ctypes.data_as(C.POINTER(C.c_float)) if n.size else None
        e.texcoords = tc.ctypes.data_as(C.POINTER(C.c_float)) if tc.size else None
        e.indices = idx.ctypes.data_as(C.POINTER(C.c_int32))
        e.n_vertices, e.n_normals, e.n_texcoords, e.n_triangles = v.shape[0], n.shape[0], tc.shape[0], idx.shape[0]
        e.material_index = int(mat_id)
        e.texture_index = int(mesh_textures[i]) if mesh_textures is not None else -1
    mats = np.ascontiguousarray(np.asarray(materials, np.float32).reshape(-1, PT_MAT_FLOATS))
    tarr = (Texture * max(1, len(textures)))()
    for i, t in enumerate(textures):
        tarr[i], k = _texture(t)
        keep.append(k)
    keep += [arr, mats, tarr, env]
    envp = C.byref(env) if env is not None else None
    return (arr, len(entities), mats.ctypes.data_as(C.POINTER(C.c_float)), mats.shape[0], tarr, len(textures), None, envp), keep


def _mesh_counts(entities):
    return [(int(np.asarray(m["vertices"]).reshape(-1, 3).shape[0]), int(np.asarray(m["normals"]).reshape(-1, 3).shape[0])) for m, _ in entities]


def _marshal_update(meshes, counts):
    """The pt_mesh array of pt_update_vertices.  meshes: one entry per uploaded mesh - None (unchanged) or a dict with "vertices" and /
    or "normals" (a missing or None array is passed as NULL: vertices = the mesh is unchanged, normals = keep the retained ones); the keys
    "n_vertices" / "n_normals" override a count.  counts: (n_vertices, n_normals) per mesh as uploaded, for the arrays that are not passed."""
    keep = []
    arr = (Mesh * max(1, len(meshes)))()
    for i, m in enumerate(meshes):
        m = m or {}
        e = arr[i]
        nv, nn = counts[i] if counts is not None and i < len(counts) else (0, 0)
        v, n = m.get("vertices"), m.get("normals")
        if v is not None:
            v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
            keep.append(v)
            e.vertices = v.ctypes.data_as(C.POINTER(C.c_float))
            nv = v.shape[0]
        if n is not None:
            n = np.ascontiguousarray(n, np.float32).reshape(-1, 3)
            keep.append(n)
            e.normals = n.ctypes.data_as(C.POINTER(C.c_float))
            nn = n.shape[0]
        e.n_vertices, e.n_normals = int(m.get("n_vertices", nv)), int(m.get("n_normals", nn))
    return arr, keep


class Context:
    """Thin object wrapper; device=-1 gives a host-only validation context (no render possible)."""

    def __init__(self, device=0):
        cfg = Config(device, 0)
        self._h = lib().pt_create(C.byref(cfg))
        if not self._h:
            raise PtError("pt_create failed: " + lib().pt_last_error(None).decode())
        self.device = device

    @classmethod
    def _view(cls, handle):
        """A Context over a handle somebody else owns (Group.ctx): close() forgets the handle, nothing is destroyed."""
        self = cls.__new__(cls)
        self._h = handle
        self._owned = False
        self.device = None
        return self

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_owned", True):
                lib().pt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            raise PtError("%s failed (%d): %s" % (what, rc, lib().pt_last_error(self._h).decode()))
        return rc

    def set_option(self, key, value):
        self._check(lib().pt_set_option(self._h, key.encode(), int(value)), "pt_set_option")

    def upload_scene(self, entities, materials, textures=None, mesh_textures=None, env=None):
        """entities: list of (mesh dict, material index); materials: (n,17) float32;
        textures: list of (H,W) uint32 arrays; mesh_textures: per-entity texture index (or None)."""
        args, keep = _marshal_scene(entities, materials, textures, mesh_textures, env)
        self._check(lib().pt_upload_scene(self._h, *args), "pt_upload_scene")
        self._counts = _mesh_counts(entities)
        del keep

    def update_vertices(self, meshes, counts=None):
        """pt_update_vertices (scene uploaded with option "dynamic" = 1): meshes as _marshal_update takes them, e.g. the mesh dicts of
        upload_scene with moved "vertices".  counts: only for a context that did not upload the scene itself."""
        arr, keep = _marshal_update(meshes, counts if counts is not None else getattr(self, "_counts", None))
        self._check(lib().pt_update_vertices(self._h, arr if len(meshes) else None, len(meshes)), "pt_update_vertices")
        del keep

    def update_info(self):
        """pt_debug_update_info: the last update_vertices of this context."""
        a = (C.c_double * 8)()
        self._check(lib().pt_debug_update_info(self._h, a), "pt_debug_update_info")
        return dict(device_ms=float(a[0]), h2d_bytes=int(a[1]), slivers=int(a[2]), pad=np.float32(a[3]), levels=int(a[4]))

    def set_materials(self, materials):
        mats = np.ascontiguousarray(np.asarray(materials, np.float32).reshape(-1, PT_MAT_FLOATS))
        self._check(lib().pt_set_materials(self._h, mats.ctypes.data_as(C.POINTER(C.c_float)), mats.shape[0]), "pt_set_materials")

    def set_environment(self, env):
        self._check(lib().pt_set_environment(self._h, C.byref(env)), "pt_set_environment")

    def set_pixel_shard(self, rank, world, tile=16):
        self._check(lib().pt_set_pixel_shard(self._h, rank, world, tile), "pt_set_pixel_shard")

    def render(self, cam, W, H, spp, max_depth, want_rgba8=False):
        rgb = np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        self._check(lib().pt_render(self._h, C.byref(cam), W, H, spp, max_depth, rgb.ctypes.data_as(C.POINTER(C.c_float)),
                                    rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None), "pt_render")
        return rgb, rgba

    def render_batch(self, frames, W, H, spp, max_depth, want_rgba8=False, n_materials=None, receive=True):
        """pt_render_batch: frames = list of (Camera, materials or None - the context's table).  Returns (K, H, W, 3) float32 and, with
        want_rgba8, (K, H, W) uint32: frame k is what set_materials(frames[k][1]) + render(frames[k][0]) returns.  n_materials: only
        needed when every frame passes None; receive = False: a non-root rank of a communicator (returns None, None)."""
        arr, n_mat, keep = _marshal_frames(frames)
        if n_materials is not None:
            n_mat = int(n_materials)
        K = len(frames)
        rgb = np.empty((K, H, W, 3), np.float32) if receive else None
        rgba = np.empty((K, H, W), np.uint32) if (want_rgba8 and receive) else None
        self._check(lib().pt_render_batch(self._h, arr if K else None, K, n_mat, W, H, spp, max_depth,
                                          rgb.ctypes.data_as(C.POINTER(C.c_float)) if rgb is not None else None,
                                          rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None), "pt_render_batch")
        del keep
        return rgb, rgba

    def render_batch_device(self, frames, W, H, spp, max_depth, d_out_rgb, d_out_rgba8=None, stream=None, n_materials=None):
        """pt_render_batch_device: asynchronous, the frames left in HBM at the device pointers (integers).  stream: a hipStream_t as an
        integer, None = the context's own stream; ordering and lifetime as render_device."""
        arr, n_mat, keep = _marshal_frames(frames)
        if n_materials is not None:
            n_mat = int(n_materials)
        self._check(lib().pt_render_batch_device(self._h, arr if frames else None, len(frames), n_mat, W, H, spp, max_depth, C.c_void_p(d_out_rgb),
                                                 C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None),
                    "pt_render_batch_device")
        del keep

    def render_into(self, cam, W, H, spp, max_depth, rgb, rgba8=None):
        """pt_render into caller-owned arrays (e.g. a PinnedFrame); rgb may be None on the non-root ranks of a communicator."""
        self._check(lib().pt_render(self._h, C.byref(cam), W, H, spp, max_depth, rgb.ctypes.data_as(C.POINTER(C.c_float)) if rgb is not None else None,
                                    rgba8.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba8 is not None else None), "pt_render")

    def render_aov(self, cam, W, H, n_samples, receive=True):
        """pt_render_aov: the guide buffers of the frame, (H, W, 8) float32 = albedo r g b, alpha, normal x y z, depth per pixel (first hit
        only; include/mi355pt.h "guide pass").  receive = False: a non-root rank of a communicator (returns None)."""
        out = np.empty((H, W, 8), np.float32) if receive else None
        self._check(lib().pt_render_aov(self._h, C.byref(cam), W, H, n_samples, out.ctypes.data_as(C.POINTER(C.c_float)) if receive else None), "pt_render_aov")
        return out

    def render_aov_device(self, cam, W, H, n_samples, d_out_aov, stream=None):
        """pt_render_aov_device: asynchronous, W*H*8 floats left in HBM at the device pointer d_out_aov; synchronize() waits for it.
        stream: a hipStream_t as an integer, None = the context's own stream; ordering and lifetime as render_device."""
        self._check(lib().pt_render_aov_device(self._h, C.byref(cam), W, H, n_samples, C.c_void_p(d_out_aov), C.c_void_p(stream) if stream else None),
                    "pt_render_aov_device")

    def aov_host(self, cam, W, H, n_samples, pixel_ids=None):
        """pt_debug_aov_host, the CPU twin of render_aov (works on a host-only context): (n, 8) float32 for the listed launch-index pixel ids
        x + W*y; pixel_ids None: every pixel, returned as (H, W, 8) in the framebuffer order of render_aov (row 0 = the top row, y = H-1)."""
        whole = pixel_ids is None
        ids = np.arange(W * H, dtype=np.uint32) if whole else np.ascontiguousarray(pixel_ids, np.uint32).reshape(-1)
        out = np.zeros((ids.size, 8), np.float32)
        n = lib().pt_debug_aov_host(self._h, C.byref(cam), W, H, n_samples, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, out.ctypes.data_as(C.POINTER(C.c_float)))
        if n < 0:
            self._check(int(n), "pt_debug_aov_host")
        return out.reshape(H, W, 8)[::-1].copy() if whole else out

    def render_aov_follow(self, cam, W, H, params=None, receive=True):
        """pt_render_aov_follow: the guide buffers (H, W, 8) with the guide ray following mirrors and glass (include/mi355pt.h "guide pass,
        follow mode"); params: AovParams (aov_default_params), None = the defaults.  receive = False: a non-root rank of a communicator."""
        out = np.empty((H, W, 8), np.float32) if receive else None
        self._check(lib().pt_render_aov_follow(self._h, C.byref(cam), W, H, C.byref(params) if params is not None else None,
                                               out.ctypes.data_as(C.POINTER(C.c_float)) if receive else None), "pt_render_aov_follow")
        return out

    def render_aov_follow_device(self, cam, W, H, d_out_aov, params=None, stream=None):
        """pt_render_aov_follow_device: asynchronous, W*H*8 floats left in HBM at d_out_aov; conventions of render_aov_device."""
        self._check(lib().pt_render_aov_follow_device(self._h, C.byref(cam), W, H, C.byref(params) if params is not None else None, C.c_void_p(d_out_aov),
                                                      C.c_void_p(stream) if stream else None), "pt_render_aov_follow_device")

    def render_aov_batch(self, frames, W, H, params=None, n_materials=None, receive=True):
        """pt_render_aov_batch: frames as render_batch.  Returns (K, H, W, 8) float32: frame k is what set_materials(frames[k][1]) +
        render_aov_follow(frames[k][0], params) returns.  n_materials: only needed when every frame passes None; receive = False: a
        non-root rank of a communicator (returns None)."""
        arr, n_mat, keep = _marshal_frames(frames)
        if n_materials is not None:
            n_mat = int(n_materials)
        K = len(frames)
        out = np.empty((K, H, W, 8), np.float32) if receive else None
        self._check(lib().pt_render_aov_batch(self._h, arr if K else None, K, n_mat, W, H, C.byref(params) if params is not None else None,
                                              out.ctypes.data_as(C.POINTER(C.c_float)) if receive else None), "pt_render_aov_batch")
        del keep
        return out

    def render_aov_batch_device(self, frames, W, H, d_out_aov, params=None, stream=None, n_materials=None):
        """pt_render_aov_batch_device: asynchronous, K * W*H*8 floats left in HBM at d_out_aov; conventions of render_batch_device."""
        arr, n_mat, keep = _marshal_frames(frames)
        if n_materials is not None:
            n_mat = int(n_materials)
        self._check(lib().pt_render_aov_batch_device(self._h, arr if frames else None, len(frames), n_mat, W, H, C.byref(params) if params is not None else None,
                                                     C.c_void_p(d_out_aov), C.c_void_p(stream) if stream else None), "pt_render_aov_batch_device")
        del keep

    def aov_follow_host(self, cam, W, H, params=None, pixel_ids=None):
        """pt_debug_aov_follow_host, the CPU twin of render_aov_follow (works on a host-only context); pixel_ids and result as aov_host."""
        whole = pixel_ids is None
        ids = np.arange(W * H, dtype=np.uint32) if whole else np.ascontiguousarray(pixel_ids, np.uint32).reshape(-1)
        out = np.zeros((ids.size, 8), np.float32)
        n = lib().pt_debug_aov_follow_host(self._h, C.byref(cam), W, H, C.byref(params) if params is not None else None, ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size,
                                           out.ctypes.data_as(C.POINTER(C.c_float)))
        if n < 0:
            self._check(int(n), "pt_debug_aov_follow_host")
        return out.reshape(H, W, 8)[::-1].copy() if whole else out

    def _denoise(self, fn, what, rgb, aov, params, want_rgba8, in_place):
        aov = np.ascontiguousarray(aov, np.float32)
        H, W = aov.shape[0], aov.shape[1]
        src = rgb if in_place else np.ascontiguousarray(rgb, np.float32)
        assert src.dtype == np.float32 and src.flags["C_CONTIGUOUS"] and src.shape == (H, W, 3) and aov.shape == (H, W, 8)
        out = src if in_place else np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        fp = C.POINTER(C.c_float)
        rc = fn(self._h, src.ctypes.data_as(fp), aov.ctypes.data_as(fp), W, H, C.byref(params) if params is not None else None, out.ctypes.data_as(fp),
                rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None)
        if rc < 0:
            self._check(int(rc), what)
        return out, rgba

    def denoise(self, rgb, aov, params=None, want_rgba8=False, in_place=False):
        """pt_denoise: rgb (H, W, 3) as render returns it and aov (H, W, 8) as render_aov returns it -> the filtered frame (and its RGBA8
        image).  params: a DenoiseParams (None: the defaults).  in_place: the result overwrites rgb (a contiguous float32 array)."""
        return self._denoise(lib().pt_denoise, "pt_denoise", rgb, aov, params, want_rgba8, in_place)

    def denoise_host(self, rgb, aov, params=None, want_rgba8=False, in_place=False):
        """pt_debug_denoise_host, the CPU twin of denoise (works on a host-only context)."""
        return self._denoise(lib().pt_debug_denoise_host, "pt_debug_denoise_host", rgb, aov, params, want_rgba8, in_place)

    def denoise_batch(self, rgb, aov, params=None, want_rgba8=False, in_place=False):
        """pt_denoise_batch: rgb (K, H, W, 3) as render_batch returns it and aov (K, H, W, 8) as render_aov_batch returns it -> the K filtered
        frames (and their RGBA8 images); frame k is what denoise(rgb[k], aov[k], params) returns.  in_place: the result overwrites rgb."""
        aov = np.ascontiguousarray(aov, np.float32)
        K, H, W = aov.shape[0], aov.shape[1], aov.shape[2]
        src = rgb if in_place else np.ascontiguousarray(rgb, np.float32)
        assert src.dtype == np.float32 and src.flags["C_CONTIGUOUS"] and src.shape == (K, H, W, 3) and aov.shape == (K, H, W, 8)
        out = src if in_place else np.empty((K, H, W, 3), np.float32)
        rgba = np.empty((K, H, W), np.uint32) if want_rgba8 else None
        fp = C.POINTER(C.c_float)
        self._check(lib().pt_denoise_batch(self._h, src.ctypes.data_as(fp), aov.ctypes.data_as(fp), K, W, H, C.byref(params) if params is not None else None,
                                           out.ctypes.data_as(fp), rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None), "pt_denoise_batch")
        return out, rgba

    def denoise_batch_device(self, d_rgb, d_aov, K, W, H, d_out_rgb, params=None, d_out_rgba8=None, stream=None):
        """pt_denoise_batch_device: asynchronous, device pointers to K frames back to back (d_out_rgb may equal d_rgb); conventions of
        denoise_device."""
        self._check(lib().pt_denoise_batch_device(self._h, C.c_void_p(d_rgb), C.c_void_p(d_aov), K, W, H, C.byref(params) if params is not None else None,
                                                  C.c_void_p(d_out_rgb), C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None),
                    "pt_denoise_batch_device")

    def denoise_device(self, d_rgb, d_aov, W, H, d_out_rgb, params=None, d_out_rgba8=None, stream=None):
        """pt_denoise_device: asynchronous, device pointers (integers; d_out_rgb may equal d_rgb); synchronize() waits for it.  stream: a
        hipStream_t as an integer, None = the context's own stream; ordering and lifetime as render_device."""
        self._check(lib().pt_denoise_device(self._h, C.c_void_p(d_rgb), C.c_void_p(d_aov), W, H, C.byref(params) if params is not None else None, C.c_void_p(d_out_rgb),
                                            C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None), "pt_denoise_device")

    # ---- upsampling (pt_upsample*) ----
    def _upsample(self, fn, what, rgb_lo, aov_lo, aov_hi, params, want_rgba8):
        aov_lo = np.ascontiguousarray(aov_lo, np.float32)
        aov_hi = np.ascontiguousarray(aov_hi, np.float32)
        rgb_lo = np.ascontiguousarray(rgb_lo, np.float32)
        h, w = aov_lo.shape[0], aov_lo.shape[1]
        H, W = aov_hi.shape[0], aov_hi.shape[1]
        assert rgb_lo.shape == (h, w, 3) and aov_lo.shape == (h, w, 8) and aov_hi.shape == (H, W, 8)
        out = np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        fp = C.POINTER(C.c_float)
        rc = fn(self._h, rgb_lo.ctypes.data_as(fp), aov_lo.ctypes.data_as(fp), w, h, aov_hi.ctypes.data_as(fp), W, H, C.byref(params) if params is not None else None,
                out.ctypes.data_as(fp), rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None)
        if rc < 0:
            self._check(int(rc), what)
        return out, rgba

    def upsample(self, rgb_lo, aov_lo, aov_hi, params=None, want_rgba8=False):
        """pt_upsample: rgb_lo (h, w, 3) and aov_lo (h, w, 8) as render / render_aov return them at the low size, aov_hi (H, W, 8) at the
        full size -> the (H, W, 3) frame (and its RGBA8 image).  params: an UpsampleParams (None: the defaults)."""
        return self._upsample(lib().pt_upsample, "pt_upsample", rgb_lo, aov_lo, aov_hi, params, want_rgba8)

    def upsample_host(self, rgb_lo, aov_lo, aov_hi, params=None, want_rgba8=False):
        """pt_debug_upsample_host, the CPU twin of upsample (works on a host-only context)."""
        return self._upsample(lib().pt_debug_upsample_host, "pt_debug_upsample_host", rgb_lo, aov_lo, aov_hi, params, want_rgba8)

    def upsample_device(self, d_rgb_lo, d_aov_lo, w, h, d_aov_hi, W, H, d_out_rgb, params=None, d_out_rgba8=None, stream=None):
        """pt_upsample_device: asynchronous, device pointers (integers; the outputs must not overlap the inputs); synchronize() waits for
        it.  stream: a hipStream_t as an integer, None = the context's own stream; ordering and lifetime as render_device."""
        self._check(lib().pt_upsample_device(self._h, C.c_void_p(d_rgb_lo), C.c_void_p(d_aov_lo), w, h, C.c_void_p(d_aov_hi), W, H,
                                             C.byref(params) if params is not None else None, C.c_void_p(d_out_rgb), C.c_void_p(d_out_rgba8) if d_out_rgba8 else None,
                                             C.c_void_p(stream) if stream else None), "pt_upsample_device")

    # ---- progressive accumulation (pt_accum_*) ----
    def accum_begin(self, cam, W, H, max_depth):
        """pt_accum_begin: a frame that grows by accum_add; fixes camera, size, depth and the pixel shard."""
        self._check(lib().pt_accum_begin(self._h, C.byref(cam), W, H, max_depth), "pt_accum_begin")
        self._accum_shape = (H, W)

    def accum_add(self, params=None, want_rgb=True, want_rgba8=False):
        """pt_accum_add: params an AccumParams (None: the defaults) -> (rgb (H, W, 3) or None, rgba8 (H, W) or None) of the frame so far."""
        H, W = self._accum_shape
        rgb = np.empty((H, W, 3), np.float32) if want_rgb else None
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        self._check(lib().pt_accum_add(self._h, C.byref(params) if params is not None else None, rgb.ctypes.data_as(C.POINTER(C.c_float)) if want_rgb else None,
                                       rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if want_rgba8 else None), "pt_accum_add")
        return rgb, rgba

    def accum_add_device(self, params=None, d_out_rgb=None, d_out_rgba8=None, stream=None):
        """pt_accum_add_device: asynchronous, the frame so far left in HBM at the device pointers (integers, each may be None); stream and
        ordering as render_device.  An add that selects its pixels waits on the host for the size of its active set."""
        self._check(lib().pt_accum_add_device(self._h, C.byref(params) if params is not None else None, C.c_void_p(d_out_rgb) if d_out_rgb else None,
                                              C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None), "pt_accum_add_device")

    def accum_read(self):
        """pt_accum_read -> dict(rgb (H, W, 3), rgba8, noise, samples (H, W each)) in framebuffer order."""
        H, W = self._accum_shape
        out = dict(rgb=np.empty((H, W, 3), np.float32), rgba8=np.empty((H, W), np.uint32), noise=np.empty((H, W), np.float32), samples=np.empty((H, W), np.uint32))
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._check(lib().pt_accum_read(self._h, out["rgb"].ctypes.data_as(fp), out["rgba8"].ctypes.data_as(up), out["noise"].ctypes.data_as(fp),
                                        out["samples"].ctypes.data_as(up)), "pt_accum_read")
        return out

    def accum_info(self):
        i = AccumInfo()
        self._check(lib().pt_accum_info_get(self._h, C.byref(i)), "pt_accum_info_get")
        return {k: getattr(i, k) for k, _ in AccumInfo._fields_}

    def accum_end(self):
        self._check(lib().pt_accum_end(self._h), "pt_accum_end")

    def accum_state(self):
        """pt_debug_accum_state -> dict(sum, half (H, W, 3), n, n_half, passes (H, W)): the raw state in framebuffer order."""
        H, W = self._accum_shape
        out = dict(sum=np.empty((H, W, 3), np.float32), half=np.empty((H, W, 3), np.float32), n=np.empty((H, W), np.uint32), n_half=np.empty((H, W), np.uint32),
                   passes=np.empty((H, W), np.uint32))
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self._check(lib().pt_debug_accum_state(self._h, out["sum"].ctypes.data_as(fp), out["half"].ctypes.data_as(fp), out["n"].ctypes.data_as(up),
                                               out["n_half"].ctypes.data_as(up), out["passes"].ctypes.data_as(up)), "pt_debug_accum_state")
        return out

    def accum_resolve_host(self, sum_, seen, half, n, n_half, passes, active, owned, n_samples):
        """pt_debug_accum_resolve_host on flat arrays (sum, seen, half: (N, 3) float32; n, n_half, passes: (N,) uint32; active, owned: (N,)
        uint8).  The inputs are not changed -> dict(seen, half, n, n_half, passes, rgb, rgba8, noise)."""
        fp, up, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        s = np.ascontiguousarray(sum_, np.float32)
        N = s.shape[0]
        o = dict(seen=np.array(seen, np.float32), half=np.array(half, np.float32), n=np.array(n, np.uint32), n_half=np.array(n_half, np.uint32),
                 passes=np.array(passes, np.uint32), rgb=np.empty((N, 3), np.float32), rgba8=np.empty(N, np.uint32), noise=np.empty(N, np.float32))
        a, w = np.ascontiguousarray(active, np.uint8), np.ascontiguousarray(owned, np.uint8)
        rc = lib().pt_debug_accum_resolve_host(self._h, N, s.ctypes.data_as(fp), o["seen"].ctypes.data_as(fp), o["half"].ctypes.data_as(fp), o["n"].ctypes.data_as(up),
                                               o["n_half"].ctypes.data_as(up), o["passes"].ctypes.data_as(up), a.ctypes.data_as(bp), w.ctypes.data_as(bp), int(n_samples),
                                               o["rgb"].ctypes.data_as(fp), o["rgba8"].ctypes.data_as(up), o["noise"].ctypes.data_as(fp))
        self._check(int(rc), "pt_debug_accum_resolve_host")
        return o

    def accum_select_host(self, noise, n, owned, params=None):
        """pt_debug_accum_select_host -> (active flags (N,) uint8, their count)."""
        fp, up, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        z, m, w = np.ascontiguousarray(noise, np.float32).ravel(), np.ascontiguousarray(n, np.uint32).ravel(), np.ascontiguousarray(owned, np.uint8).ravel()
        act = np.empty(z.size, np.uint8)
        rc = lib().pt_debug_accum_select_host(self._h, z.ctypes.data_as(fp), m.ctypes.data_as(up), w.ctypes.data_as(bp), z.size, C.byref(params) if params is not None else None,
                                              act.ctypes.data_as(bp))
        self._check(int(rc), "pt_debug_accum_select_host")
        return act, int(rc)

    # ---- variance-guided denoise (pt_denoise_var*, pt_accum_variance, pt_accum_denoise*) ----
    def _denoise_var(self, fn, what, rgb, var, aov, params, want_rgba8, in_place, want_var=None):
        aov = np.ascontiguousarray(aov, np.float32)
        var = np.ascontiguousarray(var, np.float32)
        H, W = aov.shape[0], aov.shape[1]
        src = rgb if in_place else np.ascontiguousarray(rgb, np.float32)
        assert src.dtype == np.float32 and src.flags["C_CONTIGUOUS"] and src.shape == (H, W, 3) and var.shape == (H, W, 3) and aov.shape == (H, W, 8)
        out = src if in_place else np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        fp = C.POINTER(C.c_float)
        args = [self._h, src.ctypes.data_as(fp), var.ctypes.data_as(fp), aov.ctypes.data_as(fp), W, H, C.byref(params) if params is not None else None, out.ctypes.data_as(fp),
                rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None]
        vout = None
        if want_var is not None:
            vout = np.empty((H, W), np.float32) if want_var else None
            args.append(vout.ctypes.data_as(fp) if vout is not None else None)
        rc = fn(*args)
        if rc < 0:
            self._check(int(rc), what)
        return (out, rgba) if want_var is None else (out, rgba, vout)

    def denoise_var(self, rgb, var, aov, params=None, want_rgba8=False, in_place=False):
        """pt_denoise_var: rgb and its per-channel variance map var (H, W, 3 each), aov (H, W, 8) -> the filtered frame (and its RGBA8 image).
        params: a DenoiseParams whose sigma_color counts standard deviations (None: denoise_var_default_params)."""
        return self._denoise_var(lib().pt_denoise_var, "pt_denoise_var", rgb, var, aov, params, want_rgba8, in_place)

    def denoise_var_host(self, rgb, var, aov, params=None, want_rgba8=False, in_place=False, want_var=False):
        """pt_debug_denoise_var_host, the CPU twin of denoise_var (works on a host-only context) -> (out, rgba8 or None, v_L (H, W) or None)."""
        return self._denoise_var(lib().pt_debug_denoise_var_host, "pt_debug_denoise_var_host", rgb, var, aov, params, want_rgba8, in_place, want_var=bool(want_var))

    def denoise_var_device(self, d_rgb, d_var, d_aov, W, H, d_out_rgb, params=None, d_out_rgba8=None, stream=None):
        """pt_denoise_var_device: asynchronous, device pointers (integers; d_out_rgb may equal d_rgb); conventions of denoise_device."""
        self._check(lib().pt_denoise_var_device(self._h, C.c_void_p(d_rgb), C.c_void_p(d_var), C.c_void_p(d_aov), W, H, C.byref(params) if params is not None else None,
                                                C.c_void_p(d_out_rgb), C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None),
                    "pt_denoise_var_device")

    def accum_variance(self):
        """pt_accum_variance -> (H, W, 3) float32: the per-channel variance of the accumulation's pixel values, framebuffer order."""
        H, W = self._accum_shape
        out = np.empty((H, W, 3), np.float32)
        self._check(lib().pt_accum_variance(self._h, out.ctypes.data_as(C.POINTER(C.c_float))), "pt_accum_variance")
        return out

    def accum_variance_host(self, sum_, half, n, n_half, owned):
        """pt_debug_accum_variance_host on flat arrays (sum, half: (N, 3) float32; n, n_half: (N,) uint32; owned: (N,) uint8) -> (rgb, var), (N, 3) each."""
        fp, up, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        s, h = np.ascontiguousarray(sum_, np.float32).reshape(-1, 3), np.ascontiguousarray(half, np.float32).reshape(-1, 3)
        m, mh, w = np.ascontiguousarray(n, np.uint32).ravel(), np.ascontiguousarray(n_half, np.uint32).ravel(), np.ascontiguousarray(owned, np.uint8).ravel()
        N = s.shape[0]
        assert h.shape[0] == N and m.size == N and mh.size == N and w.size == N
        rgb, var = np.empty((N, 3), np.float32), np.empty((N, 3), np.float32)
        rc = lib().pt_debug_accum_variance_host(self._h, N, s.ctypes.data_as(fp), h.ctypes.data_as(fp), m.ctypes.data_as(up), mh.ctypes.data_as(up), w.ctypes.data_as(bp),
                                                rgb.ctypes.data_as(fp), var.ctypes.data_as(fp))
        self._check(int(rc), "pt_debug_accum_variance_host")
        return rgb, var

    def accum_denoise(self, aov, params=None, want_rgba8=False):
        """pt_accum_denoise: the variance-guided filter on the accumulation as it stands, aov (H, W, 8) -> (rgb (H, W, 3), rgba8 or None).  It
        changes nothing of the accumulation."""
        H, W = self._accum_shape
        aov = np.ascontiguousarray(aov, np.float32)
        assert aov.shape == (H, W, 8)
        out = np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        fp = C.POINTER(C.c_float)
        self._check(lib().pt_accum_denoise(self._h, aov.ctypes.data_as(fp), C.byref(params) if params is not None else None, out.ctypes.data_as(fp),
                                           rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None), "pt_accum_denoise")
        return out, rgba

    def accum_denoise_device(self, d_aov, d_out_rgb, params=None, d_out_rgba8=None, stream=None):
        """pt_accum_denoise_device: asynchronous, device pointers (integers); stream and ordering as accum_add_device."""
        self._check(lib().pt_accum_denoise_device(self._h, C.c_void_p(d_aov), C.byref(params) if params is not None else None, C.c_void_p(d_out_rgb),
                                                  C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None), "pt_accum_denoise_device")

    # ---- reprojection (pt_accum_reproject*) ----
    def accum_reproject(self, new_cam, aov_prev, aov_cur, params=None):
        """pt_accum_reproject: the accumulation follows the surfaces to new_cam.  aov_prev / aov_cur: the guides (H, W, 8) under the
        accumulation's camera and under new_cam (may be the same array); params a ReprojectParams (None: the defaults)."""
        H, W = self._accum_shape
        prev = np.ascontiguousarray(aov_prev, np.float32)
        cur = prev if aov_cur is aov_prev else np.ascontiguousarray(aov_cur, np.float32)
        assert prev.shape == (H, W, 8) and cur.shape == (H, W, 8)
        fp = C.POINTER(C.c_float)
        self._check(lib().pt_accum_reproject(self._h, C.byref(new_cam), prev.ctypes.data_as(fp), cur.ctypes.data_as(fp), C.byref(params) if params is not None else None),
                    "pt_accum_reproject")

    def accum_reproject_device(self, new_cam, d_aov_prev, d_aov_cur, params=None, stream=None):
        """pt_accum_reproject_device: asynchronous, device pointers (integers, 16-byte aligned); stream and ordering as accum_add_device."""
        self._check(lib().pt_accum_reproject_device(self._h, C.byref(new_cam), C.c_void_p(d_aov_prev), C.c_void_p(d_aov_cur), C.byref(params) if params is not None else None,
                                                    C.c_void_p(stream) if stream else None), "pt_accum_reproject_device")

    def accum_reproject_host(self, old_cam, new_cam, aov_prev, aov_cur, state, owned=None, params=None):
        """pt_debug_accum_reproject_host, the CPU twin (works on a host-only context).  state: dict(sum, half (H, W, 3), n, n_half, passes
        (H, W)) in framebuffer order as accum_state gives it; owned (H, W) flags or None.  The inputs are not changed -> dict(sum, half, n,
        n_half, passes, rgb, rgba8, noise)."""
        prev, cur = np.ascontiguousarray(aov_prev, np.float32), np.ascontiguousarray(aov_cur, np.float32)
        H, W = prev.shape[0], prev.shape[1]
        assert prev.shape == (H, W, 8) and cur.shape == (H, W, 8)
        o = dict(sum=np.array(state["sum"], np.float32), half=np.array(state["half"], np.float32), n=np.array(state["n"], np.uint32),
                 n_half=np.array(state["n_half"], np.uint32), passes=np.array(state["passes"], np.uint32), rgb=np.empty((H, W, 3), np.float32),
                 rgba8=np.empty((H, W), np.uint32), noise=np.empty((H, W), np.float32))
        assert o["sum"].shape == (H, W, 3) and o["half"].shape == (H, W, 3) and all(o[k].shape == (H, W) for k in ("n", "n_half", "passes"))
        own = None if owned is None else np.ascontiguousarray(owned, np.uint8)
        assert own is None or own.shape == (H, W)
        fp, up, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        rc = lib().pt_debug_accum_reproject_host(self._h, C.byref(old_cam), C.byref(new_cam), W, H, prev.ctypes.data_as(fp), cur.ctypes.data_as(fp),
                                                 own.ctypes.data_as(bp) if own is not None else None, C.byref(params) if params is not None else None,
                                                 o["sum"].ctypes.data_as(fp), o["half"].ctypes.data_as(fp), o["n"].ctypes.data_as(up), o["n_half"].ctypes.data_as(up),
                                                 o["passes"].ctypes.data_as(up), o["rgb"].ctypes.data_as(fp), o["rgba8"].ctypes.data_as(up), o["noise"].ctypes.data_as(fp))
        self._check(int(rc), "pt_debug_accum_reproject_host")
        return o

    def _trace(self, fn, what, rays, occluded, extra=(), dtype=None):
        r = _rays(rays)
        out = np.empty(r.shape[0], dtype if dtype is not None else np.uint8 if occluded else HIT_DTYPE)
        rc = fn(self._h, r.ctypes.data_as(C.c_void_p), r.shape[0], *extra, out.ctypes.data_as(C.c_void_p))
        self._check(int(rc), what)
        return out

    def trace_closest(self, rays):
        """pt_trace_closest: the closest hit of every ray (RAY_DTYPE records, or (n, 6) origins and directions with tmax = +inf) as a
        HIT_DTYPE array {t, u, v, prim}; a miss is {0, 0, 0, -1} (include/mi355pt.h "ray queries")."""
        return self._trace(lib().pt_trace_closest, "pt_trace_closest", rays, False)

    def trace_occluded(self, rays):
        """pt_trace_occluded: one byte per ray, 1 = some triangle is hit within the ray's bound."""
        return self._trace(lib().pt_trace_occluded, "pt_trace_occluded", rays, True)

    def trace_rays_host(self, rays, occluded=False):
        """pt_debug_trace_rays_host, the CPU twin of trace_closest / trace_occluded (works on a host-only context)."""
        return self._trace(lib().pt_debug_trace_rays_host, "pt_debug_trace_rays_host", rays, occluded, (int(bool(occluded)),))

    def trace_closest_device(self, d_rays, n, d_out, stream=None):
        """pt_trace_closest_device: asynchronous, n pt_ray records at the device pointer d_rays (16-byte aligned), n pt_ray_hit left at
        d_out; synchronize() waits for it.  stream: a hipStream_t as an integer, None = the context's own; ordering as render_device."""
        self._check(lib().pt_trace_closest_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_out), C.c_void_p(stream) if stream else None), "pt_trace_closest_device")

    def trace_occluded_device(self, d_rays, n, d_out, stream=None):
        """pt_trace_occluded_device: the same for the occlusion flags, n bytes left at d_out."""
        self._check(lib().pt_trace_occluded_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_out), C.c_void_p(stream) if stream else None), "pt_trace_occluded_device")

    def trace_surface(self, rays):
        """pt_trace_surface: trace_closest with the surface at the hit, as a SURFACE_DTYPE array (80 bytes per ray: the hit record, hit
        point, material index, geometric and shading normal, texcoord, base colour, emission; include/mi355pt.h)."""
        return self._trace(lib().pt_trace_surface, "pt_trace_surface", rays, False, dtype=SURFACE_DTYPE)

    def trace_surface_host(self, rays):
        """pt_debug_trace_surface_host, the CPU twin of trace_surface (works on a host-only context)."""
        return self._trace(lib().pt_debug_trace_surface_host, "pt_debug_trace_surface_host", rays, False, dtype=SURFACE_DTYPE)

    def trace_surface_device(self, d_rays, n, d_out, stream=None):
        """pt_trace_surface_device: asynchronous as trace_closest_device, n pt_surface records (80 bytes each) left at d_out (16-byte aligned)."""
        self._check(lib().pt_trace_surface_device(self._h, C.c_void_p(d_rays), int(n), C.c_void_p(d_out), C.c_void_p(stream) if stream else None), "pt_trace_surface_device")

    def trace_ao(self, rays, params=None):
        """pt_trace_ao: trace_closest with the ambient occlusion at the hit, as an AO_DTYPE array (32 bytes per ray: the hit record, the
        facing normal, the fraction of the K occlusion rays that were not occluded).  params: an AoParams, None = the defaults."""
        return self._trace(lib().pt_trace_ao, "pt_trace_ao", rays, False, (C.byref(params) if params is not None else None,), dtype=AO_DTYPE)

    def trace_ao_host(self, rays, params=None, return_rays=False):
        """pt_debug_trace_ao_host, the CPU twin of trace_ao (works on a host-only context).  return_rays: also the occlusion rays, an
        (n, K) RAY_DTYPE array as trace_occluded takes them (a ray that traced none: K records that nothing occludes)."""
        r = _rays(rays)
        out = np.empty(r.shape[0], AO_DTYPE)
        ao_rays = None
        if return_rays:
            dflt = ao_default_params()
            ao_rays = np.empty((r.shape[0], int(params.n_rays if params is not None else dflt.n_rays)), RAY_DTYPE)
        rc = lib().pt_debug_trace_ao_host(self._h, r.ctypes.data_as(C.c_void_p), r.shape[0], C.byref(params) if params is not None else None,
                                          out.ctypes.data_as(C.c_void_p), ao_rays.ctypes.data_as(C.c_void_p) if ao_rays is not None and ao_rays.size else None)
        self._check(int(rc), "pt_debug_trace_ao_host")
        return (out, ao_rays) if return_rays else out

    def trace_ao_device(self, d_rays, n, d_out, params=None, stream=None):
        """pt_trace_ao_device: asynchronous as trace_closest_device, n pt_ao_hit records (32 bytes each) left at d_out (16-byte aligned)."""
        self._check(lib().pt_trace_ao_device(self._h, C.c_void_p(d_rays), int(n), C.byref(params) if params is not None else None, C.c_void_p(d_out),
                                             C.c_void_p(stream) if stream else None), "pt_trace_ao_device")

    def _trace_hits(self, fn, what, rays, k):
        r = _rays(rays)
        p = hits_params(k)
        out = np.empty((r.shape[0], min(max(int(p.max_hits), 0), PT_HITS_MAX)), HIT_DTYPE)  # (a K the call refuses: no room is needed)
        rc = fn(self._h, r.ctypes.data_as(C.c_void_p), r.shape[0], C.byref(p), out.ctypes.data_as(C.c_void_p))
        self._check(int(rc), what)
        return out

    def trace_hits(self, rays, k=None):
        """pt_trace_hits: the first K triangles along every ray in (t, id) order as an (n, K) HIT_DTYPE array; entries behind the last
        hit are misses {0, 0, 0, -1}.  k: the K (1..PT_HITS_MAX), None = the default 4, or a HitsParams (include/mi355pt.h "the first K hits")."""
        return self._trace_hits(lib().pt_trace_hits, "pt_trace_hits", rays, k)

    def trace_hits_host(self, rays, k=None):
        """pt_debug_trace_hits_host, the CPU twin of trace_hits (works on a host-only context)."""
        return self._trace_hits(lib().pt_debug_trace_hits_host, "pt_debug_trace_hits_host", rays, k)

    def trace_hits_device(self, d_rays, n, d_out, k=None, stream=None):
        """pt_trace_hits_device: asynchronous as trace_closest_device, n * K pt_ray_hit records left at d_out (16-byte aligned)."""
        self._check(lib().pt_trace_hits_device(self._h, C.c_void_p(d_rays), int(n), C.byref(hits_params(k)), C.c_void_p(d_out),
                                               C.c_void_p(stream) if stream else None), "pt_trace_hits_device")

    def _points(self, fn, what, points):
        p = _points(points)
        out = np.empty(p.shape[0], POINT_HIT_DTYPE)
        rc = fn(self._h, p.ctypes.data_as(C.c_void_p), p.shape[0], out.ctypes.data_as(C.c_void_p))
        self._check(int(rc), what)
        return out

    def closest_point(self, points):
        """pt_closest_point: the nearest triangle to every point (POINT_DTYPE records, or (n, 3) positions with radius = +inf) as a
        POINT_HIT_DTYPE array {dist, u, v, prim, q, feature}; nothing within the radius is prim = -1 and zeros (include/mi355pt.h
        "point queries")."""
        return self._points(lib().pt_closest_point, "pt_closest_point", points)

    def closest_point_host(self, points):
        """pt_debug_closest_point_host, the CPU twin of closest_point: brute force over every triangle (works on a host-only context)."""
        return self._points(lib().pt_debug_closest_point_host, "pt_debug_closest_point_host", points)

    def closest_point_device(self, d_pts, n, d_out, stream=None):
        """pt_closest_point_device: asynchronous as trace_closest_device, n pt_point records (16 bytes each) at d_pts, n pt_point_hit
        records (32 bytes each) left at d_out, both 16-byte aligned."""
        self._check(lib().pt_closest_point_device(self._h, C.c_void_p(d_pts), int(n), C.c_void_p(d_out), C.c_void_p(stream) if stream else None), "pt_closest_point_device")

    def prim_to_mesh(self, prim):
        """pt_prim_to_mesh: (entity of the upload, triangle inside it) of a global triangle id."""
        m, t = C.c_int32(-1), C.c_int32(-1)
        self._check(lib().pt_prim_to_mesh(self._h, int(prim), C.byref(m), C.byref(t)), "pt_prim_to_mesh")
        return int(m.value), int(t.value)

    def comm_init_rank(self, unique_id, rank, world):
        buf = (C.c_uint8 * PT_COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(lib().pt_comm_init_rank(self._h, buf, rank, world), "pt_comm_init_rank")

    def comm_destroy(self):
        self._check(lib().pt_comm_destroy(self._h), "pt_comm_destroy")

    def reduce_framebuffer(self, d_rgb, d_rgba8, n_pixels, stream=None):
        """pt_reduce_framebuffer; stream as render_device."""
        self._check(lib().pt_reduce_framebuffer(self._h, C.c_void_p(d_rgb), C.c_void_p(d_rgba8) if d_rgba8 else None, n_pixels,
                                                C.c_void_p(stream) if stream else None), "pt_reduce_framebuffer")

    def render_device(self, cam, W, H, spp, max_depth, d_out_rgb, d_out_rgba8=None, stream=None):
        """pt_render_device: asynchronous, the frame left in HBM at the device pointers (integers).  stream: a hipStream_t as an integer
        (the value of the handle, e.g. ctypes.c_void_p.value or torch.cuda.Stream.cuda_stream), None = the context's own stream.  The
        library orders the call after the context's last asynchronous one, whichever stream that used (include/mi355pt.h); the stream
        must live until a synchronize() after the last call on it has returned."""
        self._check(lib().pt_render_device(self._h, C.byref(cam), W, H, spp, max_depth, C.c_void_p(d_out_rgb),
                                           C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None),
                    "pt_render_device")

    def render_rays(self, rays, W, H, spp, max_depth, want_rgba8=False):
        """pt_render_rays: path-traced radiance along a ray image - W * H RAY_GEN_DTYPE records, the record of pixel (x, y) at x + W * y
        (pyhost/ray_image.py builds them).  Returns what render() returns: (H, W, 3) float32 in framebuffer order (row H - 1 - y) and,
        with want_rgba8, (H, W) uint32."""
        r = np.ascontiguousarray(rays, RAY_GEN_DTYPE).reshape(-1)
        if r.shape[0] != W * H:
            raise PtError("render_rays: %d records for a %dx%d ray image" % (r.shape[0], W, H))
        rgb = np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        self._check(lib().pt_render_rays(self._h, r.ctypes.data_as(C.c_void_p), W, H, spp, max_depth, rgb.ctypes.data_as(C.POINTER(C.c_float)),
                                         rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None), "pt_render_rays")
        return rgb, rgba

    def render_rays_device(self, d_rays, W, H, spp, max_depth, d_out_rgb, d_out_rgba8=None, stream=None):
        """pt_render_rays_device: asynchronous, W * H pt_ray_gen records at the device pointer d_rays (16-byte aligned; the caller's, valid and
        unchanged until the work has completed), the frame left in HBM as render_device leaves it.  stream and ordering as render_device."""
        self._check(lib().pt_render_rays_device(self._h, C.c_void_p(d_rays), W, H, spp, max_depth, C.c_void_p(d_out_rgb),
                                                C.c_void_p(d_out_rgba8) if d_out_rgba8 else None, C.c_void_p(stream) if stream else None),
                    "pt_render_rays_device")

    def render_aov_rays(self, rays, W, H, params=None):
        """pt_render_aov_rays: the guide buffers (H, W, 8) of render_aov_follow over a ray image - the table of render_rays (pyhost/ray_image.py
        builds them), so that a frame of render_rays can be denoised or upsampled; params: AovParams, None = the defaults (max_follow = 0
        gives first-hit guides).  Framebuffer order (row H - 1 - y), as render_aov_follow."""
        r = np.ascontiguousarray(rays, RAY_GEN_DTYPE).reshape(-1)
        if r.shape[0] != W * H:
            raise PtError("render_aov_rays: %d records for a %dx%d ray image" % (r.shape[0], W, H))
        out = np.empty((H, W, 8), np.float32)
        self._check(lib().pt_render_aov_rays(self._h, r.ctypes.data_as(C.c_void_p), W, H, C.byref(params) if params is not None else None,
                                             out.ctypes.data_as(C.POINTER(C.c_float))), "pt_render_aov_rays")
        return out

    def render_aov_rays_device(self, d_rays, W, H, d_out_aov, params=None, stream=None):
        """pt_render_aov_rays_device: asynchronous, W * H pt_ray_gen records at the device pointer d_rays (16-byte aligned; the caller's, valid
        and unchanged until the work has completed), W*H*8 floats left in HBM at d_out_aov (16-byte aligned); conventions of render_aov_device."""
        self._check(lib().pt_render_aov_rays_device(self._h, C.c_void_p(d_rays), W, H, C.byref(params) if params is not None else None, C.c_void_p(d_out_aov),
                                                    C.c_void_p(stream) if stream else None), "pt_render_aov_rays_device")

    def aov_rays_host(self, rays, W, H, params=None, pixel_ids=None):
        """pt_debug_aov_rays_host, the CPU twin of render_aov_rays (works on a host-only context); pixel_ids and result as aov_host."""
        r = np.ascontiguousarray(rays, RAY_GEN_DTYPE).reshape(-1)
        if r.shape[0] != W * H:
            raise PtError("aov_rays_host: %d records for a %dx%d ray image" % (r.shape[0], W, H))
        whole = pixel_ids is None
        ids = np.arange(W * H, dtype=np.uint32) if whole else np.ascontiguousarray(pixel_ids, np.uint32).reshape(-1)
        out = np.zeros((ids.size, 8), np.float32)
        n = lib().pt_debug_aov_rays_host(self._h, r.ctypes.data_as(C.c_void_p), W, H, C.byref(params) if params is not None else None,
                                         ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, out.ctypes.data_as(C.POINTER(C.c_float)))
        if n < 0:
            self._check(int(n), "pt_debug_aov_rays_host")
        return out.reshape(H, W, 8)[::-1].copy() if whole else out

    def synchronize(self):
        self._check(lib().pt_synchronize(self._h), "pt_synchronize")

    def stats(self):
        s = Stats()
        self._check(lib().pt_get_stats(self._h, C.byref(s)), "pt_get_stats")
        return s.as_dict()

    def closest_hit_host(self, org, direction, tmin=1e-3, tmax=1e10):
        t, u, v, p = C.c_float(), C.c_float(), C.c_float(), C.c_int32()
        rc = self._check(lib().pt_debug_closest_hit_host(self._h, _vec3(org), _vec3(direction), tmin, tmax, C.byref(t), C.byref(u), C.byref(v),
                                                         C.byref(p)), "pt_debug_closest_hit_host")
        return bool(rc), float(t.value), float(u.value), float(v.value), int(p.value)

    def closest_hit_host_n(self, rays, tmin=1e-3, tmax=1e10):
        """closest_hit_host for n rays (n x 6: origin, direction): (hit bool, t, u, v float32, id int32; -1 on a miss)."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((r.shape[0], 5), np.float32)
        n = lib().pt_debug_closest_hit_host_n(self._h, r.ctypes.data_as(C.POINTER(C.c_float)), r.shape[0], tmin, tmax, out.ctypes.data_as(C.POINTER(C.c_float)))
        if n < 0:
            self._check(int(n), "pt_debug_closest_hit_host_n")
        return out[:, 0] != 0, out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy(), out[:, 4].copy().view(np.int32)

    def _export(self, which, dtype):
        n = lib().pt_debug_export_tree(self._h, which, None, 0)
        if n < 0:
            self._check(int(n), "pt_debug_export_tree")
        a = np.zeros(int(n) // dtype.itemsize, dtype)
        if n:
            self._check(int(lib().pt_debug_export_tree(self._h, which, a.ctypes.data_as(C.c_void_p), a.nbytes)), "pt_debug_export_tree")
        return a

    def export_trees(self, device=False):
        """The hierarchy the context holds (pt_debug_export_tree): structured arrays `nodes`, `nodes4`, `nodes8`, `tris` (csrc/pt_types.h)
        and root, root4, root8, depth, depth4, depth8, pad (float32), max_leaf.  device = True: the four arrays as HBM holds them
        (PT_TREE_DEVICE), not the host copies."""
        info = self._export(4, np.dtype("<i8"))
        d = dict(zip(("root", "root4", "root8", "depth", "depth4", "depth8"), (int(x) for x in info[:6])))
        d["pad"] = np.array([int(info[6]) & 0xffffffff], np.uint32).view(np.float32)[0]
        d["max_leaf"] = int(info[7])
        d["nodes"], d["nodes4"], d["nodes8"], d["tris"] = (self._export(k | (PT_TREE_DEVICE if device else 0), t) for k, t in enumerate((NODE_DTYPE, NODE4_DTYPE, NODE8_DTYPE, TRI_DTYPE)))
        return d

    def clone_scene_from(self, other):
        self._check(lib().pt_debug_clone_scene(self._h, other._h), "pt_debug_clone_scene")

    def quad_info(self):
        a = (C.c_int64 * 8)()
        self._check(lib().pt_debug_quad_info(self._h, a), "pt_debug_quad_info")
        return dict(zip(("quad_nodes", "depth", "leaf_slots", "triangles", "empty_slots", "internal_slots", "binary_nodes", "binary_leaf_refs"), [int(x) for x in a]))

    def oct_info(self):
        a = (C.c_int64 * 8)()
        self._check(lib().pt_debug_oct_info(self._h, a), "pt_debug_oct_info")
        return dict(zip(("oct_nodes", "depth", "leaf_slots", "triangles", "empty_slots", "internal_slots", "largest_leaf", "triangle_slots"), [int(x) for x in a]))

    def read_queue(self, cap):
        """(queue_ids, input_ids, cost) of the last cost-ordered render (empty arrays if it did not sort)."""
        q = np.zeros(cap, np.uint32); i = np.zeros(cap, np.uint32); c = np.zeros(cap, np.uint8)
        n = lib().pt_debug_read_queue(self._h, q.ctypes.data_as(C.POINTER(C.c_uint32)), i.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      c.ctypes.data_as(C.POINTER(C.c_uint8)), cap)
        if n < 0:
            self._check(int(n), "pt_debug_read_queue")
        return q[:n], i[:n], c[:n]

    def set_cost_image(self, img):
        """pt_debug_set_cost_image: img (H, W) uint8 replaces the measured costs of every cost-ordered launch sequence whose launch image
        is W x H (a batch: W x K*H) from here on; None: back to the measured costs."""
        if img is None:
            self._check(lib().pt_debug_set_cost_image(self._h, None, 0, 0), "pt_debug_set_cost_image")
            return
        a = np.ascontiguousarray(img, np.uint8)
        assert a.ndim == 2
        self._check(lib().pt_debug_set_cost_image(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.shape[1], a.shape[0]), "pt_debug_set_cost_image")

    def read_finish(self, n_pixels):
        """Per pixel (x + W * y): (ms from the entry of the main launch to the pixel's last sample, rays traced - with count = 1); option latency = 1."""
        t = np.zeros(2 * n_pixels, np.uint32)
        n = lib().pt_debug_read_finish(self._h, t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size)
        if n < 0:
            self._check(int(n), "pt_debug_read_finish")
        if n < 2 * n_pixels:
            return t[:0].astype(np.float64), t[:0]
        return t[:n_pixels].astype(np.float64) / 1e5, t[n_pixels:]

    def read_tiers(self):
        """Tiers of the last whole-pixel launch: list of dicts (first queue entry, pixels, pixels per wave, first workgroup, workgroups, cost class)."""
        t = np.zeros(257, np.uint32)
        n = lib().pt_debug_read_tiers(self._h, t.ctypes.data_as(C.POINTER(C.c_uint32)), t.size)
        if n < 0:
            self._check(int(n), "pt_debug_read_tiers")
        if n == 0:
            return []
        return [dict(zip(("q0", "pixels", "per_wave", "wave0", "waves", "cost_class"), (int(x) for x in t[1 + 8 * i:7 + 8 * i]))) for i in range(int(t[0]))]

    def read_laps(self):
        """ms since kernel entry at which the last pixel finished chunk 0, 1, ... of the last wavefront launch."""
        t = np.zeros(3 * 257 + 128, np.uint64)
        n = lib().pt_debug_read_laps(self._h, t.ctypes.data_as(C.POINTER(C.c_uint64)), t.size)
        if n < 0:
            self._check(int(n), "pt_debug_read_laps")
        m = (int(n) - 64) // 3
        ms = lambda x: round((int(x) - int(t[0])) / 1e5, 2)
        return {"last_done_ms": [ms(x) for x in t[1:m]], "last_start_ms": [ms(x) for x in t[m + 1:2 * m]], "last_entry": [int(x) for x in t[2 * m + 1:3 * m]],
                "first_chunk_ticks_by_cost_class": [int(x) for x in t[3 * m:3 * m + 32]], "first_chunk_count_by_cost_class": [int(x) for x in t[3 * m + 32:3 * m + 64]]}

    def debug_eval(self, op, inputs, out_stride):
        x = np.ascontiguousarray(inputs, np.float32)
        if x.ndim == 1:
            x = x[:, None]
        out = np.empty((x.shape[0], out_stride), np.float32)
        self._check(lib().pt_debug_eval(self._h, OPS[op] if isinstance(op, str) else op, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[1],
                                        out.ctypes.data_as(C.POINTER(C.c_float)), out_stride, x.shape[0]), "pt_debug_eval")
        return out


class Group:
    """One process, N contexts behind one communicator (pt_group_* in include/mi355pt.h): pixel tiles over `devices`, one reduce onto
    devices[0].  The real RCCL refuses a device that appears twice; the stub collective of tests/stub/fake_rccl.cpp accepts it."""

    def __init__(self, devices):
        devices = [int(d) for d in devices]
        arr = (C.c_int32 * max(1, len(devices)))(*devices)
        self._g = lib().pt_group_create(arr, len(devices))
        if not self._g:
            raise PtError("pt_group_create failed: " + lib().pt_last_error(None).decode())
        self.devices = devices

    def close(self):
        if getattr(self, "_g", None):
            lib().pt_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        return lib().pt_group_last_error(self._g).decode()

    def _check(self, rc, what):
        if rc < 0:
            raise PtError("%s failed (%d): %s" % (what, rc, self.last_error()))
        return rc

    @property
    def size(self):
        return int(lib().pt_group_size(self._g))

    def ctx(self, i):
        """Rank i's context as a non-owning Context (stats, quad_info, oct_info, ...); valid until the group is closed."""
        h = lib().pt_group_ctx(self._g, int(i))
        if not h:
            raise PtError("pt_group_ctx: no rank %d in a group of %d" % (i, self.size))
        return Context._view(h)

    def upload_scene(self, entities, materials, textures=None, mesh_textures=None, env=None):
        """Arguments as Context.upload_scene: the tree is built once, on rank 0's context, and cloned to the others."""
        args, keep = _marshal_scene(entities, materials, textures, mesh_textures, env)
        self._check(lib().pt_group_upload_scene(self._g, *args), "pt_group_upload_scene")
        self._counts = _mesh_counts(entities)
        del keep

    def update_vertices(self, meshes, counts=None):
        """pt_group_update_vertices: arguments as Context.update_vertices; every device refits its own replica."""
        arr, keep = _marshal_update(meshes, counts if counts is not None else getattr(self, "_counts", None))
        self._check(lib().pt_group_update_vertices(self._g, arr if len(meshes) else None, len(meshes)), "pt_group_update_vertices")
        del keep

    def set_materials(self, materials):
        mats = np.ascontiguousarray(np.asarray(materials, np.float32).reshape(-1, PT_MAT_FLOATS))
        self._check(lib().pt_group_set_materials(self._g, mats.ctypes.data_as(C.POINTER(C.c_float)), mats.shape[0]), "pt_group_set_materials")

    def set_option(self, key, value):
        self._check(lib().pt_group_set_option(self._g, key.encode(), int(value)), "pt_group_set_option")

    def render(self, cam, W, H, spp, max_depth, want_rgba8=False):
        rgb = np.empty((H, W, 3), np.float32)
        rgba = np.empty((H, W), np.uint32) if want_rgba8 else None
        self._check(lib().pt_group_render(self._g, C.byref(cam), W, H, spp, max_depth, rgb.ctypes.data_as(C.POINTER(C.c_float)),
                                          rgba.ctypes.data_as(C.POINTER(C.c_uint32)) if rgba is not None else None), "pt_group_render")
        return rgb, rgba

    def render_aov(self, cam, W, H, n_samples):
        """pt_group_render_aov: the guide buffers (H, W, 8) of the frame, every device's own tiles reduced onto devices[0]."""
        out = np.empty((H, W, 8), np.float32)
        self._check(lib().pt_group_render_aov(self._g, C.byref(cam), W, H, n_samples, out.ctypes.data_as(C.POINTER(C.c_float))), "pt_group_render_aov")
        return out

    def render_aov_follow(self, cam, W, H, params=None):
        """pt_group_render_aov_follow: the follow-mode guide buffers (H, W, 8), reduced onto devices[0]."""
        out = np.empty((H, W, 8), np.float32)
        self._check(lib().pt_group_render_aov_follow(self._g, C.byref(cam), W, H, C.byref(params) if params is not None else None, out.ctypes.data_as(C.POINTER(C.c_float))),
                    "pt_group_render_aov_follow")
        return out
