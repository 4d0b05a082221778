"""ctypes wrapper around oracle/_ref/libref_device.so -- TEST INFRASTRUCTURE ONLY.

The library is the reference's own device code (random.hpp, math.hpp, sample_methods.hpp, the disney/ headers and
device.cu) compiled for the CPU by `make -C oracle ref REF_DIR=<reference checkout>` against the stand-in headers in
oracle/ref_shim (see ref_shim.h for what the stand-ins define).  build() makes it when a reference checkout is present;
oracle/_ref/ is never committed.  The hooks take and return the same things as the oracle's (oracle.py), so a test can
call both with one set of arguments.
"""
import ctypes as C
import os

import numpy as np

import oracle as orc

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libref_device.so")

_lib = None


def available():
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    orc.lib()  # the reference build links the oracle library (traversal, texture and libm stand-ins)
    L = C.CDLL(LIB_PATH)
    fp = C.POINTER(C.c_float)
    L.ref_rng_init.restype = C.c_uint32
    L.ref_rng_init.argtypes = [C.c_uint32, C.c_uint32]
    L.ref_rng_next.restype = C.c_float
    L.ref_rng_next.argtypes = [C.POINTER(C.c_uint32)]
    L.ref_sample_disney.argtypes = [fp, fp, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), fp, fp, fp]
    L.ref_eval_lobe.argtypes = [C.c_int, fp, fp, fp, fp, fp, fp]
    L.ref_eval_sheen.argtypes = [fp, fp, fp, fp]
    L.ref_onb.argtypes = [fp, fp, fp]
    L.ref_to_local.argtypes = [fp, fp, fp, fp, fp]
    L.ref_to_world.argtypes = [fp, fp, fp, fp, fp]
    L.ref_sample_cosine_hemisphere.argtypes = [C.c_float, C.c_float, fp]
    L.ref_refract.argtypes = [fp, fp, C.c_float, fp]
    L.ref_fresnel_equation.restype = C.c_float
    L.ref_fresnel_equation.argtypes = [fp, fp, C.c_float, C.c_float]
    L.ref_d_gtr1.restype = C.c_float
    L.ref_d_gtr1.argtypes = [fp, C.c_float]
    L.ref_d_gtr2.restype = C.c_float
    L.ref_d_gtr2.argtypes = [fp, C.c_float, C.c_float]
    L.ref_lambda.restype = C.c_float
    L.ref_lambda.argtypes = [fp, C.c_float, C.c_float]
    L.ref_uv_on_sphere.argtypes = [fp, fp]
    L.ref_scene_create.restype = C.c_void_p
    L.ref_scene_create.argtypes = [C.POINTER(orc.SceneDesc)]
    L.ref_scene_destroy.argtypes = [C.c_void_p]
    L.ref_scene_meshes.argtypes = [C.c_void_p]
    L.ref_render.argtypes = [C.c_void_p, C.POINTER(orc.Camera), C.POINTER(orc.Env), C.c_int, C.c_int, C.c_int, C.c_int, fp,
                             C.POINTER(C.c_uint32)]
    L.ref_trace_pixel.argtypes = [C.c_void_p, C.POINTER(orc.Camera), C.POINTER(orc.Env), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_int, fp, C.POINTER(C.c_uint32)]
    _lib = L
    return L


_f = orc._f
_vec3 = orc._vec3


def rng_init(u, v):
    return int(lib().ref_rng_init(u & 0xFFFFFFFF, v & 0xFFFFFFFF))


def rng_next(state):
    s = C.c_uint32(state)
    f = lib().ref_rng_next(C.byref(s))
    return float(f), int(s.value)


def sample_disney(mat, wo, rng_state, lobe=orc.LOBE_NONE):
    m, mp = _f(mat)
    f = (C.c_float * 3)()
    wi = (C.c_float * 3)()
    pdf = C.c_float(0)
    st = C.c_uint32(rng_state)
    lb = C.c_int32(lobe)
    lib().ref_sample_disney(mp, _vec3(wo), C.byref(st), C.byref(lb), f, wi, C.byref(pdf))
    return dict(f=np.array(f[:], np.float32), wi=np.array(wi[:], np.float32), pdf=np.float32(pdf.value), lobe=int(lb.value),
                state=int(st.value))


def eval_lobe(lobe, mat, wo, wh, wi):
    m, mp = _f(mat)
    f = (C.c_float * 3)()
    pdf = C.c_float(0)
    lib().ref_eval_lobe(lobe, mp, _vec3(wo), _vec3(wh), _vec3(wi), f, C.byref(pdf))
    return np.array(f[:], np.float32), np.float32(pdf.value)


def eval_sheen(mat, wo, wi):
    m, mp = _f(mat)
    f = (C.c_float * 3)()
    lib().ref_eval_sheen(mp, _vec3(wo), _vec3(wi), f)
    return np.array(f[:], np.float32)


def onb(n):
    t = (C.c_float * 3)()
    b = (C.c_float * 3)()
    lib().ref_onb(_vec3(n), t, b)
    return np.array(t[:], np.float32), np.array(b[:], np.float32)


def to_local(t, b, n, w):
    o = (C.c_float * 3)()
    lib().ref_to_local(_vec3(t), _vec3(b), _vec3(n), _vec3(w), o)
    return np.array(o[:], np.float32)


def to_world(t, b, n, w):
    o = (C.c_float * 3)()
    lib().ref_to_world(_vec3(t), _vec3(b), _vec3(n), _vec3(w), o)
    return np.array(o[:], np.float32)


def sample_cosine_hemisphere(u0, u1):
    o = (C.c_float * 3)()
    lib().ref_sample_cosine_hemisphere(u0, u1, o)
    return np.array(o[:], np.float32)


def refract(w, n, eta):
    o = (C.c_float * 3)()
    ok = lib().ref_refract(_vec3(w), _vec3(n), eta, o)
    return bool(ok), np.array(o[:], np.float32)


def fresnel_equation(i, m, eta_i, eta_t):
    return float(lib().ref_fresnel_equation(_vec3(i), _vec3(m), eta_i, eta_t))


def d_gtr1(wh, alpha):
    return float(lib().ref_d_gtr1(_vec3(wh), alpha))


def d_gtr2(wm, ax, ay):
    return float(lib().ref_d_gtr2(_vec3(wm), ax, ay))


def lambda_(w, ax, ay):
    return float(lib().ref_lambda(_vec3(w), ax, ay))


def uv_on_sphere(n):
    o = (C.c_float * 2)()
    lib().ref_uv_on_sphere(_vec3(n), o)
    return np.array(o[:], np.float32)


class Scene:
    """The reference's per-mesh buffers and entity data for a flattened triangle soup (pyhost.scene_io.flatten_scene);
    closest hits come from the oracle's query (ref_shim.h)."""

    def __init__(self, flat):
        self._keep = []
        d = orc.SceneDesc()
        n = int(flat["positions"].shape[0])
        d.n_tris = n
        pos, d.positions = _f(flat["positions"].reshape(-1))
        nrm, d.normals = _f(flat["normals"].reshape(-1))
        self._keep += [pos, nrm]
        if flat.get("texcoords") is not None:
            tc, d.texcoords = _f(flat["texcoords"].reshape(-1))
            self._keep.append(tc)
        else:
            d.texcoords = None
        mi = np.ascontiguousarray(flat["material_index"], np.int32)
        ti = np.ascontiguousarray(flat["texture_index"], np.int32)
        d.material_index = mi.ctypes.data_as(C.POINTER(C.c_int32))
        d.texture_index = ti.ctypes.data_as(C.POINTER(C.c_int32))
        mats, d.materials = _f(np.asarray(flat["materials"], np.float32).reshape(-1))
        d.n_materials = mats.size // orc.MAT_FLOATS
        texs = flat.get("textures") or []
        d.n_textures = len(texs)
        arr = (orc.Texture * max(1, len(texs)))()
        for i, t in enumerate(texs):
            tt, keep = orc._tex(t)
            arr[i] = tt
            self._keep.append(keep)
        d.textures = arr
        self._keep += [mi, ti, mats, arr]
        self.h = lib().ref_scene_create(C.byref(d))

    def __del__(self):
        try:
            if self.h:
                lib().ref_scene_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def meshes(self):
        return lib().ref_scene_meshes(self.h)

    def render(self, cam, env, W, H, spp, max_depth):
        """ray_gen over every pixel: (rgb float32 (H, W, 3) in framebuffer order, the float colour ray_gen hands to
        make_rgba; rgba8 (H, W) uint32 as ray_gen wrote it)."""
        rgb = np.zeros((H, W, 3), np.float32)
        rgba = np.zeros((H, W), np.uint32)
        rc = lib().ref_render(self.h, C.byref(cam), C.byref(env), W, H, spp, max_depth, rgb.ctypes.data_as(C.POINTER(C.c_float)),
                              rgba.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc != 0:
            raise RuntimeError("ref_render: a pixel exceeded its trace budget (endless NaN retries)")
        return rgb, rgba

    def trace_pixel(self, cam, env, W, H, px, py, spp, max_depth):
        """Per-sample radiance (spp, 3) and rng state after each sample (spp,), as oracle.Scene.trace_pixel."""
        rgb = np.zeros((spp, 3), np.float32)
        st = np.zeros(spp, np.uint32)
        rc = lib().ref_trace_pixel(self.h, C.byref(cam), C.byref(env), W, H, px, py, spp, max_depth,
                                   rgb.ctypes.data_as(C.POINTER(C.c_float)), st.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc != 0:
            raise RuntimeError("ref_trace_pixel: trace budget exceeded (endless NaN retries)")
        return rgb, st
