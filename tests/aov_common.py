"""Scenes, cameras and cases shared by tests/test_aov_host.py (CPU) and tests/test_gpu_aov.py (GPU): the guide pass (pt_render_aov).

A CASE is (scene name, W, H, n_samples); every case runs with watertight 0 and 1.  A scene is a dict: ents / mats / textures /
mesh_textures as Context.upload_scene takes them, flat (scene_io.flatten_scene, for the oracle), env (kwargs of make_env), camera
(look_from, look_at, look_up, vertical fov).  All cameras are inside the closest-hit domain of DESIGN.md 2.1: within 10 scene extents, no
ray in a triangle's plane (tests/test_aov_host.py checks that the oracle's walk and brute force agree on every ray used)."""
import os

import numpy as np

import aov_ref
import ray_battery as rb
from owl_path_tracer_amd.pyhost import scene_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
F32 = np.float32

CASES = [("cube", 37, 23, 1), ("cube", 37, 23, 5), ("cornell", 32, 24, 3), ("ico_map", 24, 16, 2), ("ico_auto", 24, 16, 2), ("ico_colour", 24, 16, 2)]
# Cornell from inside, half a unit under the ceiling and looking up and towards the open side: the frame shows the light (>= 5 % of the
# pixels hit it) and, past the ceiling's edge, the environment (>= 10 % miss); tests/test_gpu_aov.py asserts both shares from the oracle
CROSS_CAMERA = ([0.2, 1.5, 0.05], [0.45, 1.98, 0.0], [1, 0, 0.1], 105.0)
CROSS_ENV = dict(color=(0.2, 0.5, 0.9), intensity=1.5)
CROSS_SIZE = (40, 32)


def _rgba8(rng, h, w):
    px = rng.integers(0, 256, (h, w, 3)).astype(np.uint32)
    return (px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16) | (0xFF << 24)).astype(np.uint32)


def _smooth_icosphere(centre, radius):
    """tests/test_gpu_watertight.py's: 320 triangles, the normal of a vertex is its normalised position on the unit sphere, its texcoord a
    spherical map of it - whatever u, v a hit reports shows in the normal and in the texel."""
    unit = rb.icosphere(2).reshape(-1, 3)
    n = unit.astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    tc = np.stack([np.arctan2(n[:, 2], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], 1)
    v = (unit * F32(radius) + F32(centre)).astype(F32)
    return dict(vertices=v, normals=n.astype(F32), texcoords=tc.astype(F32), indices=np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3))


def _icospheres(env):
    """The smooth-icosphere scene of tests/test_gpu_watertight.py (a glass and a metallic icosphere, smooth and textured, either side of
    a small emitter), its camera outside, under the given environment; a fourth mesh has material index -1 (the defaults)."""
    rng = np.random.default_rng(20260917)
    glass = scene_io.material(base_color=(0.95, 0.97, 1.0), specular_transmission=1.0, ior=1.5, roughness=0.05, specular_transmission_roughness=0.0)
    metal = scene_io.material(base_color=(0.9, 0.7, 0.4), metallic=1.0, roughness=0.25)
    glow = scene_io.material(emission=9.0)
    mats = [("glass", glass, ""), ("metal", metal, ""), ("glow", glow, "")]
    g_centre, m_centre = (-1.25, 0.1, 0.0), (1.2, -0.05, 0.15)
    metal_mesh = _smooth_icosphere(m_centre, 0.9)
    plain = rb.mesh_of(((rb.icosphere(1) * F32(0.3)) + F32([0.1, 1.0, 0.4])).astype(F32))
    ents = [(_smooth_icosphere(g_centre, 1.0), 0), (metal_mesh, 1), (rb.mesh_of((rb.icosphere(1) * F32(0.22)).astype(F32)), 2), (plain, -1)]
    tex = _rgba8(rng, 5, 7)
    envmap = _rgba8(rng, 8, 16)
    env = dict(env, env_map=envmap) if env.get("use_map") else env
    return dict(ents=ents, mats=[m for _, m, _ in mats], flat=scene_io.flatten_scene(ents, mats, {0: tex, 1: tex}), textures=[tex], mesh_textures=[0, 0, -1, -1], env=env,
                camera=([0.4, 1.1, 4.5], [0.1, 0.2, 0.0], [0, 1, 0], 36.0))


_cache = {}


def scene(name):
    if name in _cache:
        return _cache[name]
    if name == "cube":
        sc = scene_io.load_scene_dir(ASSETS, "cube")
        tex = scene_io.checker_texture()
        c = sc["camera"]
        s = dict(ents=sc["entities"], mats=[m for _, m, _ in sc["materials"]], flat=scene_io.flatten_scene(sc["entities"], sc["materials"], {0: tex}), textures=[tex],
                 mesh_textures=[0] * len(sc["entities"]), env=dict(use_auto=True, intensity=1.0), camera=(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"]))
    elif name in ("cornell", "cornell_cross"):
        sc = scene_io.load_scene_dir(ASSETS, "cornell-box")
        c = sc["camera"]
        cross = name == "cornell_cross"
        s = dict(ents=sc["entities"], mats=[m for _, m, _ in sc["materials"]], flat=scene_io.flatten_scene(sc["entities"], sc["materials"]), textures=None, mesh_textures=None,
                 env=CROSS_ENV if cross else dict(color=(0.3, 0.6, 0.2), intensity=0.75),
                 camera=CROSS_CAMERA if cross else (c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"]))
    elif name == "ico_map":
        s = _icospheres(dict(use_map=True, intensity=1.25))
    elif name == "ico_auto":
        s = _icospheres(dict(use_auto=True, intensity=0.5))
    elif name == "ico_colour":
        s = _icospheres(dict(color=(0.25, 0.5, 1.0), intensity=2.0))
    else:
        raise KeyError(name)
    _cache[name] = s
    return s


def upload(ctx, sc, B):
    ctx.upload_scene(sc["ents"], sc["mats"], textures=sc["textures"], mesh_textures=sc["mesh_textures"], env=B.make_env(**sc["env"]))


def camera(sc, W, H, make):
    """make = B.to_camera_data or the oracle's"""
    frm, at, up, fov = sc["camera"]
    return make(tuple(frm), tuple(at), tuple(up), fov, W, H)


_ref = {}


def reference(orc, name, W, H, n, wt):
    """aov_ref's buffers of a case, (H, W, 8), computed once per session and handed out read-only."""
    key = (name, W, H, n, bool(wt))
    if key not in _ref:
        sc = scene(name)
        S = orc.Scene(sc["flat"], watertight=bool(wt))
        cam = camera(sc, W, H, orc.to_camera_data).as_array()
        a = aov_ref.aov(S, sc["flat"], sc["env"], cam, W, H, n)
        a.setflags(write=False)
        _ref[key] = a
    return _ref[key]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = g != w
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        raise AssertionError("%s: %d of %d floats differ in bits (%d pixels); first at %s: got %r, want %r" % (
            what, int(bad.sum()), bad.size, int(bad.reshape(-1, 8).any(1).sum()) if bad.size % 8 == 0 else -1, i, np.asarray(got)[i], np.asarray(want)[i]))
