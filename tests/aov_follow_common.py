"""Scenes, cameras and cases shared by tests/test_aov_follow_host.py (CPU) and tests/test_gpu_aov_follow.py (GPU): the follow mode of the
guide pass (pt_render_aov_follow).  The scenes of tests/aov_common.py plus two:

mirror_wall  a checker-textured wall in the plane z = 0; to its right a flat mirror (metallic 1, roughness 0, colour (0.9, 0.7, 0.4)) turned
             towards the wall and the camera; in front of the wall's left part a glass pane of two parallel quads (specular_transmission 1,
             ior 1.5, both roughnesses 0, outward normals); a small emitter in front of the wall; the automatic environment.  From its
             camera the frame holds the wall seen directly, in the mirror and through the pane, mirror pixels whose reflected ray leaves
             the scene, and primary misses above the wall (tests/test_aov_follow_host.py asserts each from the oracle's hits).
tir          the camera inside a closed glass icosphere (ior 1.5, smooth normals) away from its centre: some rays leave, some reflect
             internally.

A CASE is (scene, W, H, n_samples, max_follow, roughness_max) = a FRAME in a MODE, the full cross product; every case runs with
watertight 0 and 1.  All cameras keep every ray, follow rays included, inside the closest-hit domain of DESIGN.md 2.1 (the host test
checks the oracle's walk against its brute force on every ray the cases use)."""
import numpy as np

import aov_common as AC
import aov_follow_ref
from owl_path_tracer_amd.pyhost import scene_io

F32 = np.float32
ROOT = AC.ROOT
MIRROR_COLOUR = (0.9, 0.7, 0.4)
# (the ico metal has roughness 0.25: followed at roughness_max 0.3, not at 0.2)
FRAMES = [(name, W, H, n) for name in ("mirror_wall", "tir", "ico_map", "ico_colour") for (W, H) in ((24, 16), (37, 23)) for n in (1, 3)]
MODES = [(k, r) for k in (0, 1, 2, 4) for r in (0.3, 0.2)]
CASES = [f + m for f in FRAMES for m in MODES]
# mirror_wall materials
M_WALL, M_MIRROR, M_GLASS, M_GLOW = 0, 1, 2, 3


def _quad(p0, p1, p2, p3, normal, tcs=None):
    """Two triangles p0 p1 p2, p0 p2 p3 with one normal; tcs: the four texcoords or None"""
    v = np.array([p0, p1, p2, p0, p2, p3], F32)
    tc = np.zeros((0, 2), F32) if tcs is None else np.array([tcs[0], tcs[1], tcs[2], tcs[0], tcs[2], tcs[3]], F32)
    return dict(vertices=v, normals=np.tile(F32(normal), (6, 1)), texcoords=tc, indices=np.arange(6, dtype=np.int32).reshape(2, 3))


def _mirror_wall():
    wall = scene_io.material(base_color=(0.8, 0.8, 0.8), roughness=0.9)
    mirror = scene_io.material(base_color=MIRROR_COLOUR, metallic=1.0, roughness=0.0)
    glass = scene_io.material(base_color=(0.95, 0.97, 1.0), specular_transmission=1.0, ior=1.5, roughness=0.0, specular_transmission_roughness=0.0)
    glow = scene_io.material(emission=6.0)
    mats = [("wall", wall, ""), ("mirror", mirror, ""), ("glass", glass, ""), ("glow", glow, "")]
    ents = [
        (_quad((-4.1, -1.45, 0.0), (3.9, -1.45, 0.0), (3.9, 1.55, 0.0), (-4.1, 1.55, 0.0), (0, 0, 1), ((0, 0), (2, 0), (2, 0.75), (0, 0.75))), M_WALL),
        # the mirror: a vertical quad right of the camera's axis, nearly at right angles to the wall: it shows the camera the wall
        (_quad((2.4, -1.15, 3.6), (1.9, -1.15, 1.0), (1.9, 1.25, 1.0), (2.4, 1.25, 3.6), (-0.982, 0.0, 0.189)), M_MIRROR),
        # the pane: front face towards the camera, back face towards the wall, normals outward
        (_quad((-3.3, -0.95, 1.2), (-1.2, -0.95, 1.2), (-1.2, 1.05, 1.2), (-3.3, 1.05, 1.2), (0, 0, 1)), M_GLASS),
        (_quad((-3.3, -0.95, 1.1), (-3.3, 1.05, 1.1), (-1.2, 1.05, 1.1), (-1.2, -0.95, 1.1), (0, 0, -1)), M_GLASS),
        (_quad((0.35, 0.55, 0.3), (0.8, 0.55, 0.3), (0.8, 0.95, 0.3), (0.35, 0.95, 0.3), (0, 0, 1)), M_GLOW),
    ]
    tex = scene_io.checker_texture()
    return dict(ents=ents, mats=[m for _, m, _ in mats], flat=scene_io.flatten_scene(ents, mats, {M_WALL: tex}), textures=[tex], mesh_textures=[0, -1, -1, -1, -1],
                env=dict(use_auto=True, intensity=1.0), camera=([-0.37, 0.23, 6.1], [0.05, 0.12, 0.0], [0, 1, 0], 58.0))


def _tir():
    glass = scene_io.material(base_color=(0.9, 0.95, 1.0), specular_transmission=1.0, ior=1.5, roughness=0.0, specular_transmission_roughness=0.0)
    floor = scene_io.material(base_color=(0.6, 0.3, 0.2), roughness=0.8)
    mats = [("glass", glass, ""), ("floor", floor, "")]
    ents = [(AC._smooth_icosphere((0.0, 0.0, 0.0), 1.0), 0),
            (_quad((-6.0, -1.6, -6.0), (-6.0, -1.6, 6.0), (6.0, -1.6, 6.0), (6.0, -1.6, -6.0), (0, 1, 0)), 1)]
    tex = AC._rgba8(np.random.default_rng(20261018), 6, 9)
    return dict(ents=ents, mats=[m for _, m, _ in mats], flat=scene_io.flatten_scene(ents, mats, {0: tex}), textures=[tex], mesh_textures=[0, -1],
                env=dict(color=(0.4, 0.7, 1.0), intensity=1.5), camera=([0.8, 0.1, 0.25], [0.2, -0.3, -0.9], [0, 1, 0], 100.0))


def scene(name):
    if name not in AC._cache:
        if name == "mirror_wall":
            AC._cache[name] = _mirror_wall()
        elif name == "tir":
            AC._cache[name] = _tir()
    return AC.scene(name)


upload, camera, bits, assert_same = AC.upload, AC.camera, AC.bits, AC.assert_same
_ref = {}


def reference(orc, name, W, H, n, max_follow, roughness_max, wt, want_log=False):
    """aov_follow_ref's buffers of a case, (H, W, 8), and its log: computed once per session and handed out read-only."""
    key = (name, W, H, n, max_follow, float(roughness_max), bool(wt))
    if key not in _ref:
        sc = scene(name)
        S = orc.Scene(sc["flat"], watertight=bool(wt))
        cam = camera(sc, W, H, orc.to_camera_data).as_array()
        a, r = aov_follow_ref.aov(S, sc["flat"], sc["env"], cam, W, H, n, max_follow, roughness_max, want_log=True)
        a.setflags(write=False)
        _ref[key] = (a, r)
    return _ref[key] if want_log else _ref[key][0]


def params(B, n, max_follow, roughness_max):
    return B.aov_default_params(n_samples=n, max_follow=max_follow, roughness_max=roughness_max)
