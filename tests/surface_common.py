"""Scenes, rays and cases shared by tests/test_trace_surface_host.py (CPU) and tests/test_gpu_trace_surface.py (GPU): pt_trace_surface,
closest hit with the surface record at the hit.

Two families of rays, both inside the closest-hit domain:
  TABLES   the zero-jitter tables of tests/aov_rays_common.py on its four scenes (Cornell, the textured cube, mirror_wall, tir - vertex
           normals, texcoords, textures, an emitter, glass) as pt_ray records with tmax = +inf: the pixel-centre rays of the scene's
           camera at 20 x 13 and 64 x 48 and the 24 x 16 probes.  Every ray is compared.
  BATTERY  every scene of tests/ray_battery.py with the rays and the brute-force truth of tests/trace_rays_common.py (flat normals, no
           texcoords, the default material); compared where trace_rays_common.compared says so.
A CASE is dict(flat, rays (n, 6), rec (pt_ray records), truth (the oracle's brute force), want (surface_ref's records), mask (or None)),
computed once per process and handed out read-only.  Every comparison is bit for bit on the 80 bytes."""
import numpy as np

import aov_rays_common as AR
import ray_battery as rb
import ray_image_ref as RR
import surface_ref
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B
from owl_path_tracer_amd.pyhost import scene_io

F32 = np.float32
SCENES = AR.SCENES
TABLES = [(name, kind, W, H) for name in SCENES for (kind, W, H) in (("centres", 20, 13), ("centres", 64, 48), ("probes",) + AR.PROBE_SIZE)]
GPU_TABLES = [(name, kind, W, H) for (name, kind, W, H) in TABLES if (W, H) != (20, 13)]
EMISSION = 2.5  # of the wall of mirror_wall under emitting_wall(): a textured emitter, which no scene has by itself
scene, upload = AR.scene, AR.upload
_cache = {}


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, tuple):
            for a in v:
                a.setflags(write=False)
    return case


def table_case(orc, name, kind, W, H, watertight=False):
    key = (name, kind, W, H, bool(watertight))
    if key not in _cache:
        flat = scene(name)["flat"]
        o, d = RR.rays_through(*AR.rays_of(name, kind, W, H, orc.to_camera_data))
        rays = np.concatenate([o, d], 1).astype(F32)
        truth = orc.Scene(flat, watertight=bool(watertight)).intersect_n(rays, use_bvh=False)
        _cache[key] = _frozen(dict(flat=flat, rays=rays, rec=B.make_rays(rays), truth=truth, want=surface_ref.surface(flat, truth), mask=None))
    return _cache[key]


def battery_flat(tris):
    """The flat scene of a battery soup as rb.upload hands it to the library: one mesh, normals (0, 1, 0), no texcoords, material 0."""
    return scene_io.flatten_scene([(rb.mesh_of(tris), 0)], [("a", scene_io.MAT_DEFAULT, "")])


def battery_case(orc, name, watertight=False):
    key = ("battery", name, bool(watertight))
    if key not in _cache:
        bt = TC.battery(orc, name, watertight)
        flat = battery_flat(bt["tris"])
        _cache[key] = _frozen(dict(flat=flat, rays=bt["rays"], rec=B.make_rays(bt["rays"]), truth=bt["truth"], want=surface_ref.surface(flat, bt["truth"]), mask=bt["mask"],
                                   tris=bt["tris"], cls=bt["cls"]))
    return _cache[key]


def emitting_wall():
    """mirror_wall's material table with the textured wall emitting: (table for pt_set_materials, the same for surface_ref)."""
    mats = np.stack(scene("mirror_wall")["mats"]).astype(F32)
    mats[0, 16] = F32(EMISSION)
    return mats


def same(got, want, mask=None):
    ok = ~surface_ref.differ(got, want)
    return ok if mask is None else (ok | ~mask)


def assert_same(got, want, mask, what):
    assert got.dtype.itemsize == 80 and want.dtype.itemsize == 80 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ok = same(got, want, mask)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: %d of %d compared records differ; first: ray %d\n got  %r\n want %r" % (
            what, int((~ok).sum()), int(mask.sum()) if mask is not None else got.shape[0], i, got[i], want[i]))


def first16(rec):
    """The first 16 bytes of every surface record as pt_ray_hit records."""
    return np.ascontiguousarray(rec.view(np.uint8).reshape(rec.shape[0], 80)[:, :16]).view(B.HIT_DTYPE).reshape(-1)


def miss_bytes():
    """The 80 bytes of a miss."""
    m = np.zeros(1, surface_ref.DTYPE)
    m["prim"], m["material"] = -1, -1
    return m.view(np.uint8).copy()
