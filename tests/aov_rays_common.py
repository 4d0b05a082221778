"""Scenes, ray images and cases shared by tests/test_aov_rays_host.py (CPU) and tests/test_gpu_aov_rays.py (GPU): the guide pass over a
ray image (pt_render_aov_rays).

The scenes are those of tests/aov_common.py and tests/aov_follow_common.py: Cornell, the textured cube, mirror_wall (a mirror and a
window pane in front of a textured wall) and tir (the camera inside a glass sphere).  Two kinds of table with zero jitter, both built
the way tests/test_gpu_ray_image.py builds them - the tests choose org and a target L, never dir, which is fl(L - org):

  centres  the pixel-centre rays of the scene's camera at W x H (ray_image_ref.pixel_centre_targets);
  probes   24 x 16 unrelated rays: origins anywhere in the scene's box, a seeded twelve up to 5 extents outside (half of those look back
           at the scene), directions uniform on the sphere.

and the two kinds of tests/ray_tables.py whose jitter differs from record to record, so that a pixel that took another record's du / dv,
a stale record, the other draw or the terms in another order shows:

  scrambled  org, dir, du and dv all per pixel, an eighth of the records without du, without dv and without both, NaN in the reserved floats;
  equirect   a panorama from inside the scene, the jitter shrinking towards the poles.

A CASE is (scene, kind, W, H, n_samples, max_follow); roughness_max is the default 0.3.  CASES are the zero-jitter ones.  JITTER_CASES
are on mirror_wall and tir, where followed rays start from jittered ones (and one frame each on Cornell and the cube): the shapes 1 x 1,
7 x 9 (under one wave, partial 8 x 8 blocks), 20 x 13, 130 x 3 (more blocks than rows), 3 x 130 and 64 x 48 (many waves); n_samples 1, 3
and 16; max_follow 0 and 4 - not the full cross product, each value with each shape class (NK).  A 1 x 1 panorama has no jitter to
speak of (du = 0, dv parallel to dir): no equirect case there."""
import os
import re

import numpy as np

import aov_follow_common as FC
import aov_rays_ref
import ray_image_ref as RR
import ray_tables as RT

F32 = np.float32
ROOT = FC.ROOT
SCENES = ("cornell", "cube", "mirror_wall", "tir")
PROBE_SIZE = (24, 16)
ROUGHNESS_MAX = 0.3
CASES = [(name, "centres", W, H, n, k) for name in SCENES for (W, H) in ((20, 13), (64, 48)) for n in (1, 3) for k in (0, 4)]
CASES += [(name, "probes") + PROBE_SIZE + (n, k) for name in SCENES for n in (1, 3) for k in (0, 4)]
JITTER_KINDS = ("scrambled", "equirect")
JITTER_SHAPES = ((1, 1), (7, 9), (20, 13), (130, 3), (3, 130), (64, 48))
NK = {(64, 48): ((1, 4), (3, 0)), (20, 13): ((1, 0), (3, 4), (16, 0), (16, 4))}
NK_SMALL = ((1, 0), (3, 4), (16, 4))
JITTER_CASES = [(name, kind, W, H, n, k) for name in ("mirror_wall", "tir") for kind in JITTER_KINDS for (W, H) in JITTER_SHAPES
                if not (kind == "equirect" and W * H == 1) for (n, k) in NK.get((W, H), NK_SMALL)]
JITTER_CASES += [(name, "scrambled", 20, 13, 3, 4) for name in ("cornell", "cube")]

scene, upload, camera, bits, assert_same, params = FC.scene, FC.upload, FC.camera, FC.bits, FC.assert_same, FC.params
_tables = {}
_ref = {}


def record_dtype():
    """pt_ray_gen as numpy sees it, without the library: org, dir, du, dv at bytes 0, 16, 32, 48 of 64."""
    return np.dtype([("org", "<f4", (3,)), ("reserved0", "<f4"), ("dir", "<f4", (3,)), ("reserved1", "<f4"),
                     ("du", "<f4", (3,)), ("reserved2", "<f4"), ("dv", "<f4", (3,)), ("reserved3", "<f4")])


def fixed_table(orgs, targets):
    """(table of zero-jitter records {org, fl(target - org), 0, 0}, orgs, targets) in float32."""
    o, d = RR.rays_through(orgs, targets)
    t = np.zeros(o.shape[0], record_dtype())
    t["org"], t["dir"] = o, d
    return t


def centre_rays(name, W, H, make):
    """(orgs, targets) of the pixel-centre rays of the scene's camera; make = B.to_camera_data or the oracle's (the same 12 floats)."""
    cam = camera(scene(name), W, H, make).as_array()
    return np.tile(cam[0:3], (W * H, 1)).astype(F32), RR.pixel_centre_targets(cam, W, H)


def probe_rays(name, W, H):
    """tests/test_gpu_ray_image.py's probe rays, for the scenes of this module."""
    P = scene(name)["flat"]["positions"].reshape(-1, 3).astype(np.float64)
    lo, hi = P.min(0), P.max(0)
    ext = float((hi - lo).max())
    rng = np.random.default_rng(20261101 + SCENES.index(name))
    n = W * H
    orgs = lo + (hi - lo) * rng.random((n, 3))
    far = rng.choice(n, 12, replace=False)  # a seeded few outside, up to 5 extents from the box's centre
    u = rng.normal(size=(12, 3))
    orgs[far] = 0.5 * (lo + hi) + u / np.linalg.norm(u, axis=1, keepdims=True) * ext * rng.uniform(1.0, 5.0, (12, 1))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[far[:6]] = 0.5 * (lo + hi) - orgs[far[:6]]  # half of those look back at the scene
    d[far[:6]] /= np.linalg.norm(d[far[:6]], axis=1, keepdims=True)
    orgs = orgs.astype(F32)
    return orgs, (orgs.astype(np.float64) + d).astype(F32)


def rays_of(name, kind, W, H, make):
    """(orgs, targets) of a case's table, computed once."""
    key = (name, kind, W, H)
    if key not in _tables:
        o, L = centre_rays(name, W, H, make) if kind == "centres" else probe_rays(name, W, H)
        o.setflags(write=False)
        L.setflags(write=False)
        _tables[key] = (o, L)
    return _tables[key]


def table(name, kind, W, H, make):
    if kind in JITTER_KINDS:
        return RT.table(kind, name, W, H)
    return fixed_table(*rays_of(name, kind, W, H, make))


def reference(orc, name, kind, W, H, n, max_follow, wt, want_samples=False):
    """aov_rays_ref's buffers of a case, (H, W, 8), and its first-hit record: computed once per session and handed out read-only."""
    key = (name, kind, W, H, n, max_follow, bool(wt))
    if key not in _ref:
        sc = scene(name)
        S = orc.Scene(sc["flat"], watertight=bool(wt))
        a, r = aov_rays_ref.aov(S, sc["flat"], sc["env"], table(name, kind, W, H, orc.to_camera_data), W, H, n, max_follow, ROUGHNESS_MAX, want_samples=True)
        a.setflags(write=False)
        _ref[key] = (a, r)
    return _ref[key] if want_samples else _ref[key][0]


def precondition(orc, name, kind, W, H, n, max_follow):
    """The precondition of tests/ray_tables.py for a jittered case, in guide buffers: aov_rays_ref's buffers of the case's table differ, in
    at least half (RT.CAP) of all pixels, from its buffers of the table with du / dv rolled by one record, with the jitter zeroed and
    with du and dv exchanged - asserted, computed once per session; returns {variant: share}.  (A 1 x 1 table has no neighbour.)"""
    key = ("pre", name, kind, W, H, n, max_follow)
    if key not in _ref:
        sc = scene(name)
        S = orc.Scene(sc["flat"])
        want = reference(orc, name, kind, W, H, n, max_follow, 0)
        t = table(name, kind, W, H, orc.to_camera_data)
        out = {}
        for what, f in RT.VARIANTS:
            if what == "neighbour" and W * H == 1:
                continue
            other = aov_rays_ref.aov(S, sc["flat"], sc["env"], f(t), W, H, n, max_follow, ROUGHNESS_MAX)
            out[what] = float((bits(other) != bits(want)).any(-1).mean())
        _ref[key] = out
    out = _ref[key]
    for what, share in out.items():
        assert share >= RT.CAP, "%s %s %dx%d n=%d max_follow=%d: the guide buffers differ from the '%s' table's in %.1f %% of the pixels only (%r)" % (
            name, kind, W, H, n, max_follow, what, 100 * share, out)
    return out


def camera_of(B, c12):
    """B.Camera of 12 floats (origin, llc, horizontal, vertical)."""
    cam = B.Camera()
    a = np.asarray(c12, F32)
    cam.origin[:], cam.llc[:], cam.horizontal[:], cam.vertical[:] = a[0:3].tolist(), a[3:6].tolist(), a[6:9].tolist(), a[9:12].tolist()
    return cam


def jitter_records(dtype, n_images=8):
    """Eight records {org = 0, dir, du, dv}: |dir| 0.5..2, |du|, |dv| up to 0.2 |dir|."""
    rng = np.random.default_rng(64)
    out = []
    for _ in range(n_images):
        d = rng.normal(size=3)
        d = (d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)).astype(F32)
        du, dv = ((v / np.linalg.norm(v) * np.linalg.norm(d) * rng.uniform(0.02, 0.2)).astype(F32) for v in rng.normal(size=(2, 3)))
        t = np.zeros(1, dtype)
        t["dir"], t["du"], t["dv"] = d, du, dv
        out.append(t)
    return out


def lds_bytes_of_the_guide_kernels():
    """(PT_LDS_STACK + PT_AOV_PARK) * 64 * 4 from the sources' own defines."""
    csrc = os.path.join(ROOT, "owl-path-tracer_amd", "csrc")
    stack = int(re.search(r"#define PT_LDS_STACK (\d+)", open(os.path.join(csrc, "pt_trace.h")).read()).group(1))
    park = int(re.search(r"#define PT_AOV_PARK (\d+)", open(os.path.join(csrc, "pt_aov_follow.h")).read()).group(1))
    return (stack + park) * 64 * 4
