"""Frames shared by tests/test_batch_guides_host.py (CPU) and tests/test_gpu_batch_guides.py (GPU): the batch forms of the guide pass and
of the denoiser (pt_render_aov_batch, pt_denoise_batch).

GUIDE FRAMES, on two scenes of aov_follow_common.py.  A frame is (camera index, table variant):
  mirror_wall  three cameras - the scene's own, and its look_from moved by +0.3 and -0.3 in x - and three tables: the scene's own (passed
               as NULL), the mirror made diffuse (metallic 0), the mirror's colour and the glass's ior changed;
  ico_map      two cameras (its own, look_from + 0.3 in x) and the same three variants on its metal and glass icospheres.
tests/test_batch_guides_host.py holds the CPU twin of every frame to tests/aov_follow_ref.py over a `flat` built with the frame's table,
i.e. the moved cameras keep their rays inside the closest-hit domain of DESIGN.md 2.1; the GPU test then holds the batch to the twin and
to the single-frame calls.

DENOISE FRAMES: the frames of denoise_common.py of one size stacked, frame f seeded seed + 101 * f (frame 0 is the case's own frame, so
denoise_common.reference applies to it); the references of the other frames come from tests/denoise_ref.py, once per session."""
import numpy as np

import aov_follow_common as FC
import aov_follow_ref
import denoise_common as DC
import denoise_ref
from owl_path_tracer_amd.pyhost import scene_io

F32 = np.float32
M_METAL = {"mirror_wall": FC.M_MIRROR, "ico_map": 1}
M_GLASS = {"mirror_wall": FC.M_GLASS, "ico_map": 0}
TEXTURED = {"mirror_wall": (FC.M_WALL,), "ico_map": (0, 1)}  # the materials whose meshes carry the scene's texture (flatten_scene)
SHIFT_X = (0.0, 0.3, -0.3)
FRAMES = {"mirror_wall": [(0, "own"), (1, "diffuse"), (2, "tinted")], "ico_map": [(0, "own"), (1, "tinted"), (0, "diffuse")]}
SIZES = [(37, 23), (24, 16)]  # H is no multiple of 8: the last block row of a frame sticks out, the next frame's blocks start fresh
IDX_METALLIC, IDX_IOR = scene_io.MAT_INDEX["metallic"], scene_io.MAT_INDEX["ior"]

scene, upload, bits, assert_same, params = FC.scene, FC.upload, FC.bits, FC.assert_same, FC.params


def table(name, variant):
    """The (n, 17) float32 material table of a variant; None for the scene's own (a NULL table in the batch)."""
    if variant == "own":
        return None
    mats = np.stack(scene(name)["mats"]).astype(F32).copy()
    if variant == "diffuse":
        mats[M_METAL[name], IDX_METALLIC] = 0.0
    elif variant == "tinted":
        mats[M_METAL[name], 0:3] = (0.3, 0.8, 0.55)
        mats[M_GLASS[name], IDX_IOR] = 1.25
    else:
        raise KeyError(variant)
    return mats


def camera(name, j, W, H, make):
    """Camera j of the scene (make = B.to_camera_data or the oracle's)."""
    frm, at, up, fov = scene(name)["camera"]
    frm = (frm[0] + SHIFT_X[j], frm[1], frm[2])
    return make(tuple(frm), tuple(at), tuple(up), fov, W, H)


def frames(name, W, H, B, which=None):
    """The batch of the scene as Context.render_aov_batch takes it: [(Camera, table or None)]."""
    return [(camera(name, j, W, H, B.to_camera_data), table(name, v)) for j, v in (FRAMES[name] if which is None else which)]


_flat, _ref, _twin, _dn = {}, {}, {}, {}


def flat(name, variant):
    """scene_io.flatten_scene of the scene with the variant's table."""
    key = (name, variant)
    if key not in _flat:
        sc = scene(name)
        t = table(name, variant)
        rows = sc["mats"] if t is None else list(t)
        _flat[key] = scene_io.flatten_scene(sc["ents"], [("m%d" % i, m, "") for i, m in enumerate(rows)], {m: sc["textures"][0] for m in TEXTURED[name]})
    return _flat[key]


def reference(orc, name, frame, W, H, n, max_follow, roughness_max, want_log=False):
    """aov_follow_ref's buffers (H, W, 8) of frame (camera index, variant), and its log: once per session, read-only."""
    j, variant = frame
    key = (name, j, variant, W, H, n, max_follow, float(roughness_max))
    if key not in _ref:
        fl = flat(name, variant)
        S = orc.Scene(fl, watertight=False)
        a, r = aov_follow_ref.aov(S, fl, scene(name)["env"], camera(name, j, W, H, orc.to_camera_data).as_array(), W, H, n, max_follow, roughness_max, want_log=True)
        a.setflags(write=False)
        _ref[key] = (a, r)
    return _ref[key] if want_log else _ref[key][0]


def twin(B, name, frame, W, H, n, max_follow, roughness_max):
    """pt_debug_aov_follow_host of the frame on a host-only context that holds the frame's table: once per session, read-only."""
    j, variant = frame
    key = (name, j, variant, W, H, n, max_follow, float(roughness_max))
    if key not in _twin:
        h = B.Context(-1)
        try:
            upload(h, scene(name), B)
            t = table(name, variant)
            if t is not None:
                h.set_materials(t)
            a = h.aov_follow_host(camera(name, j, W, H, B.to_camera_data), W, H, params(B, n, max_follow, roughness_max))
        finally:
            h.close()
        a.setflags(write=False)
        _twin[key] = a
    return _twin[key]


def denoise_stack(cid, K, bad_in=None):
    """K frames of the size of denoise_common's case cid: (rgb (K, H, W, 3), aov (K, H, W, 8)).  bad_in: the one frame with bad guides
    (None: as the case says, in every frame)."""
    _, W, H, _, seed, bad = DC.case(cid)
    fr = [DC.frame(W, H, seed + 101 * f, bad if bad_in is None else f == bad_in) for f in range(K)]
    return np.stack([a for a, _ in fr]), np.stack([g for _, g in fr])


def denoise_reference(cid, f, bad_in=None):
    """denoise_ref's (out, rgba8) of frame f of denoise_stack(cid, ...): once per session, read-only."""
    _, W, H, prm, seed, bad = DC.case(cid)
    if f == 0 and bad_in is None:
        return DC.reference(cid)
    key = (cid, f, bad_in)
    if key not in _dn:
        rgb, aov = DC.frame(W, H, seed + 101 * f, bad if bad_in is None else f == bad_in)
        out, rgba = denoise_ref.denoise(rgb, aov, **prm)
        out.setflags(write=False)
        rgba.setflags(write=False)
        _dn[key] = (out, rgba)
    return _dn[key]
