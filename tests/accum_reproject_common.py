"""Cameras, states and comparisons shared by tests/test_accum_reproject_host.py (CPU) and tests/test_gpu_accum_reproject.py (GPU)."""
import numpy as np

import accum_reproject_ref as RR
from owl_path_tracer_amd.pyhost import binding as B

F32, U32 = np.float32, np.uint32
KEYS = ("sum", "half", "n", "n_half", "passes", "rgb", "rgba8", "noise")
STATE = ("sum", "half", "n", "n_half", "passes")


def rot_y(v, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    x, y, z = v
    return np.array([c * x + s * z, y, -s * x + c * z])


def look(frm, at, up, fov, W, H):
    return B.to_camera_data(tuple(float(x) for x in frm), tuple(float(x) for x in at), tuple(float(x) for x in up), float(fov), W, H)


def pair(kind, view, W, H, depth=None, deg=2.0):
    """(old camera, new camera) of a camera move; view = (look_from, look_at, look_up, vertical fov).  depth: the distance at which the
    sideways step is a third of the frame's width (None: that of look_at); deg: the orbit's angle."""
    frm, at, up, fov = (np.asarray(v, np.float64) if i < 3 else v for i, v in enumerate(view))
    old = look(frm, at, up, fov, W, H)
    if kind == "identical":
        return old, look(frm, at, up, fov, W, H)
    if kind == "orbit":  # about the vertical through look_at
        return old, look(at + rot_y(frm - at, deg), at, up, fov, W, H)
    if kind == "sideways":  # (the image plane of pt_to_camera_data lies at distance 1)
        h = np.asarray(list(old.horizontal), np.float64)
        step = h * ((np.linalg.norm(at - frm) if depth is None else depth) / 3.0)
        return old, look(frm + step, at + step, up, fov, W, H)
    if kind == "away":  # the OLD camera looks the other way: every lam <= 0
        return look(frm, frm - (at - frm), up, fov, W, H), look(frm, at, up, fov, W, H)
    if kind == "roll":  # 90 degrees about the view axis
        fwd = (at - frm) / np.linalg.norm(at - frm)
        return old, look(frm, at, np.cross(fwd, up), fov, W, H)
    raise KeyError(kind)


def random_state(rng, W, H, pairs_7_3=True):
    """dict(sum, half, n, n_half, passes) in framebuffer order: n in 0..400, n_half in {0, n / 2, (7, 3)} by thirds."""
    n = rng.integers(0, 401, (H, W)).astype(U32)
    which = rng.integers(0, 3, (H, W))
    n_half = np.where(which == 0, 0, n // 2).astype(U32)
    if pairs_7_3:
        n = np.where(which == 2, 7, n).astype(U32)
        n_half = np.where(which == 2, 3, n_half).astype(U32)
    n_half = np.where(n < 2, 0, n_half).astype(U32)
    mean = rng.uniform(0.0, 3.0, (H, W, 3))
    sum_ = (mean * n[..., None]).astype(F32)
    half = (sum_ * (n_half / np.maximum(n, 1))[..., None] + rng.standard_normal((H, W, 3)) * np.sqrt(n_half)[..., None] * 0.5).astype(F32)
    half = np.where((n_half == 0)[..., None], F32(0), half).astype(F32)
    passes = np.where(n == 0, 0, np.where(n_half == 0, 1, rng.integers(2, 9, (H, W)))).astype(U32)
    return dict(sum=sum_, half=half, n=n, n_half=n_half, passes=passes)


def same(a, b):
    """Bit for bit, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return (a.view(U32) == np.ascontiguousarray(b, F32).view(U32)) | (np.isnan(a) & np.isnan(b))
    return a == b


def assert_state(got, want, what, keys=KEYS):
    for k in keys:
        ok = same(got[k], want[k])
        assert ok.all(), "%s: %s differs in %d of %d entries" % (what, k, int((~ok).sum()), ok.size)


def ref(old, new, prev, cur, state, owned=None, params=None):
    """tests/accum_reproject_ref.py for binding cameras and a ReprojectParams (None: the defaults)"""
    p = params if params is not None else B.reproject_default_params()
    return RR.reproject(old.as_array(), new.as_array(), prev, cur, state, owned, max_history=p.max_history, depth_tol=p.depth_tol, normal_min=p.normal_min,
                        albedo_tol=p.albedo_tol)
