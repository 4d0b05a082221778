"""Scenes, rays and cases shared by tests/test_trace_ao_host.py (CPU) and tests/test_gpu_trace_ao.py (GPU): pt_trace_ao, fused ambient
occlusion over the caller's rays.

CASES: the 64 x 48 pixel-centre tables of tests/surface_common.py on its four scenes (the textured cube, Cornell, mirror_wall, tir) and
the closed icosphere of tests/ray_battery.py (ico1280, flat normals (0, 1, 0)) seen from outside and from inside, 1000 rays each.
SETTINGS: n_rays 1, 4 and 16, both flag values, a radius of a quarter of the scene's extent and +inf, two seeds.
A case is computed once per process and handed out read-only; want() and mask() are tests/ao_ref.py's records and its rule for the
records a bit-for-bit comparison takes, cached per setting (one pass over the stream at K = 16 serves K = 1 and 4 and both radii).
CAP: at most 1 % of a case's records may be left out, none on the axis-aligned scenes (AXIS_ALIGNED)."""
import numpy as np

import ao_ref
import ray_battery as rb
import surface_common as SC
from owl_path_tracer_amd.pyhost import binding as B

F32 = np.float32
TABLE_SCENES = ("cube", "cornell", "mirror_wall", "tir")
ICO = ("ico_out", "ico_in")
CASES = TABLE_SCENES + ICO
AXIS_ALIGNED = ("cube",)
KS = (1, 4, 16)
K_MAX = 16
FLAGS = (0, 1)
SEEDS = (0, 20261021)
RADII = ("quarter", "inf")
MAX_LEFT_OUT = 0.01
_cases, _prep, _want, _mask = {}, {}, {}, {}


def _ico_rays(tris, centre, half, inside):
    rng = np.random.default_rng(515 if inside else 516)
    n = 1000
    if inside:
        return rb.closed_mesh_rays(tris, centre, half, rng, n)["random"]
    u = rng.normal(size=(n, 3))
    o = centre + 4.0 * rb.CLOSED_RADIUS * u / np.linalg.norm(u, axis=1, keepdims=True)
    aim = centre + rng.uniform(-1.0, 1.0, (n, 3)) * 1.1 * rb.CLOSED_RADIUS  # a part of them passes the sphere
    o = o.astype(F32)
    return np.ascontiguousarray(np.concatenate([o, (aim - o).astype(F32)], 1), F32)


def case(orc, name, watertight=False):
    """dict(name, flat, rays (n, 6), rec (pt_ray records), truth, S (oracle scene), extent, upload(ctx))."""
    key = (name, bool(watertight))
    if key in _cases:
        return _cases[key]
    if name in TABLE_SCENES:
        tc = SC.table_case(orc, name, "centres", 64, 48, watertight)
        flat, rays, rec, truth = tc["flat"], tc["rays"], tc["rec"], tc["truth"]
        S = orc.Scene(flat, watertight=bool(watertight))

        def upload(ctx, name=name):
            SC.upload(ctx, SC.scene(name), B)
    else:
        tris, centre, half = rb.make_closed_mesh("ico1280")
        flat = SC.battery_flat(tris)
        rays = _ico_rays(tris, centre, half, name == "ico_in")
        S = orc.Scene(flat, watertight=bool(watertight))
        truth = S.intersect_n(rays, use_bvh=False)
        rec = B.make_rays(rays)
        for a in (rays, rec) + tuple(truth):
            a.setflags(write=False)

        def upload(ctx, tris=tris):
            rb.upload(ctx, tris)
    extent = float(np.ptp(np.asarray(flat["positions"], np.float64).reshape(-1, 3), axis=0).max())
    _cases[key] = dict(name=name, wt=bool(watertight), flat=flat, rays=rays, rec=rec, truth=truth, S=S, extent=extent, upload=upload)
    return _cases[key]


def radius_of(c, which):
    return F32(np.inf) if which == "inf" else F32(0.25 * c["extent"])


def params(c, K, flags, which, seed):
    return B.ao_default_params(n_rays=K, flags=flags, radius=float(radius_of(c, which)), seed=seed)


def prep(c, flags, seed):
    key = (c["name"], c["wt"], flags, seed)
    if key not in _prep:
        _prep[key] = ao_ref.prepare(c["S"], c["flat"], c["rays"], c["truth"], flags, seed, K_MAX)
    return _prep[key]


def want(c, K, flags, which, seed):
    key = (c["name"], c["wt"], K, flags, which, seed)
    if key not in _want:
        w = ao_ref.finish(c["S"], prep(c, flags, seed), K, radius_of(c, which))
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def mask(c, K, flags, seed):
    """The compared records, and the check of the cap."""
    key = (c["name"], c["wt"], K, flags, seed)
    if key not in _mask:
        m = ao_ref.compared(c["S"], c["flat"], c["rays"], c["truth"], prep(c, flags, seed), K)
        m.setflags(write=False)
        out = int((~m).sum())
        assert out <= (0 if c["name"] in AXIS_ALIGNED else MAX_LEFT_OUT * m.size), "%s K=%d flags=%d seed=%d: %d of %d records left out" % (c["name"], K, flags, seed, out, m.size)
        _mask[key] = m
    return _mask[key]


def assert_same(got, wanted, m, what):
    assert got.dtype.itemsize == 32 and wanted.dtype.itemsize == 32 and got.shape == wanted.shape, (what, got.dtype, got.shape, wanted.shape)
    bad = ao_ref.differ(got, wanted)
    if m is not None:
        bad &= m
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError("%s: %d of %d compared records differ; first: ray %d\n got  %r\n want %r" % (
            what, int(bad.sum()), int(m.sum()) if m is not None else got.shape[0], i, got[i], wanted[i]))


def first16(rec):
    """The first 16 bytes of every record as pt_ray_hit records."""
    return np.ascontiguousarray(rec.view(np.uint8).reshape(rec.shape[0], 32)[:, :16]).view(B.HIT_DTYPE).reshape(-1)


def clear_of(rec, K):
    """clear = ao * K, exactly: ao = clear * (1 / K) in float32 and K <= 4096."""
    c = np.rint(rec["ao"].astype(np.float64) * K).astype(np.int64)
    assert (c.astype(F32) * (F32(1.0) / F32(K)) == rec["ao"]).all()
    return c
