"""Ray images that can tell records apart, shared by tests/test_ray_image_host.py, tests/test_gpu_ray_image.py, tests/test_aov_rays_host.py
and tests/test_gpu_aov_rays.py.  Seeded numpy only: the scenes' boxes come from tests/aov_follow_common.py and the panorama from pyhost/ray_image.py, both host-side
Python; no kernel and no C code of the library takes part in a table.

scrambled   all four vectors of every record vary per pixel: org uniform in the inner 80 % of the scene's box (outside the closed metal
            icosphere of the ico scenes, where no light arrives: DARK; inside tir's glass sphere: ONLY), dir uniform on the sphere
            with length 0.5 to 2, du and dv independent random directions of 0.05 to 0.5 times |dir|; about an eighth of the records
            have du = 0, an eighth dv = 0 and an eighth both; the reserved floats are NaN.  |du * rx + dv * ry| < |dir| for all draws, so
            no sample's direction vanishes.
equirect    pyhost/ray_image.equirect from a point inside the scene: a panorama whose jitter shrinks towards the poles.

What makes a frame of such a table a test of the record is `precondition`: the oracle's frame of the table differs, in at least HALF of
all pixels, from its frame of the same table with du / dv rolled by one record ("neighbour"), with the jitter zeroed ("zeroed") and with
du and dv exchanged ("exchanged") - a kernel that read another pixel's jitter, dropped it or swapped the draws would be caught by a
bit-for-bit comparison in at least that many pixels.  The cap is fixed; a table that does not reach it is changed, never the cap.

Measured with the oracle alone, depth 8: the share of pixels that differ, in per cent, under neighbour / zeroed / exchanged (a 1 x 1
image has no neighbour; a 1 x 1 panorama has du = 0 and dv parallel to dir, so its jitter cannot move the ray: no equirect table at 1 x 1).

  table      scene       size        4 spp: nb  zero  exch    64 spp: nb  zero  exch
  scrambled  cornell    1 x 1         - 100.0 100.0         - 100.0 100.0
  scrambled  cornell    7 x 9      73.0  66.7  65.1      73.0  68.3  68.3
  scrambled  cornell   20 x 13     78.5  68.5  69.6      81.2  71.9  71.9
  scrambled  cornell   64 x 48     75.4  66.4  65.9      78.4  68.9  68.8
  scrambled  cornell  130 x 3      80.3  67.2  68.5      82.3  69.5  69.5
  scrambled  cornell    3 x 130    73.1  62.6  63.3      74.6  64.6  64.6
  equirect   cornell    7 x 9      87.3  90.5  87.3      95.2  95.2  95.2
  equirect   cornell   20 x 13     86.5  88.8  87.7      90.0  90.0  90.0
  equirect   cornell   64 x 48     82.9  85.1  84.7      86.0  86.1  86.1
  equirect   cornell  130 x 3      86.7  91.0  90.8      91.5  91.3  91.5
  equirect   cornell    3 x 130    96.7  95.9  98.2     100.0 100.0 100.0
  scrambled  cube       1 x 1         - 100.0 100.0         - 100.0 100.0
  scrambled  cube       7 x 9      92.1  76.2  76.2     100.0  84.1  84.1
  scrambled  cube      20 x 13     92.3  81.9  81.9      97.7  86.5  86.5
  scrambled  cube      64 x 48     92.7  82.5  82.5      98.8  88.0  88.0
  scrambled  cube     130 x 3      94.1  80.8  80.8      98.2  84.4  84.4
  scrambled  cube       3 x 130    94.1  85.1  85.1      99.5  90.3  90.3
  equirect   cube       7 x 9     100.0 100.0 100.0     100.0 100.0 100.0
  equirect   cube      20 x 13    100.0 100.0 100.0     100.0 100.0 100.0
  equirect   cube      64 x 48    100.0 100.0 100.0     100.0 100.0 100.0
  equirect   cube     130 x 3     100.0 100.0 100.0     100.0 100.0 100.0
  equirect   cube       3 x 130   100.0 100.0 100.0     100.0 100.0 100.0
  scrambled  ico_map    1 x 1         - 100.0 100.0         - 100.0 100.0
  scrambled  ico_map    7 x 9      76.2  66.7  61.9      85.7  73.0  73.0
  scrambled  ico_map   20 x 13     78.1  61.9  60.0      83.1  70.0  68.1
  scrambled  ico_map   64 x 48     78.5  64.3  59.5      84.3  70.5  69.6
  scrambled  ico_map  130 x 3      77.4  64.6  62.3      83.6  69.5  68.5
  scrambled  ico_map    3 x 130    78.7  64.9  60.0      85.9  71.0  70.8
  equirect   ico_map    7 x 9      98.4 100.0 100.0     100.0 100.0 100.0
  equirect   ico_map   20 x 13     90.4  98.8  95.0      99.6 100.0  99.6
  equirect   ico_map   64 x 48     81.4  90.0  88.0      77.4  88.8  86.8
  equirect   ico_map  130 x 3      90.5  99.5  99.0      94.9 100.0 100.0
  equirect   ico_map    3 x 130    99.5  99.5  99.0     100.0 100.0 100.0

The guide pass (tests/aov_rays_common.py JITTER_CASES, asserted per case by its `precondition`): the same shares in the 8-float guide
buffers of tests/aov_rays_ref.py, the smallest over the case's (n_samples / max_follow) pairs named at the end of the line.  The first
scrambled table of tir, with origins anywhere in the inner box, reached 35 to 49 % only and 0 % at 1 x 1: see ONLY.

  table      scene          size          nb  zero  exch     n_samples / max_follow
  scrambled  mirror_wall    1 x 1         - 100.0 100.0     1/0 3/4 16/4
  scrambled  mirror_wall    7 x 9      96.8  84.1  84.1     1/0 3/4 16/4
  scrambled  mirror_wall   20 x 13     98.8  88.1  88.1     1/0 3/4 16/0 16/4
  scrambled  mirror_wall  130 x 3      98.7  87.4  87.2     1/0 3/4 16/4
  scrambled  mirror_wall    3 x 130    98.7  87.7  87.7     1/0 3/4 16/4
  scrambled  mirror_wall   64 x 48     98.6  87.5  87.5     1/4 3/0
  equirect   mirror_wall    7 x 9     100.0 100.0 100.0     1/0 3/4 16/4
  equirect   mirror_wall   20 x 13    100.0 100.0 100.0     1/0 3/4 16/0 16/4
  equirect   mirror_wall  130 x 3     100.0 100.0 100.0     1/0 3/4 16/4
  equirect   mirror_wall    3 x 130   100.0 100.0 100.0     1/0 3/4 16/4
  equirect   mirror_wall   64 x 48     99.9 100.0 100.0     1/4 3/0
  scrambled  tir            1 x 1         - 100.0 100.0     1/0 3/4 16/4
  scrambled  tir            7 x 9     100.0  88.9  88.9     1/0 3/4 16/4
  scrambled  tir           20 x 13     98.5  86.5  86.5     1/0 3/4 16/0 16/4
  scrambled  tir          130 x 3      96.2  82.6  82.6     1/0 3/4 16/4
  scrambled  tir            3 x 130    99.2  88.7  88.7     1/0 3/4 16/4
  scrambled  tir           64 x 48     98.5  88.0  88.0     1/4 3/0
  equirect   tir            7 x 9     100.0 100.0 100.0     1/0 3/4 16/4
  equirect   tir           20 x 13    100.0 100.0  99.6     1/0 3/4 16/0 16/4
  equirect   tir          130 x 3     100.0 100.0 100.0     1/0 3/4 16/4
  equirect   tir            3 x 130   100.0 100.0 100.0     1/0 3/4 16/4
  equirect   tir           64 x 48    100.0 100.0 100.0     1/4 3/0
  scrambled  cornell       20 x 13     88.1  78.8  78.8     3/4
  scrambled  cube          20 x 13     97.7  86.5  86.5     3/4

The environment decides how discriminating a scene is: under a constant environment every path that leaves the scene at the same bounce
with the same throughput gives the same radiance whatever its first direction was, so the cube (automatic environment: a gradient in
dir.y) and ico_map (a map) tell directions apart where they miss, Cornell where they hit."""
import numpy as np

import aov_follow_common as FC

F32 = np.float32
DTYPE = np.dtype([("org", "<f4", (3,)), ("reserved0", "<f4"), ("dir", "<f4", (3,)), ("reserved1", "<f4"),
                  ("du", "<f4", (3,)), ("reserved2", "<f4"), ("dv", "<f4", (3,)), ("reserved3", "<f4")])
SEED = 20261020
CAP = 0.5
_tables = {}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def box_of(flat):
    P = np.asarray(flat["positions"], np.float64).reshape(-1, 3)
    return P.min(0), P.max(0)


def scrambled_in_box(lo, hi, W, H, seed, dark=(), only=None):
    """The scrambled table of the module's docstring for the box [lo, hi], drawn from `seed` in a fixed order.  dark: (centre, radius)
    of balls no origin may lie in; an origin drawn inside one is drawn again.  only: (centre, radius) of the one ball every origin must
    lie in: the origins are uniform in the part of the inner box inside it (drawn in the ball's cube, clipped to the inner box, and
    drawn again while outside the ball)."""
    rng = np.random.default_rng(seed)
    n = W * H
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    t = np.zeros(n, DTYPE)
    if only is None:
        org = lo + (hi - lo) * (0.1 + 0.8 * rng.random((n, 3)))
    else:
        c, r = np.asarray(only[0], np.float64), float(only[1])
        blo, bhi = np.maximum(lo + 0.1 * (hi - lo), c - r), np.minimum(hi - 0.1 * (hi - lo), c + r)
        org = blo + (bhi - blo) * rng.random((n, 3))
        while True:
            outside = np.linalg.norm(org - c, axis=1) >= r
            if not outside.any():
                break
            org[outside] = blo + (bhi - blo) * rng.random((int(outside.sum()), 3))
    for c, r in dark:
        for _ in range(64):
            inside = np.linalg.norm(org - np.asarray(c, np.float64), axis=1) < r
            if not inside.any():
                break
            org[inside] = lo + (hi - lo) * (0.1 + 0.8 * rng.random((int(inside.sum()), 3)))
        assert not inside.any()
    t["org"] = org
    length = rng.uniform(0.5, 2.0, (n, 1))
    t["dir"] = _unit(rng, n) * length
    du = _unit(rng, n) * length * rng.uniform(0.05, 0.5, (n, 1))
    dv = _unit(rng, n) * length * rng.uniform(0.05, 0.5, (n, 1))
    kind = rng.integers(0, 8, n)  # 0: du = 0, 1: dv = 0, 2: both, 3..7: neither
    du[(kind == 0) | (kind == 2)] = 0.0
    dv[(kind == 1) | (kind == 2)] = 0.0
    t["du"], t["dv"] = du, dv
    for k in range(4):
        t["reserved%d" % k] = np.nan
    return t


# Where a scene is closed and lets no light in, a record cannot show anything: the inside of ico_map's metal icosphere (tests/aov_common.py:
# centre (1.2, -0.05, 0.15), radius 0.9) holds 23 % of the inner box and 98 % of the frames' pixels from there are black whatever the
# record says, which kept that scene's 4 spp frames below the cap (44 to 50 % under "exchanged").  No origin is drawn there.
DARK = {"ico_map": (((1.2, -0.05, 0.15), 0.9),), "ico_auto": (((1.2, -0.05, 0.15), 0.9),), "ico_colour": (((1.2, -0.05, 0.15), 0.9),)}
# A 1 x 1 image is one draw of a record, and one pixel either differs or does not: the draw (a further word of the seed) is the first
# whose record has du and dv both nonzero and whose pixel differs under "zeroed" and "exchanged" at 4 and at 64 spp in the oracle.
DRAW = {("cornell", 1, 1): 2}
# tir is a glass icosphere of radius 1 over a 12 x 12 floor under a constant environment: from nearly everywhere in that box a ray leaves
# without touching anything and its pixel is the environment whatever the record says - 35 to 49 % of the pixels told the tables apart.
# The origins lie inside the sphere (within 0.9 of its centre: inside every face of the icosphere), where every ray meets glass.
ONLY = {"tir": ((0.0, 0.0, 0.0), 0.9)}


def scrambled(name, W, H):
    """The scrambled table of scene `name` (tests/aov_common.py, tests/aov_follow_common.py) at W x H: one table per (name, W, H),
    read-only."""
    key = ("scrambled", name, W, H)
    if key not in _tables:
        lo, hi = box_of(FC.scene(name)["flat"])
        t = scrambled_in_box(lo, hi, W, H, [SEED, sum(map(ord, name)), W, H, DRAW.get((name, W, H), 0)], DARK.get(name, ()), ONLY.get(name))
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


# A point inside each scene from which the panorama sees it: inside the Cornell box, beside the cube, in front of the mirror wall, inside
# tir's glass sphere away from its centre.  ico_map's is inside the glass icosphere, away from its centre: from between the icospheres
# (first choice, (-0.05, 0.55, 0.6)) most pixels of a 64 x 48 panorama see one texel of the 16 x 8 environment map with all their samples and
# only 38 % of the 4 spp frame told the tables apart; through the glass every sample's direction shows in the throughput.
EQUIRECT_ORIGIN = {"cornell": (0.11, 0.93, 0.27), "cube": (1.7, 0.6, 1.3), "ico_map": (-1.0, 0.3, 0.2), "mirror_wall": (0.3, 0.2, 2.2), "tir": (0.35, 0.1, -0.2)}


def equirect(name, W, H):
    """pyhost/ray_image.equirect(EQUIRECT_ORIGIN[name], W, H) with the records' dtype of this module; read-only."""
    key = ("equirect", name, W, H)
    if key not in _tables:
        from owl_path_tracer_amd.pyhost import ray_image as RI

        t = np.ascontiguousarray(RI.equirect(EQUIRECT_ORIGIN[name], W, H), DTYPE)
        t.setflags(write=False)
        _tables[key] = t
    return _tables[key]


def table(kind, name, W, H):
    return {"scrambled": scrambled, "equirect": equirect}[kind](name, W, H)


def neighbour(t):
    """The table whose record i has the du / dv of record i - 1 (the last record's for record 0)."""
    r = t.copy()
    r["du"], r["dv"] = np.roll(t["du"], 1, axis=0), np.roll(t["dv"], 1, axis=0)
    return r


def zeroed(t):
    r = t.copy()
    r["du"] = 0.0
    r["dv"] = 0.0
    return r


def exchanged(t):
    r = t.copy()
    r["du"], r["dv"] = t["dv"], t["du"]
    return r


VARIANTS = (("neighbour", neighbour), ("zeroed", zeroed), ("exchanged", exchanged))


def differing_share(a, b):
    """The share of pixels of two (H, W, 3) float32 frames that differ in some bit."""
    return float((np.ascontiguousarray(a, F32).view(np.uint32) != np.ascontiguousarray(b, F32).view(np.uint32)).any(-1).mean())


def precondition(S, env, t, W, H, spp, depth, want=None):
    """{variant: share of differing pixels} of the oracle's frame of `t` (`want`, if the caller has it) against its frames of the three
    wrong tables, each asserted to reach CAP.  A 1 x 1 table has no neighbour: that variant is left out there."""
    if want is None:
        want = S.render_rays(t, env, W, H, spp, depth)[0]
    out = {}
    for what, f in VARIANTS:
        if what == "neighbour" and W * H == 1:
            continue
        out[what] = differing_share(want, S.render_rays(f(t), env, W, H, spp, depth)[0])
    for what, share in out.items():
        assert share >= CAP, "the frame of this table differs from the '%s' table's in %.1f %% of the pixels only: it could not tell them apart (%r)" % (what, 100 * share, out)
    return out
