"""What tests/test_trace_hits_host.py (CPU) and tests/test_gpu_trace_hits.py (GPU) share: the cases of pt_trace_hits - the scenes of the
ray battery with its rays, and small constructed scenes - each with the chains of tests/hits_ref.py for its compared rays, computed once
per process and never changed.

CONSTRUCTED SCENES
  stack          20 parallel unit quads (40 triangles) at z = 1, 1.5, ..., 10.5 and rays across them: straight ones, which cross all 20 -
                 K = 16 cuts their list - and tilted ones, which leave the stack through its side after fewer.
  stack_doubled  the same stack with every second quad stored twice with identical vertices, the copy right behind the original: the
                 copy of triangle id has id + 2, and t, u, v bit-equal to the original's.  doubled_expectation() builds the whole list of
                 a ray from its chain by that construction.
Both carry, behind the 240 rays across, the bounds of the definition on ray 0 (a straight ray): tmax exactly the t of its third quad (in
the plain stack: its 3rd hit, kept), nextafter(t, 0) (gone), NaN, +inf, -1, 1e-3, and exactly the t of its second quad - in the doubled
stack a tie AT the bound, both partners kept."""
import numpy as np

import hits_ref
import ray_battery as rb
import trace_rays_common as TC
from owl_path_tracer_amd.pyhost import binding as B

KS = (1, 2, 3, 4, 16)       # the host test's K; 3: not a power of two, 16: PT_HITS_MAX
GPU_KS = (1, 3, 16)
N_QUADS, N_ACROSS = 20, 240
CONSTRUCTED = ("stack", "stack_doubled")
_cache = {}


def stack_scene(doubled):
    """((n, 3, 3) triangles, ids of the triangles that have a copy at id + 2)."""
    tris, has_copy = [], []
    for q in range(N_QUADS):
        z = 1.0 + 0.5 * q
        p = np.float32([[-1, -1, z], [1, -1, z], [1, 1, z], [-1, 1, z]])
        quad = [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
        if doubled and q % 2 == 1:
            has_copy += [len(tris), len(tris) + 1]
            tris += quad
        tris += quad
    return np.asarray(tris, np.float32), np.asarray(has_copy, np.int32)


def stack_rays(S):
    """pt_ray records: N_ACROSS rays across the stack from z = 0 (every third straight along +z, the others tilted by up to 0.35 in x and
    y), then seven copies of ray 0 with the bounds of the module docstring; (records, index of the first bound ray)."""
    rng = np.random.default_rng(2030)
    org = np.concatenate([rng.uniform(-0.9, 0.9, (N_ACROSS, 2)), np.zeros((N_ACROSS, 1))], 1)
    tilt = rng.uniform(-0.35, 0.35, (N_ACROSS, 2)) * (np.arange(N_ACROSS) % 3 != 0)[:, None]
    rays = np.concatenate([org, tilt, np.ones((N_ACROSS, 1))], 1).astype(np.float32)
    rec = B.make_rays(np.concatenate([rays, np.repeat(rays[:1], 7, 0)]))
    levels = hits_ref.chain(S, rays[0, :3], rays[0, 3:], np.inf)[:, 0].view(np.float32)
    rec["tmax"][N_ACROSS:] = [levels[2], np.nextafter(levels[2], np.float32(0)), np.nan, np.inf, -1.0, 1e-3, levels[1]]
    return rec, N_ACROSS


def case(orc, name):
    """dict(tris, rec (pt_ray records), mask (the compared rays), idx (their indices), chain, length (hits_ref.chains of rec[idx]),
    real (hits_ref.Real); constructed scenes: has_copy, bounds (index of the first bound ray))."""
    if name not in _cache:
        c = {}
        if name in CONSTRUCTED:
            c["tris"], c["has_copy"] = stack_scene(name == "stack_doubled")
            S = rb.oracle_scene(orc, c["tris"])
            c["rec"], c["bounds"] = stack_rays(S)
            c["mask"] = np.ones(c["rec"].shape[0], bool)
        else:
            bt = TC.battery(orc, name)
            S = bt["S"]
            c["tris"], c["rec"], c["mask"] = bt["tris"], B.make_rays(bt["rays"]), bt["mask"]  # tmax = +inf
        c["idx"] = np.nonzero(c["mask"])[0]
        c["chain"], c["length"] = hits_ref.chains(S, c["rec"], c["idx"])
        c["real"] = hits_ref.Real(orc, c["tris"])
        c["rec"].setflags(write=False)
        _cache[name] = c
    return _cache[name]


def names():
    return list(rb.scene_names()) + list(CONSTRUCTED)


def assert_rule(c, lists, what):
    """The rule of tests/hits_ref.py on the compared rays of case c; lists: (n, K) records of ALL its rays."""
    hits_ref.assert_lists(lists[c["idx"]], c["chain"], c["length"], c["rec"][c["idx"]], c["real"], what)


def doubled_expectation(c, K):
    """The lists of the stack_doubled case by construction: every level of a ray's chain, followed by its copy (id + 2, the same t, u, v)
    where the triangle has one, cut at K.  (A chain stops at hits_ref.LEVELS > K levels: enough for the first K entries.)"""
    n = c["rec"].shape[0]
    want = np.zeros((n, K), B.HIT_DTYPE)
    want["prim"] = -1
    for i in range(n):
        out = []
        for lv in c["chain"][i, :c["length"][i]]:
            e = (lv[0:1].view(np.float32)[0], lv[1:2].view(np.float32)[0], lv[2:3].view(np.float32)[0], int(lv[3:4].view(np.int32)[0]))
            out.append(e)
            if e[3] in c["has_copy"]:
                out.append(e[:3] + (e[3] + 2,))
        for j, e in enumerate(out[:K]):
            want[i, j] = e
    return want


def same_lists(a, b):
    """Per ray: all K * 16 bytes equal."""
    return (np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1) == np.ascontiguousarray(b).view(np.uint8).reshape(b.shape[0], -1)).all(1)


def assert_same_lists(got, want, mask, what, rec=None):
    ok = same_lists(got, want) | (~mask if mask is not None else False)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError("%s: %d of %d lists differ; first: ray %d\n got  %r\n want %r%s" % (what, int((~ok).sum()), got.shape[0], i, got[i], want[i],
                                                                                                  "" if rec is None else "\n ray %r" % rec[i]))
