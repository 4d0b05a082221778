"""The device's closest-hit walks refereed against exact geometry (tests/exact_hit.py; tests/test_exact_hit.py is the CPU half).

Op "closest_hit" and the six probe ops (the render kernel's own quad and group walks, both slab forms) through pt_debug_eval, builders
0 / 1 / 2 x leaf sizes 1 / 4 / 7, on the ten battery scenes: R1 (the reported hit is real), R2 (nothing certain was missed), R3
(decided rays have one answer) on EVERY ray - classes 8 and 9 and origins beyond 10 extents included, where test_gpu_ray_probes.py
can only count.  The referee's tables are computed once per scene and looked up 63 times.

The closed meshes of ray_battery.py (rays from strictly inside must hit, by geometry): the leak set - reported misses - of every op
equals the oracle's brute force's, and the rules hold; a leak is legal only where no triangle is certainly hit.

One image-level figure, measured: primary rays through the pixel centres of a small frame with the camera of
assets/configs/c4_dragon.json on the battery's REDUCED dragon stand-in (24 004 triangles; the full 871 k one is out of a numpy
referee's reach), op "quad".  Leaked = a certainly-hit triangle lies in front of the reported one by more than both bounds (zero, by
R2); possibly leaked = an open triangle does.

PT_WRITE_PROFILES=1 adds the section "gpu" to profiles/r08_exact_hit.json.
"""
import json
import os
import time

import numpy as np
import pytest

import exact_hit as X
import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B
from test_exact_hit import N_PER_CLASS, note_tightness, write_profile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = rb.scene_names()
BUILDERS = (0, 1, 2)
LEAVES = (1, 4, 7)
_report = {"rays_per_class_requested": N_PER_CLASS, "measured_on": "MI355X: op closest_hit and the six probe ops, builders 0 / 1 / 2, leaf sizes 1 / 4 / 7",
           "scenes": {}, "closed_meshes": {}, "tightness": {}}


def _launches(tris):
    """(label, op, answer rows) for the 63 launches on one scene."""
    for builder in BUILDERS:
        for leaf in LEAVES:
            ctx = B.Context(0)
            ctx.set_option("bvh_builder", builder)
            ctx.set_option("leaf_size", leaf)
            rb.upload(ctx, tris)
            if builder == 0 and leaf == 4:
                X.check_triangle_records(tris, ctx.export_trees()["tris"])

            def run(op, rays, ctx=ctx):
                return ctx.debug_eval(op, rays, 5 if op == "closest_hit" else 6)

            yield "builder %d leaf %d" % (builder, leaf), run
            ctx.close()


@pytest.mark.parametrize("name", SCENES)
def test_device_walks_obey_the_rules(orc, name):
    b = rb.referee_battery(orc, name, N_PER_CLASS)
    tris, rays, cls, T = b["tris"], b["rays"], b["cls"], b["tables"]
    assert set(rb.CLASSES) <= set(np.unique(cls))
    held = rb.bands(rays, rb.scene_measure(tris), cls)[0]
    dec = T.decided.astype(bool)
    assert dec[held & (cls == 1)].mean() >= 0.9 and dec[held].mean() >= 0.5, "too few decided rays: the rules would be vacuous"
    t0, n = time.time(), 0
    for label, run in _launches(tris):
        for op in ("closest_hit",) + B.PROBE_OPS:
            ans = X.answer_of_probe(run(op, rays))
            res = X.assert_rules(T, ans, "%s, %s, on %s" % (op, label, name), with_t=not op.startswith("group"), cls=cls)
            note_tightness(_report["tightness"], res, cls, ans[0])
            n += 1
    _report["scenes"][name] = dict(triangles=int(tris.shape[0]), rays=int(rays.shape[0]), rays_per_class=b["n"], launches=n, referee_s=round(b["seconds"], 1),
                                   launches_and_lookups_s=round(time.time() - t0, 1), decided_class1_inside=round(float(dec[held & (cls == 1)].mean()), 4),
                                   decided_all_inside=round(float(dec[held].mean()), 4))


@pytest.mark.parametrize("name", rb.closed_mesh_names())
def test_closed_meshes_leak_where_the_oracle_leaks(orc, name):
    tris, centre, half = rb.make_closed_mesh(name)
    S = rb.oracle_scene(orc, tris)
    sets = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(77), min(N_PER_CLASS, 2000))
    tables = {k: X.Tables(tris, r) for k, r in sets.items()}
    want = {k: S.intersect_n(r, use_bvh=False)[0] for k, r in sets.items()}
    assert all((rb.origin_extents(r, rb.scene_measure(tris)) <= rb.DOMAIN_EXTENTS).all() for r in sets.values()), "origins inside the domain"
    rec = _report["closed_meshes"][name] = dict(triangles=int(tris.shape[0]))
    for label, run in _launches(tris):
        for sname, rays in sets.items():
            for op in ("closest_hit",) + B.PROBE_OPS:
                ans = X.answer_of_probe(run(op, rays))
                res = X.assert_rules(tables[sname], ans, "%s, %s, on %s / %s" % (op, label, name, sname), with_t=not op.startswith("group"))
                note_tightness(_report["tightness"], res, np.full(rays.shape[0], 10 if sname == "random" else 11), ans[0])
                assert np.array_equal(ans[0], want[sname]), "%s, %s, on %s / %s: the leak set differs from the oracle's brute force's" % (op, label, name, sname)
                rec.setdefault(sname, {})[op] = [int((~ans[0]).sum()), int(rays.shape[0])]


def test_c4_primary_rays_possibly_leaked(orc):
    """Measured, not asserted - except that no ray may have leaked for certain (R2)."""
    with open(os.path.join(ROOT, "assets", "dragon.json")) as fh:
        c = json.load(fh)["camera"]
    W, H = 32, 24
    cam = B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H).as_array().astype(np.float64)
    origin, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    x, y = np.meshgrid((np.arange(W) + 0.5) / W, (np.arange(H) + 0.5) / H)
    target = llc + x.reshape(-1, 1) * hor + y.reshape(-1, 1) * ver
    rays = np.concatenate([np.tile(origin.astype(np.float32), (W * H, 1)), rb._unit32(target - origin)], 1).astype(np.float32)
    tris = rb.make_scene("dragon")
    t0 = time.time()
    T = X.Tables(tris, rays)
    ctx = B.Context(0)
    rb.upload(ctx, tris)
    ans = X.answer_of_probe(ctx.debug_eval("quad", rays, 6))
    ctx.close()
    X.assert_rules(T, ans, "quad on the primary rays of the reduced dragon stand-in")
    hit = ans[0]
    pos = T.lookup(np.where(hit, ans[4], -1))
    rep_lo = np.where(hit, T.t[np.maximum(pos, 0)] - T.et[np.maximum(pos, 0)], np.inf)
    rep_lo = np.where(np.isnan(rep_lo), -np.inf, rep_lo)
    leaked = T.cert_hi < rep_lo
    # an open triangle in front of the reported one by more than both bounds (on a miss: any open triangle), or one whose t has no bound
    with np.errstate(all="ignore"):
        front = ~T.cert.astype(bool) & ((T.t + T.et < rep_lo[T.ray_of]) & (T.t - T.et > X.K_TMIN) | ~np.isfinite(T.et))
    possibly = np.zeros(rays.shape[0], bool)
    possibly[T.ray_of[front]] = True
    assert not leaked.any()
    _report["c4_primary_rays"] = dict(scene="reduced dragon stand-in (ray_battery 'dragon')", triangles=int(tris.shape[0]), frame=[W, H], rays=int(rays.shape[0]), op="quad",
                                      hits=int(hit.sum()), leaked=int(leaked.sum()), possibly_leaked=int(possibly.sum()), possibly_leaked_share=round(float(possibly.mean()), 6),
                                      decided=round(float(T.decided.mean()), 4), seconds=round(time.time() - t0, 1))
    print(_report["c4_primary_rays"])


def test_zz_write_profile():
    if len(_report["scenes"]) == len(SCENES):
        t = _report["tightness"]
        _report["tightness_max"] = max(t.values()) if t else 0.0
        write_profile("gpu", _report)
