"""Rays handed to the walks the product runs, checked one by one against brute force.

The probe ops of pt_debug_eval (include/mi355pt.h, ops 30..35) send caller-chosen rays through the render kernel's own device
functions: ray_inv -> node4_step -> leaf_test with the whole stack in LDS ("quad") and with the short LDS stack + HBM overflow column
("quad_ovf"), and traverse_groups itself ("group": oct nodes, eight lanes per ray, 100 rays per wave in 24 slots, groups parked and
resumed), each in the fma and in the subtracting slab form.  Every op x builders 0 (host SAH), 1 (device LBVH), 2 (device PLOC) x
leaf sizes 1, 4, 7 on the scenes and the ray battery of tests/ray_battery.py; truth is the oracle's brute force over all triangles,
and EVERY ray is compared with it (no stride, no share): hit and id equal, t, u, v bit for bit (the group walk does not carry t: u,
v, id).  That bar holds on the domain on which the closest hit is defined at all - origins within 10 extents, ray_battery.py
origin_extents and DESIGN 2.1; beyond it, and for the battery's classes 8 / 9 (rays coplanar with a general triangle to rounding, grazing an edge below 1e-2 rad),
brute force and the oracle's OWN hierarchy disagree - and mismatches there are counted
per op (10-42 extents, where the product still uses the fma form, and beyond 42) and recorded, not asserted.  Also: the structure checks of test_tree_structure.py on the device-built trees, every probe against the old lane-per-pixel
"closest_hit" op and against closest_hit_host, and that the overflow column and the park area really were used.

Default size: 2 000 rays per class, ~21 000 rays per scene, ten scenes, 63 launches each: 9.5 s for this file on an MI355X box with
16 host threads (tests/test_gpu_fuzz.py: ~15 s).  PT_PROBE_RAYS=N for a larger sweep, PT_WRITE_PROFILES=1 records counts and times in
profiles/r06_ray_probes.json: run once with 10 000 (1.03 M rays, 13.5 s) - no mismatch inside the domain in any of the 54 (op,
builder, leaf size) combinations per scene, none at 10-42 extents, 31 (quad) / 18 (group) of 252 000 beyond 42 extents.
Every counted mismatch outside the domain must lie between two admissible hits: both answers satisfy R1 and R2 of tests/exact_hit.py.
"""
import json
import os
import time

import numpy as np
import pytest

import exact_hit
import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = rb.scene_names()
BUILDERS = (0, 1, 2)
LEAVES = (1, 4, 7)
N_PER_CLASS = int(os.environ.get("PT_PROBE_RAYS", "2000"))
_report = {"rays_per_class": N_PER_CLASS, "scenes": {}, "mismatches_outside_the_domain": {}}


def _truth(orc, tris):
    S = rb.oracle_scene(orc, tris)
    host = B.Context(-1)
    rb.upload(host, tris)
    t4 = rb.trees_of(host.export_trees())[1]
    used = t4.ref != -1
    planes = np.stack([t4.lo[used], t4.hi[used]], 1) if t4.n_nodes else None
    rays, cls = rb.make_rays(tris, np.random.default_rng(4242), N_PER_CLASS, planes=planes, hit_fn=lambda r: S.intersect_n(r, use_bvh=True)[:2])
    t0 = time.time()
    truth = S.intersect_n(rays, use_bvh=False)
    return rays, cls, truth, host, time.time() - t0


def _bad(truth, out, with_t):
    hit, t, u, v, prim = truth
    got_hit = out[:, 0] != 0
    bad = (got_hit != hit) | (out[:, 4].copy().view(np.int32) != prim)
    for k, want in ((1, t), (2, u), (3, v)):
        if k == 1 and not with_t:
            continue
        bad |= hit & (np.ascontiguousarray(out[:, k]).view(np.uint32) != want.view(np.uint32))
    return bad


@pytest.mark.parametrize("name", SCENES)
def test_probes_against_brute_force(orc, name):
    tris = rb.make_scene(name)
    rays, cls, truth, host, brute_s = _truth(orc, tris)
    assert set(rb.CLASSES) <= set(np.unique(cls))
    # the third witness, without a GPU in it: the product's binary tree walked on the host
    hh = host.closest_hit_host_n(rays)
    inside = rb.bands(rays, rb.scene_measure(tris), cls)[0]
    assert not (_bad(truth, np.stack([hh[0].astype(np.float32), hh[1], hh[2], hh[3], hh[4].view(np.float32)], 1), True) & inside).any()
    host.close()
    t_gpu = 0.0
    max_sp, parks = 0, 0
    referee = exact_hit.OnDemand(tris, rays)  # for the counted mismatches: they may differ, but only between two admissible hits
    for builder in BUILDERS:
        for leaf in LEAVES:
            ctx = B.Context(0)
            ctx.set_option("bvh_builder", builder)
            ctx.set_option("leaf_size", leaf)
            rb.upload(ctx, tris)
            ex = ctx.export_trees()
            rb.check_structure(ex)  # on the tree this builder made
            held, mid, far = rb.bands(rays, rb.scene_measure(tris), cls)
            assert abs(float(ex["pad"]) / (1e-5 * rb.scene_measure(tris)) - 1.0) < 1e-5, "pad = 1e-5 x max(extent, max |coordinate|)"
            copl = np.isin(cls, rb.OUTSIDE)
            t0 = time.time()
            old = ctx.debug_eval("closest_hit", rays, 5)
            b = _bad(truth, old, True) & held
            assert not b.any(), "closest_hit, builder %d leaf %d: %d rays differ; first: class %d %r" % (builder, leaf, b.sum(), cls[b][0], rays[b][0].tolist())
            for op in B.PROBE_OPS:
                out = ctx.debug_eval(op, rays, 6)
                group, exact = op.startswith("group"), op.endswith("exact")
                b = _bad(truth, out, not group)
                rec = _report["mismatches_outside_the_domain"].setdefault("%s/%s" % (name, op), [0, 0, 0, 0, 0, 0])
                for k, m in ((0, mid), (2, far), (4, copl)):  # [mismatches, rays] at 10-42 extents, beyond 42, classes 8 / 9
                    rec[k] += int((b & m).sum())
                    rec[k + 1] += int(m.sum())
                out_idx = np.nonzero(b & ~held)[0]
                for who, ans in ((op, exact_hit.answer_of_probe(out)), ("brute force", truth)):
                    wrong = referee.inadmissible(out_idx, ans, with_t=not group or who != op)
                    assert wrong.size == 0, "%s and brute force differ outside the domain (%s, builder %d leaf %d) and %s's answer breaks R1 or R2 of tests/exact_hit.py on %d rays; first: class %d %r" % (
                        op, name, builder, leaf, who, wrong.size, cls[wrong[0]], rays[wrong[0]].tolist())
                bh = b & held
                print("%s builder %d leaf %d %-14s mismatches %d of %d held; 10-42 extents %d of %d; beyond %d of %d" % (name, builder, leaf, op, bh.sum(), held.sum(), (b & mid).sum(), mid.sum(), (b & far).sum(), far.sum()))
                assert not bh.any(), "%s, builder %d leaf %d: %d of %d rays differ from brute force; first: class %d %r got %r want %r" % (
                    op, builder, leaf, bh.sum(), held.sum(), cls[bh][0], rays[bh][0].tolist(), out[bh][0].tolist(), [float(x[bh][0]) for x in truth])
                # ... and with the lane-per-pixel walk, bit for bit
                same = (out[held][:, [0, 2, 3, 4]].view(np.uint32) == old[held][:, [0, 2, 3, 4]].view(np.uint32)).all()
                assert same, op
                if op.startswith("quad_ovf"):
                    max_sp = max(max_sp, int(out[:, 5].max()))
                if group:
                    parks = max(parks, int(out[:, 5].max()))
            t_gpu += time.time() - t0
            ctx.close()
    if rays.shape[0] > 2 * 24:
        assert parks > 0, "no group phase of the group probe ended with parked groups"
    _report["scenes"][name] = dict(triangles=int(tris.shape[0]), rays=int(rays.shape[0]), brute_force_s=round(brute_s, 2), probes_s=round(t_gpu, 2),
                                   deepest_stack_entry=max_sp, parked_phases_max=parks)
    if os.environ.get("PT_WRITE_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "r06_ray_probes.json"), "w") as fh:
            json.dump(_report, fh, indent=1)


def test_overflow_column_is_really_used(orc):
    """The sliver strip's quad tree needs more stack than the LDS part holds (read-back depth), and rays along the strip push past it."""
    tris = rb.make_scene("strip")
    ctx = B.Context(0)
    ctx.set_option("leaf_size", 1)
    rb.upload(ctx, tris)
    ex = ctx.export_trees()
    assert 3 * ex["depth4"] + 1 > B.PT_LDS_STACK
    rng = np.random.default_rng(5)
    n = 4000  # rays that run the length of the strip just above / through it: every box along it is hit
    o = np.stack([rng.uniform(-2, 0, n), rng.uniform(0, 1e-3, n), rng.uniform(-1e-4, 1e-4, n)], 1).astype(np.float32)
    d = rb._unit32(np.stack([np.ones(n), rng.normal(0, 1e-6, n), rng.normal(0, 1e-5, n)], 1))
    rays = np.concatenate([o, d], 1)
    S = rb.oracle_scene(orc, tris)
    truth = S.intersect_n(rays, use_bvh=False)
    for op in ("quad_ovf", "quad_ovf_exact", "quad", "quad_exact"):
        out = ctx.debug_eval(op, rays, 6)
        assert not _bad(truth, out, True).any(), op
        print(op, "deepest stack entry", out[:, 5].max())
        assert out[:, 5].max() > B.PT_LDS_STACK, "%s: no push went past LDS entry %d (deepest %d)" % (op, B.PT_LDS_STACK, out[:, 5].max())
    ctx.close()


def test_probe_ops_refuse_what_they_cannot_do():
    ctx = B.Context(0)
    with pytest.raises(B.PtError):
        ctx.debug_eval("quad", np.zeros((4, 6), np.float32), 6)  # no scene
    rb.upload(ctx, rb.make_scene("rects"))
    with pytest.raises(B.PtError):
        ctx.debug_eval("quad", np.zeros((4, 6), np.float32), 5)  # six floats out
    with pytest.raises(B.PtError):
        ctx.debug_eval(36, np.zeros((4, 6), np.float32), 6)
    ctx.close()
