"""The hierarchies the walks run on, and the claim that carries them: "boxes only have to be conservative" (DESIGN 2.1).  No GPU.

Three layers, on the scenes and the ray battery of tests/ray_battery.py (shared with tests/test_gpu_ray_probes.py):

* STRUCTURE of the binary, quad and oct arrays read back with pt_debug_export_tree: every triangle in exactly one leaf of each tree,
  every child referenced once and in range, every slot's box around ALL vertices below it with the full pad, quad / oct boxes taken
  from the binary tree, depth fields equal to the measured depths (the stack bounds 3 * depth4 + 1 and 7 * depth8 + 1 rest on them).
* SLAB-TEST CONSERVATIVENESS, EMULATED: for every (ray, triangle) pair where the oracle's brute force reports that triangle as the
  closest hit, every box on the way from the root to the triangle's leaf must pass the product's slab test - in float32 numpy, both
  forms, octant-ordered (quad walk) and min / max (binary, group walk), for the correctly rounded reciprocal and its two neighbours
  (v_rcp_f32 is within 1 ulp), clamped as ray_inv clamps, with the hit's own t as the bound.  Asserted on the domain on which the
  closest hit is defined (origins within 10 extents: ray_battery.py origin_extents); culled boxes beyond it are counted.
* THE DEFINITION: oracle BVH walk == oracle brute force == closest_hit_host (the product's binary tree walked on the host), hit and
  id equal, t, u, v bit for bit, zero mismatches on every class, on that domain (the far-origin class reaches beyond it, classes 8
  and 9 - coplanar rays, grazing below 1e-2 rad - lie outside it: counted).

PT_WRITE_PROFILES=1 writes the measured margins and counts to profiles/r06_slab_margins.json (run once; the file is committed).
~50 s on 8 threads (2 000 rays per class and scene, ~21 000 rays per scene; PT_PROBE_RAYS=N for more).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = rb.scene_names()
CONFIGS = [(1, 1), (4, 1), (7, 1), (1, 0), (4, 0), (7, 0)]  # (leaf_size, wide_leaves)
N_PER_CLASS = int(os.environ.get("PT_PROBE_RAYS", "2000"))
_cache = {}


def _host_ctx(tris, leaf, wide):
    ctx = B.Context(-1)
    ctx.set_option("leaf_size", leaf)
    ctx.set_option("wide_leaves", wide)
    rb.upload(ctx, tris)
    return ctx


def _battery(orc, name):
    """Scene, rays, classes and the brute-force truth, once per scene."""
    if name not in _cache:
        tris = rb.make_scene(name)
        S = rb.oracle_scene(orc, tris)
        ctx = _host_ctx(tris, 4, 1)
        ex = ctx.export_trees()
        t4 = rb.trees_of(ex)[1]
        used = t4.ref != -1
        planes = np.stack([t4.lo[used], t4.hi[used]], 1) if t4.n_nodes else None
        rays, cls = rb.make_rays(tris, np.random.default_rng(4242), N_PER_CLASS, planes=planes, hit_fn=lambda r: S.intersect_n(r, use_bvh=True)[:2])
        t0 = time.time()
        truth = S.intersect_n(rays, use_bvh=False)
        _cache[name] = dict(tris=tris, S=S, rays=rays, cls=cls, truth=truth, pad=ex["pad"], brute_s=time.time() - t0)
        ctx.close()
    return _cache[name]


def _mismatches(a, b):
    """Rays on which two (hit, t, u, v, id) results differ: hit and id equal, t, u, v bit for bit where hit."""
    hit = a[0]
    bad = (a[0] != b[0]) | (a[4] != b[4])
    for k in (1, 2, 3):
        bad |= hit & (a[k].view(np.uint32) != b[k].view(np.uint32))
    return np.nonzero(bad)[0]


@pytest.mark.parametrize("name", SCENES)
def test_tree_structure(name):
    tris = rb.make_scene(name)
    for leaf, wide in CONFIGS:
        ctx = _host_ctx(tris, leaf, wide)
        ex = ctx.export_trees()
        info = rb.check_structure(ex, wide)
        q, o = ctx.quad_info(), ctx.oct_info()
        assert info["quad"]["nodes"] == q["quad_nodes"] and info["oct"]["nodes"] == o["oct_nodes"]
        assert ex["max_leaf"] <= leaf and ex["tris"].size >= tris.shape[0]
        ctx.close()


def test_export_rejects_small_buffers_and_unknown_arrays():
    import ctypes as C

    ctx = _host_ctx(rb.make_scene("rects"), 4, 1)
    L = B.lib()
    need = L.pt_debug_export_tree(ctx._h, 1, None, 0)
    assert need > 0 and need % 128 == 0
    buf = (C.c_uint8 * int(need))()
    assert L.pt_debug_export_tree(ctx._h, 1, buf, need - 1) == -1  # PT_E_INVALID
    assert L.pt_debug_export_tree(ctx._h, 1, buf, need) == need
    assert L.pt_debug_export_tree(ctx._h, 9, None, 0) == -1
    empty = B.Context(-1)
    assert L.pt_debug_export_tree(empty._h, 0, None, 0) == -4  # PT_E_NO_SCENE


@pytest.mark.parametrize("name", SCENES)
def test_closest_hit_definition(orc, name):
    """Oracle BVH walk (leaf sizes 1, 4, 7) and closest_hit_host (leaf sizes 1, 4, 7) against the oracle's brute force: zero mismatches."""
    b = _battery(orc, name)
    rays, cls, truth = b["rays"], b["cls"], b["truth"]
    assert set(rb.CLASSES) <= set(np.unique(cls)), "every class of the battery is drawn"
    assert 0.02 < truth[0].mean() < 0.999 or name in ("one_leaf", "soup1"), "the battery both hits and misses"
    held, mid, far = rb.bands(rays, rb.scene_measure(b["tris"]), cls)
    copl = np.isin(cls, rb.OUTSIDE)
    assert held.sum() > 0.8 * held.size
    referee = exact_hit.OnDemand(b["tris"], rays)  # for the counted mismatches: they may differ, but only between two admissible hits
    for leaf in (1, 4, 7):
        S = b["S"] if leaf == 4 else rb.oracle_scene(orc, b["tris"], leaf_size=leaf)
        ctx = _host_ctx(b["tris"], leaf, 1)
        for who, got in (("oracle BVH walk", S.intersect_n(rays, use_bvh=True)), ("closest_hit_host", ctx.closest_hit_host_n(rays))):
            m = np.zeros(rays.shape[0], bool)
            m[_mismatches(truth, got)] = True
            rec = _outside.setdefault(who, [0, 0, 0, 0, 0, 0])  # [mismatches, rays] at 10-42 extents, beyond 42, rays of classes 8 / 9
            for k, band in ((0, mid), (2, far), (4, copl)):
                rec[k] += int((m & band).sum())
                rec[k + 1] += int(band.sum())
            for whose, ans in ((who, got), ("brute force", truth)):
                wrong = referee.inadmissible(np.nonzero(m & ~held)[0], ans)
                assert wrong.size == 0, "%s (leaf %d) and brute force differ outside the domain and %s's answer breaks R1 or R2 of tests/exact_hit.py on %d rays; first: class %d %r" % (
                    who, leaf, whose, wrong.size, cls[wrong[0]], rays[wrong[0]].tolist())
            bad = np.nonzero(m & held)[0]
            assert bad.size == 0, "%s (leaf %d) differs from brute force on %d rays; first: class %d %r" % (who, leaf, bad.size, cls[bad[0]], rays[bad[0]].tolist())
        ctx.close()


_outside = {}
_margins = {}


@pytest.mark.parametrize("name", SCENES)
def test_slab_tests_pass_every_box_on_the_way_to_the_closest_hit(orc, name):
    b = _battery(orc, name)
    rays, cls, (hit, t, _, _, prim) = b["rays"], b["cls"], b["truth"]
    sel = np.nonzero(hit)[0]
    o, d, tb, c = rays[sel, :3], rays[sel, 3:], t[sel], cls[sel]
    invs = rb.ray_inv_variants(d)
    failures = []
    n_pairs = 0
    for leaf, wide in CONFIGS:
        ctx = _host_ctx(b["tris"], leaf, wide)
        ex = ctx.export_trees()
        ctx.close()
        held, mid, far = rb.bands(rays[sel], rb.scene_measure(b["tris"]), c)
        # the bound of the emulation is the hit's own t, and t = (in-plane placement error) / sin(grazing angle) off: below 1e-2 it is not
        # a usable bound (the real walks carry the best t so far, not this one) - counted by decade instead
        sg = rb.sin_grazing(rays[sel], b["tris"][prim[sel]])
        held = held & (sg >= rb.MIN_SIN_GRAZING)
        graz = [(sg < 1e-4) & ~far & ~mid, (sg >= 1e-4) & (sg < 1e-3) & ~far & ~mid, (sg >= 1e-3) & (sg < 1e-2) & ~far & ~mid]
        slot_of_id = np.full(ex["tris"].size, -1, np.int64)
        real = ex["tris"]["id"] != 0x7fffffff
        slot_of_id[ex["tris"]["id"][real]] = np.nonzero(real)[0]
        tslot = slot_of_id[prim[sel]]
        for T in rb.trees_of(ex):
            if T.n_nodes == 0 or (T.name != "oct" and wide == 0):  # wide_leaves only changes the oct nodes
                continue
            paths = rb.TreePaths(T, ex["tris"].size)
            for lvl in paths.levels(tslot):
                on = lvl >= 0
                n_pairs += int(on.sum())
                for exact in (0, 1):
                    for ulp, inv in zip((-1, 0, 1), invs):
                        ok, margin = rb.slab_margin(T.lo[lvl[on]], T.hi[lvl[on]], o[on], inv[on], tb[on], bool(exact), T.name == "quad")
                        claimed = held[on]
                        for k in np.unique(c[on]):
                            key = ("exact" if exact else "fma", int(k))
                            m = (c[on] == k) & claimed
                            rec = _margins.setdefault(key, dict(min_margin_ulps=float("inf"), boxes=0, culled_at_10_to_42_extents=0, boxes_at_10_to_42_extents=0, culled_beyond_42_extents=0, boxes_beyond_42_extents=0,
                                                         culled_sin_below_1e_4=0, boxes_sin_below_1e_4=0, culled_sin_1e_4_to_1e_3=0, boxes_sin_1e_4_to_1e_3=0, culled_sin_1e_3_to_1e_2=0, boxes_sin_1e_3_to_1e_2=0))
                            if m.any():
                                rec["min_margin_ulps"] = min(rec["min_margin_ulps"], float(margin[m].min()))
                                rec["boxes"] += int(m.sum())
                            for tag, band in (("at_10_to_42_extents", mid[on]), ("beyond_42_extents", far[on]), ("sin_below_1e_4", graz[0][on]), ("sin_1e_4_to_1e_3", graz[1][on]), ("sin_1e_3_to_1e_2", graz[2][on])):
                                out = (c[on] == k) & band
                                rec["culled_" + tag] += int((~ok[out]).sum())
                                rec["boxes_" + tag] += int(out.sum())
                        bad = np.nonzero(~ok & claimed)[0]
                        if bad.size:
                            i = np.nonzero(on)[0][bad[0]]
                            failures.append("%s tree, leaf %d, wide %d, %s form, rcp %+d ulp: %d boxes culled; first: class %d ray %r t %r" %
                                            (T.name, leaf, wide, "subtracting" if exact else "fma", ulp, bad.size, c[i], rays[sel[i]].tolist(), float(tb[i])))
    assert not failures, "\n".join(failures[:20])
    assert n_pairs > 0 or not hit.any()
    if os.environ.get("PT_WRITE_PROFILES") == "1" and name == SCENES[-1]:
        doc = {"what": "smallest margin (exit distance x 1.0000004 - entry distance, in float32 ulps of the exit distance) of the emulated slab tests over every box "
                       "between the root and the closest hit's leaf; reciprocal at -1 / 0 / +1 ulp; all scenes, leaf sizes 1 / 4 / 7, three trees",
               "fma_note": "the fma is emulated as a float64 product-sum rounded to float32 (two roundings)",
               "rays_per_class_and_scene": N_PER_CLASS, "scenes": SCENES,
               "by_form_and_class": {"%s/%d %s" % (f, k, rb.CLASSES.get(k) or rb.OUTSIDE_NAMES[k]): dict(v, min_margin_ulps=v["min_margin_ulps"] if np.isfinite(v["min_margin_ulps"]) else None)
                                     for (f, k), v in sorted(_margins.items())},
               "definition_mismatches_outside_the_domain [at 10-42 extents, rays, beyond 42, rays, coplanar, rays]": _outside,
               "brute_force_seconds": {n: round(_cache[n]["brute_s"], 1) for n in _cache}}
        with open(os.path.join(ROOT, "profiles", "r06_slab_margins.json"), "w") as fh:
            json.dump(doc, fh, indent=1)
