"""Every closest-hit walk that runs without a GPU, refereed against exact geometry (tests/exact_hit.py).  No GPU.

Until here every geometric truth of this suite was float32 Moeller-Trumbore written twice (csrc/pt_trace.h, oracle/pt_oracle.c).  The
referee evaluates each (ray, triangle) pair in float64 with a derived bound on what the float32 sequence may return, decides exact
zeros in rational arithmetic, and asserts three rules on EVERY ray of the battery of tests/ray_battery.py - all classes, 8 and 9
included, all bands, far origins included:

R1 the reported hit is real, R2 nothing certain was missed, R3 decided rays have one answer (exact_hit.py states them).

* the ten battery scenes: the oracle's brute force, the oracle's walk and closest_hit_host at leaf sizes 1 / 4 / 7.  The share of
  DECIDED rays is a condition, not a statistic (R1 / R2 are vacuous where the bounds are infinite): at least 0.9 of the class-1 rays
  and at least 0.5 of all rays inside the domain, on every scene.  The triangle records the product holds are the input triangles
  or points, the latter exactly where the sliver rule says so.
* closed meshes with shared float32 vertices (a box, icospheres of 320 and 1 280 triangles, one 4 extents off the origin), rays from
  strictly inside, random and aimed at shared edges / vertices: exact geometry says every ray hits.  The triangle test is not
  watertight, so LEAKS (reported misses) are counted, not asserted to be zero; they are legal only where no triangle is certainly hit
  (R2), and the walk's leak set must equal brute force's.
* the referee bites: a float32 numpy restatement of tri_eval + brute force passes, five deliberately wrong variants of it each
  violate a rule.
* tightness: the largest |float32 - exact| / bound per quantity and class (<= 1 by R1) is recorded.

The referee visits every pair in numpy (~1 us each): PT_PROBE_RAYS per class on small scenes, fewer on large ones
(ray_battery.referee_rays_per_class), never fewer than every class.  PT_WRITE_PROFILES=1 records the figures in
profiles/r08_exact_hit.json (section "cpu"; tests/test_gpu_exact_hit.py adds "gpu").
"""
import json
import os

import numpy as np
import pytest

import exact_hit as X
import ray_battery as rb
from owl_path_tracer_amd.pyhost import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r08_exact_hit.json")
SCENES = rb.scene_names()
N_PER_CLASS = int(os.environ.get("PT_PROBE_RAYS", "2000"))
LEAVES = (1, 4, 7)
_report = {"rays_per_class_requested": N_PER_CLASS, "measured_on": "CPU: the oracle (brute force, walk) and closest_hit_host", "scenes": {}, "closed_meshes": {}, "tightness": {}}


def write_profile(section, doc):
    if os.environ.get("PT_WRITE_PROFILES") != "1":
        return
    whole = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            whole = json.load(fh)
    whole[section] = doc
    with open(PROFILE, "w") as fh:
        json.dump(whole, fh, indent=1, sort_keys=True)


def band_masks(rays, cls, tris):
    held, mid, far = rb.bands(rays, rb.scene_measure(tris), cls)
    return (("inside", held), ("10_to_42_extents", mid), ("beyond_42_extents", far), ("classes_8_9", np.isin(cls, rb.OUTSIDE)))


def decided_shares(tables, rays, cls, tris):
    """{class: {band: [decided, rays]}} and the two conditions of the issue."""
    out = {}
    dec = tables.decided.astype(bool)
    for c in sorted(int(x) for x in np.unique(cls)):
        for bn, band in band_masks(rays, cls, tris):
            m = (cls == c) & band
            if m.any():
                out.setdefault(str(c), {})[bn] = [int(dec[m].sum()), int(m.sum())]
    held = band_masks(rays, cls, tris)[0][1]
    return out, float(dec[held & (cls == 1)].mean()), float(dec[held].mean())


def note_tightness(store, res, cls, hit):
    for q in ("t", "u", "v"):
        r = res["ratio_" + q]
        for c in np.unique(cls[hit]):
            k = "%s/%s" % (q, {10: "closed mesh, random", 11: "closed mesh, edges and vertices"}.get(int(c), "class %d" % c))
            store[k] = max(store.get(k, 0.0), float(r[hit & (cls == c)].max()))


@pytest.mark.parametrize("name", SCENES)
def test_rules_on_the_battery(orc, name):
    b = rb.referee_battery(orc, name, N_PER_CLASS)
    tris, rays, cls, T = b["tris"], b["rays"], b["cls"], b["tables"]
    assert set(rb.CLASSES) <= set(np.unique(cls)), "every class of the battery is drawn"
    shares, class1, overall = decided_shares(T, rays, cls, tris)
    print("%s: %d triangles, %d rays (%d per class), referee %.1f s, decided inside the domain: class 1 %.3f, all %.3f; %d exact fallbacks" % (
        name, tris.shape[0], rays.shape[0], b["n"], b["seconds"], class1, overall, T.exact_fallbacks))
    assert class1 >= 0.9, "%s: only %.3f of the class-1 rays inside the domain are decided: the rules would be vacuous" % (name, class1)
    assert overall >= 0.5, "%s: only %.3f of the rays inside the domain are decided" % (name, overall)
    answers = [("oracle brute force", b["S"].intersect_n(rays, use_bvh=False))]
    for leaf in LEAVES:
        S = b["S"] if leaf == 4 else rb.oracle_scene(orc, tris, leaf_size=leaf)
        answers.append(("oracle walk, leaf %d" % leaf, S.intersect_n(rays, use_bvh=True)))
        ctx = B.Context(-1)
        ctx.set_option("leaf_size", leaf)
        rb.upload(ctx, tris)
        answers.append(("closest_hit_host, leaf %d" % leaf, ctx.closest_hit_host_n(rays)))
        if leaf == 4:
            sl = X.check_triangle_records(tris, ctx.export_trees()["tris"])
        ctx.close()
    for who, ans in answers:
        res = X.assert_rules(T, ans, "%s on %s" % (who, name), cls=cls)
        note_tightness(_report["tightness"], res, cls, ans[0])
    _report["scenes"][name] = dict(triangles=int(tris.shape[0]), rays=int(rays.shape[0]), rays_per_class=b["n"], referee_s=round(b["seconds"], 1),
                                   decided_class1_inside=round(class1, 4), decided_all_inside=round(overall, 4), decided_by_class_and_band=shares,
                                   decided_by_tie_rule=int(T.tie.sum()), slivers_collapsed=sl["collapsed"], exact_fallbacks=int(T.exact_fallbacks))


@pytest.mark.parametrize("name", rb.closed_mesh_names())
def test_closed_meshes_leak_only_where_nothing_is_certain(orc, name):
    tris, centre, half = rb.make_closed_mesh(name)
    S = rb.oracle_scene(orc, tris)
    n = min(N_PER_CLASS, 2000)  # per ray set: 1 280 triangles at most
    rec = _report["closed_meshes"][name] = dict(triangles=int(tris.shape[0]))
    ctx = B.Context(-1)
    rb.upload(ctx, tris)
    for sname, rays in rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(77), n).items():
        T = X.Tables(tris, rays)
        brute = S.intersect_n(rays, use_bvh=False)
        walk = S.intersect_n(rays, use_bvh=True)
        host = ctx.closest_hit_host_n(rays)
        for who, ans in (("oracle brute force", brute), ("oracle walk", walk), ("closest_hit_host", host)):
            res = X.assert_rules(T, ans, "%s on %s / %s" % (who, name, sname))
            note_tightness(_report["tightness"], res, np.full(rays.shape[0], 10 if sname == "random" else 11), ans[0])
        assert np.array_equal(walk[0], brute[0]) and np.array_equal(host[0], brute[0]), "the leak set of a walk differs from brute force's"
        # the published rate, from many more rays than the referee takes (oracle only: the C brute force)
        big = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(78), 100 * n)[sname]
        hb, hw = S.intersect_n(big, use_bvh=False)[0], S.intersect_n(big, use_bvh=True)[0]
        assert np.array_equal(hb, hw)
        rec[sname] = dict(rays=int(rays.shape[0]), leaks=int((~brute[0]).sum()), decided=round(float(T.decided.mean()), 4),
                          leaks_without_referee=[int((~hb).sum()), int(big.shape[0])])
        print("%s / %s: %d of %d rays leak (referee present), %d of %d (oracle only)" % (name, sname, (~brute[0]).sum(), rays.shape[0], (~hb).sum(), big.shape[0]))
    ctx.close()


@pytest.mark.parametrize("sub", (5, 6))
def test_leaks_of_ordinary_rays_by_tessellation(orc, sub):
    """Random directions from inside finer icospheres (20 480 / 81 920 triangles), the oracle's walk: the leaks are counted, and every
    leaking ray is handed to the referee - no triangle may be certainly hit (R2)."""
    tris = (rb.icosphere(sub) * np.float32(rb.CLOSED_RADIUS)).astype(np.float32)
    S = rb.oracle_scene(orc, tris)
    rng = np.random.default_rng(5 + sub)
    n = 4000000
    rays = np.concatenate([rng.uniform(-0.6, 0.6, (n, 3)).astype(np.float32), rb._unit32(rng.normal(size=(n, 3)))], 1)
    ans = S.intersect_n(rays, use_bvh=True)
    leaks = np.nonzero(~ans[0])[0]
    if leaks.size:
        sub_ans = tuple(a[leaks] for a in ans)
        X.assert_rules(X.Tables(tris, rays[leaks]), sub_ans, "oracle walk on the leaking rays of the %d-triangle icosphere" % tris.shape[0])
    print("icosphere of %d triangles: %d of %d random rays from inside leak" % (tris.shape[0], leaks.size, n))
    _report["closed_meshes"]["ico%d" % tris.shape[0]] = dict(triangles=int(tris.shape[0]), random=dict(rays=n, leaks=int(leaks.size), walk="oracle walk only"))


# ---------------------------------------------------------------------------------------------------------------------
# the referee must bite: tri_eval restated in float32 numpy, and five wrong variants of it
# ---------------------------------------------------------------------------------------------------------------------
def _cross32(a, b):
    return [a[(i + 1) % 3] * b[(i + 2) % 3] - a[(i + 2) % 3] * b[(i + 1) % 3] for i in range(3)]


def _dot32(a, b):
    return a[2] * b[2] + (a[1] * b[1] + a[0] * b[0])


def restated_brute_force(tris, rays, wrong=None):
    """tri_eval + the minimum over all triangles in float32 numpy (unfused), slivers never hit.  `wrong`: one of WRONG."""
    tris = np.asarray(tris, np.float32)
    never = X.sliver_classes(tris)[0]
    n, nt = rays.shape[0], tris.shape[0]
    hit, t_o, u_o, v_o, id_o = np.zeros(n, bool), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, -1, np.int32)
    p0, p1, p2 = ([tris[None, :, k, i] for i in range(3)] for k in range(3))
    step = max(1, 400000 // nt)
    tmin = np.float32(0.0) if wrong == "t_above_zero" else rb.K_TMIN
    with np.errstate(all="ignore"):
        e1, e2 = [p1[i] - p0[i] for i in range(3)], [p2[i] - p0[i] for i in range(3)]
        for lo in range(0, n, step):
            r = rays[lo:lo + step]
            o, d = [r[:, None, i] for i in range(3)], [r[:, None, 3 + i] for i in range(3)]
            pv = _cross32(d, e2)
            inv = np.float32(1.0) / _dot32(e1, pv)
            tv = [o[i] - p0[i] for i in range(3)]
            u = _dot32(tv, pv) * inv
            qv = _cross32(tv, e1)
            v = _dot32(d, qv) * inv
            t = _dot32(e2, qv) * inv
            assert t.dtype == np.float32 and u.dtype == np.float32
            ok = (u >= 0) & (v >= 0) & ((u <= 1) if wrong == "u_alone_below_one" else (u + v <= 1)) & (t > tmin) & ~never[None, :]
            if wrong == "last_triangle_untested":
                ok[:, -1] = False
            tt = np.where(ok, t, np.float32(np.inf))
            if wrong == "tie_break_reversed":
                k = nt - 1 - tt[:, ::-1].argmin(1)
            else:
                k = tt.argmin(1)  # the first minimum: ties go to the lower id
            rows = np.arange(r.shape[0])
            h = ok[rows, k]
            hit[lo:lo + step], id_o[lo:lo + step] = h, np.where(h, k, -1)
            t_o[lo:lo + step], u_o[lo:lo + step], v_o[lo:lo + step] = (np.where(h, x[rows, k], 0) for x in (t, u, v))
    if wrong == "u_v_swapped":
        u_o, v_o = v_o, u_o
    return hit, t_o, u_o, v_o, id_o


WRONG = ("last_triangle_untested", "u_alone_below_one", "t_above_zero", "u_v_swapped", "tie_break_reversed")
BITE_SCENES = ("one_leaf", "rects", "soup2")


def test_the_restated_triangle_test_passes(orc):
    for name in BITE_SCENES:
        b = rb.referee_battery(orc, name, N_PER_CLASS)
        ans = restated_brute_force(b["tris"], b["rays"])
        X.assert_rules(b["tables"], ans, "float32 numpy restatement on %s" % name, cls=b["cls"])
        # and it is the definition: hit and id of the oracle's brute force inside the domain (t, u, v differ where the product fuses)
        held = rb.bands(b["rays"], rb.scene_measure(b["tris"]), b["cls"])[0] & b["tables"].decided.astype(bool)
        truth = b["S"].intersect_n(b["rays"], use_bvh=False)
        assert np.array_equal(ans[0][held], truth[0][held]) and np.array_equal(ans[4][held], truth[4][held])


@pytest.mark.parametrize("wrong", WRONG)
def test_a_wrong_triangle_test_is_caught(orc, wrong):
    caught = []
    for name in BITE_SCENES:
        b = rb.referee_battery(orc, name, N_PER_CLASS)
        ans = restated_brute_force(b["tris"], b["rays"], wrong)
        try:
            X.assert_rules(b["tables"], ans, "variant %s on %s" % (wrong, name), cls=b["cls"])
        except AssertionError as e:
            msg = str(e)
            assert ("R1" in msg or "R2" in msg or "R3" in msg) and "first: class" in msg and "ray " in msg, "the message names the rule and the first offending ray"
            caught.append("%s: %s" % (name, msg.split("violates ")[1][:2]))
    print(wrong, "->", caught)
    assert caught, "the referee did not notice the variant '%s' on any of %r" % (wrong, BITE_SCENES)
    _report.setdefault("wrong_variants_caught_by", {})[wrong] = caught


def test_zz_write_profile():
    """Last in the file: the figures gathered above, with PT_WRITE_PROFILES=1 (and the whole file run)."""
    if len(_report["scenes"]) == len(SCENES):
        t = _report["tightness"]
        assert all(v <= 1.0 for v in t.values())
        _report["tightness_max"] = max(t.values()) if t else 0.0
        write_profile("cpu", _report)
