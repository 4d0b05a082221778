"""Random cases for the guide pass, shared by tests/test_guide_fuzz_host.py (CPU) and tests/test_gpu_guide_fuzz.py (GPU).

draw_guide_case(seed) takes test_gpu_fuzz.draw_case(seed) - scene, textures, environment, camera and size stay - and draws on top of it,
in a fixed order from a generator of its own (the beauty fuzz's sequence does not move), what the definition of the follow mode
(include/mi355pt.h "guide pass, follow mode") branches on and the hand-built scenes of aov_common.py / aov_follow_common.py never hold:

  entities   every mesh of two or more triangles is cut into two entities of its material, triangle order kept (draw_case's meshes are
             unindexed: triangle k owns vertices 3k .. 3k+2).  Geometry and triangle ids are draw_case's, the entity layout is not the
             beauty fuzz's: the drawn materials find two to eight entities instead of one to four;
  normals    on about a quarter of the meshes about 15 % of the vertex normals become (0,0,0), get a NaN or get an inf; now and then one
             mesh has every normal zero;
  materials  beyond the issue's list, in 20 % of the cases (60 % at max_follow 8) every row of the table is first turned mirror or clear
             glass, a hall of mirrors in which guide rays reach max_follow = 8.  Then, each on the next entity of a drawn order, over the
             row of that entity's material or as a new row: often a smooth mirror (roughness 0, roughness_max or the float32 just above
             it); often a glass (its transmission roughness drawn the same way, clearcoat 0, ior 1, 1.45, 2.4, NaN, 0 or +inf; ior NaN
             makes normalize(wi) non-finite at every angle, 0 and +inf at normal incidence only); sometimes a second glass with ior NaN,
             0 or +inf on purpose; sometimes an emitter whose other fields classify as mirror; sometimes an exact tie mw == gw.
             Sometimes a NaN in metallic, roughness, specular_transmission, clearcoat or the base colour of a row in use.  Where the
             case has a texture, the entities of the textured material 0 are the last to be given another material;
  default    one entity of some cases has material_index -1;
  pass       n_samples 1..5, max_follow 0 1 2 4 8, roughness_max 0 0.2 0.3 1, watertight 0 or 1;
  instance   ONE of: bvh_builder 0 1 2, leaf_size 1 4 7, box_exact -1 0 1, quad 0 (watertight 0 only), a pixel shard (rank, world 2..9,
             tile 1 4 16 32);
  batch      (used with watertight 0) 2..4 frames, each with a camera near the case's and its own table: the case's, a copy with one row
             turned mirror, diffuse or NaN, or None for the context's.

reference(orc, seed) holds what tests/aov_follow_ref.py and tests/aov_ref.py make of a case - computed once per process and handed out
read-only -, the census of the definition's branches taken (from the restatement's log alone) and, for every ray of every round, whether
the oracle's walk equals its brute force (the closest-hit domain of DESIGN.md 2.1).  twin(B, seed): the CPU twins on a host-only context.

PT_GUIDE_FUZZ_CASES=N for more cases than the default of either file, PT_GUIDE_FUZZ_SEED to move the sequence, PT_GUIDE_FUZZ_ONLY=seed
for one case alone (a failure prints its seed)."""
import json
import os

import numpy as np

import aov_follow_ref as FR
import aov_ref
from owl_path_tracer_amd.pyhost import scene_io
from test_gpu_fuzz import draw_case

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "r17_guide_fuzz.json")
DEFAULT_SEED0 = 20265019  # chosen with the draw probabilities so that the default seed set meets the census of test_guide_fuzz_host.py
SEED0 = int(os.environ.get("PT_GUIDE_FUZZ_SEED", str(DEFAULT_SEED0)))
ROUGHNESS_MAX = (0.0, 0.2, 0.3, 1.0)
MAX_FOLLOW = (0, 1, 2, 4, 8)
IORS = (1.0, 1.45, 2.4, float("nan"), 0.0, float("inf"))
NAN_FIELDS = (FR.METALLIC, FR.ROUGHNESS, FR.SPEC_TRANS, FR.CLEARCOAT, 0, 1, 2)
# the options an instance sets and what they go back to (bvh_builder and leaf_size act at the upload)
OPTION_DEFAULTS = {"bvh_builder": 3, "leaf_size": 4, "box_exact": -1, "quad": 1}
AT_UPLOAD = ("bvh_builder", "leaf_size")
# the census: every key must occur in at least MIN_CASES cases and MIN_SAMPLES samples of the default seed set (test_guide_fuzz_host.py)
CENSUS_KEYS = ("bad_normal_on_a_followed_material", "emitter_that_would_be_followed", "nan_material_hit", "default_material_hit", "non_finite_direction",
               "stopped_by_max_follow_8", "stopped_by_max_follow_1", "total_internal_reflection", "ior_1_pass_through", "miss_after_a_follow",
               "texture_lookup_on_a_followed_path", "roughness_at_roughness_max_followed", "roughness_just_above_not_followed", "mw_equals_gw_tie")
MIN_CASES, MIN_SAMPLES = 3, 50


def seeds(default_n):
    only = os.environ.get("PT_GUIDE_FUZZ_ONLY")
    if only:
        return [int(only)]
    return [SEED0 + i for i in range(int(os.environ.get("PT_GUIDE_FUZZ_CASES", str(default_n))))]


def _rough(rng, rmax):
    """0, roughness_max or the float32 just above it"""
    return F32(rng.choice([F32(0.0), F32(rmax), np.nextafter(F32(rmax), F32(np.inf))], p=[0.4, 0.4, 0.2]))


def _halves(mesh):
    """A mesh of draw_case (unindexed: triangle k owns vertices 3k .. 3k+2) cut into two of the same triangles in the same order."""
    n = mesh["indices"].shape[0]
    if n < 2:
        return [mesh]
    cut = lambda a, b: dict(vertices=mesh["vertices"][3 * a:3 * b], normals=mesh["normals"][3 * a:3 * b], texcoords=mesh["texcoords"][3 * a:3 * b],
                            indices=np.arange(3 * (b - a), dtype=np.int32).reshape(-1, 3))
    return [cut(0, n // 2), cut(n // 2, n)]


class _Placer:
    """Drawn rows go to the entities in a drawn order, one after the other (round again when there are more rows than entities): over the
    row of that entity's material (every entity of that material gets it) or behind the table."""

    def __init__(self, rng, rows, ent_mat):
        self.rng, self.rows, self.ent_mat, self.order, self.k = rng, rows, ent_mat, rng.permutation(len(ent_mat)), 0

    def spare(self, material):
        """The entities of `material` go to the end of the order: they are taken only when the others are used up."""
        self.order = np.array(sorted(self.order, key=lambda e: self.ent_mat[e] == material), int)

    def next_entity(self):
        e = int(self.order[self.k % len(self.order)])
        self.k += 1
        return e

    def place(self, row):
        e = self.next_entity()
        if self.ent_mat[e] >= 0 and self.rng.random() < 0.3:
            self.rows[self.ent_mat[e]] = row
        else:
            self.rows.append(row)
            self.ent_mat[e] = len(self.rows) - 1


def draw_guide_case(seed):
    c = draw_case(seed)
    rng = np.random.default_rng([int(seed), 0x6775696465])
    # pass parameters
    n = int(rng.integers(1, 6))
    max_follow = int(rng.choice(MAX_FOLLOW, p=[0.15, 0.2, 0.15, 0.2, 0.3]))
    rmax = float(rng.choice(ROUGHNESS_MAX))
    wt = int(rng.integers(0, 2))
    # normals
    # every mesh of two or more triangles becomes two entities of its material, triangle order kept: the geometry and the triangle ids are
    # draw_case's, and the drawn materials find more than its one to four entities
    meshes, ent_mat = [], []
    for m, mid in c["ents"]:
        for part in _halves(m):
            meshes.append(dict(part, normals=np.array(part["normals"], F32)))
            ent_mat.append(int(mid))
    for m in meshes:
        nv = m["normals"].shape[0]
        bad = (rng.random(nv) < 0.15) & (rng.random() < 0.25)
        what, comp, sign = rng.integers(0, 3, nv), rng.integers(0, 3, nv), rng.choice([-1.0, 1.0], nv)
        for i in np.nonzero(bad)[0]:
            if what[i] == 0:
                m["normals"][i] = 0.0
            else:
                m["normals"][i, comp[i]] = np.nan if what[i] == 1 else sign[i] * np.inf
    k = int(rng.integers(0, len(meshes)))
    if rng.random() < 0.1:
        meshes[k]["normals"][:] = 0.0
    # materials
    rows = [np.array(r, F32) for r in c["mats"]]
    base = lambda: rng.uniform(0.2, 1.0, 3).astype(F32)
    u = rng.random(8)
    placer = _Placer(rng, rows, ent_mat)
    if c["texs"] is not None:  # the textured material stays in sight: a followed ray can reach a texture lookup
        placer.spare(0)
    if u[6] < (0.6 if max_follow == 8 else 0.2):  # a hall of mirrors and clear glass: every row becomes followed, so that guide rays reach max_follow = 8
        for i, r in enumerate(rows):
            r[FR.EMISSION], r[FR.CLEARCOAT] = 0.0, 0.0
            if (i + int(u[6] * 1000)) % 2:
                r[FR.METALLIC], r[FR.ROUGHNESS], r[FR.SPEC_TRANS] = 1.0, 0.0, 0.0
            else:
                r[FR.METALLIC], r[FR.SPEC_TRANS], r[FR.SPEC_TRANS_ROUGHNESS], r[FR.IOR] = 0.0, 1.0, 0.0, float(rng.choice([1.0, 1.45]))
    if u[0] < 0.85:
        placer.place(scene_io.material(base_color=base(), metallic=1.0, roughness=_rough(rng, rmax), clearcoat=float(rng.choice([0.0, 1.0]))))
    if u[1] < 0.85:
        placer.place(scene_io.material(base_color=base(), specular_transmission=1.0, specular_transmission_roughness=_rough(rng, rmax), clearcoat=0.0,
                                                     roughness=float(rng.random()), ior=float(rng.choice(IORS, p=[0.35, 0.15, 0.15, 0.15, 0.1, 0.1]))))
    if u[7] < 0.25:  # on purpose: a glass whose ior makes normalize(wi) non-finite (NaN always; 0 and +inf at normal incidence)
        placer.place(scene_io.material(base_color=base(), specular_transmission=1.0, specular_transmission_roughness=0.0, clearcoat=0.0,
                                       ior=float(rng.choice([float("nan"), 0.0, float("inf")], p=[0.6, 0.2, 0.2]))))
    if u[2] < 0.3:
        placer.place(scene_io.material(base_color=base(), metallic=1.0, roughness=0.0, emission=float(rng.uniform(0.5, 20.0))))
    if u[3] < 0.3:
        placer.place(scene_io.material(base_color=base(), metallic=0.5, specular_transmission=1.0, roughness=0.0, specular_transmission_roughness=0.0))
    if u[4] < 0.35:  # in a row that some entity uses
        rows[max(0, ent_mat[placer.next_entity()])][int(rng.choice(NAN_FIELDS))] = np.nan
    if u[5] < 0.35:
        ent_mat[placer.next_entity()] = -1
    mats = np.stack(rows).astype(F32)
    ents = list(zip(meshes, ent_mat))
    texs, mesh_tex, tex_by_mat = c["texs"], None, None
    if texs is not None:  # draw_case's rule: the texture lies on the meshes of material 0
        mesh_tex, tex_by_mat = [0 if mid == 0 else -1 for mid in ent_mat], {0: texs[0]}
    # instance
    kind = int(rng.integers(0, 5))
    if kind == 3 and wt:  # the binary walk has no watertight test
        kind = 2
    world = int(rng.integers(2, 10))
    shard_draw = (int(rng.integers(0, world)), world, int(rng.choice([1, 4, 16, 32])))
    value = int(rng.integers(0, 3))
    option, shard = None, None
    if kind == 0:
        option = ("bvh_builder", value)
    elif kind == 1:
        option = ("leaf_size", (1, 4, 7)[value])
    elif kind == 2:
        option = ("box_exact", value - 1)
    elif kind == 3:
        option = ("quad", 0)
    else:
        shard = shard_draw
    # batch
    frm, at, up, fov = c["camera"]
    reach = float(np.linalg.norm(np.asarray(frm) - np.asarray(at)))
    batch = []
    for _ in range(int(rng.integers(2, 5))):
        cam = ([float(x) for x in np.asarray(frm) + rng.normal(0, 0.02, 3) * reach], at, up, fov)
        v = int(rng.integers(0, 5))
        r, f = int(rng.integers(0, mats.shape[0])), int(rng.choice(NAN_FIELDS))
        t = None if v == 4 else mats.copy()
        if v == 1:  # mirror
            t[r, FR.METALLIC], t[r, FR.ROUGHNESS], t[r, FR.SPEC_TRANS], t[r, FR.CLEARCOAT], t[r, FR.EMISSION] = 1.0, 0.0, 0.0, 0.0, 0.0
        elif v == 2:  # diffuse
            t[r, FR.METALLIC], t[r, FR.SPEC_TRANS] = 0.0, 0.0
        elif v == 3:
            t[r, f] = np.nan
        batch.append((cam, t))
    return dict(seed=seed, ents=ents, mats=mats, W=c["W"], H=c["H"], env=c["env"], texs=texs, mesh_tex=mesh_tex, tex_by_mat=tex_by_mat, camera=c["camera"],
                n=n, max_follow=max_follow, roughness_max=rmax, wt=wt, option=option, shard=shard, batch=batch if not wt else None)


def describe(c):
    return "guide fuzz case seed=%d (%dx%d, n=%d, max_follow=%d, roughness_max=%g, watertight=%d, %s, %d triangles)" % (
        c["seed"], c["W"], c["H"], c["n"], c["max_follow"], c["roughness_max"], c["wt"], c["option"] or ("shard", c["shard"]), sum(len(m["indices"]) for m, _ in c["ents"]))


def flat_of(c):
    return scene_io.flatten_scene(c["ents"], [("m%d" % i, m, "") for i, m in enumerate(c["mats"])], c["tex_by_mat"])


def census(log, mats, max_follow, rmax):
    """{key of CENSUS_KEYS: samples} of one logged frame, from the restatement's log and the material table alone."""
    out = dict.fromkeys(CENSUS_KEYS, 0)
    mats = np.asarray(mats, F32).reshape(-1, FR.orc.MAT_FLOATS)
    rmax32, above = F32(rmax), np.nextafter(F32(rmax), F32(np.inf))
    for step, e in enumerate(log["log"]):
        h = e["hit"]
        if step >= 1:
            out["miss_after_a_follow"] += int((~h).sum())
        mi, stop, kind, went, tex, n_ok = e["mat"][h], e["stop"][h], e["kind"][h], e["went_on"][h], e["tex"][h], e["n_ok"][h]
        m = np.where((mi >= 0)[:, None], mats[np.maximum(mi, 0)], aov_ref.MAT_DEFAULT[None, :]).astype(F32)
        lobe = FR.classify(m, rmax)
        with np.errstate(invalid="ignore"):
            one = F32(1.0)
            mw, gw = m[:, FR.METALLIC], (one - m[:, FR.METALLIC]) * m[:, FR.SPEC_TRANS]
            dw, cw = (one - m[:, FR.SPEC_TRANS]) * (one - m[:, FR.METALLIC]), F32(0.25) * m[:, FR.CLEARCOAT]
            mirror_w, glass_w = (mw > gw) & (mw > dw) & (mw > cw), (gw > mw) & (gw > dw) & (gw > cw)
            tie = (mw == gw) & (mw > dw) & (mw > cw) & (m[:, FR.ROUGHNESS] <= rmax32) & (m[:, FR.SPEC_TRANS_ROUGHNESS] <= rmax32)
        none = stop == FR.STOP_CLASSIFIED_NONE
        add = lambda key, mask: out.__setitem__(key, out[key] + int(np.count_nonzero(mask)))
        add("bad_normal_on_a_followed_material", (stop == FR.STOP_BAD_NORMAL) & (lobe != FR.NONE))
        add("emitter_that_would_be_followed", (stop == FR.STOP_EMITTER) & (lobe != FR.NONE) & (step != max_follow) & n_ok)
        add("nan_material_hit", np.isnan(m[:, list(NAN_FIELDS)]).any(1))
        add("default_material_hit", mi < 0)
        add("non_finite_direction", stop == FR.STOP_NON_FINITE_DIRECTION)
        if max_follow in (1, 8):
            add("stopped_by_max_follow_%d" % max_follow, (stop == FR.STOP_CAP) & (lobe != FR.NONE) & n_ok)  # (the cap alone stopped it)
        add("total_internal_reflection", e["tir"][h])
        add("ior_1_pass_through", (kind == FR.GLASS) & (m[:, FR.IOR] == one) & went)
        add("texture_lookup_on_a_followed_path", tex & (step >= 1))
        add("roughness_at_roughness_max_followed", went & (((kind == FR.MIRROR) & (m[:, FR.ROUGHNESS] == rmax32)) | ((kind == FR.GLASS) & (m[:, FR.SPEC_TRANS_ROUGHNESS] == rmax32))))
        add("roughness_just_above_not_followed", none & ((mirror_w & (m[:, FR.ROUGHNESS] == above)) | (glass_w & (m[:, FR.SPEC_TRANS_ROUGHNESS] == above))))
        add("mw_equals_gw_tie", none & tie)
    return out


def census_of(orc, seed_list):
    """({key: cases}, {key: samples}) of the main frames of the seeds"""
    cases, samples = dict.fromkeys(CENSUS_KEYS, 0), dict.fromkeys(CENSUS_KEYS, 0)
    for seed in seed_list:
        for k, v in reference(orc, seed)["census"].items():
            samples[k] += v
            cases[k] += v > 0
    return cases, samples


def _domain(S, log):
    """(rays checked, rays on which the oracle's walk differs from its brute force in hit, t bits or id) over every round of a log"""
    rays, bad = 0, 0
    for e in log["log"]:
        hit, t, _, _, prim = S.intersect_n(e["rays"], use_bvh=True)
        differs = (hit != e["hit"]) | (prim != e["prim"]) | (hit & (t.view(np.uint32) != e["t"].view(np.uint32)))
        rays += int(hit.size)
        bad += int(differs.sum())
    return rays, bad


def ocamera(orc, c, cam=None):
    frm, at, up, fov = cam or c["camera"]
    return orc.to_camera_data(tuple(frm), tuple(at), tuple(up), fov, c["W"], c["H"]).as_array()


def bcamera(B, c, cam=None):
    frm, at, up, fov = cam or c["camera"]
    return B.to_camera_data(frm, at, up, fov, c["W"], c["H"])


def params(B, c, max_follow=None):
    return B.aov_default_params(n_samples=c["n"], max_follow=c["max_follow"] if max_follow is None else max_follow, roughness_max=c["roughness_max"])


_ref, _twin = {}, {}


def _frozen(a):
    a.setflags(write=False)
    return a


def reference(orc, seed):
    """dict(case, follow (H, W, 8), first (H, W, 8), batch [(H, W, 8)] or None, census, followed, rays, outside): the restatements of the
    case's frames; rays / outside: the rays of all their rounds and how many of them leave the closest-hit domain."""
    if seed not in _ref:
        c = draw_guide_case(seed)
        fl = flat_of(c)
        S = orc.Scene(fl, watertight=bool(c["wt"]))
        W, H = c["W"], c["H"]
        follow, log = FR.aov(S, fl, c["env"], ocamera(orc, c), W, H, c["n"], c["max_follow"], c["roughness_max"], want_log=True)
        rays, outside = _domain(S, log)
        first = aov_ref.aov(S, fl, c["env"], ocamera(orc, c), W, H, c["n"])
        batch = None
        if c["batch"] is not None:
            batch = []
            for cam, table in c["batch"]:
                a, lg = FR.aov(S, fl, c["env"], ocamera(orc, c, cam), W, H, c["n"], c["max_follow"], c["roughness_max"], materials=table, want_log=True)
                r, o = _domain(S, lg)
                rays, outside = rays + r, outside + o
                batch.append(_frozen(a))
        _ref[seed] = dict(case=c, follow=_frozen(follow), first=_frozen(first), batch=batch, census=census(log, c["mats"], c["max_follow"], c["roughness_max"]),
                          followed=bool(any(e["went_on"].any() for e in log["log"])), rays=rays, outside=outside)
    return _ref[seed]


def twin(B, seed):
    """dict(follow, first, follow0, batch): pt_debug_aov_follow_host / pt_debug_aov_host of the case on a host-only context with the default
    hierarchy (the closest hit does not depend on it), the batch frames by pt_set_materials + pt_debug_aov_follow_host."""
    if seed not in _twin:
        c = draw_guide_case(seed)
        h = B.Context(-1)
        try:
            h.upload_scene(c["ents"], c["mats"], textures=c["texs"], mesh_textures=c["mesh_tex"], env=B.make_env(**c["env"]))
            h.set_option("watertight", c["wt"])
            cam, W, H = bcamera(B, c), c["W"], c["H"]
            out = dict(follow=_frozen(h.aov_follow_host(cam, W, H, params(B, c))), first=_frozen(h.aov_host(cam, W, H, c["n"])),
                       follow0=_frozen(h.aov_follow_host(cam, W, H, params(B, c, 0))), batch=None)
            if c["batch"] is not None:
                out["batch"] = []
                for fcam, table in c["batch"]:
                    h.set_materials(c["mats"] if table is None else table)
                    out["batch"].append(_frozen(h.aov_follow_host(bcamera(B, c, fcam), W, H, params(B, c))))
        finally:
            h.close()
        _twin[seed] = out
    return _twin[seed]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same(got, want, c, what):
    """Every float of every pixel, as bits (a NaN equals only the same NaN)."""
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (describe(c), what, g.shape, w.shape)
    bad = g != w
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %s: %d of %d floats differ in bits (%d pixels); first at %s: got %r, want %r" % (
            describe(c), what, int(bad.sum()), bad.size, int(bad.reshape(-1, 8).any(1).sum()), i, np.asarray(got)[i], np.asarray(want)[i]))


def write_profile(section, doc):
    """PT_WRITE_PROFILES=1: the keys of `doc` go into `section` of the report; what other test functions wrote there stays."""
    if os.environ.get("PT_WRITE_PROFILES") != "1":
        return
    whole = {}
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            whole = json.load(fh)
    whole.setdefault(section, {}).update(doc)
    with open(PROFILE, "w") as fh:
        json.dump(whole, fh, indent=1, sort_keys=True)


# ---- the sliver strip seen along its axis: the guide kernels' HBM overflow column ------------------------------------------------
# ray_battery's strip (3000 slivers in the plane z = 0, x = 0 .. 9000; at leaf_size 1 its quad tree is 9 levels deep, so the walk's stack
# of 3 * 9 + 1 entries exceeds the 12 LDS entries) and behind its far end a checker-textured wall of +-0.05 in y and z at x = 9100 whose
# shading normal is tilted by a few 1e-6: turned mirror (pt_set_materials) it sends the guide rays back along the strip.  The camera
# sits before the near end and looks along the axis through 1e-3 degrees: every ray passes the boxes of the whole strip.
STRIP_W, STRIP_H, STRIP_N, STRIP_MAX_FOLLOW, STRIP_ROUGHNESS_MAX = 24, 16, 2, 4, 0.3
STRIP_CAMERA = ([-2.0, 5e-4, 0.0], [9000.0, 5e-4, 0.0], [0, 1, 0], 1e-3)
STRIP_SHIFTS_Y = (0.0, 2.5e-4, -3.75e-4)  # the batch's cameras: parts of the strip's width of 1e-3
STRIP_WALL = 1  # the wall's material row
_strip = {}


def strip_scene():
    if not _strip:
        import ray_battery as rb

        x, a = F32(9100.0), F32(0.05)
        v = np.array([(x, -a, -a), (x, a, -a), (x, a, a), (x, -a, -a), (x, a, a), (x, -a, a)], F32)
        tc = np.array([(0, 0), (3, 0), (3, 3), (0, 0), (3, 3), (0, 3)], F32)
        wall = dict(vertices=v, normals=np.tile(F32([-1.0, 4e-6, 1e-6]), (6, 1)), texcoords=tc, indices=np.arange(6, dtype=np.int32).reshape(2, 3))
        strip = dict(rb.mesh_of(rb.make_scene("strip")), texcoords=np.zeros((9000, 2), F32))
        rows = [scene_io.material(base_color=(0.7, 0.6, 0.5), roughness=0.8), scene_io.material(base_color=(0.8, 0.8, 0.8), roughness=0.9)]
        mirror = np.stack(rows).astype(F32)
        mirror[STRIP_WALL, FR.METALLIC], mirror[STRIP_WALL, FR.ROUGHNESS] = 1.0, 0.0
        ents = [(strip, 0), (wall, STRIP_WALL)]
        tex = scene_io.checker_texture()
        _strip.update(ents=ents, mats=rows, mirror=mirror, textures=[tex], mesh_textures=[-1, 0], env=dict(use_auto=True, intensity=1.0),
                      flat=scene_io.flatten_scene(ents, [("strip", rows[0], ""), ("wall", rows[1], "")], {STRIP_WALL: tex}))
    return _strip


def strip_camera(make, shift_y=0.0):
    frm, at, up, fov = STRIP_CAMERA
    return make((frm[0], frm[1] + shift_y, frm[2]), (at[0], at[1] + shift_y, at[2]), tuple(up), fov, STRIP_W, STRIP_H)


_strip_ref = {}


def strip_reference(orc, wt):
    """dict(first, follow (the wall a mirror), batch (watertight 0: the follow frames of STRIP_SHIFTS_Y, the wall a mirror in frames 0 and
    1 and diffuse in frame 2), wall_share, albedos, rays, outside) of the strip frame, once per process."""
    if wt not in _strip_ref:
        sc = strip_scene()
        S = orc.Scene(sc["flat"], leaf_size=1, watertight=bool(wt))
        cam = strip_camera(orc.to_camera_data).as_array()
        W, H, n = STRIP_W, STRIP_H, STRIP_N
        smp = aov_ref.samples(S, sc["flat"], sc["env"], cam, W, H, n, np.arange(W * H))
        first = aov_ref.aov(S, sc["flat"], sc["env"], cam, W, H, n)
        follow, log = FR.aov(S, sc["flat"], sc["env"], cam, W, H, n, STRIP_MAX_FOLLOW, STRIP_ROUGHNESS_MAX, materials=sc["mirror"], want_log=True)
        rays, outside = _domain(S, log)
        batch = None
        if not wt:
            batch = []
            for f, dy in enumerate(STRIP_SHIFTS_Y):
                a, lg = FR.aov(S, sc["flat"], sc["env"], strip_camera(orc.to_camera_data, dy).as_array(), W, H, n, STRIP_MAX_FOLLOW, STRIP_ROUGHNESS_MAX,
                               materials=sc["mirror"] if f < 2 else None, want_log=True)
                r, o = _domain(S, lg)
                rays, outside = rays + r, outside + o
                batch.append(_frozen(a))
        wall_prims = np.asarray(sc["flat"]["material_index"])[np.maximum(smp["prim"], 0)] == STRIP_WALL
        _strip_ref[wt] = dict(first=_frozen(first), follow=_frozen(follow), batch=batch, wall_share=float((smp["hit"] & wall_prims).mean()),
                              albedos=int(np.unique(bits(first[..., :3]).reshape(-1, 3), axis=0).shape[0]), rays=rays, outside=outside,
                              followed=int(sum(e["went_on"].sum() for e in log["log"])))
    return _strip_ref[wt]


def strip_twin(B, wt):
    """The same frames from the CPU twins on a host-only context (leaf_size 1, as the GPU test's context)."""
    sc = strip_scene()
    h = B.Context(-1)
    try:
        h.set_option("leaf_size", 1)
        h.upload_scene(sc["ents"], sc["mats"], textures=sc["textures"], mesh_textures=sc["mesh_textures"], env=B.make_env(**sc["env"]))
        h.set_option("watertight", wt)
        W, H = STRIP_W, STRIP_H
        prm = B.aov_default_params(n_samples=STRIP_N, max_follow=STRIP_MAX_FOLLOW, roughness_max=STRIP_ROUGHNESS_MAX)
        out = dict(first=h.aov_host(strip_camera(B.to_camera_data), W, H, STRIP_N), depth4=h.export_trees()["depth4"], batch=None)
        h.set_materials(sc["mirror"])
        out["follow"] = h.aov_follow_host(strip_camera(B.to_camera_data), W, H, prm)
        if not wt:
            out["batch"] = []
            for f, dy in enumerate(STRIP_SHIFTS_Y):
                h.set_materials(sc["mirror"] if f < 2 else np.stack(sc["mats"]))
                out["batch"].append(h.aov_follow_host(strip_camera(B.to_camera_data, dy), W, H, prm))
    finally:
        h.close()
    return out
