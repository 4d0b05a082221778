"""Option "watertight" = 1 on the GPU: every walk of the wavefront render path with the watertight triangle test (pt_kernel_wt.hip).

* Ray probes 30..35 (the render kernel's own device functions) against tests/watertight_ref.py - brute force in float32 numpy - on
  EVERY ray of the battery inside the 10-extent domain: hit and id equal, t, u, v bit for bit (34 / 35 carry no t), for builders
  0 / 1 / 2 x leaf sizes 1 / 4 / 7 on the battery's small scenes.  Outside the domain: counted, not asserted (ray_battery.py).
* Closed meshes with shared float32 vertices, 2 000 rays per set from strictly inside: zero leaks through all six probes.
* Frames of 48 x 40 at 40 spp on the Cornell box (six materials, an emitter, closed meshes): bit-identical, with equal work counters,
  through the quad walk, the group walk forced on and off, the fallback instance, the instrumented instance, both slab forms,
  schedule 0, the whole-pixel schedule forced, the sum of three pixel shards, and two contexts in one pt_group over the stub
  collective.  A frame with watertight = 0 after one with watertight = 1 is the frame of before - the oracle's, bit for bit.
* Invariant frame: camera inside a closed icosphere whose only material is an emitter, black environment.  The oracle (watertight =
  0's twin) says the model gives one constant there; every pixel of the watertight frame must be exactly that constant.
* The oracle's watertight twin (Scene(..., watertight=True); tests/test_oracle_watertight.py ties it to watertight_ref.py and shows that
  its frames do not depend on its hierarchy) is the bit-level reference of the frames: the Cornell frame every path test of this
  file compares with - float, RGBA8 and the work counters -, a 64 x 48 Cornell frame at 256 spp, and three scenes where t, u, v
  reach the shading (a textured cube under the sky, the four lobes + sheen on spheres, smooth textured icospheres of glass and
  metal under an environment map, seen from outside and from inside the glass), each through the default path, the group walk, the
  fallback instance and the subtracting slab form.  tests/test_gpu_fuzz.py does the same on its random scenes.
* The 256 spp frame keeps its tie to the Moeller-Trumbore oracle frame of the same seed: relRMSE within the stated bar for "same
  algorithm, different rounding" (<= 1e-2 at >= 256 spp).
* The three refusals (option kernel = 1, the validation kernel's closest-hit op, pt_render_batch) are PT_E_INVALID with a message.
* `pt_main --watertight` writes the PNG of the binding's RGBA8 frame.

PT_WRITE_PROFILES=1 records the figures in profiles/r09_watertight.json (section "gpu").
"""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ray_battery as rb
import rccl_stub
import watertight_ref as WR
from owl_path_tracer_amd.pyhost import binding as B, scene_io

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "assets")
PT_MAIN = os.path.join(ROOT, "owl-path-tracer_amd", "pt_main")
SMALL_SCENES = ("rects", "one_leaf", "soup1", "soup2", "soup3", "soup_offset30", "strip")
N_PER_CLASS = 200
N_CLOSED = 2000
BUILDERS = (0, 1, 2)
LEAVES = (1, 4, 7)
W_, H_, SPP, DEPTH = 48, 40, 40, 16
CORNELL_ENV = dict(color=(1, 1, 1), intensity=0.0)
PATH_INDEPENDENT = ("samples", "rays", "scatters", "env_misses", "nan_retries")  # work that does not depend on the walk or the schedule
_report = {"probes": {}, "closed_meshes": {}, "frames": {}, "frames_against_the_oracle": {}}


def _battery(orc, name, n_per_class=N_PER_CLASS):
    """The rays of ray_battery.referee_battery (same seed, same planes, same count per class) without the referee's tables."""
    tris = rb.make_scene(name)
    n = rb.referee_rays_per_class(tris.shape[0], n_per_class)
    S = rb.oracle_scene(orc, tris)
    host = B.Context(-1)
    host.set_option("leaf_size", 4)
    host.set_option("wide_leaves", 1)
    rb.upload(host, tris)
    t4 = rb.trees_of(host.export_trees())[1]
    host.close()
    used = t4.ref != -1
    planes = np.stack([t4.lo[used], t4.hi[used]], 1) if t4.n_nodes else None
    rays, cls = rb.make_rays(tris, np.random.default_rng(4242), n, planes=planes, hit_fn=lambda r: S.intersect_n(r, use_bvh=True)[:2])
    return tris, rays, cls, S


def _answer(out):
    out = np.asarray(out, np.float32)
    return out[:, 0] != 0, out[:, 1].copy(), out[:, 2].copy(), out[:, 3].copy(), np.ascontiguousarray(out[:, 4]).view(np.int32)


@pytest.mark.parametrize("name", SMALL_SCENES)
def test_probes_equal_the_reference(orc, name):
    tris, rays, cls, S = _battery(orc, name)
    assert set(rb.CLASSES) <= set(np.unique(cls))
    ref, n64 = WR.brute_force(tris, rays)
    held, mid, far = rb.bands(rays, rb.scene_measure(tris), cls)
    outside = np.isin(cls, rb.OUTSIDE)
    rec = _report["probes"][name] = dict(triangles=int(tris.shape[0]), rays=int(rays.shape[0]), rays_inside_the_domain=int(held.sum()), mismatches_outside_the_domain={})
    for builder in BUILDERS:
        for leaf in LEAVES:
            ctx = B.Context(0)
            ctx.set_option("bvh_builder", builder)
            ctx.set_option("leaf_size", leaf)
            ctx.set_option("watertight", 1)
            rb.upload(ctx, tris)
            for op in B.PROBE_OPS:
                got = _answer(ctx.debug_eval(op, rays, 6))
                group = op.startswith("group")
                bad = WR.compare(ref, got, held, with_t=not group)
                assert bad.size == 0, "%s on %s, builder %d leaf %d: %d of %d rays inside the domain differ from the reference; first: class %d %r got %r want %r" % (
                    op, name, builder, leaf, bad.size, held.sum(), cls[bad[0]], rays[bad[0]].tolist(), [x[bad[0]].item() for x in got], [x[bad[0]].item() for x in ref])
                o = rec["mismatches_outside_the_domain"].setdefault(op, [0, 0, 0, 0, 0, 0])
                for k, m in ((0, mid), (2, far), (4, outside)):  # [mismatches, rays] at 10-42 extents, beyond 42, classes 8 / 9
                    o[k] += int(WR.compare(ref, got, m, with_t=not group).size)
                    o[k + 1] += int(m.sum())
            if builder == 0 and leaf == 4:  # the switch back on the same context and scene: Moeller-Trumbore again, the oracle's brute force
                ctx.set_option("watertight", 0)
                mt = _answer(ctx.debug_eval("quad", rays, 6))
                bad = WR.compare(S.intersect_n(rays, use_bvh=False), mt, held)
                assert bad.size == 0, "watertight = 0 after 1, %s: %d rays differ from the oracle's brute force" % (name, bad.size)
            ctx.close()
    print(name, rec)


@pytest.mark.parametrize("name", rb.closed_mesh_names())
def test_closed_meshes_do_not_leak_through_any_probe(name):
    tris, centre, half = rb.make_closed_mesh(name)
    sets = rb.closed_mesh_rays(tris, centre, half, np.random.default_rng(77), N_CLOSED)
    ctx = B.Context(0)
    rb.upload(ctx, tris)
    rec = _report["closed_meshes"][name] = dict(triangles=int(tris.shape[0]))
    for sname, rays in sets.items():
        ref, _ = WR.brute_force(tris, rays)
        assert ref[0].all()
        ctx.set_option("watertight", 0)
        before = int((ctx.debug_eval("quad", rays, 6)[:, 0] == 0).sum())
        ctx.set_option("watertight", 1)
        for op in B.PROBE_OPS:
            got = _answer(ctx.debug_eval(op, rays, 6))
            assert got[0].all(), "%s: %d of %d rays from inside %s (%s) leak; first %r" % (op, (~got[0]).sum(), rays.shape[0], name, sname, rays[~got[0]][0].tolist())
            bad = WR.compare(ref, got, with_t=not op.startswith("group"))
            assert bad.size == 0, "%s on %s / %s: %d rays differ from the reference; first %r" % (op, name, sname, bad.size, rays[bad[0]].tolist())
        rec[sname] = dict(rays=int(rays.shape[0]), leaks_watertight_0=before, leaks_watertight_1=0)
    ctx.close()
    print(name, rec)
    assert rec["edges_and_vertices"]["leaks_watertight_0"] > 0, "the aimed set is where Moeller-Trumbore leaks: without leaks before, zero after shows nothing"


# ---------------------------------------------------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_frame(a, b, what):
    bad = _bits(a) != _bits(b)
    assert not bad.any(), "%s: %d of %d floats differ" % (what, bad.sum(), bad.size)


@pytest.fixture(scope="module")
def cornell_wt(cornell):
    """One context with the Cornell box, its camera, the watertight frame through the default path, that frame's work counters
    (instrumented instance) and the Moeller-Trumbore frame of the same context."""
    ctx = B.Context(0)
    mats = np.stack([m for _, m, _ in cornell["materials"]]).astype(np.float32)
    ctx.upload_scene(cornell["entities"], mats, env=B.make_env(**CORNELL_ENV))
    c = cornell["camera"]
    cam = B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W_, H_)
    mt, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
    ctx.set_option("watertight", 1)
    wt, wt8 = ctx.render(cam, W_, H_, SPP, DEPTH, want_rgba8=True)
    st = ctx.stats()
    assert st["kernel_variant"] in (2, 3) and st["vgprs"] <= 168
    ctx.set_option("count", 1)
    counted, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
    cst = ctx.stats()
    ctx.set_option("count", 0)
    _same_frame(counted, wt, "instrumented instance == product instance")
    assert cst["samples"] == W_ * H_ * SPP and cst["rays"] > cst["samples"]
    _report["frames"]["default_path"] = dict(kernel_variant=int(st["kernel_variant"]), vgprs=int(st["vgprs"]), vgprs_instrumented=int(cst["vgprs"]),
                                             float64_branch_pairs=[int(cst["trav"][2]), int(cst["tris"])])
    yield dict(ctx=ctx, cam=cam, mt=mt, wt=wt, wt8=wt8, counters={k: int(cst[k]) for k in PATH_INDEPENDENT}, mats=mats)
    ctx.close()


def test_the_watertight_frame_is_another_frame_of_the_same_scene(cornell_wt):
    """t, u, v come from another operation sequence, so the bits differ; the picture does not: every pixel is lit the same way."""
    wt, mt = cornell_wt["wt"], cornell_wt["mt"]
    assert (_bits(wt) != _bits(mt)).any(), "watertight = 1 rendered the Moeller-Trumbore frame bit for bit: the option did not reach the kernel"
    assert np.isfinite(wt).all() and wt.std() > 0.01
    assert abs(float(wt.mean()) / float(mt.mean()) - 1.0) < 0.05  # (40 spp: the two frames are two roundings of one estimate)


def test_the_cornell_frame_is_the_watertight_oracles(cornell_wt, orc, cornell):
    """Every path test of this file compares with cornell_wt["wt"]: a mistake all paths share - t, u, v handed wrongly from the leaf
    step to the shading - passes them all.  This anchors that frame: the oracle with its switch at 1 renders it bit for bit, in
    float and in RGBA8, and counts the same work."""
    c = cornell["camera"]
    S = orc.Scene(cornell["flat"], watertight=True)
    want, want8, cnt = S.render(orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W_, H_), orc.make_env(**CORNELL_ENV), W_, H_, SPP, DEPTH,
                                want_rgba8=True, want_counters=True)
    _same_frame(cornell_wt["wt"], want, "Cornell, watertight = 1 == the watertight oracle")
    np.testing.assert_array_equal(cornell_wt["wt8"], want8)
    assert set(PATH_INDEPENDENT) <= set(cnt), "orc_counters holds all five"
    assert cornell_wt["counters"] == {k: int(cnt[k]) for k in PATH_INDEPENDENT}
    differ = int((_bits(want) != _bits(cornell_wt["mt"])).any(-1).sum())
    _report["frames_against_the_oracle"]["cornell_48x40"] = dict(pixels=W_ * H_, pixels_that_differ_from_switch_0=differ)
    assert differ > 0


PATHS = [
    ("quad walk only", {"groups": 0}, {"groups": 1}),
    ("group walk always", {"groups": 2}, {"groups": 1}),
    ("fallback instance", {"fallback": 1}, {"fallback": 0}),
    ("fma slab form", {"box_exact": 0}, {"box_exact": -1}),
    ("subtracting slab form", {"box_exact": 1}, {"box_exact": -1}),
    ("subtracting slab form, fallback", {"box_exact": 1, "fallback": 1}, {"box_exact": -1, "fallback": 0}),
    ("subtracting slab form, group walk", {"box_exact": 1, "groups": 2}, {"box_exact": -1, "groups": 1}),
    ("schedule 0", {"schedule": 0}, {"schedule": 1}),
    ("ring schedule", {"whole": 0}, {"whole": -1}),
    ("whole pixels forced", {"whole": 1}, {"whole": -1}),
    ("spp_per_launch", {"spp_per_launch": 7}, {"spp_per_launch": 0}),
]


@pytest.mark.parametrize("label,opts,reset", PATHS, ids=[p[0].replace(" ", "_").replace(",", "") for p in PATHS])
def test_frame_through_the_render_paths(cornell_wt, label, opts, reset):
    ctx, cam = cornell_wt["ctx"], cornell_wt["cam"]
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        got, got8 = ctx.render(cam, W_, H_, SPP, DEPTH, want_rgba8=True)
        st = ctx.stats()
        ctx.set_option("count", 1)
        counted, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
        cst = ctx.stats()
    finally:
        ctx.set_option("count", 0)
        for k, v in reset.items():
            ctx.set_option(k, v)
    if "fallback" in opts:
        assert st["kernel_variant"] == 3 and 128 < st["vgprs"] <= 168
    if "whole" in opts:
        assert (st["whole_pixels"] != 0) == (opts["whole"] == 1)
    _same_frame(got, cornell_wt["wt"], label)
    np.testing.assert_array_equal(got8, cornell_wt["wt8"])
    _same_frame(counted, cornell_wt["wt"], label + ", instrumented")
    assert {k: int(cst[k]) for k in PATH_INDEPENDENT} == cornell_wt["counters"], label


def test_frame_is_the_sum_of_three_pixel_shards(cornell_wt):
    ctx, cam = cornell_wt["ctx"], cornell_wt["cam"]
    acc = np.zeros_like(cornell_wt["wt"])
    total = dict.fromkeys(PATH_INDEPENDENT, 0)
    try:
        for r in range(3):
            ctx.set_pixel_shard(r, 3, 16)
            part, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
            own = np.zeros(W_ * H_, bool)
            own[B.shard_pixels(W_, H_, 16, r, 3)] = True
            own = own.reshape(H_, W_)[::-1]
            assert not part[~own].any(), "rank %d wrote outside its tiles" % r
            acc += part
            ctx.set_option("count", 1)
            ctx.render(cam, W_, H_, SPP, DEPTH)
            cst = ctx.stats()
            ctx.set_option("count", 0)
            for k in PATH_INDEPENDENT:
                total[k] += int(cst[k])
    finally:
        ctx.set_option("count", 0)
        ctx.set_pixel_shard(0, 1, 16)
    _same_frame(acc, cornell_wt["wt"], "sum of three shards")
    assert total == cornell_wt["counters"]


def test_two_contexts_in_one_group_over_the_stub_collective(cornell_wt, tmp_path):
    """pt_group_set_option carries the key to every context of the group (one child process: tests/group_child.py); the frame is the
    single context's, and a group that sets the key back to 0 renders the Moeller-Trumbore frame."""
    steps = [["upload", "cornell"], ["option", "watertight", 1], ["render", "cornell", W_, H_, SPP, DEPTH, 1, "wt"], ["option", "watertight", 0],
             ["render", "cornell", W_, H_, SPP, DEPTH, 0, "mt"]]
    sf = tmp_path / "steps.json"
    sf.write_text(json.dumps(steps))
    out = str(tmp_path / "got")
    rc, so, se = rccl_stub.run_child([sys.executable, os.path.join(ROOT, "tests", "group_child.py"), "steps", out, "0,0", str(sf)], rccl_stub.stub_env(), 300)
    assert rc == 0, "child exited with %s\n%s\n%s" % (rc, so[-2000:], se[-4000:])
    assert json.load(open(os.path.join(out, "info.json")))["size"] == 2
    _same_frame(np.load(os.path.join(out, "wt_rgb.npy")), cornell_wt["wt"], "group of 2, watertight = 1")
    np.testing.assert_array_equal(np.load(os.path.join(out, "wt_rgba8.npy")), cornell_wt["wt8"])
    _same_frame(np.load(os.path.join(out, "mt_rgb.npy")), cornell_wt["mt"], "group of 2, watertight back to 0")


def test_watertight_0_after_1_is_the_frame_of_before(cornell_wt, orc, cornell):
    """The frame of before is the oracle's, bit for bit (tests/test_gpu_parity.py): the switch leaves nothing behind in the context."""
    ctx, cam = cornell_wt["ctx"], cornell_wt["cam"]
    c = cornell["camera"]
    want, _, _ = orc.Scene(cornell["flat"]).render(orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W_, H_), orc.make_env(**CORNELL_ENV), W_, H_, SPP, DEPTH)
    try:
        ctx.set_option("watertight", 1)
        ctx.render(cam, W_, H_, SPP, DEPTH)
        ctx.set_option("watertight", 0)
        got, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
        assert ctx.stats()["kernel_variant"] == 2
    finally:
        ctx.set_option("watertight", 1)
    _same_frame(got, want, "watertight = 0 after 1 == oracle")
    _same_frame(got, cornell_wt["mt"], "watertight = 0 after 1 == watertight = 0 before")


def test_invariant_frame_inside_a_closed_emitter(orc):
    """Every path from inside a closed mesh of one emitter ends at its first hit with the emission; nothing else is in the scene and the
    environment is black.  So the frame is one constant - unless a ray finds a seam.  The camera looks at a vertex of the mesh."""
    tris = (rb.icosphere(3) * np.float32(rb.CLOSED_RADIUS)).astype(np.float32)
    mat = scene_io.MAT_DEFAULT.copy()
    mat[16] = 2.0  # emission
    ents = [(rb.mesh_of(tris), 0)]
    look_from, look_at = [0.11, -0.07, 0.05], [float(x) for x in tris[0, 0]]
    W, H, spp = 48, 40, 16
    want, _, _ = orc.Scene(scene_io.flatten_scene(ents, [("glow", mat, "")])).render(orc.to_camera_data(look_from, look_at, [0, 1, 0], 70.0, W, H), orc.make_env(color=(0, 0, 0), intensity=0.0), W, H, spp, 8)
    const = np.unique(_bits(want))
    assert const.size == 1 and want.flat[0] == 2.0, "the model gives one constant here (the oracle, Moeller-Trumbore: none of these rays meets a seam)"
    ctx = B.Context(0)
    ctx.upload_scene(ents, [mat], env=B.make_env(color=(0, 0, 0), intensity=0.0))
    ctx.set_option("watertight", 1)
    cam = B.to_camera_data(look_from, look_at, [0, 1, 0], 70.0, W, H)
    for opts in ({}, {"groups": 2}, {"fallback": 1}):
        for k, v in opts.items():
            ctx.set_option(k, v)
        got, _ = ctx.render(cam, W, H, spp, 8)
        assert (_bits(got) == const[0]).all(), "%r: %d of %d values are not the constant %r" % (opts, (_bits(got) != const[0]).sum(), got.size, float(want.flat[0]))
        for k in opts:
            ctx.set_option(k, {"groups": 1, "fallback": 0}[k])
    ctx.close()


def test_statistical_tie_to_the_oracle(orc, cornell):
    """Against the Moeller-Trumbore oracle frame - same algorithm, other rounding of t, u, v -: the stated bar for such a pair at >= 256
    spp is relRMSE <= 1e-2 (tools/tolerance_calibration.py: rmse over all values / mean luminance of the reference).
    Against the WATERTIGHT oracle frame of the same seed there is nothing statistical left: bit for bit."""
    W, H, spp = 64, 48, 256
    c = cornell["camera"]
    S = orc.Scene(cornell["flat"])
    ocam = orc.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)
    want, _, _ = S.render(ocam, orc.make_env(**CORNELL_ENV), W, H, spp, DEPTH)
    S.set_watertight(True)
    want_wt, _, _ = S.render(ocam, orc.make_env(**CORNELL_ENV), W, H, spp, DEPTH)
    ctx = B.Context(0)
    ctx.upload_scene(cornell["entities"], np.stack([m for _, m, _ in cornell["materials"]]).astype(np.float32), env=B.make_env(**CORNELL_ENV))
    ctx.set_option("watertight", 1)
    got, _ = ctx.render(B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H), W, H, spp, DEPTH)
    ctx.close()
    a, b = want.astype(np.float64), got.astype(np.float64)
    lum = 0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]
    rel = float(np.sqrt(((a - b) ** 2).mean())) / float(lum.mean())
    same = float((_bits(want) == _bits(got)).all(-1).mean())
    print("watertight frame vs oracle, %dx%d at %d spp: relRMSE %.3e, %.1f %% of the pixels bit-identical" % (W, H, spp, rel, 100 * same))
    _report["frames"]["statistical_tie"] = dict(size=[W, H], spp=spp, rel_rmse=rel, identical_pixels=same)
    assert rel <= 1e-2, rel
    _same_frame(got, want_wt, "Cornell at %d spp == the watertight oracle" % spp)


# ---------------------------------------------------------------------------------------------------------------------
# three scenes where t, u, v reach the shading: interpolated normals, texels, refraction
# ---------------------------------------------------------------------------------------------------------------------
ORACLE_PATHS = [("default path", {}), ("group walk always", {"groups": 2}), ("fallback instance", {"fallback": 1}), ("subtracting slab form", {"box_exact": 1})]
PATH_RESET = {"groups": 1, "fallback": 0, "box_exact": -1}


def _rgba8(rng, h, w):
    px = rng.integers(0, 256, (h, w, 3)).astype(np.uint32)
    return (px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16) | (0xFF << 24)).astype(np.uint32)


def _smooth_icosphere(centre, radius):
    """rb.icosphere(2), 320 triangles whose neighbours share bit-identical float32 vertices; the normal of a vertex is its normalised
    position on the unit sphere, its texcoord a spherical map of it: whatever u, v a hit reports shows in the normal and in the texel."""
    unit = rb.icosphere(2).reshape(-1, 3)
    n = unit.astype(np.float64)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    tc = np.stack([np.arctan2(n[:, 2], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], 1)
    v = (unit * np.float32(radius) + np.float32(centre)).astype(np.float32)
    return dict(vertices=v, normals=n.astype(np.float32), texcoords=tc.astype(np.float32), indices=np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3))


def _scene_cube(cube):
    """The C1 cube of test_cube_image_bitwise_c1 (checker texture, sky environment) at 128 x 96, 16 spp, depth 4."""
    tex = scene_io.checker_texture()
    c = cube["camera"]
    return dict(ents=cube["entities"], mats=[m for _, m, _ in cube["materials"]], flat=cube["flat"], textures=[tex], mesh_textures=[0], env=dict(use_auto=True, intensity=1.0),
                cameras=[(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"])], size=(128, 96, 16, 4))


def _scene_materials():
    """The scene of test_material_coverage_image_bitwise (glass, clearcoat, sheen, metal: the car.json material set on spheres, a
    textured ground, an emitter) at its own size."""
    from owl_path_tracer_amd.pyhost import procedural

    _, car = scene_io.parse_scene(os.path.join(ASSETS, "car.json"))
    mats = [(n, m, "") for n, m, _ in car]
    meshes = []
    for i, (name, m, _) in enumerate(mats):
        if name == "Ground":
            meshes.append((name, procedural.quad((-6, 0, -6), (-6, 0, 6), (6, 0, 6), (6, 0, -6), (0, 1, 0), uv=True)))
        elif name == "Light":
            meshes.append((name, procedural.quad((-2, 4, -2), (2, 4, -2), (2, 4, 2), (-2, 4, 2), (0, -1, 0))))
        else:
            a = 2 * np.pi * i / len(mats)
            meshes.append((name, procedural.uv_sphere((2.2 * np.cos(a), 0.5, 2.2 * np.sin(a)), 0.5, nu=24, nv=12)))
    ents = scene_io.build_entities(meshes, mats)
    gi = [n for n, _, _ in mats].index("Ground")
    tex = scene_io.checker_texture(32, 32, 4)
    return dict(ents=ents, mats=[m for _, m, _ in mats], flat=scene_io.flatten_scene(ents, mats, {gi: tex}), textures=[tex], mesh_textures=[0 if mid == gi else -1 for _, mid in ents],
                env=dict(use_auto=True, intensity=0.6), cameras=[([0, 3.5, 6.5], [0, 0.4, 0], [0, 1, 0], 45)], size=(96, 64, 24, 16))


def _scene_icospheres():
    """A glass and a metallic icosphere, both smooth and textured, either side of a small emitter, under an environment map; one
    camera outside that looks at a vertex of the metallic mesh, one inside the glass sphere.  64 x 48, 33 spp, depth 16."""
    rng = np.random.default_rng(20260917)
    glass = scene_io.material(base_color=(0.95, 0.97, 1.0), specular_transmission=1.0, ior=1.5, roughness=0.05, specular_transmission_roughness=0.0)
    metal = scene_io.material(base_color=(0.9, 0.7, 0.4), metallic=1.0, roughness=0.25)
    glow = scene_io.material(emission=9.0)
    mats = [("glass", glass, ""), ("metal", metal, ""), ("glow", glow, "")]
    g_centre, m_centre = (-1.25, 0.1, 0.0), (1.2, -0.05, 0.15)
    metal_mesh = _smooth_icosphere(m_centre, 0.9)
    ents = [(_smooth_icosphere(g_centre, 1.0), 0), (metal_mesh, 1), (rb.mesh_of((rb.icosphere(1) * np.float32(0.22)).astype(np.float32)), 2)]
    tex = _rgba8(rng, 5, 7)
    envmap = _rgba8(rng, 8, 16)
    outside = np.float64([0.4, 1.1, 4.5])
    k = int(np.argmin(np.linalg.norm(metal_mesh["vertices"].astype(np.float64) - outside, axis=1)))  # the vertex nearest to the camera: it faces it
    cameras = [([float(x) for x in outside], [float(x) for x in metal_mesh["vertices"][k]], [0, 1, 0], 55.0),
               ([g_centre[0] + 0.31, g_centre[1] - 0.12, g_centre[2] + 0.2], [0.0, 0.0, 0.0], [0, 1, 0], 95.0)]
    return dict(ents=ents, mats=[m for _, m, _ in mats], flat=scene_io.flatten_scene(ents, mats, {0: tex, 1: tex}), textures=[tex], mesh_textures=[0, 0, -1],
                env=dict(use_map=True, intensity=1.0, env_map=envmap), cameras=cameras, size=(64, 48, 33, 16))


def _frames_against_the_oracle(orc, name, sc):
    """Every camera of the scene through the four paths with watertight = 1, against the oracle's watertight frame: float bits and
    RGBA8.  Returns, per camera, how many pixels of the oracle's frame differ from its switch-0 frame."""
    W, H, spp, depth = sc["size"]
    S = orc.Scene(sc["flat"])
    want, differ = [], []
    for frm, at, up, fov in sc["cameras"]:
        ocam = orc.to_camera_data(tuple(frm), tuple(at), tuple(up), fov, W, H)
        S.set_watertight(False)
        mt, _, _ = S.render(ocam, orc.make_env(**sc["env"]), W, H, spp, depth)
        S.set_watertight(True)
        wt, wt8, _ = S.render(ocam, orc.make_env(**sc["env"]), W, H, spp, depth, want_rgba8=True)
        assert np.isfinite(wt).all() and wt.std() > 0.01
        want.append((wt, wt8))
        differ.append(int((_bits(wt) != _bits(mt)).any(-1).sum()))
    ctx = B.Context(0)
    ctx.upload_scene(sc["ents"], sc["mats"], textures=sc["textures"], mesh_textures=sc["mesh_textures"], env=B.make_env(**sc["env"]))
    ctx.set_option("watertight", 1)
    try:
        for label, opts in ORACLE_PATHS:
            for k, v in opts.items():
                ctx.set_option(k, v)
            for i, (frm, at, up, fov) in enumerate(sc["cameras"]):
                got, got8 = ctx.render(B.to_camera_data(frm, at, up, fov, W, H), W, H, spp, depth, want_rgba8=True)
                st = ctx.stats()
                if "fallback" in opts:
                    assert st["kernel_variant"] == 3
                _same_frame(got, want[i][0], "%s, camera %d, %s" % (name, i, label))
                np.testing.assert_array_equal(got8, want[i][1])
            for k in opts:
                ctx.set_option(k, PATH_RESET[k])
    finally:
        ctx.close()
    _report["frames_against_the_oracle"][name] = dict(size=[W, H], spp=spp, depth=depth, paths=[p[0] for p in ORACLE_PATHS], pixels=W * H, pixels_that_differ_from_switch_0=differ)
    print(name, _report["frames_against_the_oracle"][name])
    return differ


def test_cube_frame_is_the_watertight_oracles(orc, cube):
    _frames_against_the_oracle(orc, "cube", _scene_cube(cube))


def test_material_coverage_frame_is_the_watertight_oracles(orc):
    _frames_against_the_oracle(orc, "material_coverage", _scene_materials())


def test_smooth_icosphere_frames_are_the_watertight_oracles(orc):
    """On this scene a u / v exchange or a wrong t changes the interpolated normal, the texel and the refracted ray.  That the frames
    are frames of the option and not of the other test: 395 of the 3 072 pixels of the oracle's frame from outside and 1 137 of the
    frame from inside the glass differ in bits from its switch-0 frame (material coverage: 1 641 of 6 144; the cube, whose
    coordinates are small integers: 0 of 12 288 - there both tests are exact)."""
    differ = _frames_against_the_oracle(orc, "smooth_icospheres", _scene_icospheres())
    assert all(d > 0 for d in differ), differ


def test_the_three_refusals(cornell_wt):
    ctx, cam = cornell_wt["ctx"], cornell_wt["cam"]
    invalid = r"\(-1\)"  # PT_E_INVALID
    with pytest.raises(B.PtError, match=invalid) as e:
        ctx.set_option("kernel", 1)
    assert "watertight" in str(e.value)
    rays = np.tile(np.float32([0, 1, 3, 0, 0, -1]), (4, 1))
    with pytest.raises(B.PtError, match=invalid) as e:
        ctx.debug_eval("closest_hit", rays, 5)
    assert "watertight" in str(e.value)
    frames = [(cam, None), (cam, cornell_wt["mats"])]
    with pytest.raises(B.PtError, match=invalid) as e:
        ctx.render_batch(frames, W_, H_, SPP, DEPTH, n_materials=cornell_wt["mats"].shape[0])
    assert "watertight" in str(e.value)
    # nothing was rendered with the other test instead, and the context still renders
    got, _ = ctx.render(cam, W_, H_, SPP, DEPTH)
    _same_frame(got, cornell_wt["wt"], "after the refusals")
    ctx.debug_eval("quad", rays, 6)


def test_pt_main_watertight_flag(cornell_wt, tmp_path):
    """`pt_main --watertight` on the Cornell box at the fixture's size: the PNG is the binding's RGBA8 frame with watertight = 1 and not
    the one without the flag; `--watertight --batch 2` exits 1 with a message."""
    from PIL import Image

    a = tmp_path / "assets"
    shutil.copytree(ASSETS, a)
    s = json.load(open(os.path.join(ASSETS, "configs", "c2_cornell-box.json")))
    s.update(buffer_size=[W_, H_], max_samples=SPP, max_path_depth=DEPTH)
    sphere = [m for _, m, _ in scene_io.load_scene_dir(ASSETS, "cornell-box")["materials"]][1]
    s["test"] = dict(name="wt", material_name="sphere", attribute_name="metallic", material_type=2, values=[float(sphere[4]), float(sphere[4])], step_size=1.0)
    (a / "settings.json").write_text(json.dumps(s))
    name = "cornell-box_wt_metallic(%.1f).png" % float(sphere[4])
    imgs = {}
    for flag in ([], ["--watertight"]):
        d = tmp_path / ("out%d" % len(flag))
        os.makedirs(d)
        r = subprocess.run([PT_MAIN, "--assets", str(a), "--out", str(d)] + flag, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        imgs[len(flag)] = np.asarray(Image.open(d / name)).view(np.uint32).reshape(H_, W_)
    np.testing.assert_array_equal(imgs[1], cornell_wt["wt8"])
    assert (imgs[0] != imgs[1]).any()
    r = subprocess.run([PT_MAIN, "--assets", str(a), "--out", str(tmp_path), "--watertight", "--batch", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and r.stderr.startswith("error: ") and "--watertight" in r.stderr, r.stderr[-1000:]


def test_zz_write_profile():
    """Last in the file: the figures gathered above, with PT_WRITE_PROFILES=1 (and the whole file run)."""
    if os.environ.get("PT_WRITE_PROFILES") != "1" or len(_report["probes"]) != len(SMALL_SCENES):
        return
    path = os.path.join(ROOT, "profiles", "r09_watertight.json")
    whole = {}
    if os.path.exists(path):
        with open(path) as fh:
            whole = json.load(fh)
    whole["gpu"] = _report  # (the oracle's own figures - battery rays, fuzz cases - are section "oracle": tests/test_oracle_watertight.py)
    with open(path, "w") as fh:
        json.dump(whole, fh, indent=1, sort_keys=True)
