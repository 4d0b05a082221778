"""The guide kernels on random scenes, bit for bit, no pixel left out (the beauty path has tests/test_gpu_fuzz.py; this is the guide path's).

* RANDOM CASES (tests/guide_fuzz_common.py: bad normals, NaN materials, emitters that would be followed, ior 1 / NaN / 0 / inf, roughness at
  and just above roughness_max, mw == gw, material_index -1, max_follow up to 8, coincident and degenerate geometry, textures), each on one
  of: a device-built tree, leaf_size 1 / 4 / 7, a forced slab form, the binary walk, a pixel shard with tile 1 / 4 / 16 / 32.
  pt_render_aov_follow, pt_render_aov and pt_render_aov_follow at max_follow = 0 against tests/aov_follow_ref.py / tests/aov_ref.py and
  against the CPU twins; with watertight 0 also pt_render_aov_batch of 2..4 frames (own camera, own table or None) against the
  restatement, the twin and pt_set_materials + pt_render_aov_follow on the same context.  After every call pt_synchronize reports no
  error (the walk's step and stack bounds raise it), pt_get_stats one launch and at most 128 VGPRs.  48 cases by default in two
  functions; PT_GUIDE_FUZZ_CASES / _SEED / _ONLY as in guide_fuzz_common.py; a failure prints the seed.
* Every fourth case, and every case whose GPU guide buffers hold a non-finite value, sends those buffers and a seeded random frame through
  pt_denoise: == pt_debug_denoise_host, RGBA8 included.  Each half of the default seed set has such a non-finite case (asserted).
* The census of the host file over the 48 seeds that run here: every branch occurs in at least one case.
* THE HBM OVERFLOW COLUMN OF THE GUIDE KERNELS (sized and indexed by their own code, pt_guides.cpp A.cap / blockIdx.x * ovf_levels * 64):
  the sliver strip at leaf_size 1 seen along its axis.  Precondition, asserted: at least 5 % of the frame's sample-0 camera rays push
  past LDS entry 12 (probe op quad_ovf).  First-hit and follow (the far wall turned mirror: the follow rays walk the strip back), both
  triangle tests, both slab forms, and the batch form with K = 3.  What this can see: the column is sized for stack_entries + 3 = 31
  entries, 19 of them in HBM, and the strip's walks reach entry 25 (14 HBM levels).  A missing blockIdx term, a wrong lane term or a
  column stride of fewer than 14 levels makes waves overwrite each other's entries and changes pixels.  A stride short by one to
  five levels does not: the three spare entries and the gap between the bound 28 and the deepest walk are never written, so no
  correct walk can show it.
* MORE 8 x 8 BLOCKS THAN WAVES IN ONE FRAME: mirror_wall at 1048 x 520 (asserted against pt_get_stats' grid), unsharded and as rank 1 of
  3: the wrapped block loop and the `continue`s inside it.
* TILE ROUNDING: tiles 1, 4, 8 deal alike and 9 as 16; the three ranks sum bit for bit to the unsharded frame.
* A SCENE THAT IS ONE LEAF (no nodes of any kind; found by the random cases: the guide pass sent it to the binary walk and so refused it
  with watertight = 1): served by the quad instances with both triangle tests, refused only with quad = 0.
PT_WRITE_PROFILES=1 writes the counts to profiles/r17_guide_fuzz.json, section "gpu"."""
import time

import numpy as np
import pytest

import aov_follow_common as FC
import aov_follow_ref
import aov_ref
import ray_battery as rb
import guide_fuzz_common as G
from owl_path_tracer_amd.pyhost import binding as B, scene_io

pytestmark = pytest.mark.gpu

F32 = np.float32
N_DEFAULT = 48
DEFAULT_SEEDS = [G.DEFAULT_SEED0 + i for i in range(N_DEFAULT)]


def _after(ctx, what):
    """No walk ran out of its step or stack bound; one launch; the four-waves-per-SIMD register budget."""
    ctx.synchronize()
    st = ctx.stats()
    assert st["launches"] == 1 and st["block"] == 64 and 0 < st["vgprs"] <= 128, (what, st)
    return st


def _owned(W, H, shard):
    own = np.zeros(W * H, bool)
    own[B.shard_pixels(W, H, shard[2], shard[0], shard[1])] = True
    return own.reshape(H, W)[::-1]  # framebuffer order


def _case(gpu, host, orc, seed, denoise):
    """One case on `gpu`; returns (frames compared, pixels compared, denoise chain run, its guide buffers held a non-finite value).  The
    chain runs where `denoise` says so and wherever the GPU's guide buffers hold a non-finite value."""
    r, t = G.reference(orc, seed), G.twin(B, seed)
    c = r["case"]
    W, H, n = c["W"], c["H"], c["n"]
    cam, prm = G.bcamera(B, c), G.params(B, c)
    own = _owned(W, H, c["shard"]) if c["shard"] else None
    want = lambda a: a if own is None else np.where(own[..., None], a, F32(0.0))  # the other ranks' pixels are +0
    frames, chained, bad_guides = 0, False, False
    try:
        if c["option"] and c["option"][0] in G.AT_UPLOAD:
            gpu.set_option(*c["option"])
        gpu.upload_scene(c["ents"], c["mats"], textures=c["texs"], mesh_textures=c["mesh_tex"], env=B.make_env(**c["env"]))
        if c["option"] and c["option"][0] not in G.AT_UPLOAD:
            gpu.set_option(*c["option"])
        gpu.set_option("watertight", c["wt"])
        if c["shard"]:
            gpu.set_pixel_shard(*c["shard"])
        follow = gpu.render_aov_follow(cam, W, H, prm)
        _after(gpu, G.describe(c))
        G.assert_same(follow, want(r["follow"]), c, "pt_render_aov_follow vs aov_follow_ref")
        G.assert_same(follow, want(t["follow"]), c, "pt_render_aov_follow vs pt_debug_aov_follow_host")
        first = gpu.render_aov(cam, W, H, n)
        _after(gpu, G.describe(c))
        G.assert_same(first, want(r["first"]), c, "pt_render_aov vs aov_ref")
        G.assert_same(first, want(t["first"]), c, "pt_render_aov vs pt_debug_aov_host")
        follow0 = gpu.render_aov_follow(cam, W, H, G.params(B, c, 0))
        _after(gpu, G.describe(c))
        G.assert_same(follow0, first, c, "pt_render_aov_follow at max_follow = 0 vs pt_render_aov")
        G.assert_same(follow0, want(t["follow0"]), c, "pt_render_aov_follow at max_follow = 0 vs the twin")
        frames += 3
        if c["batch"] is not None:
            fr = [(G.bcamera(B, c, fcam), table) for fcam, table in c["batch"]]
            out = gpu.render_aov_batch(fr, W, H, prm, n_materials=c["mats"].shape[0])
            _after(gpu, G.describe(c))
            for f, (fcam, table) in enumerate(fr):
                G.assert_same(out[f], want(r["batch"][f]), c, "pt_render_aov_batch, frame %d of %d vs aov_follow_ref" % (f, len(fr)))
                G.assert_same(out[f], want(t["batch"][f]), c, "pt_render_aov_batch, frame %d of %d vs the twin" % (f, len(fr)))
                gpu.set_materials(c["mats"] if table is None else table)
                G.assert_same(out[f], gpu.render_aov_follow(fcam, W, H, prm), c, "pt_render_aov_batch, frame %d of %d vs pt_set_materials + pt_render_aov_follow" % (f, len(fr)))
                _after(gpu, G.describe(c))
            frames += len(fr)
        bad_guides = not np.isfinite(follow).all()
        chained = bool(denoise or bad_guides)
        if chained:
            rgb = np.random.default_rng(seed).uniform(0.0, 4.0, (H, W, 3)).astype(F32)
            dp = B.denoise_default_params(iterations=3, flags=B.PT_DENOISE_DEMODULATE if seed & 4 else 0)
            got, got8 = gpu.denoise(rgb, follow, dp, want_rgba8=True)
            gpu.synchronize()
            ref, ref8 = host.denoise_host(rgb, follow, dp, want_rgba8=True)
            bad = G.bits(got) != G.bits(ref)
            assert not bad.any(), "%s: pt_denoise of the GPU's guide buffers vs pt_debug_denoise_host: %d of %d floats differ in bits" % (G.describe(c), int(bad.sum()), bad.size)
            assert (got8 == ref8).all(), "%s: pt_denoise RGBA8 differs from pt_debug_denoise_host" % G.describe(c)
    finally:
        gpu.set_pixel_shard(0, 1, 16)
        gpu.set_option("watertight", 0)
        if c["option"]:
            gpu.set_option(c["option"][0], G.OPTION_DEFAULTS[c["option"][0]])
    return frames, frames * W * H, chained, bad_guides


def _random_cases(orc, part, parts):
    seeds = G.seeds(N_DEFAULT)
    mine = [s for i, s in enumerate(seeds) if i * parts // len(seeds) == part]
    gpu, host = B.Context(0), B.Context(-1)
    t0 = time.time()
    frames = pixels = chains = bad_chains = 0
    try:
        for seed in mine:
            f, p, chained, bad_guides = _case(gpu, host, orc, seed, (seed - seeds[0]) % 4 == 0)
            frames, pixels, chains, bad_chains = frames + f, pixels + p, chains + chained, bad_chains + bad_guides
    finally:
        gpu.close()
        host.close()
    seconds = time.time() - t0
    print("guide fuzz, part %d of %d: %d cases, %d frames, %d pixels compared bit for bit with restatement and twin, none left out; %d denoise chains, %d of them on non-finite "
          "guide buffers (%.1f s)" % (part + 1, parts, len(mine), frames, pixels, chains, bad_chains, seconds))
    G.write_profile("gpu", {"random_cases_part_%d" % (part + 1): dict(seed0=mine[0] if mine else None, cases=len(mine), frames_compared=frames, pixels_compared=pixels,
                                                                      pixels_left_out=0, denoise_chains=chains, denoise_chains_on_non_finite_guides=bad_chains,
                                                                      seconds=round(seconds, 1))})
    if seeds == DEFAULT_SEEDS:  # (a property of the default seed set: each half holds frames with non-finite guide values)
        assert bad_chains >= 1, "no denoise chain of this half ran on non-finite guide buffers"


def test_random_cases_bitwise_first_half(orc):
    _random_cases(orc, 0, 2)


def test_random_cases_bitwise_second_half(orc):
    _random_cases(orc, 1, 2)


def test_the_gpu_seed_set_takes_every_branch(orc):
    """The census of test_guide_fuzz_host.py restricted to the 48 seeds that run on the device (from the restatement's log, which the two
    functions above hold the kernels to bit for bit): every branch occurs in at least one of them."""
    cases, samples = G.census_of(orc, DEFAULT_SEEDS)
    for k in G.CENSUS_KEYS:
        print("%-40s %3d cases %8d samples" % (k, cases[k], samples[k]))
    G.write_profile("gpu", dict(census_of_the_gpu_seed_set={k: dict(cases=cases[k], samples=samples[k]) for k in G.CENSUS_KEYS}))
    missing = [k for k in G.CENSUS_KEYS if cases[k] < 1]
    assert not missing, "no case of the GPU's default seed set takes these branches: %r" % missing


def _strip_case(wt, **kw):
    return dict(dict(seed=-1, W=G.STRIP_W, H=G.STRIP_H, n=G.STRIP_N, max_follow=G.STRIP_MAX_FOLLOW, roughness_max=G.STRIP_ROUGHNESS_MAX, wt=wt, option=("leaf_size", 1), shard=None,
                     ents=G.strip_scene()["ents"]), **kw)


def test_overflow_column_of_the_guide_kernels(orc):
    sc = G.strip_scene()
    W, H, n = G.STRIP_W, G.STRIP_H, G.STRIP_N
    cam = G.strip_camera(B.to_camera_data)
    prm = B.aov_default_params(n_samples=n, max_follow=G.STRIP_MAX_FOLLOW, roughness_max=G.STRIP_ROUGHNESS_MAX)
    own_table = np.stack(sc["mats"]).astype(F32)
    ctx, t0 = B.Context(0), time.time()
    try:
        ctx.set_option("leaf_size", 1)
        ctx.upload_scene(sc["ents"], sc["mats"], textures=sc["textures"], mesh_textures=sc["mesh_textures"], env=B.make_env(**sc["env"]))
        stack_entries = 3 * ctx.export_trees()["depth4"] + 1
        assert stack_entries > B.PT_LDS_STACK
        # the precondition: the frame's own camera rays push past the LDS part of the stack
        rays = aov_ref.camera_rays(G.strip_camera(orc.to_camera_data).as_array(), W, H, 1, np.arange(W * H)).reshape(-1, 6)
        deepest = ctx.debug_eval("quad_ovf", rays, 6)[:, 5]
        share = float((deepest > B.PT_LDS_STACK).mean())
        print("strip: %.1f %% of the %d sample-0 camera rays push past LDS entry %d (deepest %d of %d)" % (100 * share, rays.shape[0], B.PT_LDS_STACK, deepest.max(), stack_entries))
        report = dict(share_of_probe_rays_past_lds_entry_12=share, deepest_stack_entry=int(deepest.max()), stack_entries=stack_entries)
        assert share >= 0.05
        compared = 0
        for wt in (0, 1):
            r, t = G.strip_reference(orc, wt), G.strip_twin(B, wt)
            ctx.set_option("watertight", wt)
            for be in (0, 1):
                ctx.set_option("box_exact", be)
                c = _strip_case(wt, option=("leaf_size 1, box_exact", be))
                ctx.set_materials(own_table)
                first = ctx.render_aov(cam, W, H, n)
                assert _after(ctx, c)["stack_entries"] == stack_entries
                G.assert_same(first, r["first"], c, "pt_render_aov vs aov_ref")
                G.assert_same(first, t["first"], c, "pt_render_aov vs pt_debug_aov_host")
                ctx.set_materials(sc["mirror"])
                follow = ctx.render_aov_follow(cam, W, H, prm)
                assert _after(ctx, c)["stack_entries"] == stack_entries
                G.assert_same(follow, r["follow"], c, "pt_render_aov_follow, the wall a mirror, vs aov_follow_ref")
                G.assert_same(follow, t["follow"], c, "pt_render_aov_follow, the wall a mirror, vs pt_debug_aov_follow_host")
                compared += 2
                if not wt:  # context's table: the mirror; frame 1 takes it (None), frame 2 the wall diffuse
                    fr = [(G.strip_camera(B.to_camera_data, dy), (sc["mirror"], None, own_table)[f]) for f, dy in enumerate(G.STRIP_SHIFTS_Y)]
                    out = ctx.render_aov_batch(fr, W, H, prm, n_materials=2)
                    assert _after(ctx, c)["stack_entries"] == stack_entries
                    for f, (fcam, table) in enumerate(fr):
                        G.assert_same(out[f], r["batch"][f], c, "pt_render_aov_batch, frame %d vs aov_follow_ref" % f)
                        G.assert_same(out[f], t["batch"][f], c, "pt_render_aov_batch, frame %d vs the twin" % f)
                        ctx.set_materials(sc["mirror"] if table is None else table)
                        G.assert_same(out[f], ctx.render_aov_follow(fcam, W, H, prm), c, "pt_render_aov_batch, frame %d vs pt_set_materials + pt_render_aov_follow" % f)
                        _after(ctx, c)
                    compared += len(fr)
        report.update(frames_compared=compared, pixels_compared=compared * W * H, seconds=round(time.time() - t0, 1))
        G.write_profile("gpu", dict(overflow=report))
    finally:
        ctx.close()


_wall = {}


def _wall_twin(W, H, n, prm):
    """(first, follow) of mirror_wall from the CPU twins, once per size."""
    key = (W, H, n)
    if key not in _wall:
        h = B.Context(-1)
        try:
            FC.upload(h, FC.scene("mirror_wall"), B)
            cam = FC.camera(FC.scene("mirror_wall"), W, H, B.to_camera_data)
            _wall[key] = (h.aov_host(cam, W, H, n), h.aov_follow_host(cam, W, H, prm))
        finally:
            h.close()
    return _wall[key]


def test_more_blocks_than_waves_in_one_frame():
    W, H, n = 1048, 520, 1
    prm = FC.params(B, n, 4, 0.3)
    sc = FC.scene("mirror_wall")
    cam = FC.camera(sc, W, H, B.to_camera_data)
    first_t, follow_t = _wall_twin(W, H, n, prm)
    assert (FC.bits(first_t) != FC.bits(follow_t)).any()
    blocks = ((W + 7) // 8) * ((H + 7) // 8)
    ctx, t0 = B.Context(0), time.time()
    try:
        FC.upload(ctx, sc, B)
        for shard in (None, (1, 3, 16)):
            want = (lambda a: a) if shard is None else (lambda a, own=_owned(W, H, shard): np.where(own[..., None], a, F32(0.0)))
            if shard:
                ctx.set_pixel_shard(*shard)
            first = ctx.render_aov(cam, W, H, n)
            st = _after(ctx, "mirror_wall %dx%d" % (W, H))
            assert 0 < st["grid"] < blocks, "the frame must have more 8 x 8 blocks (%d) than the launch has waves (%d)" % (blocks, st["grid"])
            FC.assert_same(first, want(first_t), "pt_render_aov %dx%d, shard %s vs the twin" % (W, H, shard))
            follow = ctx.render_aov_follow(cam, W, H, prm)
            st = _after(ctx, "mirror_wall %dx%d" % (W, H))
            assert 0 < st["grid"] < blocks
            FC.assert_same(follow, want(follow_t), "pt_render_aov_follow %dx%d, shard %s vs the twin" % (W, H, shard))
        print("mirror_wall %dx%d: %d blocks of 8 x 8 on a grid of %d waves" % (W, H, blocks, st["grid"]))
        G.write_profile("gpu", dict(wrap=dict(width=W, height=H, blocks=blocks, grid=st["grid"], pixels_compared=4 * W * H, seconds=round(time.time() - t0, 1))))
    finally:
        ctx.set_pixel_shard(0, 1, 16)
        ctx.close()


def test_tile_rounding():
    """pt_guides.cpp rounds a shard tile up to a multiple of 8 (at least 8) as pt_shard_pixels does: 1, 4 and 8 are one dealing, 9 is 16's."""
    W, H, n, world = 40, 32, 2, 3
    prm = FC.params(B, n, 4, 0.3)
    sc = FC.scene("mirror_wall")
    cam = FC.camera(sc, W, H, B.to_camera_data)
    ctx = B.Context(0)
    try:
        FC.upload(ctx, sc, B)
        full = {"follow": ctx.render_aov_follow(cam, W, H, prm), "first": ctx.render_aov(cam, W, H, n)}
        first_t, follow_t = _wall_twin(W, H, n, prm)
        FC.assert_same(full["follow"], follow_t, "unsharded follow vs the twin")
        FC.assert_same(full["first"], first_t, "unsharded first hit vs the twin")
        parts = {}
        for tile in (1, 4, 8, 9, 16):
            total = {k: np.zeros_like(v) for k, v in full.items()}
            for rank in range(world):
                ctx.set_pixel_shard(rank, world, tile)
                got = {"follow": ctx.render_aov_follow(cam, W, H, prm), "first": ctx.render_aov(cam, W, H, n)}
                _after(ctx, "tile %d rank %d" % (tile, rank))
                own = _owned(W, H, (rank, world, tile))
                assert own.any() and not own.all()
                for k in got:
                    FC.assert_same(got[k], np.where(own[..., None], full[k], F32(0.0)), "tile %d, rank %d of %d, %s: owned pixels as unsharded, the others +0" % (tile, rank, world, k))
                    total[k] = total[k] + got[k]
                parts[tile, rank] = got
            for k in full:
                FC.assert_same(total[k], full[k], "tile %d, %s: the sum of the %d ranks" % (tile, k, world))
        for rank in range(world):
            for k in full:
                for tile in (4, 8):
                    FC.assert_same(parts[tile, rank][k], parts[1, rank][k], "rank %d, %s: tile %d deals as tile 1" % (rank, k, tile))
                FC.assert_same(parts[9, rank][k], parts[16, rank][k], "rank %d, %s: tile 9 deals as tile 16" % (rank, k))
        assert any((FC.bits(parts[8, r]["follow"]) != FC.bits(parts[16, r]["follow"])).any() for r in range(world)), "tiles 8 and 16 must deal differently at 40 x 32"
    finally:
        ctx.set_pixel_shard(0, 1, 16)
        ctx.close()


def test_scene_of_one_leaf(orc):
    """Three triangles under leaf_size 4: the root is a leaf, there are no quad nodes.  The walk of the quad instances is then one leaf
    step, so "watertight" = 1 is served like any other scene; only "quad" = 0 leaves the binary walk, which refuses it."""
    W, H, n = 19, 13, 2
    ents, mats = [(rb.mesh_of(rb.make_scene("one_leaf")), 0)], [scene_io.material(base_color=(0.9, 0.6, 0.3), metallic=1.0, roughness=0.0)]
    env = dict(color=(0.2, 0.5, 0.9), intensity=1.5)
    look = ((0.6, 0.9, 2.5), (0.4, 0.3, 0.0), (0, 1, 0), 50.0)
    cam, prm = B.to_camera_data(*look, W, H), FC.params(B, n, 4, 0.3)
    flat = scene_io.flatten_scene(ents, [("mirror", mats[0], "")])
    ctx, host = B.Context(0), B.Context(-1)
    try:
        for c in (ctx, host):
            c.upload_scene(ents, mats, env=B.make_env(**env))
        assert ctx.export_trees()["nodes4"].size == 0 and ctx.export_trees()["root4"] < -1
        for wt in (0, 1):
            S = orc.Scene(flat, watertight=bool(wt))
            ocam = orc.to_camera_data(*look, W, H).as_array()
            want_first, want_follow = aov_ref.aov(S, flat, env, ocam, W, H, n), aov_follow_ref.aov(S, flat, env, ocam, W, H, n, 4, 0.3)
            assert (FC.bits(want_first) != FC.bits(want_follow)).any() and want_first[..., 3].min() == 0 and want_first[..., 3].max() == 1
            for c in (ctx, host):
                c.set_option("watertight", wt)
            first = ctx.render_aov(cam, W, H, n)
            assert _after(ctx, "one leaf, watertight %d" % wt)["stack_entries"] == 1
            FC.assert_same(first, want_first, "one leaf, watertight %d: pt_render_aov vs aov_ref" % wt)
            FC.assert_same(first, host.aov_host(cam, W, H, n), "one leaf, watertight %d: pt_render_aov vs the twin" % wt)
            follow = ctx.render_aov_follow(cam, W, H, prm)
            _after(ctx, "one leaf, watertight %d" % wt)
            FC.assert_same(follow, want_follow, "one leaf, watertight %d: pt_render_aov_follow vs aov_follow_ref" % wt)
            FC.assert_same(follow, host.aov_follow_host(cam, W, H, prm), "one leaf, watertight %d: pt_render_aov_follow vs the twin" % wt)
        ctx.set_option("quad", 0)  # (watertight is 1)
        for call in (lambda: ctx.render_aov(cam, W, H, n), lambda: ctx.render_aov_follow(cam, W, H, prm)):
            with pytest.raises(B.PtError, match=r"\(-1\)") as e:
                call()
            assert "watertight" in str(e.value) and "quad" in str(e.value)
        ctx.set_option("watertight", 0)
        FC.assert_same(ctx.render_aov_follow(cam, W, H, prm), aov_follow_ref.aov(orc.Scene(flat), flat, env, ocam, W, H, n, 4, 0.3), "one leaf, quad = 0: the binary walk")
    finally:
        ctx.close()
        host.close()
