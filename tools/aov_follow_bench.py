"""What the follow mode of the guide pass costs and what it buys (pt_render_aov_follow).

    python tools/aov_follow_bench.py [--size 1920x1080] [--samples 4] [--repeats 20] [--warmup 3] [--out profiles/r15_aov_follow.json]
    python tools/aov_follow_bench.py --quality [--out profiles/r15_aov_follow.json]

Cost (one MI355X; without a GPU the tool fails, there is no fallback).  kernel_ms of pt_stats - HIP events around the one launch - median
of --repeats runs after --warmup runs, the three calls alternating so that all see the same machine:
  * pt_render_aov against pt_render_aov_follow at max_follow 0 and 4 on the C4 stand-in, which has no followed surface: the price of the
    mode where it does nothing;
  * the same on the glass and metal icospheres under the environment map (tests/aov_common.py "ico_map"): the price where it works.
The comparison basis is pt_render_aov in the same run.  The follow buffers at max_follow 0 are compared with pt_render_aov's, bit for bit.

Quality (--quality; CPU only: the oracle and the twins).  An 8 spp frame of the oracle filtered by pt_debug_denoise_host (defaults +
PT_DENOISE_DEMODULATE) with first-hit guides and with follow guides (twins, n = 4), relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2)))
against the oracle's high-sample frame: mirror_wall 64 x 48 against 1024 spp over the pixels whose first hit is the mirror or the pane
(what tests/test_aov_follow_host.py asserts), and ico_map 256 x 192 against 2048 spp over the whole frame and over the pixels the two
guide sets differ in.

Each mode writes its own section of --out and leaves the other as it is.  Measurement only: nothing here is asserted by the test suite."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cost(a, B):
    import aov_common as AC
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    W, H = (int(x) for x in a.size.split("x"))
    n = a.samples
    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ico = AC.scene("ico_map")
    frm, at, up, fov = ico["camera"]
    scenes = [("C4 stand-in (dragon.json on procedural.dragon_standin), black environment: no followed surface",
               lambda c: c.upload_scene(scene_io.build_entities(procedural.dragon_standin(), mats), [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=0.0)),
               B.to_camera_data([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, W, H)),
              ("glass and metal icospheres under an environment map (tests/aov_common.py ico_map)", lambda c: AC.upload(c, ico, B),
               B.to_camera_data(tuple(frm), tuple(at), tuple(up), fov, W, H))]
    rows = []
    for what, upload, cam in scenes:
        ctx = B.Context(0)  # raises without a gfx950 device
        try:
            upload(ctx)
            calls = [("pt_render_aov", lambda: ctx.render_aov(cam, W, H, n)),
                     ("pt_render_aov_follow, max_follow 0", lambda: ctx.render_aov_follow(cam, W, H, B.aov_default_params(n_samples=n, max_follow=0))),
                     ("pt_render_aov_follow, max_follow 4", lambda: ctx.render_aov_follow(cam, W, H, B.aov_default_params(n_samples=n, max_follow=4)))]
            ms = {k: [] for k, _ in calls}
            geo, buf = {}, {}
            for i in range(a.warmup + a.repeats):
                for k, f in calls:
                    buf[k] = f()
                    st = ctx.stats()
                    if i >= a.warmup:
                        ms[k].append(st["kernel_ms"])
                    geo[k] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], grid=st["grid"])
            same0 = bool((bits(buf[calls[0][0]]) == bits(buf[calls[1][0]])).all())
            followed = float((bits(buf[calls[0][0]]) != bits(buf[calls[2][0]])).any(-1).mean())
        finally:
            ctx.close()
        base = statistics.median(ms[calls[0][0]])
        row = dict(scene=what, kernel_ms={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in ms.items()},
                   over_pt_render_aov={k: statistics.median(v) / base for k, v in ms.items()}, launch=geo, max_follow_0_bit_identical_to_pt_render_aov=same0,
                   pixels_changed_by_max_follow_4=followed)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not same0:
            raise SystemExit("max_follow = 0 differs from pt_render_aov")
    return dict(size=[W, H], n_samples=n, repeats=a.repeats, warmup=a.warmup, timer="pt_stats.kernel_ms (HIP events around the launch), median", measured=True, rows=rows)


def quality(B):
    import aov_follow_common as FC
    import oracle as orc

    rows = []
    for name, W, H, spp_ref in (("mirror_wall", 64, 48, 1024), ("ico_map", 256, 192, 2048)):
        sc = FC.scene(name)
        S = orc.Scene(sc["flat"])
        ocam = FC.camera(sc, W, H, orc.to_camera_data)
        env = orc.make_env(**sc["env"])
        noisy, _, _ = S.render(ocam, env, W, H, 8, 8)
        ref, _, _ = S.render(ocam, env, W, H, spp_ref, 8)
        ctx = B.Context(-1)
        try:
            FC.upload(ctx, sc, B)
            cam = FC.camera(sc, W, H, B.to_camera_data)
            prm = B.denoise_default_params(flags=B.PT_DENOISE_DEMODULATE)
            g_first, g_follow = ctx.aov_host(cam, W, H, 4), ctx.aov_follow_host(cam, W, H, B.aov_default_params(n_samples=4))
            with_first, _ = ctx.denoise_host(noisy, g_first, prm)
            with_follow, _ = ctx.denoise_host(noisy, g_follow, prm)
            one = ctx.aov_host(cam, W, H, 1)
        finally:
            ctx.close()
        masks = {"whole frame": np.ones((H, W), bool), "pixels the two guide sets differ in": (bits(g_first) != bits(g_follow)).any(-1)}
        if name == "mirror_wall":  # the test's mask: sample 0's first hit is the mirror or the pane (their albedos, from the first-hit twin at n = 1)
            glass = np.float32(sc["mats"][FC.M_GLASS][:3])
            masks["first hit is the mirror or the pane"] = (one[..., :3] == np.float32(FC.MIRROR_COLOUR)).all(-1) | (one[..., :3] == glass).all(-1)
        row = dict(scene=name, size=[W, H], spp=[8, spp_ref], guides="twins at n = 4; follow: default parameters (max_follow 4, roughness_max 0.3)", rel_rmse={})
        for k, m in masks.items():
            row["rel_rmse"][k] = dict(pixels=int(m.sum()), noisy=rel_rmse(noisy[m], ref[m]), filtered_with_first_hit_guides=rel_rmse(with_first[m], ref[m]),
                                      filtered_with_follow_guides=rel_rmse(with_follow[m], ref[m]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(metric="relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))); filter: pt_debug_denoise_host, default parameters + PT_DENOISE_DEMODULATE", rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_aov_follow.json"))
    a = ap.parse_args()
    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.quality:
        rec["quality"] = quality(B)
    else:
        rec["cost"] = cost(a, B)
    rec.setdefault("cost", dict(measured=False, note="not recorded yet: needs an MI355X (python tools/aov_follow_bench.py)"))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
