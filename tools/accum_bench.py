"""What splitting a frame into adds costs and what adaptive adds buy (pt_accum_*; include/mi355pt.h, "progressive accumulation").

    python tools/accum_bench.py [--repeats 20] [--warmup 3] [--frames FILE.npz] [--out profiles/r17_accum.json]
    python tools/accum_bench.py --quality --frames FILE.npz [--out profiles/r17_accum.json]

Cost (one MI355X; without a GPU the tool fails, there is no fallback).  Two scenes: C2 (assets/configs/c2_cornell-box.json: Cornell at
512 x 512, depth 16) and the C4 stand-in of bench.py at 1920 x 1080, depth 16; 256 samples per pixel.  Every figure is the median of
--repeats runs after --warmup runs, the variants alternating inside a repetition so that all see the same machine.  Two clocks: the sum of
pt_stats.kernel_ms of the calls (HIP events: first launch .. end of resolve) and the host clock around the blocking calls (read-back of the
last image included, as pt_render's includes its own).
  (a) splitting: K = 1, 2, 4, 16 uniform adds of 256 / K samples against pt_render(256) in the same run, and 1024 samples in 2 and 4 adds
      against pt_render(1024) (adds of 512 and 256 samples: where splitting stops mattering); the frames are compared bit for bit.
      "no render": an add whose active set is empty (every pixel at its cap) - select, the 4-byte count to the host, resolve - i.e. what an
      add costs beside its render launches.
  (b) adaptive, with the scene LIT (environment use_auto = 1, intensity 1, as tests/test_gpu_accum.py: under the black environment of the
      two configurations more than half the pixels are exactly 0 and have noise 0, so no threshold leaves half of them active): 16 + 16
      uniform samples, threshold = the median of the noise map (half the pixels stay active), then adds of 32 with that threshold and a
      cap of 256 until none is active; against uniform adds to the same cap (16 + 16 + 7 x 32) and pt_render(256) of the lit scene.
      --frames: the C2 frames of both and the sample map, for --quality.
Quality (--quality; CPU only): relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) of the two C2 frames of (b) against the oracle's
2048-spp frame of the lit scene, as tools/aov_follow_bench.py --quality computes it.

Each mode writes its own section of --out and leaves the other as it is.  Measurement only: nothing here is asserted by the test suite."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

SPP, CAP, SPP_BIG = 256, 256, 1024
LIT = dict(use_auto=True, intensity=1.0)  # the environment of part (b)


# what each variant is set against
BASE = {"pt_render(1024)": "pt_render(1024)", "1024 in 2": "pt_render(1024)", "1024 in 4": "pt_render(1024)", "pt_render, lit": "pt_render, lit",
        "uniform to the cap": "pt_render, lit", "adaptive to the cap": "pt_render, lit", "no render": "pt_render, lit"}


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def med(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def c2():
    from owl_path_tracer_amd.pyhost import scene_io

    s = json.load(open(os.path.join(ROOT, "assets", "configs", "c2_cornell-box.json")))
    sc = scene_io.load_scene_dir(os.path.join(ROOT, "assets"), s["scene"])
    return s, sc


def scenes(B):
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    s, sc = c2()
    W, H = s["buffer_size"]
    c = sc["camera"]
    env = dict(color=tuple(s["environment_color"]), intensity=s["environment_intensity"])
    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    return [("C2", "assets/configs/c2_cornell-box.json", W, H, s["max_path_depth"], env,
             lambda ctx: ctx.upload_scene(sc["entities"], [m for _, m, _ in sc["materials"]], env=B.make_env(**env)),
             B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H)),
            ("C4 stand-in", "dragon.json on procedural.dragon_standin, black environment (bench.py)", 1920, 1080, 16, dict(color=(1, 1, 1), intensity=0.0),
             lambda ctx: ctx.upload_scene(scene_io.build_entities(procedural.dragon_standin(), mats), [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=0.0)),
             B.to_camera_data([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, 1920, 1080))]


def run_adds(ctx, B, cam, W, H, depth, plan):
    """plan: list of AccumParams.  -> (rgb of the last add, kernel ms summed, host ms, active pixels per add); begin and end are not timed."""
    ctx.accum_begin(cam, W, H, depth)
    k_ms, active, rgb = 0.0, [], None
    t0 = time.perf_counter()
    for i, p in enumerate(plan):
        rgb, _ = ctx.accum_add(p, want_rgb=i + 1 == len(plan))
        k_ms += ctx.stats()["kernel_ms"]
        active.append(ctx.accum_info()["active_pixels"])
    host_ms = (time.perf_counter() - t0) * 1e3
    return rgb, k_ms, host_ms, active


def cost(a, B):
    rows = []
    frames = {}
    P = lambda n, cap=0, thr=0.0: B.accum_default_params(n_samples=n, max_pixel_samples=cap, noise_threshold=thr)
    for name, what, W, H, depth, env, upload, cam in scenes(B):
        ctx = B.Context(0)  # raises without a gfx950 device
        try:
            upload(ctx)
            # the threshold of (b), from the lit scene's own noise map after 32 samples
            ctx.set_environment(B.make_env(**LIT))
            ctx.accum_begin(cam, W, H, depth)
            ctx.accum_add(P(16), want_rgb=False)
            ctx.accum_add(P(16), want_rgb=False)
            noise = ctx.accum_read()["noise"]
            ctx.accum_end()
            thr = float(np.median(noise))
            assert np.isfinite(thr) and thr > 0, thr
            uniform_plan = [P(16, CAP), P(16, CAP)] + [P(32, CAP)] * 7
            ms = {k: dict(kernel=[], host=[]) for k in ("pt_render", "K=1", "K=2", "K=4", "K=16", "pt_render(1024)", "1024 in 2", "1024 in 4", "no render", "pt_render, lit",
                                                                "uniform to the cap", "adaptive to the cap")}
            same, adaptive = {}, {}
            for i in range(a.warmup + a.repeats):
                def note(key, k_ms, h_ms):
                    if i >= a.warmup:
                        ms[key]["kernel"].append(k_ms)
                        ms[key]["host"].append(h_ms)
                ctx.set_environment(B.make_env(**env))
                t0 = time.perf_counter()
                ref, _ = ctx.render(cam, W, H, SPP, depth)
                h_ms = (time.perf_counter() - t0) * 1e3
                note("pt_render", ctx.stats()["kernel_ms"], h_ms)
                for K in (1, 2, 4, 16):
                    rgb, k_ms, h_ms, _ = run_adds(ctx, B, cam, W, H, depth, [P(SPP // K)] * K)
                    note("K=%d" % K, k_ms, h_ms)
                    same["K=%d" % K] = bool((bits(rgb) == bits(ref)).all())
                    ctx.accum_end()
                t0 = time.perf_counter()
                big, _ = ctx.render(cam, W, H, SPP_BIG, depth)
                h_ms = (time.perf_counter() - t0) * 1e3
                note("pt_render(1024)", ctx.stats()["kernel_ms"], h_ms)
                for K in (2, 4):
                    rgb, k_ms, h_ms, _ = run_adds(ctx, B, cam, W, H, depth, [P(SPP_BIG // K)] * K)
                    note("1024 in %d" % K, k_ms, h_ms)
                    same["1024 in %d" % K] = bool((bits(rgb) == bits(big)).all())
                    ctx.accum_end()
                ctx.set_environment(B.make_env(**LIT))
                t0 = time.perf_counter()
                ref, _ = ctx.render(cam, W, H, SPP, depth)
                h_ms = (time.perf_counter() - t0) * 1e3
                note("pt_render, lit", ctx.stats()["kernel_ms"], h_ms)
                # (b) uniform adds to the cap, then one more add: every pixel is at its cap, so it selects nothing and renders nothing
                rgb_u, k_ms, h_ms, _ = run_adds(ctx, B, cam, W, H, depth, uniform_plan)
                note("uniform to the cap", k_ms, h_ms)
                same["uniform to the cap"] = bool((bits(rgb_u) == bits(ref)).all())
                t0 = time.perf_counter()
                ctx.accum_add(P(32, CAP), want_rgb=False)
                h_ms = (time.perf_counter() - t0) * 1e3
                st = ctx.stats()
                assert st["launches"] == 0, st
                note("no render", st["kernel_ms"], h_ms)
                ctx.accum_end()
                # (b) adaptive: the same first 32 samples, then only the pixels above the threshold, until none is left or all are capped
                ctx.accum_begin(cam, W, H, depth)
                k_ms, active = 0.0, []
                t0 = time.perf_counter()
                for p in [P(16, CAP), P(16, CAP)] + [P(32, CAP, thr)] * 7:
                    ctx.accum_add(p, want_rgb=False)
                    k_ms += ctx.stats()["kernel_ms"]
                    active.append(ctx.accum_info()["active_pixels"])
                    if active[-1] == 0:
                        break
                rd = ctx.accum_read()
                note("adaptive to the cap", k_ms, (time.perf_counter() - t0) * 1e3)
                info = ctx.accum_info()
                ctx.accum_end()
                adaptive = dict(noise_threshold=thr, adds=len(active), active_pixels_per_add=[int(x) for x in active], samples_total=int(info["samples_total"]),
                                uniform_samples_total=W * H * CAP, share_of_uniform_samples=info["samples_total"] / (W * H * CAP),
                                share_active_in_first_adaptive_add=active[2] / (W * H) if len(active) > 2 else 0.0,
                                sample_map=dict(min=int(rd["samples"].min()), mean=float(rd["samples"].mean()), max=int(rd["samples"].max())),
                                share_of_pixels_with_noise_0_after_32=float((noise == 0).mean()), environment="use_auto = 1, intensity = 1")
                if name == "C2":
                    frames = dict(adaptive=rd["rgb"], uniform=rgb_u, samples=rd["samples"], size=np.array([W, H]), threshold=np.float32(thr))
        finally:
            ctx.close()
        row = dict(scene=name, what=what, size=[W, H], spp=SPP, depth=depth, kernel_ms={k: med(v["kernel"]) for k, v in ms.items()}, host_ms={k: med(v["host"]) for k, v in ms.items()},
                   over_pt_render=dict(kernel={k: statistics.median(v["kernel"]) / statistics.median(ms[BASE.get(k, "pt_render")]["kernel"]) for k, v in ms.items()},
                                       host={k: statistics.median(v["host"]) / statistics.median(ms[BASE.get(k, "pt_render")]["host"]) for k, v in ms.items()},
                                       base={k: BASE.get(k, "pt_render") for k in ms}),
                   bit_identical_to_pt_render=same, adaptive=adaptive)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if not all(same.values()):
            raise SystemExit("a split frame differs from pt_render: %r" % same)
    if a.frames and frames:
        np.savez_compressed(a.frames, **frames)
    return dict(repeats=a.repeats, warmup=a.warmup, measured=True, rows=rows,
                timers="kernel: sum of pt_stats.kernel_ms of the calls (HIP events); host: time.perf_counter around the blocking calls; medians")


def quality(a):
    import oracle as orc
    from owl_path_tracer_amd.pyhost import scene_io

    f = np.load(a.frames)
    W, H = (int(x) for x in f["size"])
    s, sc = c2()
    assert [W, H] == list(s["buffer_size"])
    S = orc.Scene(scene_io.flatten_scene(sc["entities"], sc["materials"]))
    c = sc["camera"]
    cam = orc.to_camera_data(tuple(c["look_from"]), tuple(c["look_at"]), tuple(c["look_up"]), c["vertical_fov"], W, H)
    env = orc.make_env(**LIT)
    t0 = time.time()
    ref, _, _ = S.render(cam, env, W, H, a.ref_spp, s["max_path_depth"])
    lit = f["samples"] > 32
    row = dict(scene="C2, lit (environment use_auto = 1, intensity = 1)", size=[W, H], reference_spp=a.ref_spp, oracle_seconds=time.time() - t0, noise_threshold=float(f["threshold"]),
               samples=dict(adaptive=int(f["samples"].sum()), uniform=W * H * CAP),
               rel_rmse={"whole frame": dict(pixels=W * H, adaptive=rel_rmse(f["adaptive"], ref), uniform=rel_rmse(f["uniform"], ref)),
                         "pixels the adaptive run gave more than 32 samples": dict(pixels=int(lit.sum()), adaptive=rel_rmse(f["adaptive"][lit], ref[lit]), uniform=rel_rmse(f["uniform"][lit], ref[lit])),
                         "pixels it stopped at 32": dict(pixels=int((~lit).sum()), adaptive=rel_rmse(f["adaptive"][~lit], ref[~lit]), uniform=rel_rmse(f["uniform"][~lit], ref[~lit]))})
    print(json.dumps(row), flush=True)
    return dict(metric="relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) against the oracle's frame; frames: the C2 run of the cost section", rows=[row])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--frames", default="")
    ap.add_argument("--ref-spp", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_accum.json"))
    a = ap.parse_args()
    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.quality:
        if not a.frames:
            raise SystemExit("--quality needs --frames FILE.npz (written by a cost run)")
        rec["quality"] = quality(a)
    else:
        rec["cost"] = cost(a, B)
    rec.setdefault("cost", dict(measured=False, note="not recorded yet: needs an MI355X (python tools/accum_bench.py)"))
    rec.setdefault("quality", dict(measured=False, note="not recorded yet: python tools/accum_bench.py --quality --frames FILE.npz after a cost run"))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
