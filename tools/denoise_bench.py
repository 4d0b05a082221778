"""What the denoiser costs and what it buys: pt_denoise on one MI355X.

    python tools/denoise_bench.py [--write] [--size 1920x1080] [--repeats 20] [--warmups 3]

Cost, on the C4 stand-in at --size (one build, one context):
  * the input is the library's own: pt_render at 16 spp (depth 8) and pt_render_aov at n = 4, both timed beside the filter (kernel_ms of
    pt_stats: HIP events around the kernels; median of --repeats after --warmups);
  * the filter with the default parameters at L = 1 .. 5: kernel_ms from the first to the last filter kernel.  The prepare and finish
    kernels are the same for every L, so median(L) - median(L - 1) is iteration L - 1 (step 2^(L-1)) and median(1) - that of
    iteration 0 cannot be split further: it is reported as "prepare + finish + iteration 0";
  * effective bytes/s of an iteration against the 64 B per pixel it must move at least (48 B of records read for the centre, 16 B
    written; the other 24 taps are re-reads that caches may or may not serve).
Quality, on three scenes of tests/aov_common.py (Cornell, the textured cube, the icospheres under the environment map) at 256 x 192:
  8 spp against 2048 spp (depth 8), guides at n = 1, relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) of the noisy frame and of the
  filtered one over sigma_color in {1, 2, 4, 8} x the demodulation flag.
The timed output is compared with the CPU twin bit for bit on a frame of the same scene at 1/16 of the size (the twin is slow at 1080p).
--write stores the record as profiles/r14_denoise.json.  Measurement only: nothing here is asserted by the test suite, and without a GPU
the tool fails (there is no fallback)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B, procedural, scene_io

    def timed(call, stats):
        for _ in range(a.warmups):
            call()
        ms = []
        for _ in range(a.repeats):
            call()
            ms.append(stats()["kernel_ms"])
        return dict(median=statistics.median(ms), min=min(ms), max=max(ms))

    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ents = scene_io.build_entities(procedural.dragon_standin(), mats)
    ctx = B.Context(0)  # raises without a gfx950 device
    ctx.upload_scene(ents, [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=1.0))
    cam = B.to_camera_data([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, W, H)
    frame = {}

    def render():
        frame["rgb"], _ = ctx.render(cam, W, H, 16, 8)

    def guides():
        frame["aov"] = ctx.render_aov(cam, W, H, 4)

    rec = dict(workload="C4 stand-in (dragon.json on procedural.dragon_standin), %dx%d, white environment" % (W, H), repeats=a.repeats, warmups=a.warmups)
    rec["pt_render_16spp_depth8_kernel_ms"] = timed(render, ctx.stats)
    rec["pt_render_aov_n4_kernel_ms"] = timed(guides, ctx.stats)
    print(json.dumps({k: rec[k] for k in ("pt_render_16spp_depth8_kernel_ms", "pt_render_aov_n4_kernel_ms")}), flush=True)
    by_L, geo = {}, {}
    for L in range(1, 6):
        p = B.denoise_default_params(iterations=L)
        by_L[L] = timed(lambda: ctx.denoise(frame["rgb"], frame["aov"], p), ctx.stats)
        st = ctx.stats()
        geo = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], launches=st["launches"])
    floor_bytes = 64.0 * W * H
    its = []
    for i in range(1, 5):
        ms = by_L[i + 1]["median"] - by_L[i]["median"]
        its.append(dict(iteration=i, step=1 << i, kernel_ms=ms, effective_bytes_per_s=floor_bytes / (ms * 1e-3) if ms > 0 else None))
    rec["denoise_kernel_ms_by_iterations"] = {str(L): v for L, v in by_L.items()}
    rec["denoise_L5_total_kernel_ms"] = by_L[5]
    rec["denoise_prepare_finish_iteration0_kernel_ms"] = by_L[1]["median"]
    rec["denoise_iterations"] = its
    rec["denoise_L5_effective_bytes_per_s"] = 5 * floor_bytes / (by_L[5]["median"] * 1e-3)
    rec["denoise_launch"] = geo
    rec["floor_bytes_per_pixel_and_iteration"] = 64
    print(json.dumps({k: rec[k] for k in ("denoise_L5_total_kernel_ms", "denoise_prepare_finish_iteration0_kernel_ms", "denoise_iterations", "denoise_launch")}), flush=True)
    # the filter that was timed is the definition's: a small frame of the same scene against the CPU twin
    w, h = max(1, W // 16), max(1, H // 16)
    scam = B.to_camera_data([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, w, h)
    rgb, _ = ctx.render(scam, w, h, 16, 8)
    aov = ctx.render_aov(scam, w, h, 4)
    got, got8 = ctx.denoise(rgb, aov, None, want_rgba8=True)
    host = B.Context(-1)
    want, want8 = host.denoise_host(rgb, aov, None, want_rgba8=True)
    host.close()
    ctx.close()
    same = bool((got.view(np.uint32) == want.view(np.uint32)).all() and (got8 == want8).all())
    rec["twin_check"] = dict(size=[w, h], bit_identical=same)
    print(json.dumps(dict(twin_check=rec["twin_check"])), flush=True)
    if not same:
        raise SystemExit("the filtered frame differs from the CPU twin")

    import aov_common as AC

    qW, qH = 256, 192
    grid = []
    for name in ("cornell", "cube", "ico_map"):
        sc = AC.scene(name)
        c = B.Context(0)
        AC.upload(c, sc, B)
        qcam = AC.camera(sc, qW, qH, B.to_camera_data)
        noisy, _ = c.render(qcam, qW, qH, 8, 8)
        ref, _ = c.render(qcam, qW, qH, 2048, 8)
        g = c.render_aov(qcam, qW, qH, 1)
        row = dict(scene=name, size=[qW, qH], noisy_rel_rmse=rel_rmse(noisy, ref), denoised_rel_rmse={})
        for flag in (0, 1):
            for sigma in (1.0, 2.0, 4.0, 8.0):
                out, _ = c.denoise(noisy, g, B.denoise_default_params(sigma_color=sigma, flags=flag))
                row["denoised_rel_rmse"]["sigma_color=%g,flags=%d" % (sigma, flag)] = rel_rmse(out, ref)
        c.close()
        grid.append(row)
        print(json.dumps(row), flush=True)
    rec["quality"] = dict(metric="relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))), 8 spp against 2048 spp, depth 8, guides at n = 1, L = 5", rows=grid)
    if a.write:
        with open(os.path.join(ROOT, "profiles", "r14_denoise.json"), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
