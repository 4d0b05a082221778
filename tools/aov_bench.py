"""What the guide pass costs: pt_render_aov on the C4 stand-in at 1920 x 1080 with n = 1, 4 and 16 samples per pixel, one MI355X.

    python tools/aov_bench.py [--write] [--size 1920x1080] [--samples 1,4,16] [--repeats 7]

Per sample count, on one build and one context, alternating the two so that both see the same machine:
  * guide: kernel_ms of pt_render_aov (HIP events around the one launch; pt_stats) and Grays/s = W * H * n / kernel time;
  * yardstick: kernel_ms of pt_render with max_depth = 1 at spp = n - the same primary rays (sample 0 exactly; the later samples are
    each pass's own jitter) through the wavefront kernel, which shades every hit and samples a BSDF before the path ends.
Each figure is the median of --repeats runs after one warm-up per shape; min and max are recorded beside it.  While at it the guide
buffers are compared with the CPU twin on a sample of pixels, bit for bit.  --write stores the record as profiles/r11_aov.json.
Measurement only: nothing here is asserted by the test suite, and without a GPU the tool fails (there is no fallback)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--samples", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    counts = [int(x) for x in a.samples.split(",")]

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B, procedural, scene_io

    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ents = scene_io.build_entities(procedural.dragon_standin(), mats)
    table = [m for _, m, _ in mats]
    env = dict(color=(1, 1, 1), intensity=0.0)
    ctx = B.Context(0)  # raises without a gfx950 device
    ctx.upload_scene(ents, table, env=B.make_env(**env))
    cam = B.to_camera_data([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, W, H)
    rows = []
    for n in counts:
        ctx.render_aov(cam, W, H, n)  # warm-up of both shapes: buffers, pixel queue, code objects
        ctx.render(cam, W, H, n, 1)
        g_ms, y_ms, geo = [], [], {}
        for _ in range(a.repeats):
            buf = ctx.render_aov(cam, W, H, n)
            st = ctx.stats()
            g_ms.append(st["kernel_ms"])
            geo = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], grid=st["grid"], stack_entries=st["stack_entries"])
            ctx.render(cam, W, H, n, 1)
            y_ms.append(ctx.stats()["kernel_ms"])
        rays = W * H * n
        med = lambda v: statistics.median(v)
        row = dict(n_samples=n, guide_kernel_ms=dict(median=med(g_ms), min=min(g_ms), max=max(g_ms)), guide_grays_per_s=rays / (med(g_ms) * 1e6),
                   yardstick_kernel_ms=dict(median=med(y_ms), min=min(y_ms), max=max(y_ms)), yardstick_grays_per_s=rays / (med(y_ms) * 1e6),
                   guide_over_yardstick=med(g_ms) / med(y_ms), coverage=float(buf[..., 3].mean()), guide_launch=geo)
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the buffers that were timed are the definition's: a sample of pixels against the CPU twin
    n = counts[0]
    buf = ctx.render_aov(cam, W, H, n)
    ids = np.random.default_rng(1).choice(W * H, 4096, replace=False).astype(np.uint32)
    host = B.Context(-1)
    host.upload_scene(ents, table, env=B.make_env(**env))
    want = host.aov_host(cam, W, H, n, pixel_ids=ids)
    host.close()
    got = buf[::-1].reshape(-1, 8)[ids]
    same = bool((np.ascontiguousarray(got).view(np.uint32) == want.view(np.uint32)).all())
    ctx.close()
    rec = dict(workload="C4 stand-in (dragon.json on procedural.dragon_standin), %dx%d, black environment" % (W, H), repeats=a.repeats,
               yardstick="pt_render, max_depth = 1, spp = n_samples, same context and build", rows=rows, twin_check=dict(pixels=int(ids.size), n_samples=n, bit_identical=same))
    print(json.dumps(dict(twin_check=rec["twin_check"])))
    if not same:
        raise SystemExit("the timed buffers differ from the CPU twin")
    if a.write:
        with open(os.path.join(ROOT, "profiles", "r11_aov.json"), "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
