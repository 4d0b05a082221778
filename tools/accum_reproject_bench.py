"""What moving an accumulation to a new camera costs and what it buys: pt_accum_reproject on one MI355X.

    python tools/accum_reproject_bench.py [--write] [--out FILE] [--size 1920x1080] [--repeats 20] [--warmups 3]

The C4 stand-in at --size, depth 8, white environment, guides from pt_render_aov at n = 1.
cost:  an accumulation of 8 + 8 samples is begun anew before every repeat and moved along a 2 degree orbit; kernel_ms of pt_stats (HIP
  events around the one kernel) as the median of --repeats after --warmups.  In the same run, as yardsticks: pt_accum_denoise (a streaming
  kernel family over the same frame) and an add with an empty active set (max_pixel_samples = 1: select, the wait for its count, resolve).
  The bytes the reproject kernel must move come from the shapes: per owned pixel 2 x 32 (guide records) + 1 + 1 (owned flags) + 36 (the
  source's sum, half, n, n_half, passes) read and 36 + 12 (seen) + 4 (noise) + 12 + 4 (image) written = 170; the achieved rate is that
  over the median.  The moved state of a frame at 1/16 of the size is compared with the CPU twin bit for bit.
orbit: frames along an 8-step orbit of 2 degrees each, one add of 8 samples per frame, two ways on device buffers and one stream:
  (a) reproject + add + pt_accum_denoise on ONE accumulation; (b) pt_accum_begin + add + pt_denoise for every frame.  Both include the
  frame's guide pass.  Wall time per frame (host clock around the calls and a pt_synchronize), relRMSE of the last frame of each against a
  1024-spp pt_render at that camera, and the share of pixels that kept history at every step.
--write merges the sections into profiles/r19_accum_reproject.json; --out FILE into another file.  Measurement only: nothing here is
asserted by the test suite, and without a GPU the run fails (there is no fallback)."""
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
PROFILE = os.path.join(ROOT, "profiles", "r19_accum_reproject.json")
F32, U32 = np.float32, np.uint32
BYTES_PER_PIXEL = 2 * 32 + 2 + 36 + 36 + 12 + 4 + 12 + 4
DEPTH, STEP_DEG = 8, 2.0


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def merge(path, sections):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.update(sections)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def spread(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def run(B, a):
    import accum_reproject_common as RC
    import async_common as AS
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    W, H = (int(x) for x in a.size.split("x"))
    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ents = scene_io.build_entities(procedural.dragon_standin(), mats)
    ctx = B.Context(0)  # raises without a gfx950 device
    ctx.upload_scene(ents, [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=1.0))
    frm, at, up, fov = np.array([4.0, 2.5, 0.0]), np.array([0.0, 0.75, 0.0]), [0.0, 1.0, 0.0], 50.0
    cam = lambda step, w=W, h=H: RC.look(at + RC.rot_y(frm - at, STEP_DEG * step), at, up, fov, w, h)
    add8 = B.accum_default_params(n_samples=8)

    # ---- cost ----
    cam0, cam1 = cam(0), cam(1)
    aov0, aov1 = ctx.render_aov(cam0, W, H, 1), ctx.render_aov(cam1, W, H, 1)
    ms = dict(reproject=[], accum_denoise=[], empty_add=[])
    shares = []
    launch = {}
    for i in range(a.warmups + a.repeats):
        ctx.accum_begin(cam0, W, H, DEPTH)
        ctx.accum_add(add8, want_rgb=False)
        ctx.accum_add(add8, want_rgb=False)
        ctx.accum_add(B.accum_default_params(n_samples=8, max_pixel_samples=1), want_rgb=False)  # (before the move: every pixel has its 16 samples)
        assert ctx.accum_info()["active_pixels"] == 0
        t = dict(empty_add=ctx.stats()["kernel_ms"])
        ctx.accum_reproject(cam1, aov0, aov1, None)
        st = ctx.stats()
        t["reproject"] = st["kernel_ms"]
        launch["pt_accum_reproject"] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], launches=st["launches"])
        share = float((ctx.accum_read()["samples"] > 0).mean())
        ctx.accum_denoise(aov1, None)
        t["accum_denoise"] = ctx.stats()["kernel_ms"]
        if i >= a.warmups:
            for k, v in t.items():
                ms[k].append(v)
            shares.append(share)
    ctx.accum_end()
    med = statistics.median(ms["reproject"])
    cost = dict(workload="C4 stand-in (dragon.json on procedural.dragon_standin), %dx%d, white environment, depth %d; accumulation of 8 + 8 samples begun anew before every "
                         "repeat, moved along a %g degree orbit; guides at n = 1" % (W, H, DEPTH, STEP_DEG),
                repeats=a.repeats, warmups=a.warmups, pt_accum_reproject_kernel_ms=spread(ms["reproject"]), pt_accum_denoise_kernel_ms=spread(ms["accum_denoise"]),
                empty_add_kernel_ms=spread(ms["empty_add"]), launch=launch, history_share=shares[0], bytes_per_pixel=BYTES_PER_PIXEL, bytes_moved=BYTES_PER_PIXEL * W * H,
                achieved_gb_per_s=BYTES_PER_PIXEL * W * H / (med * 1e-3) / 1e9, ratio_to_pt_accum_denoise=med / statistics.median(ms["accum_denoise"]))
    print(json.dumps(dict(cost=cost)), flush=True)

    # the moved state of a small frame against the CPU twin
    w, h = max(1, W // 16), max(1, H // 16)
    c0, c1 = cam(0, w, h), cam(1, w, h)
    g0, g1 = ctx.render_aov(c0, w, h, 1), ctx.render_aov(c1, w, h, 1)
    ctx.accum_begin(c0, w, h, DEPTH)
    ctx.accum_add(add8, want_rgb=False)
    ctx.accum_add(add8, want_rgb=False)
    before = ctx.accum_state()
    ctx.accum_reproject(c1, g0, g1, None)
    after = dict(ctx.accum_state(), **{k: v for k, v in ctx.accum_read().items() if k != "samples"})
    ctx.accum_end()
    host = B.Context(-1)
    twin = host.accum_reproject_host(c0, c1, g0, g1, before, None, None)
    host.close()
    identical = all(bool(RC.same(after[k], twin[k]).all()) for k in RC.KEYS)
    cost["checks"] = dict(twin=dict(size=[w, h], bit_identical=identical))

    # ---- orbit ----
    steps = 8
    s = AS.stream(0, nonblocking=True)
    guides = [AS.DeviceFrame(W, H, floats=8), AS.DeviceFrame(W, H, floats=8)]
    noisy, out = AS.DeviceFrame(W, H), AS.DeviceFrame(W, H)
    orbit = dict(steps=steps, step_degrees=STEP_DEG, samples_per_frame=8, reference_spp=1024)
    try:
        def reprojected(record):
            times, kept = [], []
            ctx.accum_begin(cam(0), W, H, DEPTH)
            ctx.render_aov_device(cam(0), W, H, 1, guides[0].rgb, stream=s)
            ctx.accum_add_device(add8, None, None, stream=s)
            ctx.synchronize()
            for k in range(1, steps + 1):
                prev, cur = guides[(k - 1) % 2], guides[k % 2]
                t0 = time.perf_counter()
                ctx.render_aov_device(cam(k), W, H, 1, cur.rgb, stream=s)
                ctx.accum_reproject_device(cam(k), prev.rgb, cur.rgb, None, stream=s)
                if record:
                    ctx.synchronize()
                    kept.append(float((ctx.accum_read()["samples"] > 0).mean()))
                ctx.accum_add_device(add8, None, None, stream=s)
                ctx.accum_denoise_device(cur.rgb, out.rgb, None, stream=s)
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            frame = out.read()[0]
            samples = ctx.accum_read()["samples"]
            ctx.accum_end()
            return times, kept, frame, samples

        def restarted():
            times = []
            for k in range(1, steps + 1):
                t0 = time.perf_counter()
                ctx.accum_begin(cam(k), W, H, DEPTH)
                ctx.render_aov_device(cam(k), W, H, 1, guides[0].rgb, stream=s)
                ctx.accum_add_device(add8, noisy.rgb, None, stream=s)
                ctx.denoise_device(noisy.rgb, guides[0].rgb, W, H, out.rgb, None, stream=s)
                ctx.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            frame = out.read()[0]
            ctx.accum_end()
            return times, frame

        reprojected(False)  # warm-up of both ways: buffers allocated, kernels loaded
        restarted()
        _, kept, _, _ = reprojected(True)
        t_a, _, frame_a, samples = reprojected(False)
        t_b, frame_b = restarted()
        ref = ctx.render(cam(steps), W, H, 1024, DEPTH)[0]
        orbit.update(reproject_add_accum_denoise_ms_per_frame=spread(t_a), begin_add_denoise_ms_per_frame=spread(t_b), history_share_per_step=kept,
                     mean_samples_per_pixel_last_frame=float(samples.mean()), rel_rmse_last_frame=dict(reproject_add_accum_denoise=rel_rmse(frame_a, ref),
                                                                                                      begin_add_denoise=rel_rmse(frame_b, ref)))
    finally:
        for f in guides + [noisy, out]:
            f.free()
        AS.destroy_streams()
        ctx.close()
    print(json.dumps(dict(orbit=orbit, checks=cost["checks"])), flush=True)
    if not identical:
        raise SystemExit("the moved state differs from the CPU twin")
    return dict(cost=cost, orbit=orbit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    a = ap.parse_args()

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    sections = run(B, a)
    if a.write:
        merge(PROFILE, sections)
    if a.out:
        merge(a.out, sections)


if __name__ == "__main__":
    main()
