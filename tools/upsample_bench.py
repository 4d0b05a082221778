"""What rendering fewer pixels and upsampling costs and buys: pt_upsample on one MI355X.

    python tools/upsample_bench.py [--write] [--out FILE] [--size 1920x1080] [--repeats 20] [--warmups 3] [--quality] [--quality-only]

The C4 stand-in, depth 8, white environment, guides from pt_render_aov at n = 1; the low frame is ceil(W / 2) x ceil(H / 2).
kernels:  kernel_ms of pt_stats (HIP events from the first to the last kernel: prepare over the low frame + upsample over the high one) of
  pt_upsample at taps 2 and taps 4, beside pt_denoise at --size in the same run; median of --repeats after --warmups.  The bytes per high
  pixel come from the shapes: the upsample kernel reads its own 32-byte guide record and writes 12 + 4 bytes - 48 bytes of HBM traffic
  per high pixel - and taps^2 x 48 bytes of low records, which are shared by four high pixels each and by the neighbouring windows:
  the whole low record set (48 bytes per low pixel; 25 MB at 960 x 540) is written by prepare just before and fits the Infinity Cache, so
  those loads are cache traffic.  Per low pixel prepare reads 44 and writes 48 bytes.  The rate printed is therefore (48 + (44 + 48 + 48) /
  4) bytes per high pixel over the median: a floor on what moved, mostly but not only HBM - not an HBM figure.
end_to_end:  on one non-blocking caller stream, device buffers, wall time per frame around the calls and a pt_synchronize:
  (a) pt_render_device at the low size (16 spp), pt_render_aov_device at both sizes, pt_denoise_device at the low size, pt_upsample_device;
  (b) pt_render_device (16 spp) + pt_render_aov_device + pt_denoise_device at --size.
quality (--quality; CPU only, --quality-only skips the GPU sections): aov_common's Cornell and textured cube from the oracle, 128 x 96 at
  256 spp -> 256 x 192, guides from pt_debug_aov_host at n = 4, against the oracle's 1024-spp frame at 256 x 192: relRMSE
  of the CPU twin as plain bilinear (every sigma +inf, flag 0, taps 2), at the defaults, and at taps 2.
--write merges the sections into profiles/r20_upsample.json; --out FILE into another file.  Measurement only: nothing here is asserted by
the test suite, and without a GPU the GPU sections fail (there is no fallback)."""
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
PROFILE = os.path.join(ROOT, "profiles", "r20_upsample.json")
DEPTH, SPP, FACTOR, REF_SPP = 8, 16, 2, 1024
INF = float("inf")


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


def run_gpu(B, a):
    import accum_reproject_common as RC
    import async_common as AS
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    W, H = (int(x) for x in a.size.split("x"))
    w, h = (W + FACTOR - 1) // FACTOR, (H + FACTOR - 1) // FACTOR
    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ents = scene_io.build_entities(procedural.dragon_standin(), mats)
    ctx = B.Context(0)  # raises without a gfx950 device
    ctx.upload_scene(ents, [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=1.0))
    cam = RC.look(np.array([4.0, 2.5, 0.0]), np.array([0.0, 0.75, 0.0]), [0.0, 1.0, 0.0], 50.0, W, H)  # ONE camera for both sizes
    workload = "C4 stand-in (dragon.json on procedural.dragon_standin), %dx%d -> %dx%d, white environment, depth %d, %d spp, guides at n = 1" % (w, h, W, H, DEPTH, SPP)

    # ---- kernels ----
    lo, _ = ctx.render(cam, w, h, SPP, DEPTH)
    full, _ = ctx.render(cam, W, H, SPP, DEPTH)
    g_lo, g_hi = ctx.render_aov(cam, w, h, 1), ctx.render_aov(cam, W, H, 1)
    ms = dict(upsample_taps2=[], upsample_taps4=[], denoise=[])
    launch = {}
    for i in range(a.warmups + a.repeats):
        t = {}
        for taps in (2, 4):
            ctx.upsample(lo, g_lo, g_hi, B.upsample_default_params(taps=taps))
            st = ctx.stats()
            t["upsample_taps%d" % taps] = st["kernel_ms"]
            launch["pt_upsample"] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], launches=st["launches"])
        ctx.denoise(full, g_hi, None)
        t["denoise"] = ctx.stats()["kernel_ms"]
        if i >= a.warmups:
            for k, v in t.items():
                ms[k].append(v)
    bytes_per_high_pixel = 48 + (44 + 48 + 48) / float(FACTOR * FACTOR)
    kernels = dict(workload=workload, repeats=a.repeats, warmups=a.warmups, launch=launch, pt_upsample_taps2_kernel_ms=spread(ms["upsample_taps2"]),
                   pt_upsample_taps4_kernel_ms=spread(ms["upsample_taps4"]), pt_denoise_full_size_kernel_ms=spread(ms["denoise"]),
                   bytes_per_high_pixel=bytes_per_high_pixel, tap_bytes_per_high_pixel_from_cache={"taps2": 4 * 48, "taps4": 16 * 48}, low_records_bytes=48 * w * h,
                   floor_gb_per_s={k: bytes_per_high_pixel * W * H / (statistics.median(ms["upsample_" + k]) * 1e-3) / 1e9 for k in ("taps2", "taps4")},
                   rate_is_an_hbm_figure=False)
    print(json.dumps(dict(kernels=kernels)), flush=True)
    host = B.Context(-1)
    sw, sh = max(1, w // 16), max(1, h // 16)
    sW, sH = sw * FACTOR, sh * FACTOR
    s_lo, _ = ctx.render(cam, sw, sh, SPP, DEPTH)
    sg_lo, sg_hi = ctx.render_aov(cam, sw, sh, 1), ctx.render_aov(cam, sW, sH, 1)
    identical = bool((ctx.upsample(s_lo, sg_lo, sg_hi)[0].view(np.uint32) == host.upsample_host(s_lo, sg_lo, sg_hi)[0].view(np.uint32)).all())
    host.close()
    kernels["checks"] = dict(twin=dict(size=[sw, sh, sW, sH], bit_identical=identical))

    # ---- end to end ----
    s = AS.stream(0, nonblocking=True)
    d_lo, d_glo, d_ghi, d_out, d_full = AS.DeviceFrame(w, h), AS.DeviceFrame(w, h, floats=8), AS.DeviceFrame(W, H, floats=8), AS.DeviceFrame(W, H), AS.DeviceFrame(W, H)
    t_up, t_full = [], []
    try:
        for i in range(a.warmups + a.repeats):
            t0 = time.perf_counter()
            ctx.render_device(cam, w, h, SPP, DEPTH, d_lo.rgb, stream=s)
            ctx.render_aov_device(cam, w, h, 1, d_glo.rgb, stream=s)
            ctx.render_aov_device(cam, W, H, 1, d_ghi.rgb, stream=s)
            ctx.denoise_device(d_lo.rgb, d_glo.rgb, w, h, d_lo.rgb, None, stream=s)
            ctx.upsample_device(d_lo.rgb, d_glo.rgb, w, h, d_ghi.rgb, W, H, d_out.rgb, None, stream=s)
            ctx.synchronize()
            t1 = time.perf_counter()
            ctx.render_device(cam, W, H, SPP, DEPTH, d_full.rgb, stream=s)
            ctx.render_aov_device(cam, W, H, 1, d_ghi.rgb, stream=s)
            ctx.denoise_device(d_full.rgb, d_ghi.rgb, W, H, d_full.rgb, None, stream=s)
            ctx.synchronize()
            t2 = time.perf_counter()
            if i >= a.warmups:
                t_up.append((t1 - t0) * 1e3)
                t_full.append((t2 - t1) * 1e3)
    finally:
        for f in (d_lo, d_glo, d_ghi, d_out, d_full):
            f.free()
        AS.destroy_streams()
        ctx.close()
    end_to_end = dict(workload=workload, repeats=a.repeats, warmups=a.warmups, low_render_guides_denoise_upsample_ms_per_frame=spread(t_up),
                      full_render_guides_denoise_ms_per_frame=spread(t_full), ratio=statistics.median(t_up) / statistics.median(t_full))
    print(json.dumps(dict(end_to_end=end_to_end)), flush=True)
    if not identical:
        raise SystemExit("the upsampled frame differs from the CPU twin")
    return dict(kernels=kernels, end_to_end=end_to_end)


def run_quality(B, a):
    import aov_common as AC
    import oracle as orc

    w, h, W, H = 128, 96, 256, 192
    host = B.Context(-1)
    quality = dict(sizes=[w, h, W, H], low_spp=256, reference_spp=REF_SPP, depth=DEPTH, guide_samples=4, metric="relRMSE, sqrt(mean((x - ref)^2 / (ref^2 + 1e-2)))")
    bilinear = dict(taps=2, flags=0, sigma_normal=INF, sigma_depth=INF, sigma_albedo=INF)
    for name in ("cornell", "cube"):
        sc = AC.scene(name)
        S = orc.Scene(sc["flat"])
        cam = AC.camera(sc, W, H, orc.to_camera_data)
        env = orc.make_env(**sc["env"])
        lo, _, _ = S.render(cam, env, w, h, 256, DEPTH)
        ref, _, _ = S.render(cam, env, W, H, REF_SPP, DEPTH)
        ctx = B.Context(-1)
        AC.upload(ctx, sc, B)
        bcam = AC.camera(sc, W, H, B.to_camera_data)
        g_lo, g_hi = ctx.aov_host(bcam, w, h, 4), ctx.aov_host(bcam, W, H, 4)
        ctx.close()
        quality[name] = dict(bilinear=rel_rmse(host.upsample_host(lo, g_lo, g_hi, B.upsample_default_params(**bilinear))[0], ref),
                             defaults=rel_rmse(host.upsample_host(lo, g_lo, g_hi, None)[0], ref),
                             taps2=rel_rmse(host.upsample_host(lo, g_lo, g_hi, B.upsample_default_params(taps=2))[0], ref))
        print(json.dumps({name: quality[name]}), flush=True)
    host.close()
    return dict(quality=quality)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    sections = {}
    if not a.quality_only:
        sections.update(run_gpu(B, a))
    if a.quality or a.quality_only:
        sections.update(run_quality(B, a))
    if a.write:
        merge(PROFILE, sections)
    if a.out:
        merge(a.out, sections)


if __name__ == "__main__":
    main()
