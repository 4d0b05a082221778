"""What the variance-guided denoiser buys and what it costs: pt_denoise_var / pt_accum_denoise beside pt_denoise.

    python tools/denoise_var_bench.py --quality [--write]            (CPU only)
    python tools/denoise_var_bench.py [--write] [--out FILE] [--size 1920x1080] [--repeats 20] [--warmups 3]   (one MI355X)

--quality, from the CPU twins in float32 (no GPU): three scenes of tests/aov_common.py (Cornell against 2048 spp, the icospheres under
  the map and the textured cube against 1024 spp) at 64 x 48, depth 8, guides from pt_debug_aov_host at n = 1.  An accumulation of
  n = 8 / 64 / 256 samples in two equal adds is emulated on the oracle (sum = n * R(n), half = sum - n/2 * R(n/2)), its variance map comes
  from pt_debug_accum_variance_host, and relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) is taken of the unfiltered frame, of
  pt_debug_denoise_host and of pt_debug_denoise_var_host, each at its defaults.  Also the registers and scratch of the four kernels, from
  `make asm-denoise-var`.
Without --quality, on the GPU, the C4 stand-in at --size: an accumulation of 8 + 8 samples (depth 8) and guides at n = 1; then pt_denoise
  (on pt_accum_read's frame), pt_denoise_var (the same frame with pt_accum_variance's map) and pt_accum_denoise in the same run, each
  kernel_ms of pt_stats (HIP events from the first to the last kernel) as the median of --repeats after --warmups, and the two ratios
  to pt_denoise.  pt_accum_denoise's result is compared with pt_denoise_var's bit for bit, and a frame at 1/16 of the size with the twin.
--write merges the section that was produced ("quality" and "kernels", or "cost") into profiles/r18_denoise_var.json; --out FILE into
another file.  Measurement only: nothing here is asserted by the test suite, and without a GPU the cost run fails (there is no fallback)."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
PROFILE = os.path.join(ROOT, "profiles", "r18_denoise_var.json")
F32, U32 = np.float32, np.uint32


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def merge(path, sections):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.update(sections)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def quality(B):
    import aov_common as AC
    import oracle as orc

    W, H, depth = 64, 48, 8
    host = B.Context(-1)
    rows = []
    for name, n_ref in (("cornell", 2048), ("ico_map", 1024), ("cube", 1024)):
        sc = AC.scene(name)
        AC.upload(host, sc, B)
        aov = host.aov_host(AC.camera(sc, W, H, B.to_camera_data), W, H, 1)
        S, cam, env = orc.Scene(sc["flat"]), AC.camera(sc, W, H, orc.to_camera_data), orc.make_env(**sc["env"])
        R = lambda n: S.render(cam, env, W, H, n, depth)[0]
        ref = R(n_ref)
        for n in (8, 64, 256):
            full, first = R(n), R(n // 2)
            sum_ = (F32(n) * full).astype(F32)
            half = (sum_ - (F32(n // 2) * first).astype(F32)).astype(F32)
            N = W * H
            rgb, var = host.accum_variance_host(sum_.reshape(N, 3), half.reshape(N, 3), np.full(N, n, U32), np.full(N, n - n // 2, U32), np.ones(N, np.uint8))
            rgb, var = rgb.reshape(H, W, 3), var.reshape(H, W, 3)
            row = dict(scene=name, reference_spp=n_ref, spp=n, noisy=rel_rmse(rgb, ref), pt_denoise=rel_rmse(host.denoise_host(rgb, aov, None)[0], ref),
                       pt_denoise_var=rel_rmse(host.denoise_var_host(rgb, var, aov, None)[0], ref))
            rows.append(row)
            print(json.dumps(row), flush=True)
    host.close()
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "owl-path-tracer_amd", "csrc"), "asm-denoise-var"], capture_output=True, text=True)
    blocks = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)", r.stdout + r.stderr, flags=re.S)
    kernels = {re.search(r"pt_[a-z_]+_kernel", nm).group(0): dict(vgprs=int(v), scratch_bytes_per_lane=int(sz), waves_per_simd=int(occ)) for nm, v, sz, occ in blocks}
    print(json.dumps(kernels), flush=True)
    return dict(quality=dict(metric="relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))); 64 x 48, depth 8, guides at n = 1; accumulations of two equal adds emulated on the "
                                    "oracle; CPU twins in float32, every filter at its defaults (pt_denoise: sigma_color 4 absolute; pt_denoise_var: 3 standard deviations)",
                             rows=rows), kernels=kernels)


def cost(B, a):
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    W, H = (int(x) for x in a.size.split("x"))

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
    look = ([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0)
    rec = dict(workload="C4 stand-in (dragon.json on procedural.dragon_standin), %dx%d, white environment, accumulation of 8 + 8 samples at depth 8, guides at n = 1" % (W, H),
               repeats=a.repeats, warmups=a.warmups)

    def accumulation(w, h):
        cam = B.to_camera_data(*look, w, h)
        ctx.accum_begin(cam, w, h, 8)
        ctx.accum_add(B.accum_default_params(n_samples=8), want_rgb=False)
        ctx.accum_add(B.accum_default_params(n_samples=8), want_rgb=False)
        return ctx.accum_read()["rgb"], ctx.accum_variance(), ctx.render_aov(cam, w, h, 1)

    rgb, var, aov = accumulation(W, H)
    geo = {}
    for key, call in (("pt_denoise", lambda: ctx.denoise(rgb, aov, None)), ("pt_denoise_var", lambda: ctx.denoise_var(rgb, var, aov, None)), ("pt_accum_denoise", lambda: ctx.accum_denoise(aov, None))):
        rec[key + "_kernel_ms"] = timed(call, ctx.stats)
        st = ctx.stats()
        geo[key] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], launches=st["launches"])
        print(json.dumps({key: rec[key + "_kernel_ms"], "launch": geo[key]}), flush=True)
    rec["launch"] = geo
    base = rec["pt_denoise_kernel_ms"]["median"]
    rec["ratio_to_pt_denoise"] = dict(pt_denoise_var=rec["pt_denoise_var_kernel_ms"]["median"] / base, pt_accum_denoise=rec["pt_accum_denoise_kernel_ms"]["median"] / base)
    a_out, a8 = ctx.accum_denoise(aov, None, want_rgba8=True)
    v_out, v8 = ctx.denoise_var(rgb, var, aov, None, want_rgba8=True)
    parts = bool((a_out.view(U32) == v_out.view(U32)).all() and (a8 == v8).all())
    ctx.accum_end()
    w, h = max(1, W // 16), max(1, H // 16)
    rgb, var, aov = accumulation(w, h)
    got, got8 = ctx.accum_denoise(aov, None, want_rgba8=True)
    ctx.accum_end()
    ctx.close()
    host = B.Context(-1)
    want, want8, _ = host.denoise_var_host(rgb, var, aov, None, want_rgba8=True)
    host.close()
    twin = bool((got.view(U32) == want.view(U32)).all() and (got8 == want8).all())
    rec["checks"] = dict(accum_denoise_equals_denoise_var_of_its_parts=parts, twin=dict(size=[w, h], bit_identical=twin))
    print(json.dumps(dict(ratio_to_pt_denoise=rec["ratio_to_pt_denoise"], checks=rec["checks"])), flush=True)
    if not (parts and twin):
        raise SystemExit("the filtered frame differs from its parts or from the CPU twin")
    return dict(cost=rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    a = ap.parse_args()

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    sections = quality(B) if a.quality else cost(B, a)
    if a.write:
        merge(PROFILE, sections)
    if a.out:
        merge(a.out, sections)


if __name__ == "__main__":
    main()
