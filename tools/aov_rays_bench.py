"""What the guide pass over a ray image costs and what it buys (pt_render_aov_rays).

    python tools/aov_rays_bench.py [--size 1920x1080] [--samples 4] [--repeats 20] [--warmup 3] [--out profiles/r23_aov_rays.json]
    python tools/aov_rays_bench.py --quality [--pano 128x64] [--out profiles/r23_aov_rays.json]

Cost (one MI355X; without a GPU the tool fails, there is no fallback).  Device buffers, the table in HBM; kernel_ms of pt_stats - HIP
events around the one launch - median of --repeats runs after --warmup runs, the calls alternating so that all see the same machine:
pt_render_aov_follow_device of the camera against pt_render_aov_rays_device of ray_image.pinhole(cam), at max_follow 0 and 4, on the C4
stand-in (no followed surface) and on the glass and metal icospheres under the environment map (tests/aov_common.py "ico_map").  The
device form cannot see the records and takes the subtracting slab form unless option "box_exact" says otherwise, while the camera's
frame takes the fma form: the ray image is measured under "box_exact" = 0 (like for like - the ratio that is the gather's) and under the
default.  Record only: no ratio is fixed in advance.

Quality (--quality; CPU only: the oracle and the twins).  The icospheres under the environment map as an equirectangular panorama from the
camera position, one ray per pixel centre: 8 spp from the oracle, per ray through its degenerate camera as ray_image_ref.oracle_pixels
does; guides from pt_debug_aov_rays_host at n = 4 over the same table; pt_debug_denoise_host with the defaults + PT_DENOISE_DEMODULATE;
relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) against the oracle's 1024 spp frame of the same rays for the noisy frame and for the
frame filtered with max_follow = 0 and with max_follow = 4 guides.  Reported, not asserted.

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


def rel_rmse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2))))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def cost(a, B):
    import aov_common as AC
    import async_common as AS
    from owl_path_tracer_amd.pyhost import procedural, ray_image, scene_io

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
        table, out = AS.DeviceFrame(W, H, floats=16), AS.DeviceFrame(W, H, floats=8)
        try:
            upload(ctx)
            AS.to_device(table.rgb, ray_image.pinhole(cam, W, H))

            def rays(k, form):
                ctx.set_option("box_exact", form)
                ctx.render_aov_rays_device(table.rgb, W, H, out.rgb, B.aov_default_params(n_samples=n, max_follow=k))
                ctx.set_option("box_exact", -1)

            calls = []
            for k in (0, 4):
                calls.append(("pt_render_aov_follow, max_follow %d" % k, lambda k=k: ctx.render_aov_follow_device(cam, W, H, out.rgb, B.aov_default_params(n_samples=n, max_follow=k))))
                calls.append(("pt_render_aov_rays, max_follow %d, box_exact 0" % k, lambda k=k: rays(k, 0)))
                calls.append(("pt_render_aov_rays, max_follow %d, default slab form" % k, lambda k=k: rays(k, -1)))
            ms = {k: [] for k, _ in calls}
            geo = {}
            for i in range(a.warmup + a.repeats):
                for k, f in calls:
                    f()
                    st = ctx.stats()  # waits for the launch's end
                    if i >= a.warmup:
                        ms[k].append(st["kernel_ms"])
                    geo[k] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], grid=st["grid"])
            ctx.synchronize()
        finally:
            ctx.close()
            table.free()
            out.free()
        row = dict(scene=what, kernel_ms={k: spread(v) for k, v in ms.items()}, launch=geo, over_pt_render_aov_follow={}, run_to_run_spread={})
        for k in (0, 4):
            base = ms["pt_render_aov_follow, max_follow %d" % k]
            for form in ("box_exact 0", "default slab form"):
                key = "pt_render_aov_rays, max_follow %d, %s" % (k, form)
                # the ratio of the medians, and the ratios of the paired runs (call i of one against call i of the other)
                pairs = [x / y for x, y in zip(ms[key], base)]
                row["over_pt_render_aov_follow"][key] = dict(of_medians=statistics.median(ms[key]) / statistics.median(base), paired=spread(pairs))
            row["run_to_run_spread"]["max_follow %d" % k] = {name: (max(v) - min(v)) / statistics.median(v) for name, v in ms.items() if "max_follow %d" % k in name}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return dict(size=[W, H], n_samples=n, repeats=a.repeats, warmup=a.warmup, table="ray_image.pinhole(cam), in HBM", measured=True,
                timer="pt_stats.kernel_ms (HIP events around the launch), median; device buffers", rows=rows)


def quality(a, B):
    import aov_common as AC
    import oracle as orc
    import ray_image_ref as RR
    from owl_path_tracer_amd.pyhost import ray_image

    W, H = (int(x) for x in a.pano.split("x"))
    name, spp, spp_ref, depth = "ico_map", 8, 1024, 8
    sc = AC.scene(name)
    S = orc.Scene(sc["flat"])
    env = orc.make_env(**sc["env"])
    eye = np.float32(sc["camera"][0])
    x = np.tile(np.arange(W, dtype=np.float64), H) + 0.5
    y = np.repeat(np.arange(H, dtype=np.float64), W) + 0.5
    orgs = np.tile(eye, (W * H, 1)).astype(np.float32)
    targets = (orgs.astype(np.float64) + ray_image.equirect_direction(x, y, W, H)).astype(np.float32)  # the pixel centres of ray_image.equirect
    _, dirs = RR.rays_through(orgs, targets)
    table = ray_image.fixed(orgs, dirs, W, H)
    t0 = time.time()
    noisy, _ = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, spp, depth)
    t1 = time.time()
    ref, _ = RR.oracle_pixels(orc, S, env, orgs, targets, W, H, spp_ref, depth)
    t2 = time.time()
    ctx = B.Context(-1)
    try:
        AC.upload(ctx, sc, B)
        prm = B.denoise_default_params(flags=B.PT_DENOISE_DEMODULATE)
        g0 = ctx.aov_rays_host(table, W, H, B.aov_default_params(n_samples=4, max_follow=0))
        g4 = ctx.aov_rays_host(table, W, H, B.aov_default_params(n_samples=4, max_follow=4))
        with0, _ = ctx.denoise_host(noisy, g0, prm)
        with4, _ = ctx.denoise_host(noisy, g4, prm)
    finally:
        ctx.close()
    masks = {"whole frame": np.ones((H, W), bool), "pixels the two guide sets differ in": (bits(g0) != bits(g4)).any(-1), "covered pixels (alpha 1)": g0[..., 3] == 1}
    row = dict(scene="%s as an equirectangular panorama from its camera position, one zero-jitter ray per pixel centre" % name, size=[W, H], spp=[spp, spp_ref], depth=depth,
               guides="pt_debug_aov_rays_host at n = 4, roughness_max 0.3", oracle_seconds=dict(noisy=round(t1 - t0, 1), reference=round(t2 - t1, 1)), rel_rmse={})
    for k, m in masks.items():
        row["rel_rmse"][k] = dict(pixels=int(m.sum()), noisy=rel_rmse(noisy[m], ref[m]), filtered_with_max_follow_0_guides=rel_rmse(with0[m], ref[m]),
                                  filtered_with_max_follow_4_guides=rel_rmse(with4[m], ref[m]))
    print(json.dumps(row), flush=True)
    return dict(metric="relRMSE = sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))); filter: pt_debug_denoise_host, default parameters + PT_DENOISE_DEMODULATE; reported, not asserted",
                rows=[row])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--pano", default="128x64")
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_aov_rays.json"))
    a = ap.parse_args()
    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.quality:
        rec["quality"] = quality(a, B)
    else:
        rec["cost"] = cost(a, B)
    rec.setdefault("cost", dict(measured=False, note="not recorded yet: needs an MI355X (python tools/aov_rays_bench.py)"))
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
