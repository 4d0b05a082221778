"""What a ray image costs: pt_render_rays_device against pt_render_device on one MI355X.

    python tools/ray_image_bench.py [--write] [--out FILE] [--size 1920x1080] [--pano 2048x1024] [--spp 64] [--depth 8] [--repeats 20] [--warmups 3]

Scene: the C4 stand-in (dragon.json on procedural.dragon_standin), bench.py's camera.  Frames, all into device buffers, tables in HBM:
  pt_render             the camera's frame, the yardstick;
  pinhole               pt_render_rays of ray_image.pinhole(cam): the same frame up to an ulp in the directions, one 64-byte gather per sample;
  pinhole_zero_jitter   the same table with du = dv = 0 (every sample of a pixel along one ray: the gather with the most coherent paths);
  equirect              a --pano panorama from the camera position (ray_image.equirect).
The device form cannot see the records and takes the subtracting slab form unless option "box_exact" says otherwise; pt_render takes the fma
form for this camera.  Each ray image is therefore measured twice: "box_exact" = 0 (the slab form pt_render uses: like for like) and the
default.  Figures: kernel_ms of pt_stats (HIP events from the first launch to the last kernel end), median of --repeats after --warmups, all in
one run, as Msamples/s = W * H * spp / kernel_ms.  Record only: there is no threshold.

Also recorded, for tests/test_gpu_ray_image.py leg D: pinhole(cam, 64, 48) at 256 spp against pt_render(cam) on Cornell under the metrics of
tools/tolerance_calibration.py.

--write merges the sections into profiles/r22_ray_image.json; --out FILE into another file.  Measurement only: nothing here is asserted by
the test suite, and without a GPU it fails (there is no fallback)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
PROFILE = os.path.join(ROOT, "profiles", "r22_ray_image.json")


def merge(path, sections):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.update(sections)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def timed(ctx, a, call):
    ms = []
    for _ in range(a.warmups + a.repeats):
        call()
        ms.append(ctx.stats()["kernel_ms"])  # waits for the frame's last kernel
    ms = ms[a.warmups:]
    st = ctx.stats()
    return ms, dict(vgprs=st["vgprs"], grid=st["grid"], lds_bytes=st["lds_bytes"], kernel_variant=st["kernel_variant"], launches=st["launches"], prepass_spp=st["prepass_spp"])


def figure(ms, samples, launch):
    med = statistics.median(ms)
    return dict(msamples_per_s=round(samples / med * 1e-3, 1), kernel_ms=dict(median=med, min=min(ms), max=max(ms)), launch=launch)


def cost(B, a):
    import async_common as AS
    from owl_path_tracer_amd.pyhost import procedural, ray_image, scene_io

    W, H = (int(x) for x in a.size.split("x"))
    PW, PH = (int(x) for x in a.pano.split("x"))
    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ents = scene_io.build_entities(procedural.dragon_standin(), mats)
    ctx = B.Context(0)  # raises without a gfx950 device
    ctx.upload_scene(ents, [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=1.0))
    eye = [4.0, 2.5, 0.0]
    cam = B.to_camera_data(eye, [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, W, H)
    out = dict(scene="C4 stand-in", size=[W, H], pano=[PW, PH], spp=a.spp, depth=a.depth, repeats=a.repeats, warmups=a.warmups,
               unit="Msamples/s = W * H * spp / median kernel_ms of pt_stats (HIP events, first launch to last kernel end)", frames={})
    frame = AS.DeviceFrame(max(W, PW), max(H, PH))
    ms, launch = timed(ctx, a, lambda: ctx.render_device(cam, W, H, a.spp, a.depth, frame.rgb))
    out["frames"]["pt_render"] = figure(ms, W * H * a.spp, launch)
    print(json.dumps({"pt_render": out["frames"]["pt_render"]}), flush=True)
    pin = ray_image.pinhole(cam, W, H)
    zero = pin.copy()
    zero["du"] = 0
    zero["dv"] = 0
    for name, table, w, h in (("pinhole", pin, W, H), ("pinhole_zero_jitter", zero, W, H), ("equirect", ray_image.equirect(eye, PW, PH), PW, PH)):
        d_table = AS.DeviceFrame(w, h, floats=16)
        AS.to_device(d_table.rgb, table)
        for label, form in (("fma_slab_form", 0), ("default_subtracting_slab_form", -1)):
            ctx.set_option("box_exact", form)
            ms, launch = timed(ctx, a, lambda: ctx.render_rays_device(d_table.rgb, w, h, a.spp, a.depth, frame.rgb))
            out["frames"].setdefault(name, {})[label] = figure(ms, w * h * a.spp, launch)
        ctx.set_option("box_exact", -1)
        ctx.synchronize()
        d_table.free()
        print(json.dumps({name: out["frames"][name]}), flush=True)
    base = out["frames"]["pt_render"]["kernel_ms"]["median"]
    out["pinhole_over_pt_render"] = {k: round(out["frames"]["pinhole"][k]["kernel_ms"]["median"] / base, 4) for k in out["frames"]["pinhole"]}
    frame.free()
    ctx.close()
    return out


def jitter(B):
    import aov_common as AC
    import tolerance_calibration as T
    from owl_path_tracer_amd.pyhost import ray_image

    W, H, spp, depth = 64, 48, 256, 8
    sc = AC.scene("cornell")
    ctx = B.Context(0)
    AC.upload(ctx, sc, B)
    cam = AC.camera(sc, W, H, B.to_camera_data)
    a, a8 = ctx.render(cam, W, H, spp, depth, want_rgba8=True)
    b, b8 = ctx.render_rays(ray_image.pinhole(cam, W, H), W, H, spp, depth, want_rgba8=True)
    ctx.close()
    m = T.metrics(a, a8, b, b8)
    m.update(scene="cornell (tests/aov_common.py)", size=[W, H], spp=spp, depth=depth, pair="pt_render(cam)  vs  pt_render_rays(ray_image.pinhole(cam))",
             bars=dict(l2_p99=1e-4, l2_p999=0.04, rel_rmse=1e-2))
    print(json.dumps({"jitter_over_a_frame": m}), flush=True)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--pano", default="2048x1024")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    a = ap.parse_args()

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    sections = dict(jitter_over_a_frame=jitter(B), cost=cost(B, a))
    if a.write:
        merge(PROFILE, sections)
    if a.out:
        merge(a.out, sections)


if __name__ == "__main__":
    main()
