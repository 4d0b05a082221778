"""What the batch forms of the guide pass and the denoiser cost against the loop they replace (pt_render_aov_batch, pt_denoise_batch).

    python tools/batch_guides_bench.py [--samples 4] [--repeats 20] [--warmup 3] [--only c2|c4] [--out profiles/r16_batch_guides.json]

One MI355X (without a GPU the tool fails: there is no fallback), one run, the two versions alternating so that both see the same machine:
  A, the loop   for each frame: pt_set_materials, pt_render_aov_follow_device, pt_denoise_device   (K host waits, K * (L + 3) launches)
  B, the batch  pt_render_aov_batch_device + pt_denoise_batch_device on the same frames            (1 host wait, sequences * (L + 3) launches)
Both work on device buffers and end in pt_synchronize.  The frames are a material sweep as tools/ab_bench.py batch=K builds it (the
sphere's / the first material's metallic at K values 0..1), n = --samples and otherwise the default parameters of both calls; the colour
input of the filter is a 4 spp pt_render_batch of the same frames, rendered once.
Configurations: C2's Cornell sweep at 512 x 512 with K = 1, 4 and 8; the C4 stand-in at 1920 x 1080 with K = 4.
Timers: wall_ms = a host clock around the calls including the closing pt_synchronize; kernel_ms = pt_stats.kernel_ms of each call, read
in passes of their own (reading it waits for the call, which a wall-clock pass must not do).  Median of --repeats after --warmup.
The tool asserts A == B bit for bit (guides, filtered frames and RGBA8) at every size it times.
One condition is recorded per configuration and must hold at C2 K = 8: the guide batch's kernel_ms may exceed the sum of the K
single-frame kernel_ms of the same run by no more than that run's spread of the loop (max - min of that sum over the repeats)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def scenes(B, only):
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    out = []
    if only in (None, "c2"):
        sc = scene_io.load_scene_dir(os.path.join(ROOT, "assets"), "cornell-box")
        c = sc["camera"]
        out.append(("c2 (cornell-box, 512 x 512)", sc["entities"], sc["materials"], 512, 512, (c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"]), (1, 4, 8)))
    if only in (None, "c4"):
        _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
        out.append(("c4 stand-in (dragon.json on procedural.dragon_standin, 1920 x 1080)", scene_io.build_entities(procedural.dragon_standin(), mats), mats, 1920, 1080,
                    ([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0), (4,)))
    return out


def sweep(mats, K):
    base = np.stack([m for _, m, _ in mats]).astype(np.float32)
    names = [n for n, _, _ in mats]
    who = names.index("sphere") if "sphere" in names else 0
    tables = []
    for j in range(K):
        mm = base.copy()
        mm[who, 4] = j / max(1, K - 1)  # metallic
        tables.append(mm)
    return base, tables


def measure(ctx, B, A, what, mats, cam, W, H, K, a):
    base, tables = sweep(mats, K)
    frames = [(cam, t) for t in tables]
    prm = B.aov_default_params(n_samples=a.samples)
    dn = B.denoise_default_params()
    L = dn.iterations
    rgb = A.DeviceFrame(W, H, frames=K)
    gA, gB = A.DeviceFrame(W, H, frames=K, floats=8), A.DeviceFrame(W, H, frames=K, floats=8)
    oA, oB = A.DeviceFrame(W, H, frames=K), A.DeviceFrame(W, H, frames=K)
    npx = W * H
    try:
        ctx.render_batch_device(frames, W, H, 4, 8, rgb.rgb)
        ctx.synchronize()

        def loop(kernel_ms=None):
            for f, (c, t) in enumerate(frames):
                ctx.set_materials(t)
                ctx.render_aov_follow_device(c, W, H, gA.rgb + f * npx * 32, prm)
                if kernel_ms is not None:
                    kernel_ms[0] += ctx.stats()["kernel_ms"]
                ctx.denoise_device(rgb.rgb + f * npx * 12, gA.rgb + f * npx * 32, W, H, oA.rgb + f * npx * 12, dn, d_out_rgba8=oA.rgba8 + f * npx * 4)
                if kernel_ms is not None:
                    kernel_ms[1] += ctx.stats()["kernel_ms"]
            ctx.synchronize()

        def batch(kernel_ms=None, geo=None):
            ctx.render_aov_batch_device(frames, W, H, gB.rgb, prm)
            if kernel_ms is not None:
                st = ctx.stats()
                kernel_ms[0] += st["kernel_ms"]
                geo["guide"] = dict(launches=st["launches"], vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], grid=st["grid"], block=st["block"])
            ctx.denoise_batch_device(rgb.rgb, gB.rgb, K, W, H, oB.rgb, dn, d_out_rgba8=oB.rgba8)
            if kernel_ms is not None:
                st = ctx.stats()
                kernel_ms[1] += st["kernel_ms"]
                geo["denoise"] = dict(launches=st["launches"], vgprs=st["vgprs"], grid=st["grid"], block=st["block"])
            ctx.synchronize()

        wall = {"A": [], "B": []}
        kms = {"A": [], "B": []}
        geo = {}
        for i in range(a.warmup + a.repeats):
            for side, fn in (("A", loop), ("B", batch)):
                t0 = time.perf_counter()
                fn()
                w = (time.perf_counter() - t0) * 1e3
                k = [0.0, 0.0]
                if side == "A":
                    fn(k)
                else:
                    fn(k, geo)
                if i >= a.warmup:
                    wall[side].append(w)
                    kms[side].append(k)
        ctx.set_materials(base)
        same = {}
        for name, x, y in (("guides", gA, gB), ("filtered", oA, oB)):
            (xa, x8), (ya, y8) = x.read(), y.read()
            same[name] = bool((xa.view(np.uint32) == ya.view(np.uint32)).all())
            if name == "filtered":
                same["rgba8"] = bool((x8 == y8).all())
    finally:
        for d in (rgb, gA, gB, oA, oB):
            d.free()
    med = statistics.median
    ga, gb = [k[0] for k in kms["A"]], [k[0] for k in kms["B"]]
    da, db = [k[1] for k in kms["A"]], [k[1] for k in kms["B"]]
    spread = max(ga) - min(ga)
    row = dict(scene=what, size=[W, H], K=K, n_samples=a.samples, iterations=L, bit_identical=same,
               wall_ms=dict(A_loop=dict(median=med(wall["A"]), min=min(wall["A"]), max=max(wall["A"])), B_batch=dict(median=med(wall["B"]), min=min(wall["B"]), max=max(wall["B"]))),
               wall_ms_per_frame=dict(A_loop=med(wall["A"]) / K, B_batch=med(wall["B"]) / K),
               guide_kernel_ms=dict(A_sum_of_single_frames=dict(median=med(ga), min=min(ga), max=max(ga)), B_batch=dict(median=med(gb), min=min(gb), max=max(gb))),
               denoise_kernel_ms=dict(A_sum_of_single_frames=dict(median=med(da), min=min(da), max=max(da)), B_batch=dict(median=med(db), min=min(db), max=max(db))),
               launches=dict(A_loop=K * (L + 3), B_batch=geo["guide"]["launches"] + geo["denoise"]["launches"]), host_waits=dict(A_loop=K, B_batch=1), B_launch=geo,
               guide_batch_condition=dict(batch_minus_sum_ms=med(gb) - med(ga), loop_spread_ms=spread, holds=bool(med(gb) - med(ga) <= spread)))
    print(json.dumps(row), flush=True)
    if not all(same.values()):
        raise SystemExit("A and B differ: %r" % same)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("c2", "c4"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_batch_guides.json"))
    a = ap.parse_args()
    import ptamd

    ptamd.load()
    import async_common as A
    from owl_path_tracer_amd.pyhost import binding as B

    rows = []
    for what, ents, mats, W, H, camera, Ks in scenes(B, a.only):
        ctx = B.Context(0)  # raises without a gfx950 device
        try:
            ctx.upload_scene(ents, [m for _, m, _ in mats], env=B.make_env(color=(1, 1, 1), intensity=0.0))
            cam = B.to_camera_data(*camera, W, H)
            for K in Ks:
                rows.append(measure(ctx, B, A, what, mats, cam, W, H, K, a))
        finally:
            ctx.close()
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    kept = [r for r in rec.get("rows", []) if a.only and not r["scene"].startswith(a.only)]
    rec.update(what="A: per frame pt_set_materials + pt_render_aov_follow_device + pt_denoise_device; B: pt_render_aov_batch_device + pt_denoise_batch_device; one MI355X, one "
                    "run, A and B alternating; device buffers, each version ends in pt_synchronize",
               timers="wall_ms: host clock around the calls and the closing pt_synchronize; kernel_ms: pt_stats.kernel_ms per call, in passes of their own; median of "
                      "%d after %d warm-ups" % (a.repeats, a.warmup),
               measured=True, rows=kept + rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    bad = [r for r in rows if r["K"] == 8 and not r["guide_batch_condition"]["holds"]]
    if bad:
        raise SystemExit("the guide batch's kernel_ms at K = 8 exceeds the sum of the single frames by more than the loop's spread: %r" % bad[0]["guide_batch_condition"])


if __name__ == "__main__":
    main()
