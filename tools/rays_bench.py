"""What the ray queries cost: pt_trace_closest_device / pt_trace_occluded_device on one MI355X.

    python tools/rays_bench.py [--write] [--out FILE] [--size 1920x1080] [--repeats 20] [--warmups 3]

Scenes: the C4 stand-in (dragon.json on procedural.dragon_standin) and a 3 x 3 x 3 block of icospheres (ray_battery.icosphere(5): 552 960
triangles with shared vertices).  Rays, all in device buffers, tmax = +inf:
  primary   the rays of a --size camera through the pixel centres, in pixel order x + W * y (coherent);
  shuffled  the same rays in a random order (the same work, no coherence inside a wave);
  bounce    one cosine-weighted bounce from the hit points of the primary rays, in pixel order (the incoherent case; fewer rays: the
            primary rays that missed have none).
Figures: kernel_ms of pt_stats (HIP events around the one launch), median of --repeats after --warmups, all in one run, as Mrays/s of
closest and of occluded at "rays_refill" 0 / 16 / 32 / 48 / 63; beside them pt_render_aov_device at n = 1 on the same camera, the
library's own first-hit pass over the same primary rays (it also shades: a yardstick, not a like-for-like).
default: 32 stays unless another value is faster on BOTH scenes - summed over the three ray sets and both calls - by more than the
run-to-run spread seen in this run ((max - min) / median, the largest over all configurations); the value and the reason are recorded.
--write merges the section into profiles/r21_rays.json; --out FILE into another file.  Measurement only: nothing here is asserted by the
test suite, and without a GPU it fails (there is no fallback)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
PROFILE = os.path.join(ROOT, "profiles", "r21_rays.json")
REFILLS = (0, 16, 32, 48, 63)
DEFAULT_REFILL = 32


def merge(path, sections):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.update(sections)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def primary_rays(cam, W, H):
    """(W * H, 6) float32: origin and normalised direction through every pixel centre, in pixel order x + W * y."""
    a = cam.as_array().astype(np.float64).reshape(4, 3)  # origin, llc, horizontal, vertical
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    su, sv = ((px.reshape(-1) + 0.5) / W)[:, None], ((py.reshape(-1) + 0.5) / H)[:, None]
    d = a[1] + a[2] * su + a[3] * sv - a[0]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.broadcast_to(a[0], d.shape), d], 1).astype(np.float32)


def bounce_rays(rays, hits, soup, rng):
    """One cosine-weighted bounce from every hit: origin on the surface, direction about the geometric normal that faces the ray."""
    k = np.nonzero(hits["prim"] >= 0)[0]
    o, d = rays[k, :3].astype(np.float64), rays[k, 3:].astype(np.float64)
    p = o + hits["t"][k, None].astype(np.float64) * d
    t = soup[hits["prim"][k]].astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    n = np.where((n * d).sum(1, keepdims=True) > 0, -n, n)
    u1, u2 = rng.random(k.size), rng.random(k.size)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    helper = np.where(np.abs(n[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    tx = np.cross(helper, n)
    tx /= np.linalg.norm(tx, axis=1, keepdims=True)
    ty = np.cross(n, tx)
    w = tx * (r * np.cos(phi))[:, None] + ty * (r * np.sin(phi))[:, None] + n * np.sqrt(np.maximum(0.0, 1.0 - u1))[:, None]
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    return np.concatenate([p, w], 1).astype(np.float32)


def scenes(B):
    import accum_reproject_common as RC
    import ray_battery as rb
    from owl_path_tracer_amd.pyhost import procedural, scene_io

    _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
    ents = scene_io.build_entities(procedural.dragon_standin(), mats)
    yield ("c4_standin", ents, [m for _, m, _ in mats], (np.array([4.0, 2.5, 0.0]), np.array([0.0, 0.75, 0.0]), 50.0), RC)
    ico = rb.icosphere(5)
    offs = np.array([[x, y, z] for x in (-2.5, 0, 2.5) for y in (-2.5, 0, 2.5) for z in (-2.5, 0, 2.5)], np.float32)
    tris = np.concatenate([ico + o for o in offs]).astype(np.float32)
    yield ("icospheres_27x20480", [(rb.mesh_of(tris), 0)], [scene_io.MAT_DEFAULT], (np.array([9.0, 6.0, 7.0]), np.zeros(3), 45.0), RC)


def run(B, a):
    import async_common as AS
    import ray_battery as rb

    W, H = (int(x) for x in a.size.split("x"))
    hip = AS.hip()
    out = dict(size=[W, H], repeats=a.repeats, warmups=a.warmups, refills=list(REFILLS), unit="Mrays/s from the median kernel_ms of pt_stats (HIP events around the launch)", scenes={})
    spread_max = 0.0
    totals = {}  # scene -> refill -> summed median ms
    for name, ents, mats, (eye, at, fov), RC in scenes(B):
        ctx = B.Context(0)  # raises without a gfx950 device
        ctx.upload_scene(ents, mats, env=B.make_env(color=(1, 1, 1), intensity=1.0))
        soup = rb._soup_of(ents)
        cam = RC.look(eye, at, [0.0, 1.0, 0.0], fov, W, H)
        prim = primary_rays(cam, W, H)
        hits = ctx.trace_closest(prim)
        rng = np.random.default_rng(21)
        sets = dict(primary=prim, shuffled=prim[rng.permutation(prim.shape[0])], bounce=bounce_rays(prim, hits, soup, rng))
        rec = dict(triangles=int(soup.shape[0]), primary_hit_share=float((hits["prim"] >= 0).mean()), rays={})
        totals[name] = {r: 0.0 for r in REFILLS}
        aov = AS.DeviceFrame(W, H, floats=8)
        ms = []
        for i in range(a.warmups + a.repeats):
            ctx.render_aov_device(cam, W, H, 1, aov.rgb)
            ms.append(ctx.stats()["kernel_ms"])
        ms = ms[a.warmups:]
        aov.free()
        rec["pt_render_aov_n1"] = dict(kernel_ms=statistics.median(ms), mrays_per_s=W * H / statistics.median(ms) * 1e-3)
        for sname, rays in sets.items():
            n = rays.shape[0]
            r = B.make_rays(rays)
            d_rays, d_out = C.c_void_p(), C.c_void_p()
            AS._ok(hip.hipMalloc(C.byref(d_rays), n * 32), "hipMalloc")
            AS._ok(hip.hipMalloc(C.byref(d_out), n * 16), "hipMalloc")
            AS.to_device(d_rays.value, r)
            srec = dict(rays=int(n))
            launch = None
            for call, fn in (("closest", ctx.trace_closest_device), ("occluded", ctx.trace_occluded_device)):
                srec[call] = {}
                for refill in REFILLS:
                    ctx.set_option("rays_refill", refill)
                    ms = []
                    for i in range(a.warmups + a.repeats):
                        fn(d_rays.value, n, d_out.value)
                        st = ctx.stats()
                        ms.append(st["kernel_ms"])
                    ms = ms[a.warmups:]
                    med = statistics.median(ms)
                    spread_max = max(spread_max, (max(ms) - min(ms)) / med)
                    totals[name][refill] += med
                    srec[call][str(refill)] = dict(mrays_per_s=round(n / med * 1e-3, 1), kernel_ms=dict(median=med, min=min(ms), max=max(ms)))
                    launch = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], stack_entries=st["stack_entries"])
                srec[call]["launch"] = launch
            ctx.synchronize()
            hip.hipFree(d_rays)
            hip.hipFree(d_out)
            rec["rays"][sname] = srec
            print(json.dumps({name: {sname: srec}}), flush=True)
        ctx.close()
        out["scenes"][name] = rec
    # the default: 32 unless another value wins on both scenes by more than the spread of this run
    better = [r for r in REFILLS if r != DEFAULT_REFILL and all(totals[s][r] < totals[s][DEFAULT_REFILL] * (1.0 - spread_max) for s in totals)]
    best = min(better, key=lambda r: sum(totals[s][r] for s in totals)) if better else DEFAULT_REFILL
    out["summed_median_ms_by_refill"] = {s: {str(r): v for r, v in t.items()} for s, t in totals.items()}
    out["run_to_run_spread"] = spread_max
    out["default"] = dict(rays_refill=best, reason=("%d is faster than 32 on both scenes by more than the run-to-run spread of %.1f %%" % (best, 100 * spread_max)) if better else
                          ("no other value is faster than 32 on both scenes by more than the run-to-run spread of %.1f %%" % (100 * spread_max)))
    print(json.dumps(dict(default=out["default"], summed_median_ms_by_refill=out["summed_median_ms_by_refill"])), flush=True)
    return dict(rays=out)


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
