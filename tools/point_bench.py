"""What the nearest-surface query costs: pt_closest_point_device on one MI355X.

    python tools/point_bench.py [--write] [--out FILE] [--size 1920x1080] [--grid 128] [--repeats 20] [--warmups 3]

Scenes: those of tools/rays_bench.py, the C4 stand-in and the 3 x 3 x 3 block of icospheres.  Points, all in device buffers, radius =
+inf, about two million a set:
  grid      a regular --grid^3 lattice over the scene's box, x fastest (neighbours in a wave are neighbours in space);
  shuffled  the same points in a random order (the same work, no coherence inside a wave);
  surface   the hit points of the --size primary rays, moved 1e-3 extents along the geometric normal that faces the camera, in pixel
            order (what a proximity or contact query looks like: the answer is next to the point).
Figures: kernel_ms of pt_stats (HIP events around the one launch), median of --repeats after --warmups, all in one run, as Mpoints/s;
for scale pt_trace_closest_device over the primary rays in the same run, as Mrays/s.
THE STACK FORM.  The point kernel keeps a lane's stack entries either as the reference alone (pop and fetch: PT_POINTS_STACK_DIST = 0,
the build that ships) or with the box distance beside the reference (dropped at pop when stale: 1).  The form is a compile-time macro,
so the other one is a library of its own: `make -C owl-path-tracer_amd/csrc variant NAME=points_dist FLAGS=-DPT_POINTS_STACK_DIST=1`
and then this tool with PT_LIB_PATH=.../libmi355pt_points_dist.so.  A run measures the library it loads, names the section after that
library's form (the library says which it is) and merges it beside the other one; once both are there the file also carries their
ratio per scene and set.  --label NAME names the section otherwise: builds with another PT_POINTS_RANGES (ranges per resident wave,
csrc/pt_points_host.cpp) or PT_POINTS_LDS_WORDS.
--write merges into profiles/r28_points.json; --out FILE into another file.  Measurement only: nothing here is asserted by the test
suite, and without a GPU it fails (there is no fallback)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
PROFILE = os.path.join(ROOT, "profiles", "r28_points.json")
FORMS = {2: "stack_dist", 1: "pop_and_fetch"}


def surface_points(prim, hits, soup, ext):
    k = np.nonzero(hits["prim"] >= 0)[0]
    o, d = prim[k, :3].astype(np.float64), prim[k, 3:].astype(np.float64)
    p = o + hits["t"][k, None].astype(np.float64) * d
    t = soup[hits["prim"][k]].astype(np.float64)
    n = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    n /= np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)
    n = np.where((n * d).sum(1, keepdims=True) > 0, -n, n)
    return (p + 1e-3 * ext * n).astype(np.float32)


def timed(fn, stats, repeats, warmups):
    ms, st = [], None
    for _ in range(warmups + repeats):
        fn()
        st = stats()
        ms.append(st["kernel_ms"])
    ms = ms[warmups:]
    med = statistics.median(ms)
    return med, dict(median=med, min=min(ms), max=max(ms)), round((max(ms) - min(ms)) / med, 4), st


def run(B, a):
    import async_common as AS
    import ray_battery as rb
    import rays_bench as RB

    W, H = (int(x) for x in a.size.split("x"))
    hip = AS.hip()
    form = FORMS[int(B.lib().pt_points_entry_words())]
    out = dict(library=os.path.basename(B.LIB_PATH), size=[W, H], grid=a.grid, repeats=a.repeats, warmups=a.warmups, scenes={},
               unit="Mpoints/s (Mrays/s for pt_trace_closest_device) from the median kernel_ms of pt_stats (HIP events around the launch)")
    for name, ents, mats, (eye, at, fov), RC in RB.scenes(B):
        ctx = B.Context(0)  # raises without a gfx950 device
        ctx.upload_scene(ents, mats, env=B.make_env(color=(1, 1, 1), intensity=1.0))
        soup = rb._soup_of(ents)
        P = soup.reshape(-1, 3).astype(np.float64)
        lo, hi = P.min(0), P.max(0)
        ext = float((hi - lo).max())
        cam = RC.look(eye, at, [0.0, 1.0, 0.0], fov, W, H)
        prim = RB.primary_rays(cam, W, H)
        hits = ctx.trace_closest(prim)
        g = (np.arange(a.grid) + 0.5) / a.grid
        gz, gy, gx = np.meshgrid(g, g, g, indexing="ij")
        grid = (lo + np.stack([gx.reshape(-1), gy.reshape(-1), gz.reshape(-1)], 1) * (hi - lo)).astype(np.float32)
        rng = np.random.default_rng(28)
        sets = dict(grid=grid, shuffled=grid[rng.permutation(grid.shape[0])], surface=surface_points(prim, hits, soup, ext))
        rec = dict(triangles=int(soup.shape[0]), primary_hit_share=float((hits["prim"] >= 0).mean()), points={})
        n = prim.shape[0]
        d_in, d_out = C.c_void_p(), C.c_void_p()
        AS._ok(hip.hipMalloc(C.byref(d_in), n * 32), "hipMalloc")
        AS._ok(hip.hipMalloc(C.byref(d_out), n * 16), "hipMalloc")
        AS.to_device(d_in.value, B.make_rays(prim))
        med, ms, spread, st = timed(lambda: ctx.trace_closest_device(d_in.value, n, d_out.value), ctx.stats, a.repeats, a.warmups)
        rec["pt_trace_closest_device_primary"] = dict(rays=int(n), mrays_per_s=round(n / med * 1e-3, 1), kernel_ms=ms, spread=spread)
        hip.hipFree(d_in)
        hip.hipFree(d_out)
        for sname, x in sets.items():
            n = x.shape[0]
            pts = B.make_points(x)
            d_in, d_out = C.c_void_p(), C.c_void_p()
            AS._ok(hip.hipMalloc(C.byref(d_in), n * 16), "hipMalloc")
            AS._ok(hip.hipMalloc(C.byref(d_out), n * 32), "hipMalloc")
            AS.to_device(d_in.value, pts)
            med, ms, spread, st = timed(lambda: ctx.closest_point_device(d_in.value, n, d_out.value), ctx.stats, a.repeats, a.warmups)
            ctx.synchronize()  # PT_E_HIP: a walk ran out of its bounds
            got = np.empty(n, B.POINT_HIT_DTYPE)
            AS._ok(hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_out, got.nbytes, AS.D2H), "hipMemcpy")
            hip.hipFree(d_in)
            hip.hipFree(d_out)
            rec["points"][sname] = dict(points=int(n), mpoints_per_s=round(n / med * 1e-3, 1), kernel_ms=ms, spread=spread, found_share=float((got["prim"] >= 0).mean()),
                                        mean_dist_in_extents=float(got["dist"].astype(np.float64).mean() / ext), records_crc=int(np.bitwise_xor.reduce(got.view(np.uint32).reshape(-1))),
                                        launch=dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], stack_entries=st["stack_entries"]))
            print(json.dumps({name: {sname: rec["points"][sname]}}), flush=True)
        ctx.close()
        out["scenes"][name] = rec
    return {a.label or form: out}


def with_ratios(rec):
    """Once both forms are in the file: Mpoints/s of stack_dist over pop_and_fetch per scene and set, and whether the records agree."""
    if all(f in rec for f in FORMS.values()):
        a, b = rec["stack_dist"]["scenes"], rec["pop_and_fetch"]["scenes"]
        rec["stack_dist_over_pop_and_fetch"] = {s: {k: round(a[s]["points"][k]["mpoints_per_s"] / b[s]["points"][k]["mpoints_per_s"], 3) for k in a[s]["points"] if k in b[s]["points"]}
                                                for s in a if s in b}
        rec["records_agree"] = all(a[s]["points"][k]["records_crc"] == b[s]["points"][k]["records_crc"] for s in a if s in b for k in a[s]["points"] if k in b[s]["points"])
    return rec


def merge(path, sections):
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec.update(sections)
    with open(path, "w") as f:
        json.dump(with_ratios(rec), f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--label", help="name of the section instead of the library's stack form (further variant builds: ranges per wave, LDS levels)")
    a = ap.parse_args()

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    B.lib().pt_points_entry_words.restype = C.c_int
    sections = run(B, a)
    if a.write:
        merge(PROFILE, sections)
    if a.out:
        merge(a.out, sections)


if __name__ == "__main__":
    main()
