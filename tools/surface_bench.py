"""What the surface record costs beside the closest hit: pt_trace_surface_device against pt_trace_closest_device on one MI355X.

    python tools/surface_bench.py [--write] [--out FILE] [--size 1920x1080] [--repeats 20] [--warmups 3]

Scenes and rays are those of tools/rays_bench.py: the C4 stand-in and the 3 x 3 x 3 block of icospheres, the rays of a --size camera
through the pixel centres in pixel order (primary) and in a random order (shuffled), all in device buffers, tmax = +inf.
Figures: kernel_ms of pt_stats (HIP events around the one launch), the median of --repeats after --warmups; the two calls ALTERNATE in
one run (closest, surface, closest, ...), so both see the same clocks and caches.  Reported per scene and ray set: Grays/s of both,
their ratio (surface / closest) and the spread of each ((max - min) / median).  A surface ray moves 32 + 80 bytes of ray I/O where a
closest-hit ray moves 32 + 16, and a hit adds 112 bytes of records, the material row and a texel.
--write merges the section into profiles/r25_surface.json; --out FILE into another file.  Measurement only: nothing here is asserted by
the test suite, and without a GPU it fails (there is no fallback)."""
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
PROFILE = os.path.join(ROOT, "profiles", "r25_surface.json")


def run(B, a):
    import async_common as AS
    import rays_bench as RB

    W, H = (int(x) for x in a.size.split("x"))
    hip = AS.hip()
    out = dict(size=[W, H], repeats=a.repeats, warmups=a.warmups, unit="Grays/s from the median kernel_ms of pt_stats (HIP events around the launch); the two calls alternate in one run",
               scenes={})
    for name, ents, mats, (eye, at, fov), RC in RB.scenes(B):
        ctx = B.Context(0)  # raises without a gfx950 device
        ctx.upload_scene(ents, mats, env=B.make_env(color=(1, 1, 1), intensity=1.0))
        cam = RC.look(eye, at, [0.0, 1.0, 0.0], fov, W, H)
        prim = RB.primary_rays(cam, W, H)
        n = prim.shape[0]
        hits = ctx.trace_closest(prim)
        rec = dict(triangles=int(ctx.stats()["n_triangles"]), primary_hit_share=float((hits["prim"] >= 0).mean()), rays={})
        sets = dict(primary=prim, shuffled=prim[np.random.default_rng(21).permutation(n)])
        d_rays, d_hits, d_surf = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p, b in ((d_rays, n * 32), (d_hits, n * 16), (d_surf, n * 80)):
            AS._ok(hip.hipMalloc(C.byref(p), b), "hipMalloc")
        for sname, rays in sets.items():
            AS.to_device(d_rays.value, B.make_rays(rays))
            calls = (("closest", ctx.trace_closest_device, d_hits), ("surface", ctx.trace_surface_device, d_surf))
            ms = dict(closest=[], surface=[])
            launch = {}
            for i in range(a.warmups + a.repeats):
                for call, fn, d_out in calls:
                    fn(d_rays.value, n, d_out.value)
                    st = ctx.stats()
                    ms[call].append(st["kernel_ms"])
                    launch[call] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], stack_entries=st["stack_entries"])
            ctx.synchronize()
            srec = dict(rays=int(n))
            for call in ms:
                m = ms[call][a.warmups:]
                med = statistics.median(m)
                srec[call] = dict(grays_per_s=round(n / med * 1e-6, 3), kernel_ms=dict(median=med, min=min(m), max=max(m)), spread=round((max(m) - min(m)) / med, 4), launch=launch[call])
            srec["surface_over_closest"] = round(srec["surface"]["grays_per_s"] / srec["closest"]["grays_per_s"], 3)
            rec["rays"][sname] = srec
            print(json.dumps({name: {sname: srec}}), flush=True)
        for p in (d_rays, d_hits, d_surf):
            hip.hipFree(p)
        ctx.close()
        out["scenes"][name] = rec
    return dict(surface=out)


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
    import rays_bench as RB

    sections = run(B, a)
    if a.write:
        RB.merge(PROFILE, sections)
    if a.out:
        RB.merge(a.out, sections)


if __name__ == "__main__":
    main()
