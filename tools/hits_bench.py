"""What the list of the first K hits costs beside the closest hit: pt_trace_hits_device at K = 1, 2, 4, 8, 16 against
pt_trace_closest_device on one MI355X.

    [PT_LIB_PATH=variant.so] python tools/hits_bench.py --label NAME [--write] [--out FILE] [--size 1920x1080] [--repeats 10] [--warmups 2]

Scenes and rays are those of tools/rays_bench.py: the C4 stand-in and the 3 x 3 x 3 block of icospheres, the rays of a --size camera
through the pixel centres in pixel order (primary) and in a random order (shuffled), all in device buffers, tmax = +inf.
Figures: kernel_ms of pt_stats (HIP events around the one launch), the median of --repeats after --warmups; the six calls ALTERNATE in
one run (closest, K = 1, K = 2, ..., closest, ...), so all see the same clocks and caches.  Reported per scene and ray set: Grays/s of
each, the ratio of each K to closest (the unchanged closest-hit kernel is the yardstick of what the list costs; K = 1 computes the
same thing), the spread ((max - min) / median), the launch geometry (vgprs, lds_bytes, grid) and the share of rays whose list is full.
--label names the CANDIDATE the loaded library was built as: a tunable such as PT_HITS_RANGES (ranges per resident wave,
csrc/pt_rays_host.cpp) is a compile-time macro, so a candidate is a library of its own (make -C owl-path-tracer_amd/csrc variant
NAME=... FLAGS=...) run through PT_LIB_PATH.  (The entry3_* candidates of the profile were builds of a 3-word list entry, which is
no longer in the source.)  --write merges the candidate into profiles/r30_hits.json under candidates[label]; --out FILE into
another file.  Measurement only: nothing here is asserted by the test suite, and without a GPU it fails (there is no fallback)."""
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
PROFILE = os.path.join(ROOT, "profiles", "r30_hits.json")
KS = (1, 2, 4, 8, 16)


def run(B, a):
    import async_common as AS
    import rays_bench as RB

    W, H = (int(x) for x in a.size.split("x"))
    hip = AS.hip()
    out = dict(size=[W, H], repeats=a.repeats, warmups=a.warmups,
               unit="Grays/s from the median kernel_ms of pt_stats (HIP events around the launch); the calls alternate in one run", scenes={})
    for name, ents, mats, (eye, at, fov), RC in RB.scenes(B):
        ctx = B.Context(0)  # raises without a gfx950 device
        ctx.upload_scene(ents, mats, env=B.make_env(color=(1, 1, 1), intensity=1.0))
        cam = RC.look(eye, at, [0.0, 1.0, 0.0], fov, W, H)
        prim = RB.primary_rays(cam, W, H)
        n = prim.shape[0]
        rec = dict(triangles=int(ctx.stats()["n_triangles"]), rays={})
        sets = dict(primary=prim, shuffled=prim[np.random.default_rng(21).permutation(n)])
        d_rays, d_hits, d_list = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p, b in ((d_rays, n * 32), (d_hits, n * 16), (d_list, n * 16 * max(KS))):
            AS._ok(hip.hipMalloc(C.byref(p), b), "hipMalloc")
        last = np.empty(n, B.HIT_DTYPE)
        for sname, rays in sets.items():
            AS.to_device(d_rays.value, B.make_rays(rays))
            calls = [("closest", lambda: ctx.trace_closest_device(d_rays.value, n, d_hits.value))]
            calls += [("K%d" % K, lambda K=K: ctx.trace_hits_device(d_rays.value, n, d_list.value, K)) for K in KS]
            ms = {c: [] for c, _ in calls}
            launch = {}
            for i in range(a.warmups + a.repeats):
                for call, fn in calls:
                    fn()
                    st = ctx.stats()
                    ms[call].append(st["kernel_ms"])
                    launch[call] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], grid=st["grid"])
            ctx.synchronize()
            srec = dict(rays=int(n))
            for call in ms:
                m = ms[call][a.warmups:]
                med = statistics.median(m)
                srec[call] = dict(grays_per_s=round(n / med * 1e-6, 3), kernel_ms=dict(median=med, min=min(m), max=max(m)), spread=round((max(m) - min(m)) / med, 4), launch=launch[call])
            for K in KS:
                srec["K%d" % K]["over_closest"] = round(srec["K%d" % K]["grays_per_s"] / srec["closest"]["grays_per_s"], 3)
                # the share of rays whose list is full: entry K - 1 of the strided read-back is a hit
                ctx.trace_hits_device(d_rays.value, n, d_list.value, K)
                ctx.synchronize()
                AS._ok(hip.hipMemcpy2D(last.ctypes.data_as(C.c_void_p), C.c_size_t(16), C.c_void_p(d_list.value + (K - 1) * 16), C.c_size_t(K * 16), C.c_size_t(16), C.c_size_t(n), C.c_int(AS.D2H)), "hipMemcpy2D")
                srec["K%d" % K]["full_share"] = round(float((last["prim"] >= 0).mean()), 4)
            rec["rays"][sname] = srec
            print(json.dumps({a.label: {name: {sname: srec}}}), flush=True)
        for p in (d_rays, d_hits, d_list):
            hip.hipFree(p)
        ctx.close()
        out["scenes"][name] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    a = ap.parse_args()

    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B

    cand = run(B, a)
    for path in ([PROFILE] if a.write else []) + ([a.out] if a.out else []):
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec.setdefault("candidates", {})[a.label] = cand
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
