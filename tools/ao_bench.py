"""What fusing buys ambient occlusion: pt_trace_ao_device against the composition it replaces, on one MI355X.

    python tools/ao_bench.py [--write] [--out FILE] [--size 1920x1080] [--repeats 20] [--warmups 3] [--k 4,16,64]

Scenes and rays are those of tools/rays_bench.py: the C4 stand-in and the 3 x 3 x 3 block of icospheres, the rays of a --size camera
through the pixel centres in pixel order, all in device buffers, tmax = +inf; K occlusion rays per hit about the geometric normal,
radius +inf, seed 0.
Two things are timed, ALTERNATING in one run (fused, composed, fused, ...) so that both see the same clocks and caches:
  fused     pt_trace_ao_device: one launch;
  composed  what a caller does without it: pt_trace_surface_device over the primary rays, then pt_trace_occluded_device over the K
            occlusion rays of every hit - the very rays of the fused call, made beforehand by the CPU twin (pt_debug_trace_ao_host) and
            already in HBM.  Making the rays is NOT timed, nor the hit compaction a caller would need, so this is a lower bound.
Figures: kernel_ms of pt_stats (HIP events around the launch; for the composition the sum of its two launches), the median of --repeats
after --warmups, and the spread (max - min) / median; Grays/s counts 1 + K rays per hit and 1 per miss for both.  The fused call moves
32 bytes in and 32 out per primary ray; the composition moves 32 + 80 per primary ray and 32 * K + K per hit on top of the 32 * K bytes
somebody wrote.
--write merges the section into profiles/r26_ao.json; --out FILE into another file.  Measurement only: nothing here is asserted by the
test suite, and without a GPU it fails (there is no fallback)."""
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
PROFILE = os.path.join(ROOT, "profiles", "r26_ao.json")


def run(B, a):
    import async_common as AS
    import rays_bench as RB

    W, H = (int(x) for x in a.size.split("x"))
    ks = sorted(int(k) for k in a.k.split(","))
    hip = AS.hip()
    out = dict(size=[W, H], repeats=a.repeats, warmups=a.warmups, scenes={},
               unit="Grays/s (1 + K rays per hit, 1 per miss) from the median kernel_ms of pt_stats; fused and composed alternate in one run")
    for name, ents, mats, (eye, at, fov), RC in RB.scenes(B):
        ctx = B.Context(0)  # raises without a gfx950 device
        ctx.upload_scene(ents, mats, env=B.make_env(color=(1, 1, 1), intensity=1.0))
        cam = RC.look(eye, at, [0.0, 1.0, 0.0], fov, W, H)
        prim = B.make_rays(RB.primary_rays(cam, W, H))
        n = prim.shape[0]
        kmax = ks[-1]
        print("%s: the twin makes %d x %d occlusion rays" % (name, n, kmax), flush=True)
        twin, rays_kmax = ctx.trace_ao_host(prim, B.ao_default_params(n_rays=kmax), return_rays=True)
        hit = (twin["prim"] >= 0) & (twin["n"] != 0).any(1)
        n_hit = int(hit.sum())
        rays_hit = rays_kmax[hit]  # (n_hit, kmax): the stream is the same at every K, so the first K of a ray are its rays at n_rays = K
        del rays_kmax
        rec = dict(triangles=int(ctx.stats()["n_triangles"]), primary_rays=int(n), primary_hits=n_hit, k={})
        d_rays, d_ao, d_surf, d_occ_rays, d_occ = (C.c_void_p() for _ in range(5))
        for p, b in ((d_rays, n * 32), (d_ao, n * 32), (d_surf, n * 80), (d_occ_rays, max(n_hit * kmax * 32, 16)), (d_occ, max(n_hit * kmax, 16))):
            AS._ok(hip.hipMalloc(C.byref(p), b), "hipMalloc")
        AS.to_device(d_rays.value, prim)
        for K in ks:
            prm = B.ao_default_params(n_rays=K)
            occ_rays = np.ascontiguousarray(rays_hit[:, :K]).reshape(-1)
            AS.to_device(d_occ_rays.value, occ_rays)
            total = n + n_hit * K
            ms = dict(fused=[], composed=[])
            launch = {}
            for i in range(a.warmups + a.repeats):
                ctx.trace_ao_device(d_rays.value, n, d_ao.value, prm)
                st = ctx.stats()
                ms["fused"].append(st["kernel_ms"])
                launch["fused"] = dict(vgprs=st["vgprs"], lds_bytes=st["lds_bytes"], block=st["block"], grid=st["grid"], stack_entries=st["stack_entries"])
                ctx.trace_surface_device(d_rays.value, n, d_surf.value)
                t = ctx.stats()["kernel_ms"]
                ctx.trace_occluded_device(d_occ_rays.value, n_hit * K, d_occ.value)
                ms["composed"].append(t + ctx.stats()["kernel_ms"])
            ctx.synchronize()
            if K == ks[0]:  # the two count the same rays: checked once, outside the timing
                got = np.empty(n, B.AO_DTYPE)
                occ = np.empty(n_hit * K, np.uint8)
                AS._ok(hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_ao, got.nbytes, AS.D2H), "hipMemcpy")
                AS._ok(hip.hipMemcpy(occ.ctypes.data_as(C.c_void_p), d_occ, occ.nbytes, AS.D2H), "hipMemcpy")
                clear = np.rint(got["ao"][hit].astype(np.float64) * K).astype(np.int64)
                rec["fused_equals_composed_at_k%d" % K] = bool(((occ.reshape(n_hit, K) == 0).sum(1) == clear).all())
            krec = dict(rays=int(total))
            for call in ms:
                m = ms[call][a.warmups:]
                med = statistics.median(m)
                krec[call] = dict(grays_per_s=round(total / med * 1e-6, 3), kernel_ms=dict(median=med, min=min(m), max=max(m)), spread=round((max(m) - min(m)) / med, 4))
            krec["fused"]["launch"] = launch["fused"]
            krec["fused_over_composed"] = round(krec["fused"]["grays_per_s"] / krec["composed"]["grays_per_s"], 3)
            rec["k"][str(K)] = krec
            print(json.dumps({name: {"K=%d" % K: krec}}), flush=True)
        for p in (d_rays, d_ao, d_surf, d_occ_rays, d_occ):
            hip.hipFree(p)
        ctx.close()
        out["scenes"][name] = rec
    return dict(ao=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmups", type=int, default=3)
    ap.add_argument("--k", default="4,16,64")
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
