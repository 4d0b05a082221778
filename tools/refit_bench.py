"""What pt_update_vertices costs and what keeping the topology costs: C2 (Cornell box) and the C4 stand-in, one MI355X.

    python tools/refit_bench.py [--write] [--scenes c2,c4] [--size 1920x1080] [--spp 64]

Per scene and wobble amplitude (0, 1, 5, 20 % of the scene's extent, every vertex moved by a smooth sine field):
  * update cost: pt_update_vertices - device milliseconds from the first refit kernel to the last (HIP events, pt_debug_update_info) and
    the wall time of the call - against the wall time of pt_upload_scene of the same moved scene in the same process (medians of 5 / 3);
  * frame cost: kernel_ms of a frame at --spp after the refit against after the fresh upload (medians of 3, one warm-up each): the
    price of the tree that was built for the uploaded positions.  The two frames are compared bit for bit while at it.
--write stores the record as profiles/r10_refit.json.  Measurement only: nothing here is asserted by the test suite.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
AMPLITUDES = (0.0, 0.01, 0.05, 0.2)
DEPTH = 16


def workloads(names):
    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B, procedural, scene_io

    out = {}
    if "c2" in names:
        sc = scene_io.load_scene_dir(os.path.join(ROOT, "assets"), "cornell-box")
        c = sc["camera"]
        out["c2_cornell-box"] = (sc["entities"], [m for _, m, _ in sc["materials"]], lambda W, H: B.to_camera_data(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"], W, H))
    if "c4" in names:
        _, mats = scene_io.parse_scene(os.path.join(ROOT, "assets", "dragon.json"))
        ents = scene_io.build_entities(procedural.dragon_standin(), mats)
        out["c4_dragon_standin"] = (ents, [m for _, m, _ in mats], lambda W, H: B.to_camera_data([4.0, 2.5, 0.0], [0.0, 0.75, 0.0], [0.0, 1.0, 0.0], 50.0, W, H))
    return B, out


def wobble(entities, amp):
    """Every vertex moved by amp x extent x a smooth sine field of its position (float64, rounded to float32)."""
    P = np.concatenate([m["vertices"] for m, _ in entities]).astype(np.float64)
    ext = float((P.max(0) - P.min(0)).max())
    out = []
    for m, _ in entities:
        v = m["vertices"].astype(np.float64)
        out.append(dict(m, vertices=(v + amp * ext * np.sin(v[:, [1, 2, 0]] * (6.0 / ext) + np.arange(3))).astype(np.float32)))
    return out


def frame_ms(ctx, cam, W, H, spp, repeats=3):
    ctx.render(cam, W, H, spp, DEPTH)  # warm-up: buffers, pixel queue
    ms, rgb = [], None
    for _ in range(repeats):
        rgb, _ = ctx.render(cam, W, H, spp, DEPTH)
        ms.append(ctx.stats()["kernel_ms"])
    return float(np.median(ms)), rgb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--scenes", default="c2,c4")
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--spp", type=int, default=64)
    args = ap.parse_args()
    W, H = (int(x) for x in args.size.split("x"))
    B, loads = workloads(args.scenes.split(","))
    env = B.make_env(color=(1, 1, 1), intensity=0.0)
    doc = {"what": "pt_update_vertices (on-device refit, topology kept) against pt_upload_scene (rebuild) of the same moved scene; frames %dx%d at %d spp, depth %d" % (W, H, args.spp, DEPTH),
           "scenes": {}}
    for name, (ents, mats, make_cam) in loads.items():
        cam = make_cam(W, H)
        dyn = B.Context(0)
        dyn.set_option("dynamic", 1)
        t0 = time.perf_counter()
        dyn.upload_scene(ents, mats, env=env)
        rec = {"triangles": int(dyn.stats()["n_triangles"]), "bvh_depth": int(dyn.stats()["bvh_depth"]), "upload_dynamic_ms": round((time.perf_counter() - t0) * 1e3, 2), "by_amplitude": {}}
        for amp in AMPLITUDES:
            mv = wobble(ents, amp)
            wall, dev = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                dyn.update_vertices([dict(vertices=m["vertices"]) for m in mv])  # vertices only: the normals stay
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(dyn.update_info()["device_ms"])
            info = dyn.update_info()
            refit_frame, rgb_refit = frame_ms(dyn, cam, W, H, args.spp)
            up = []
            fresh = None
            for _ in range(3):
                if fresh is not None:
                    fresh.close()
                fresh = B.Context(0)
                t0 = time.perf_counter()
                fresh.upload_scene([(m, mid) for m, (_, mid) in zip(mv, ents)], mats, env=env)
                up.append((time.perf_counter() - t0) * 1e3)
            fresh_frame, rgb_fresh = frame_ms(fresh, cam, W, H, args.spp)
            fresh.close()
            r = {"update_device_ms": round(float(np.median(dev)), 3), "update_wall_ms": round(float(np.median(wall)), 3), "upload_wall_ms": round(float(np.median(up)), 2),
                 "h2d_bytes": info["h2d_bytes"], "levels": info["levels"], "frame_ms_after_refit": round(refit_frame, 3), "frame_ms_after_fresh_upload": round(fresh_frame, 3),
                 "frame_cost_of_kept_topology": round(refit_frame / fresh_frame, 3), "frames_bit_identical": bool((rgb_refit.view(np.uint32) == rgb_fresh.view(np.uint32)).all())}
            rec["by_amplitude"]["%g" % amp] = r
            print(name, "amplitude %g:" % amp, json.dumps(r), flush=True)
        dyn.close()
        doc["scenes"][name] = rec
    if args.write:
        with open(os.path.join(ROOT, "profiles", "r10_refit.json"), "w") as fh:
            json.dump(doc, fh, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
