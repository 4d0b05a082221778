"""How long a frame runs against the host time of enqueueing it: the figures behind SPP_A of tests/test_gpu_async.py, one MI355X.

    PT_LIB_PATH=<library of the commit to measure> python tools/async_measure.py [--out FILE]

Cornell box of tests/refit_common.py, depth 16, views 48 x 40, 96 x 80 and 17 x 5:
  * kernel_ms (pt_get_stats) of the blocking pt_render at 8 / 64 / 256 / 1024 spp, three frames each after one warm-up;
  * the host time of pt_render_device on a caller stream (perf_counter around the call) and hipStreamQuery of that stream right after
    it, six calls each with a pt_synchronize between them;
  * the oracle's time for the candidate frames with 16 threads.
Prints one JSON record (--out: also writes it).  profiles/r13_async.json holds the record of the parent of the commit that added the
ordering, with the choice made from it and what tests/test_gpu_async.py reported; measurement only, nothing here is asserted.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
DEPTH = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    import ptamd

    ptamd.load()
    import async_common as A
    import oracle as orc
    import refit_common as RC
    from owl_path_tracer_amd.pyhost import binding as B, scene_io

    out = {"library": os.environ.get("PT_LIB_PATH", B.LIB_PATH)}
    scene = RC.make_scene("cornell")
    materials = RC.cornell_materials()
    ctx = B.Context(0)
    RC.upload(ctx, scene, materials=[m for _, m, _ in materials], env=B.make_env(**RC.CORNELL_ENV))
    out["kernel_ms_blocking_pt_render"] = {}
    for W, H in ((48, 40), (96, 80), (17, 5)):
        cam = RC.cornell_camera(W, H, B.to_camera_data)
        ctx.render(cam, W, H, 64, DEPTH)
        for spp in (8, 64, 256, 1024):
            ms = []
            for _ in range(3):
                ctx.render(cam, W, H, spp, DEPTH)
                ms.append(round(ctx.stats()["kernel_ms"], 3))
            out["kernel_ms_blocking_pt_render"]["%dx%d@%d" % (W, H, spp)] = ms
    s = A.stream(0)
    out["enqueue_ms_pt_render_device_on_a_caller_stream"] = {}
    for W, H, spp in ((48, 40, 64), (48, 40, 256), (48, 40, 1024), (17, 5, 1024)):
        cam = RC.cornell_camera(W, H, B.to_camera_data)
        f = A.DeviceFrame(W, H)
        host_ms, queries = [], []
        for _ in range(6):
            t0 = time.perf_counter()
            ctx.render_device(cam, W, H, spp, DEPTH, f.rgb, f.rgba8, stream=s)
            t1 = time.perf_counter()
            queries.append(A.query(s))
            ctx.synchronize()
            host_ms.append(round((t1 - t0) * 1e3, 3))
        f.free()
        out["enqueue_ms_pt_render_device_on_a_caller_stream"]["%dx%d@%d" % (W, H, spp)] = dict(host_ms=host_ms, hipStreamQuery_right_after=queries)
    ctx.close()
    A.destroy_streams()
    S = orc.Scene(scene_io.flatten_scene(scene[0], materials))
    out["oracle_seconds_16_threads"] = {}
    for W, H, spp in ((48, 40, 256), (48, 40, 1024), (96, 80, 256)):
        t0 = time.perf_counter()
        S.render(RC.cornell_camera(W, H, orc.to_camera_data), orc.make_env(**RC.CORNELL_ENV), W, H, spp, DEPTH, threads=16)
        out["oracle_seconds_16_threads"]["%dx%d@%d" % (W, H, spp)] = round(time.perf_counter() - t0, 3)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
