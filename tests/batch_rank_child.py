"""One rank of tests/test_gpu_batch.py::test_batch_reduce_with_stub_collective: `python batch_rank_child.py RANK WORLD DIR`.  Every
rank opens device 0, joins the communicator (the 128-byte id travels through a file), and renders the same batch twice through
pt_render_batch - as one launch sequence and, with batch_frames = 2, as two.  Rank 0 saves the frames it received; every rank saves how
many reduces each batch issued (count_rccl_reduces of tests/stub/count_rccl.cpp, which PT_RCCL_PATH names).  Imported by the test for
the batch itself (frames_of), so that parent and children render the same frames."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 120, 72, 40, 16


def frames_of(sc):
    """Three frames of the cornell box: the scene's camera and two more, the sphere's metallic / roughness changed per frame."""
    from owl_path_tracer_amd.pyhost import binding as B

    base = np.stack([m for _, m, _ in sc["materials"]]).astype(np.float32)
    c = sc["camera"]
    views = [(c["look_from"], c["look_at"], c["look_up"], c["vertical_fov"]), ([2.6, 1.6, 0.9], [0.0, 0.9, 0.0], [0, 1, 0], 55), ([2.2, 0.6, -1.1], [0.0, 1.0, 0.1], [0, 1, 0], 62)]
    frames = []
    for k, v in enumerate(views):
        m = base.copy()
        m[1, 4] = 0.5 * k  # metallic
        m[1, 7] = 0.2 + 0.3 * k  # roughness
        frames.append((B.to_camera_data(*v, W, H), m))
    return frames


def main():
    sys.path.insert(0, ROOT)
    import ptamd

    ptamd.load()
    from owl_path_tracer_amd.pyhost import binding as B, scene_io

    rank, world, tmp = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    counter = ctypes.CDLL(os.environ["PT_RCCL_PATH"])  # the object the library loads: one counter per process
    sc = scene_io.load_scene_dir(os.path.join(ROOT, "assets"), "cornell-box")
    ctx = B.Context(0)
    ctx.upload_scene(sc["entities"], [m for _, m, _ in sc["materials"]], env=B.make_env(color=(1, 1, 1), intensity=0.0))
    idf = os.path.join(tmp, "comm_id.bin")
    if rank == 0:
        uid = B.comm_unique_id()
        with open(idf + ".tmp", "wb") as f:
            f.write(uid)
        os.replace(idf + ".tmp", idf)
    else:
        t0 = time.time()
        while not os.path.exists(idf):
            if time.time() - t0 > 120:
                raise SystemExit("no communicator id from rank 0")
            time.sleep(0.05)
        uid = open(idf, "rb").read()
    ctx.comm_init_rank(uid, rank, world)
    frames = frames_of(sc)
    reduces = {}
    for tag, cap in (("one", 0), ("cut", 2)):
        ctx.set_option("batch_frames", cap)
        before = counter.count_rccl_reduces()
        # the root asks for the RGBA8 frames, the other ranks pass no buffers at all
        rgb, rgba8 = ctx.render_batch(frames, W, H, SPP, DEPTH, want_rgba8=True, receive=rank == 0)
        reduces[tag] = counter.count_rccl_reduces() - before
        if rank == 0:
            np.save(os.path.join(tmp, "rgb_%s.npy" % tag), rgb)
            np.save(os.path.join(tmp, "rgba8_%s.npy" % tag), rgba8)
    with open(os.path.join(tmp, "reduces_%d.json" % rank), "w") as f:
        json.dump(reduces, f)
    ctx.comm_destroy()
    ctx.close()


if __name__ == "__main__":
    main()
