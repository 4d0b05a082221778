"""What the children of tests/test_gpu_batch_guides.py run behind the counting stub collective (in the manner of tests/aov_follow_child.py):

  python batch_guides_child.py rank OUT_DIR RANK WORLD    one process per rank on device 0: pt_comm_init_rank, then pt_render_aov_batch of CASE
                                                          with option "batch_frames" = BATCH_FRAMES; rank 0 receives the buffers, the others
                                                          pass NULL; every rank saves how many reduces the call issued

The parent renders the same batch with one plain context and compares bit for bit; it expects one reduce per launch sequence."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = ("mirror_wall", 40, 32, 2, 4, 0.3)  # 3 x 2 tiles of 16: both ranks of a world of two own some in every frame
BATCH_FRAMES = 2                           # the three frames of the scene: two launch sequences


def setup():
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ptamd

    ptamd.load()
    import batch_guides_common as BG
    from owl_path_tracer_amd.pyhost import binding as B

    name, W, H, n, k, r = CASE
    return BG, B, BG.scene(name), BG.frames(name, W, H, B), W, H, BG.params(B, n, k, r)


def mode_rank(out, rank, world):
    rank, world = int(rank), int(world)
    BG, B, sc, frames, W, H, prm = setup()
    counter = ctypes.CDLL(os.environ["PT_RCCL_PATH"])
    ctx = B.Context(0)
    BG.upload(ctx, sc, B)
    ctx.set_option("batch_frames", BATCH_FRAMES)
    idf = os.path.join(out, "comm_id.bin")
    if rank == 0:
        with open(idf + ".tmp", "wb") as f:
            f.write(B.comm_unique_id())
        os.replace(idf + ".tmp", idf)
    else:
        t0 = time.time()
        while not os.path.exists(idf):
            if time.time() - t0 > 120:
                raise SystemExit("no communicator id from rank 0")
            time.sleep(0.05)
    ctx.comm_init_rank(open(idf, "rb").read(), rank, world)
    before = counter.count_rccl_reduces()
    got = ctx.render_aov_batch(frames, W, H, prm, receive=rank == 0)
    reduces = counter.count_rccl_reduces() - before
    launches = ctx.stats()["launches"]
    if rank == 0:
        np.save(os.path.join(out, "rank0.npy"), got)
    with open(os.path.join(out, "reduces_%d.json" % rank), "w") as f:
        json.dump(dict(reduces=reduces, launches=launches), f)
    ctx.comm_destroy()
    ctx.close()


if __name__ == "__main__":
    os.makedirs(sys.argv[2], exist_ok=True)
    {"rank": mode_rank}[sys.argv[1]](*sys.argv[2:])
