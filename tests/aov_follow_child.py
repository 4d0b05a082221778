"""What the children of tests/test_gpu_aov_follow.py run behind the stub collective (as tests/aov_child.py for the first-hit pass):

  python aov_follow_child.py group OUT_DIR DEVICES      one process, a B.Group over DEVICES (e.g. 0,0): pt_group_render_aov_follow of CASE
  python aov_follow_child.py rank OUT_DIR RANK WORLD    one process per rank on device 0: pt_comm_init_rank, pt_render_aov_follow; rank 0
                                                        receives the buffers, the others pass NULL; every rank saves how many reduces
                                                        the call issued

The parent renders the same case with one plain context and compares bit for bit."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = ("mirror_wall", 40, 32, 2, 4, 0.3)  # 3 x 2 tiles of 16: both ranks of a world of two own some


def setup():
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ptamd

    ptamd.load()
    import aov_follow_common as FC
    from owl_path_tracer_amd.pyhost import binding as B

    name, W, H, n, k, r = CASE
    sc = FC.scene(name)
    return FC, B, sc, FC.camera(sc, W, H, B.to_camera_data), W, H, FC.params(B, n, k, r)


def mode_group(out, devices):
    FC, B, sc, cam, W, H, prm = setup()
    g = B.Group([int(d) for d in devices.split(",")])
    g.upload_scene(sc["ents"], sc["mats"], textures=sc["textures"], mesh_textures=sc["mesh_textures"], env=B.make_env(**sc["env"]))
    for wt in (0, 1):
        g.set_option("watertight", wt)
        np.save(os.path.join(out, "group_wt%d.npy" % wt), g.render_aov_follow(cam, W, H, prm))
    size = g.size
    g.close()
    with open(os.path.join(out, "group.json"), "w") as f:
        json.dump(dict(size=size), f)


def mode_rank(out, rank, world):
    rank, world = int(rank), int(world)
    FC, B, sc, cam, W, H, prm = setup()
    counter = ctypes.CDLL(os.environ["PT_RCCL_PATH"])
    ctx = B.Context(0)
    FC.upload(ctx, sc, B)
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
    got = ctx.render_aov_follow(cam, W, H, prm, receive=rank == 0)
    reduces = counter.count_rccl_reduces() - before
    if rank == 0:
        np.save(os.path.join(out, "rank0.npy"), got)
    with open(os.path.join(out, "reduces_%d.json" % rank), "w") as f:
        json.dump(dict(reduces=reduces), f)
    ctx.comm_destroy()
    ctx.close()


if __name__ == "__main__":
    os.makedirs(sys.argv[2], exist_ok=True)
    {"group": mode_group, "rank": mode_rank}[sys.argv[1]](*sys.argv[2:])
