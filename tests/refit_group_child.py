"""The child of tests/test_gpu_refit.py::test_group_update: `python tests/refit_group_child.py OUT_DIR DEVICES K W H SPP DEPTH`.  A
pt_group over DEVICES (pt_comm.cpp resolves PT_RCCL_PATH once per process, hence the child) uploads the Cornell scene of
tests/refit_common.py with option "dynamic" = 1, renders, updates every replica with movement K through pt_group_update_vertices,
renders again.  Frames go to OUT_DIR as .npy files, the ranks' update figures to info.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_dir, devices, k, W, H, spp, depth):
    import ptamd

    ptamd.load()
    import refit_common as RC
    from owl_path_tracer_amd.pyhost import binding as B

    os.makedirs(out_dir, exist_ok=True)
    scene = RC.make_scene("cornell")
    mats = [m for _, m, _ in RC.cornell_materials()]
    g = B.Group([int(d) for d in devices.split(",")])
    g.set_option("dynamic", 1)
    g.upload_scene(scene[0], mats, env=B.make_env(**RC.CORNELL_ENV))
    cam = RC.cornell_camera(W, H, B.to_camera_data)
    rgb, rgba8 = g.render(cam, W, H, spp, depth, want_rgba8=True)
    np.save(os.path.join(out_dir, "before_rgb.npy"), rgb)
    g.update_vertices(RC.moved(scene, k))
    rgb, rgba8 = g.render(cam, W, H, spp, depth, want_rgba8=True)
    np.save(os.path.join(out_dir, "after_rgb.npy"), rgb)
    np.save(os.path.join(out_dir, "after_rgba8.npy"), rgba8)
    info = dict(size=g.size, ranks=[{k_: float(v) for k_, v in g.ctx(i).update_info().items()} for i in range(g.size)])
    g.close()
    with open(os.path.join(out_dir, "info.json.tmp"), "w") as f:
        json.dump(info, f)
    os.replace(os.path.join(out_dir, "info.json.tmp"), os.path.join(out_dir, "info.json"))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], *[int(x) for x in sys.argv[3:8]])
