"""The child of tests/test_gpu_sequences.py::test_sequences_over_a_group: `python tests/seq_group_child.py OUT_DIR DEVICES SEED...`.  A
pt_group over DEVICES (pt_comm.cpp resolves PT_RCCL_PATH once per process, hence the child) runs the group projection of every
sequence (tests/seq_common.py: option "watertight" = 1, uploads, updates, tables, single frames, guide passes; a seed from
seq_common.GSEED0 on is one of the second family: follow passes, and pt_denoise on rank 0's context of the group's frame and guides) and
leaves every observation in OUT_DIR as seed_step_rgb.npy / seed_step_rgba8.npy, then done.json."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_dir, devices, seeds):
    import ptamd

    ptamd.load()
    import seq_common as SC
    from owl_path_tracer_amd.pyhost import binding as B

    os.makedirs(out_dir, exist_ok=True)
    done = {}
    for seed in seeds:
        g = B.Group([int(d) for d in devices.split(",")])
        try:
            obs = SC.run_plain(g, SC.group_projection(SC.draw_guide_sequence(seed) if seed >= SC.GSEED0 else SC.draw_sequence(seed)))
            size = g.size
        finally:
            g.close()
        for i, f, f8 in obs:
            np.save(os.path.join(out_dir, "%d_%d_rgb.npy" % (seed, i)), f)
            if f8 is not None:
                np.save(os.path.join(out_dir, "%d_%d_rgba8.npy" % (seed, i)), f8)
        done[str(seed)] = dict(size=size, steps=[i for i, _, _ in obs])
    with open(os.path.join(out_dir, "done.json.tmp"), "w") as f:
        json.dump(done, f)
    os.replace(os.path.join(out_dir, "done.json.tmp"), os.path.join(out_dir, "done.json"))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], [int(x) for x in sys.argv[3:]])
