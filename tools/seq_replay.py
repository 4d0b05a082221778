"""Print a seed's call sequence (tests/seq_common.py), and run it: `python tools/seq_replay.py <seed> [--run [K]] [--host]`.  A seed from
seq_common.GSEED0 on is one of the second family (follow guides, batch guides, the denoiser), a seed from seq_common.ASEED0 on one of the
third (an accumulation in the middle of a context's life; model: tests/accum_seq_common.py).

Without --run: the upload and the steps in words (no GPU needed).  --run: the first K steps (all without K) on a fresh context with the
runner of tests/test_gpu_sequences.py, every observation compared with the oracle, each step printed as it starts; a difference ends
the run with the runner's message (seed, step, fresh-context verdict, call list).  --host: the host-only form on a device = -1 context,
as tests/test_sequences_host.py runs it.  Shortening K until the difference goes away finds the call that leaves the stale state."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ptamd
ptamd.load()
import oracle as orc
import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B

args = sys.argv[1:]
seed = int(args[0])
host = "--host" in args
family = "accum " if seed >= SC.ASEED0 else "guide " if seed >= SC.GSEED0 else ""
seq = {"accum ": SC.draw_accum_sequence, "guide ": SC.draw_guide_sequence, "": SC.draw_sequence}[family](seed, host_only=host)
print("%ssequence seed=%d: %d steps" % (family, seed, len(seq["steps"])))
print(SC.call_list(seq))
if "--run" in args:
    k = args.index("--run")
    upto = int(args[k + 1]) if k + 1 < len(args) and args[k + 1].isdigit() else None
    orc.lib()
    model = SC.Model(orc)
    A = None
    if not host:
        import async_common as A
    ctx = B.Context(-1 if host else 0)
    try:
        got = SC.run(ctx, seq, model, upto=upto, A=A, log=lambda s: print("step" + s, flush=True))
    finally:
        ctx.close()
    print("every observation of %d steps is the oracle's; %.2f s in the library, %.2f s in the oracle" % (len(seq["steps"][:upto]), SC.run.seconds, model.seconds))
