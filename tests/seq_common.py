"""Random call sequences on ONE context, held to the oracle call by call: the generator, the model and the runner shared by
tests/test_sequences_host.py (CPU), tests/test_gpu_sequences.py (GPU) and tools/seq_replay.py.

THE GENERATOR.  draw_sequence(seed) draws an initial upload and 8 to 12 steps from np.random.default_rng(seed) in a fixed order; the
draws do not depend on host_only, which only decides how the runner observes.  A SCENE is a lit room, open towards the camera (five
walls of n x n quads each, indexed, every wall with vertices of its own), with - in the scenes of 3 and 4 meshes - a smooth textured
icosphere and a small emitter inside, and always the finite sliver mesh of tests/refit_common.py last: 98 to 368 triangles.  Material 0
is the walls' (never textured: a new base colour shows in most pixels), the camera stands in front of the open side, inside the
closest-hit domain of DESIGN.md 2.1 (within 2.2 extents of the scene), and every environment has an intensity of at least 0.3, so no
frame is dark.  Steps come in BLOCKS, so that every change is looked at before the next one:
    [change, observe]            change = update_vertices | set_materials | set_environment | set_pixel_shard | set_option watertight |
                                 set_option box_exact | one scheduler knob of the fuzz's PATHS | (every fourth sequence) upload
    [refused call, observe]      refused = a batch with watertight = 1 | update_vertices with a wrong vertex count | kernel = 1 with
                                 watertight = 1 | render_aov with n_samples = 0; the kind is seed % 4; [set_option watertight 1, guide
                                 pass] goes in front where the refusal needs it
    [render, render_aov, render] the guide pass between two renders of one state: the second render repeats the first call
    [batch, render]              a batch with tables of its own, then a single frame with the context's table
    [observe]
A batch is only drawn while watertight is 0 ([set_option watertight 0, guide pass] goes in front otherwise); every watertight switch is
followed by a guide pass, whose depth channel shows the other test's t.  The first three independent frame
sizes of a sequence are small (9..16 x 6..10), large (56..72 x 40..56), small: a growth and a shrink of at least 4.6 x in pixels, even
between a batch of three small frames and one large frame; every other size is W in 8..72, H in 6..56.

THE MODEL.  A STATE is a dict that no step modifies in place (apply() returns a new one): the uploaded scene, the current meshes,
tables, environment, shard, watertight.  expected(state, step) is the oracle's output of an observing step: orc.Scene(flatten_scene(...),
watertight=...).render per frame, pixels of other ranks zeroed; a batch is the loop of single frames; guide buffers are
tests/aov_ref.py's.  Nothing the library returns reaches the model (the shard's pixel list is pt_shard_pixels, a host function of its
own, as in tests/test_gpu_fuzz.py).

THE RUNNER.  run(ctx, seq, model) executes the steps.  A blocking observation is compared at once; an asynchronous one leaves its frame
in a DeviceFrame allocated before the first step, the next step follows with nothing in between, and ONE pt_synchronize after the last
step precedes the read-back of all of them - the library's own ordering is what is under test.  Float frames are compared as uint32
bits (NaN equals NaN), RGBA8 by value.  After every update_vertices the four arrays are read back from HBM, and then the host copies
that this first read refits, and both are held to the box definition of refit_common (V from a fresh host-only upload of the model's
meshes), whichever builder made the tree.  On a mismatch -
never after an error return - a fresh context uploads the model's state and makes the same call once: the message says whether that
one agrees with the oracle (stale state from the sequence) or not (a single-call bug), and gives seed, step and the call list.

THE SECOND FAMILY.  draw_guide_sequence(seed) (seeds from GSEED0) draws 8 to 14 steps around the eight entry points of csrc/pt_guides.cpp -
pt_render_aov_follow, pt_render_aov_batch, pt_denoise, pt_denoise_batch and their _device forms - from the same _Gen and its change
blocks; its docstring lists the blocks.  The room always has its sphere, glass or metal in three scenes out of four, with roughnesses on
both sides of the drawn roughness_max.  The model of a follow pass is tests/aov_follow_ref.py with the state's table, environment and
triangle test, of a guide batch the loop of it with each frame's table, of a filter tests/denoise_ref.py of the MODEL's frame and guide
buffers (Model.inputs): nothing the library returned reaches it.  The runner gives a blocking filter those inputs; an asynchronous one
of a chain reads the caller buffers that the two asynchronous calls before it fill - three streams, no synchronize, the library's
ordering after the context's last asynchronous call is what makes that legal - and any other one reads the model's inputs, copied to HBM
before the first step.  A filter in place leaves its result in the frame it read, which is then checked through the result only.  A
buffer no call was to write (the RGBA8 image beside guide buffers or beside a filter without one, everything handed to a refused call)
must still hold its fill pattern at the end.  After every blocking call of the family pt_get_stats' launches are the header's: 1, L + 2,
the launch sequences of pt_debug_plan_batch under the current "batch_frames", and sequences * (L + 2).

THE THIRD FAMILY.  draw_accum_sequence(seed) (seeds from ASEED0) draws 10 to 16 steps around the fifteen entry points of the progressive
accumulation - pt_accum_begin / add / read / variance / denoise / reproject / end, pt_denoise_var, pt_upsample and their _device forms - in
the middle of a context's life: three accumulations (small, large, small), adds after a scene change or a scheduler knob, selecting adds,
reprojects with guides of the step before, [add, guides, accum_denoise, upsample] blocking or asynchronous on one stream, calls of the
other two families in between, refused calls; its docstring lists the blocks.  The accumulation is stateful, so its model is not a
function of (state, step): tests/accum_seq_common.py keeps it (AccumModel: the oracle continues every active pixel from its stored stream -
oracle.Scene.accumulate - in the state current at that add; accum_ref, accum_reproject_ref, denoise_var_ref, upsample_ref do the rest),
and run() hands the family's steps to its SeqRunner: blocking steps are compared at once with pt_debug_accum_state, pt_accum_read and
pt_accum_info_get, asynchronous ones after the one pt_synchronize together with the final state; on a host-only context every step of the
model is held through the library's CPU twins instead.
"""
import ctypes as C
import time

import numpy as np

import aov_follow_ref
import aov_ref
import denoise_ref
import ray_battery as rb
import refit_common as RC
from owl_path_tracer_amd.pyhost import binding as B, scene_io

F32 = np.float32
SEED0 = 20261018
N_DEFAULT = 12
SPP = (1, 7, 32, 40, 64, 96)
DEPTHS = (1, 4, 16)
SAMPLE_BUDGET = 200_000  # oracle samples per call (about a quarter of a second on 8 cores): spp steps down SPP until the call fits
SMALL, LARGE = ((9, 17), (6, 11)), ((56, 73), (40, 57))
RENDER_OPS = ("render", "render_device", "render_batch", "render_batch_device")
AOV_OPS = ("render_aov", "render_aov_device")
FOLLOW_OPS = ("render_aov_follow", "render_aov_follow_device")
AOV_BATCH_OPS = ("render_aov_batch", "render_aov_batch_device")
DENOISE_OPS = ("denoise", "denoise_device")
DENOISE_BATCH_OPS = ("denoise_batch", "denoise_batch_device")
FILTER_OPS = DENOISE_OPS + DENOISE_BATCH_OPS
GUIDE_OPS = FOLLOW_OPS + AOV_BATCH_OPS + FILTER_OPS  # the eight entry points of the second family (draw_guide_sequence)
OBSERVING = RENDER_OPS + AOV_OPS + GUIDE_OPS
ASYNC_OPS = ("render_device", "render_batch_device", "render_aov_device") + GUIDE_OPS[1::2]
BLOCKING_OF = {"render_device": "render", "render_batch_device": "render_batch", "render_aov_device": "render_aov", **{d: b for b, d in zip(GUIDE_OPS[0::2], GUIDE_OPS[1::2])}}
REFUSED = ("batch_watertight", "update_count", "kernel_watertight", "aov_zero_samples")
# the second family
GSEED0 = 20270102
GUIDE_BUDGET = 2_500   # guide samples per call of the numpy restatement (every round of it is a brute-force walk): n steps down until the call fits
GUIDE_SAMPLE_BUDGET = 50_000   # oracle samples per call in this family (SAMPLE_BUDGET's kind): its frames are the low-sample ones a filter is for
FILTER_BUDGET = 4_100  # pixels x iterations per call of the numpy filter (25 taps of a dozen float32-exact fma each): L steps down until the call fits
MAX_FOLLOW = (0, 1, 4, 8)
ROUGHNESS_MAX = (0.0, 0.3, 1.0)
GLASS_ROUGHNESS = (0.0, 0.05, 0.5)   # specular_transmission_roughness of a glass row
METAL_ROUGHNESS = (0.0, 0.25, 0.6)   # roughness of a metal row: both sets lie on both sides of roughness_max = 0.3
GUIDE_REFUSED = ("aov_batch_watertight", "follow_max_follow", "aov_batch_materials", "denoise_iterations", "denoise_nan_sigma", "denoise_batch_no_frames")
GUIDE_LOOKS_AT = ("update_vertices", "set_materials", "set_environment", "set_pixel_shard", "watertight")  # "<kind>!": that change, looked at by a guide pass
BETWEEN = ("render_aov_follow", "render_aov_batch", "denoise", "denoise_batch")
SIGMAS = dict(sigma_color=(1.0, 4.0, 16.0), sigma_normal=(0.1, 0.25, 1.0), sigma_depth=(0.05, 0.1, 0.5), sigma_albedo=(0.1, 0.2, 1.0))
CHANGES = ("update_vertices", "set_materials", "set_environment", "set_pixel_shard", "watertight", "upload")  # the kinds whose effect must show
# the third family
ASEED0 = 20271020
ACCUM_OPS = ("accum_begin", "accum_add", "accum_add_device", "accum_read", "accum_variance", "accum_denoise", "accum_denoise_device", "accum_reproject", "accum_reproject_device",
             "accum_end", "denoise_var", "denoise_var_device", "upsample", "upsample_device")
ACCUM_ASYNC = ("accum_add_device", "accum_denoise_device", "accum_reproject_device", "denoise_var_device", "upsample_device")
BLOCKING_OF_ACCUM = {d: d[:-7] for d in ACCUM_ASYNC}
ACCUM_SPP = (1, 5, 8, 16, 40, 64)
# oracle samples per add (GUIDE_SAMPLE_BUDGET's figure).  MEASURED with it: 0.15 to 0.5 s per default seed for the whole host-only test on the CPU
# (tests/test_sequences_host.py), of which 0.03 to 0.3 s are the oracle's and the restatements'; 0.06 to 0.19 s of oracle per seed in the GPU test
# (profiles/r20_accum_sequences.json), against 0.055 to 0.184 s for the second family's seeds in profiles/r18_guide_sequences.json
ACCUM_BUDGET = 50_000
ACCUM_SMALL, ACCUM_LARGE = ((9, 17), (6, 11)), ((32, 41), (24, 31))  # 54..160 and 768..1200 pixels: a growth and a shrink of 4.8 x at least
ACCUM_CHANGES = ("watertight", "update_vertices", "set_materials", "set_environment")
ACCUM_REFUSED = ("accum_bad_params", "accum_after_shard", "accum_after_upload", "accum_no_accum")
ACCUM_TAILS = (("read",), ("denoise_var", "end"), ("upsample", "variance"), (), ("variance",), ("other", "denoise_var_device"), ("end",), (), ("read",), ("denoise_var", "other"),
               ("denoise_var_device", "variance"), ())
# scheduler knobs of the fuzz (tests/test_gpu_fuzz.py PATHS): none may change an image, so the model ignores them
KNOB_KEYS = {"groups", "whole", "express_permille", "schedule", "chunk_spp", "fallback", "slots_per_wave", "blocks_per_cu", "prepass_spp", "cost_radius", "spp_per_launch",
             "chunk_tail_min", "sticky_pct", "ns_express", "tune0", "adaptive"}


def knobs():
    from test_gpu_fuzz import PATHS

    return [p for p in PATHS if p and all(k in KNOB_KEYS for k, _ in p)]


def default_seeds(n=N_DEFAULT):
    return [SEED0 + i for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _rgba8(rng, h, w):
    px = rng.integers(0, 256, (h, w, 3)).astype(np.uint32)
    return (px[..., 0] | (px[..., 1] << 8) | (px[..., 2] << 16) | (0xFF << 24)).astype(np.uint32)


def _room(n):
    """Five walls of the cube [-1, 1]^3 (the side z = +1 is open), n x n quads each, indexed, inward normals, texcoords over each wall."""
    g = np.linspace(-1.0, 1.0, n + 1)
    V, N, T, I = [], [], [], []
    for a, s in ((0, -1.0), (0, 1.0), (1, -1.0), (1, 1.0), (2, -1.0)):
        b, c = (a + 1) % 3, (a + 2) % 3
        base = len(V)
        for i in range(n + 1):
            for j in range(n + 1):
                p = np.zeros(3)
                p[a], p[b], p[c] = s, g[i], g[j]
                nr = np.zeros(3)
                nr[a] = -s
                V.append(p)
                N.append(nr)
                T.append((i / n, j / n))
        at = lambda i, j: base + i * (n + 1) + j
        for i in range(n):
            for j in range(n):
                I += [(at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1))]
    return np.asarray(V), np.asarray(N), np.asarray(T), np.asarray(I, np.int32)


def _sphere(sub, radius, centre):
    """A smooth icosphere as tests/aov_common.py's: the normal of a vertex is its direction, its texcoord a spherical map of it."""
    unit = rb.icosphere(sub).reshape(-1, 3).astype(np.float64)
    n = unit / np.linalg.norm(unit, axis=1, keepdims=True)
    tc = np.stack([np.arctan2(n[:, 2], n[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], 1)
    return unit * radius + np.asarray(centre), n, tc


def _mesh(v, n, tc, idx, scale, offset):
    v = (np.asarray(v, np.float64) * scale + offset).astype(F32)
    return dict(vertices=v, normals=np.asarray(n, F32), texcoords=np.asarray(tc, F32).reshape(-1, 2), indices=np.asarray(idx, np.int32).reshape(-1, 3))


def _draw_env(rng, mode=None):
    mode = int(rng.integers(0, 3)) if mode is None else mode
    if mode == 0:
        return dict(use_auto=True, intensity=float(rng.uniform(0.3, 2.0)))
    if mode == 1:
        return dict(color=tuple(float(x) for x in rng.uniform(0.1, 1.0, 3)), intensity=float(rng.uniform(0.3, 3.0)))
    return dict(use_map=True, intensity=float(rng.uniform(0.3, 2.0)), env_map=_rgba8(rng, int(rng.integers(2, 17)), int(rng.integers(2, 33))))


def _specular(rng, colour):
    """The sphere's material in the second family: glass or metal in three draws out of four, with a roughness on either side of roughness_max."""
    kind = int(rng.integers(0, 8))
    if kind < 3:
        return scene_io.material(base_color=colour, specular_transmission=1.0, ior=1.5, roughness=0.05, specular_transmission_roughness=float(rng.choice(GLASS_ROUGHNESS)))
    if kind < 6:
        return scene_io.material(base_color=colour, metallic=1.0, roughness=float(rng.choice(METAL_ROUGHNESS)))
    return scene_io.material(base_color=colour) if kind == 6 else scene_io.material(base_color=colour, clearcoat=1.0, clearcoat_gloss=0.8)


def _draw_upload(rng, guide=False):
    """guide: the room of the second family - the sphere is always there, and its material is _specular's."""
    scale = float(10.0 ** rng.uniform(-1.0, 1.5))
    offset = rng.uniform(-1.0, 1.0, 3) * scale * (0.0 if rng.random() < 0.3 else float(rng.uniform(0.0, 3.0)))
    n_mesh = int(rng.integers(3, 5)) if guide else int(rng.integers(2, 5))
    n = int(rng.integers(3, 5)) if n_mesh == 2 else int(rng.integers(2, 4))  # 5 * 2 * n^2 wall triangles
    ents = [(_mesh(*_room(n), scale, offset), 0)]
    mats = [scene_io.material(base_color=tuple(rng.uniform(0.3, 0.9, 3)), roughness=float(rng.uniform(0.2, 1.0)))]
    if n_mesh >= 3:
        sub = 2 if (n_mesh == 3 and n == 2 and rng.random() < 0.5) else 1  # 320 or 80 triangles
        radius = float(rng.uniform(0.35, 0.55))
        v, nr, tc = _sphere(sub, radius, (rng.uniform(-0.3, 0.3), -0.95 + radius, rng.uniform(-0.3, 0.3)))
        ents.append((_mesh(v, nr, tc, np.arange(v.shape[0]), scale, offset), 1))
        kind = 0 if guide else int(rng.integers(0, 4))
        colour = tuple(rng.uniform(0.2, 1.0, 3))
        mats.append(_specular(rng, colour) if guide else [scene_io.material(base_color=colour, specular_transmission=1.0, ior=1.5, roughness=0.05), scene_io.material(base_color=colour, metallic=1.0, roughness=0.25),
                     scene_io.material(base_color=colour), scene_io.material(base_color=colour, clearcoat=1.0, clearcoat_gloss=0.8)][kind])
    if n_mesh >= 4:
        v, nr, tc = _sphere(0, 0.15, (rng.uniform(-0.4, 0.4), 0.7, rng.uniform(-0.4, 0.4)))
        ents.append((_mesh(v, nr, tc, np.arange(v.shape[0]), scale, offset), 2))
        mats.append(scene_io.material(emission=float(rng.uniform(5.0, 15.0))))
    ents.append((RC._finite_sliver_mesh(0, 0.3 * scale, tuple(float(x) for x in offset + np.array([-0.5, -0.6, 0.3]) * scale)), len(mats)))
    mats.append(scene_io.MAT_DEFAULT.copy())
    texs = mesh_tex = tex_by_mat = None
    textured = rng.random() < 0.4
    tex = _rgba8(rng, int(rng.integers(1, 9)), int(rng.integers(1, 9)))
    if textured and n_mesh >= 3:  # on the sphere's material
        texs, mesh_tex, tex_by_mat = [tex], [0 if mid == 1 else -1 for _, mid in ents], {1: tex}
    env = _draw_env(rng, 2 if rng.random() < 1.0 / 3.0 else int(rng.integers(0, 2)))
    return dict(op="upload", ents=ents, n_mat=len(mats), shift=1, mats=np.stack(mats).astype(F32), env=env, texs=texs, mesh_tex=mesh_tex, tex_by_mat=tex_by_mat,
                builder=int(rng.integers(0, 3)), leaf=int(rng.choice([1, 4, 7])), scale=scale, centre=[float(x) for x in offset])


def _draw_camera(rng, st):
    s, c = st["scale"], np.asarray(st["centre"])
    frm = c + np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.4, 0.5), rng.uniform(1.7, 3.2)]) * s
    at = c + rng.uniform(-0.3, 0.3, 3) * s
    up = [float(rng.uniform(-0.2, 0.2)), 1.0, float(rng.uniform(-0.1, 0.1))]
    return [float(x) for x in frm], [float(x) for x in at], up, float(rng.uniform(35.0, 75.0))


def _draw_mats(rng, mats, guide=False):
    """Another table: the walls' base colour always changes, the other rows half of the time.  guide: a glass or metal row also gets another
    of its roughnesses, which moves it across roughness_max and back."""
    m = np.array(mats, F32)
    m[0, 0:3] = (m[0, [1, 2, 0]] * F32(0.5) + rng.uniform(0.05, 0.45, 3).astype(F32))
    for r in range(1, m.shape[0]):
        if rng.random() < 0.5:
            if m[r, 16] > 0:
                m[r, 16] = F32(rng.uniform(3.0, 20.0))
            else:
                m[r, 0:3] = rng.uniform(0.1, 1.0, 3).astype(F32)
                m[r, 7] = F32(rng.uniform(0.05, 1.0))
        if guide and m[r, 4] == 1:
            m[r, 7] = F32(rng.choice(METAL_ROUGHNESS))
        if guide and m[r, 14] == 1:
            m[r, 15] = F32(rng.choice(GLASS_ROUGHNESS))
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
_geo = [0]


def apply(st, step):
    """The state after a step (a new dict; st is left alone).  Observing and refused steps, box_exact and the scheduler knobs change nothing."""
    op = step["op"]
    if op == "upload":
        _geo[0] += 1
        return dict(scene=(step["ents"], step["n_mat"], step["shift"]), meshes=[m for m, _ in step["ents"]], mats=step["mats"], env=step["env"], texs=step["texs"],
                    mesh_tex=step["mesh_tex"], tex_by_mat=step["tex_by_mat"], shard=st["shard"] if st else None, wt=st["wt"] if st else 0, batch_frames=st.get("batch_frames", 0) if st else 0, geo=_geo[0],
                    scale=step["scale"], centre=step["centre"], builder=step["builder"], leaf=step["leaf"])
    if op == "update_vertices":
        mv = RC.moved(st["scene"], step["k"], with_normals=step["with_normals"])
        meshes = []
        for i, (old, new) in enumerate(zip(st["meshes"], mv)):
            if i == step["null_mesh"]:
                meshes.append(old)
            else:
                meshes.append(dict(old, vertices=new["vertices"], normals=new["normals"] if step["with_normals"] else old["normals"]))
        _geo[0] += 1
        return dict(st, meshes=meshes, geo=_geo[0])
    if op == "set_materials":
        return dict(st, mats=step["mats"])
    if op == "set_environment":
        return dict(st, env=step["env"])
    if op == "set_pixel_shard":
        return dict(st, shard=step["shard"])
    if op == "set_option" and step["key"] == "watertight":
        return dict(st, wt=int(step["value"]))
    if op == "set_option" and step["key"] == "batch_frames":  # (no image depends on it: only the launches that pt_get_stats counts)
        return dict(st, batch_frames=int(step["value"]))
    return st


def entities(st):
    return [(m, mid) for m, (_, mid) in zip(st["meshes"], st["scene"][0])]


def update_args(st, step):
    """The mesh list of Context.update_vertices for an update step in state st (the state BEFORE the step)."""
    mv = RC.moved(st["scene"], step["k"], with_normals=step["with_normals"])
    out = []
    for i, m in enumerate(mv):
        if i == step["null_mesh"]:
            out.append(None)
        else:
            out.append(dict(vertices=m["vertices"], normals=m["normals"]) if step["with_normals"] else dict(vertices=m["vertices"]))
    return out


def own_mask(st, W, H):
    """(H, W) bool in framebuffer order: the pixels the context owns."""
    if not st["shard"]:
        return np.ones((H, W), bool)
    rank, world, tile = st["shard"]
    own = np.zeros(W * H, bool)
    own[B.shard_pixels(W, H, tile, rank, world)] = True
    return own.reshape(H, W)[::-1]


class Model:
    """The oracle's side: one orc.Scene per geometry (rebuilt after an upload or an update), tables and the triangle test set per call."""

    def __init__(self, orc):
        self.orc = orc
        self._S = {}
        self._want = {}  # one sequence's outputs by (state, call): a filter asks for its render and guides again, and so does a repeated render
        self.seconds = 0.0

    def forget(self):
        """Before another sequence: the outputs kept for the last one go."""
        self._want.clear()

    def flat(self, st):
        return self.scene(st)[1]

    def scene(self, st):
        key = st["geo"]
        if key not in self._S:
            if len(self._S) > 4:
                self._S.clear()
            flat = scene_io.flatten_scene(entities(st), [("m%d" % i, m, "") for i, m in enumerate(st["mats"])], st["tex_by_mat"])
            self._S[key] = (self.orc.Scene(flat), flat)
        S, flat = self._S[key]
        S.set_watertight(bool(st["wt"]))
        return S, flat

    def _frame(self, st, cam, mats, W, H, spp, depth):
        orc = self.orc
        S, _ = self.scene(st)
        S.set_materials(np.asarray(mats, F32))
        want, want8, _ = S.render(orc.to_camera_data(tuple(cam[0]), tuple(cam[1]), tuple(cam[2]), cam[3], W, H), orc.make_env(**st["env"]), W, H, spp, depth, want_rgba8=True)
        own = own_mask(st, W, H)
        return np.where(own[..., None], want, F32(0.0)), np.where(own, want8, np.uint32(0))

    def expected(self, st, step):
        """(floats, RGBA8 or None) of an observing step in state st."""
        t0 = time.time()
        try:
            return self._expected(st, step)
        finally:
            self.seconds += time.time() - t0

    def inputs(self, st, step):
        """(rgb, guide buffers) of a filter step: the model's own outputs of the two calls the step names (step["src"])."""
        t0 = time.time()
        try:
            return self._expected(st, step["src"]["render"])[0], self._expected(st, step["src"]["guides"])[0]
        finally:
            self.seconds += time.time() - t0

    def _expected(self, st, step):
        key = (_state_key(st), _call_key(step))
        if key not in self._want:  # (run() and visibility() start with an empty cache: it holds one sequence's outputs)
            self._want[key] = self._compute(st, step)
            for a in self._want[key]:
                if a is not None:
                    a.flags.writeable = False  # shared among the steps that ask for it
        return self._want[key]

    def _follow(self, st, cam, mats, W, H, step):
        S, flat = self.scene(st)
        a = aov_follow_ref.aov(S, flat, st["env"], self.orc.to_camera_data(tuple(cam[0]), tuple(cam[1]), tuple(cam[2]), cam[3], W, H).as_array(), W, H, step["n"],
                               step["max_follow"], step["roughness_max"], materials=np.asarray(mats, F32))
        return np.where(own_mask(st, W, H)[..., None], a, F32(0.0))

    def _compute(self, st, step):
        op, W, H = step["op"], step["W"], step["H"]
        if op in ("render", "render_device"):
            return self._frame(st, step["cam"], st["mats"], W, H, step["spp"], step["depth"])
        if op in ("render_batch", "render_batch_device"):
            fr = [self._frame(st, cam, st["mats"] if mats is None else mats, W, H, step["spp"], step["depth"]) for cam, mats in step["frames"]]
            return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
        if op in FOLLOW_OPS:
            return self._follow(st, step["cam"], st["mats"], W, H, step), None
        if op in AOV_BATCH_OPS:  # the loop of the single-frame restatement with each frame's table
            return np.stack([self._follow(st, cam, st["mats"] if mats is None else mats, W, H, step) for cam, mats in step["frames"]]), None
        if op in FILTER_OPS:
            rgb, aov = self._expected(st, step["src"]["render"])[0], self._expected(st, step["src"]["guides"])[0]
            if op in DENOISE_OPS:
                out, out8 = denoise_ref.denoise(rgb, aov, **step["params"])
            else:
                fr = [denoise_ref.denoise(rgb[f], aov[f], **step["params"]) for f in range(rgb.shape[0])]
                out, out8 = np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
            return out, (out8 if step["want_rgba8"] else None)
        assert op in AOV_OPS, op
        S, flat = self.scene(st)
        cam = step["cam"]
        a = aov_ref.aov(S, flat, st["env"], self.orc.to_camera_data(tuple(cam[0]), tuple(cam[1]), tuple(cam[2]), cam[3], W, H).as_array(), W, H, step["n"], materials=st["mats"])
        return np.where(own_mask(st, W, H)[..., None], a, F32(0.0)), None


def _state_key(st):
    env = st["env"]
    return (st["geo"], st["wt"], tuple(st["shard"] or ()), np.asarray(st["mats"], F32).tobytes(),
            tuple(sorted((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in env.items())))


def _call_key(step):
    """What of a step the model's output depends on (not the form of the call, its stream or its buffers)."""
    op = BLOCKING_OF.get(step["op"], step["op"])
    key = (op, step["W"], step["H"], repr(step.get("cam")), step.get("spp"), step.get("depth"), step.get("n"), step.get("max_follow"), step.get("roughness_max"))
    if "frames" in step:
        key += tuple((repr(cam), None if mats is None else np.asarray(mats, F32).tobytes()) for cam, mats in step["frames"])
    if op in ("denoise", "denoise_batch"):
        key += (repr(sorted(step["params"].items())), step["want_rgba8"], _call_key(step["src"]["render"]), _call_key(step["src"]["guides"]))
    return key


def states_of(seq):
    """states[i] = the state BEFORE step i (states[len] = the final one)."""
    st = apply(None, seq["upload"])
    out = [st]
    for s in seq["steps"]:
        st = apply(st, s)
        out.append(st)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------
def draw_sequence(seed, host_only=False):
    rng = np.random.default_rng(seed)
    up = _draw_upload(rng)
    n = int(rng.integers(8, 13))
    mandatory = ["update_vertices", "refused"] + (["upload"] if seed % 4 == 1 else [])
    optional = ["update_vertices", "set_materials", "set_materials", "set_environment", "set_environment", "set_pixel_shard", "set_pixel_shard", "watertight", "box_exact", "knob",
                "aov_between", "batch_single", "observe"]
    worst = {"refused": 4, "aov_between": 3, "batch_single": 4, "observe": 1}  # steps; two for every other block (refused and batch_single may need a watertight switch in front)
    sized = {"batch_single": 2, "watertight": 0}                               # frames with a size of their own; one for every other block
    blocks, used, frames = list(mandatory), sum(worst.get(b, 2) for b in mandatory), sum(sized.get(b, 1) for b in mandatory)
    order = [optional[int(i)] for i in rng.permutation(len(optional))]
    for b, p in (("aov_between", 0.35), ("batch_single", 0.5)):  # the two long blocks seldom fit at the end of the list
        if rng.random() < p:
            order.remove(b)
            order.insert(0, b)
    for b in order:
        if used + worst.get(b, 2) + max(0, 3 - frames - sized.get(b, 1)) <= n:  # (room is kept for the three frames of growth and shrink)
            blocks.append(b)
            used += worst.get(b, 2)
            frames += sized.get(b, 1)
    blocks += ["render_only"] * max(0, 3 - frames)
    blocks = [blocks[int(i)] for i in rng.permutation(len(blocks))]
    G = _Gen(rng, seed, up)
    for b in blocks:
        G.block(b)
    while len(G.steps) < n:  # fill up: the bounds above are worst cases
        G.block(("set_environment", "set_materials")[int(rng.integers(0, 2))] if n - len(G.steps) >= 2 else "render_only")
    assert 8 <= len(G.steps) <= 12, len(G.steps)
    return dict(seed=seed, host_only=bool(host_only), upload=up, steps=G.steps)


class _Gen:
    def __init__(self, rng, seed, up):
        self.rng, self.seed, self.steps = rng, seed, []
        self.st = apply(None, up)
        self.sizes = 0  # independent frame sizes drawn so far: small, large, small, then anything
        self.k = 0
        self.knobs = knobs()

    def add(self, step):
        self.steps.append(step)
        self.st = apply(self.st, step)

    def size(self, counter="sizes"):
        rng = self.rng
        k = getattr(self, counter)
        (w0, w1), (h0, h1) = (SMALL, LARGE, SMALL)[k] if k < 3 else ((8, 73), (6, 57))
        setattr(self, counter, k + 1)
        return int(rng.integers(w0, w1)), int(rng.integers(h0, h1))

    def spp(self, W, H, K=1, budget=SAMPLE_BUDGET):
        """Depth 1 shows the environment and the emitters only: it is drawn for one frame in ten."""
        i = int(self.rng.integers(0, len(SPP)))
        while i > 0 and W * H * K * SPP[i] > budget:
            i -= 1
        return SPP[i], int(self.rng.choice(DEPTHS, p=(0.1, 0.4, 0.5)))

    def stream(self):
        return [None, 0, 1][int(self.rng.integers(0, 3))]

    def set_wt(self, v):
        """The switch, then a guide pass: its depth channel is the hit's t, which the other triangle test rounds differently in a fifth
        of the pixels or more, while a frame of flat diffuse walls often stays the same bit for bit."""
        self.add(dict(op="set_option", key="watertight", value=int(v)))
        self.aov()

    def render(self, allow_batch=True, allow_aov=True):
        """One observing step.  The first three are frames (they carry the growth and the shrink)."""
        rng = self.rng
        r = rng.random()
        if allow_aov and self.sizes >= 3 and r < 0.25:
            return self.aov()
        if allow_batch and self.st["wt"] == 0 and r > 0.75:
            return self.batch()
        W, H = self.size()
        spp, depth = self.spp(W, H)
        dev = rng.random() < 0.5
        self.add(dict(op="render_device" if dev else "render", cam=_draw_camera(rng, self.st), W=W, H=H, spp=spp, depth=depth, stream=self.stream() if dev else None))

    def aov(self):
        rng = self.rng
        W, H = int(rng.integers(8, 73)), int(rng.integers(6, 57))
        dev = rng.random() < 0.5
        self.add(dict(op="render_aov_device" if dev else "render_aov", cam=_draw_camera(rng, self.st), W=W, H=H, n=int(rng.integers(1, 4)), stream=self.stream() if dev else None))

    def batch(self):
        rng = self.rng
        if self.st["wt"]:
            self.set_wt(0)
        K = int(rng.integers(2, 4))
        W, H = self.size()
        spp, depth = self.spp(W, H, K)
        null = int(rng.integers(0, K))
        frames = [(_draw_camera(rng, self.st), None if f == null else _draw_mats(rng, self.st["mats"])) for f in range(K)]
        dev = rng.random() < 0.5
        self.add(dict(op="render_batch_device" if dev else "render_batch", frames=frames, W=W, H=H, spp=spp, depth=depth, stream=self.stream() if dev else None))

    def block(self, b):
        rng, st = self.rng, self.st
        if b == "observe":
            return self.render()
        if b == "render_only":
            return self.render(allow_batch=False)
        if b == "aov_between":
            self.render(allow_batch=False, allow_aov=False)
            first = self.steps[-1]
            self.add(dict(op="render_aov", cam=first["cam"], W=first["W"], H=first["H"], n=int(rng.integers(1, 4)), stream=None))
            return self.add(dict(first))
        if b == "batch_single":
            self.batch()
            return self.render(allow_batch=False, allow_aov=False)
        if b == "refused":
            what = REFUSED[self.seed % 4]
            if what in ("batch_watertight", "kernel_watertight") and not st["wt"]:
                self.set_wt(1)
            step = dict(op="refused", what=what)
            if what == "batch_watertight":
                step.update(frames=[(_draw_camera(rng, self.st), None), (_draw_camera(rng, self.st), _draw_mats(rng, self.st["mats"]))], W=16, H=12, spp=7, depth=4)
            elif what == "update_count":
                step.update(k=int(rng.integers(1, 7)), mesh=int(rng.integers(0, len(st["meshes"]))))
            elif what == "aov_zero_samples":
                step.update(cam=_draw_camera(rng, self.st), W=16, H=12)
            self.add(step)
            return self.render()
        if self.change(b):
            self.render()

    def change(self, b):
        """One change block's change; returns whether an observation is still due (the watertight switch brings its own)."""
        rng, st = self.rng, self.st
        if b == "update_vertices":
            self.k = self.k % 6 + 1 + int(rng.integers(0, 2))
            null = int(rng.integers(0, len(st["meshes"]))) if rng.random() < 0.4 else None
            if null == 0:
                null = len(st["meshes"]) - 1  # (the walls always move: they fill the frame)
            self.add(dict(op="update_vertices", k=self.k, with_normals=bool(rng.random() < 0.5), null_mesh=null))
        elif b == "set_materials":
            self.add(dict(op="set_materials", mats=_draw_mats(rng, st["mats"])))
        elif b == "set_environment":
            mode = int(rng.integers(0, 3))
            self.add(dict(op="set_environment", env=_draw_env(rng, mode)))
        elif b == "set_pixel_shard":
            world = int(rng.integers(2, 4))
            shard = (int(rng.integers(0, 2)), world, int(rng.choice([1, 8, 16])))
            self.add(dict(op="set_pixel_shard", shard=None if st["shard"] else shard))
        elif b == "watertight":
            self.set_wt(1 - st["wt"])
            return False
        elif b == "box_exact":
            self.add(dict(op="set_option", key="box_exact", value=int(rng.choice([0, 1]))))
        elif b == "knob":
            self.add(dict(op="knob", options=self.knobs[int(rng.integers(0, len(self.knobs)))]))
        elif b == "upload":
            self.k = 0
            self.add(_draw_upload(rng))
        else:
            raise KeyError(b)
        return True


# ---------------------------------------------------------------------------------------------------------------------
# the second family: follow guides, batch guides and the denoiser
# ---------------------------------------------------------------------------------------------------------------------
def default_guide_seeds(n=N_DEFAULT):
    return [GSEED0 + i for i in range(n)]


def draw_guide_sequence(seed, host_only=False):
    """8 to 14 steps around pt_render_aov_follow, pt_render_aov_batch, pt_denoise and pt_denoise_batch (blocking and _device forms) on the
    room of _draw_upload(guide=True).  A change (_Gen.change) or a refused call is looked at by the NEXT step, which is an observation of this
    family (_GuideGen.render) or the first step of one of these blocks, each step with a form and a stream of its own draw unless said otherwise:
        denoise_chain  [render, render_aov_follow of the same view, denoise of the two]: all blocking, or all asynchronous with nothing
                       between the calls - the filter reads the two caller buffers the steps before it fill
        batch_chain    [render_batch, render_aov_batch, denoise_batch] over the same frames, the same way
        between        [render, X, the same render again], X = BETWEEN[seed % 4]
        table_kept     [render_aov_batch with tables of its own, render_aov_follow with the context's table]
        refused        [one of GUIDE_REFUSED (seed % 6)]
        batch_frames   [option "batch_frames" = 1 or 2 (0 if it is set), a batch_chain or a guide batch]: the cut must not show
        filter         [denoise or denoise_batch] of a frame and guides that no call of the sequence made (the model's own)
    A block that needs watertight = 0 puts [set_option watertight 0, follow pass] in front.  The first three FILTERED sizes of a sequence are
    small, large, small (frames x W x H grows and shrinks by more than 4 x): the filter's records are reallocated when they grow.  Blocks
    are generated in a drawn order while they fit (their cost in the state they meet is known); room stays for the refused call and a
    denoise_chain, which every sequence has."""
    rng = np.random.default_rng(seed)
    up = _draw_upload(rng, guide=True)
    n = max(int(rng.integers(8, 15)), int(rng.integers(8, 15)))  # (the long blocks need room: mostly 11 and more)
    G = _GuideGen(rng, seed, up)
    # what a sequence is for goes by its seed, so that any twelve seeds in a row have all of it; the rest is drawn
    third = (seed // 4) % 3
    mandatory = ["refused", "denoise_chain"] + [["between"], ["batch_chain"], ["table_kept", "batch_frames"]][third] + (["filter", "filter"] if seed % 2 == 0 else []) + (["upload"] if seed % 4 == 1 else []) + [GUIDE_LOOKS_AT[seed % 5] + "!"]
    # THE SCHEDULE.  `order` lists block names; a name is generated when its turn comes if it still fits into the n steps.  G.cost(b) is what
    # b takes in the state it would meet (exact: a pending change costs one observation more, a batch behind watertight = 1 the switch
    # back).  `mandatory` are this seed's blocks: they are shuffled to the front with three others and fit before anything optional does.
    special = ["table_kept", "batch_frames", "denoise_chain", "batch_chain", "filter"]
    other = ["update_vertices", "set_materials", "set_environment", "set_pixel_shard", "watertight", "box_exact", "knob", "observe", "update_vertices", "set_environment", "set_pixel_shard"]
    special = [special[int(i)] for i in rng.permutation(len(special))]
    other = [other[int(i)] for i in rng.permutation(len(other))]
    head = mandatory + other[:3]
    order = [head[int(i)] for i in rng.permutation(len(head))] + other[3:5] + special[:1] + other[5:] + special[1:]
    left = list(mandatory)  # mandatory blocks whose turn has not come: an optional block must leave room for them
    # the two blocks EVERY sequence has are placed whatever came before, so their worst cases (a pending change to look at first, the
    # switch to watertight = 1 in front of the refused batch) are kept free from the start: 8 steps at most, and n >= 8
    hard = {"refused": 3 + 2 * (GUIDE_REFUSED[seed % 6] == "aov_batch_watertight"), "denoise_chain": 3}  # in every sequence: their worst cases stay free (8 steps at most)
    for b in order:
        due = b in left
        if due:
            left.remove(b)
        room = n - len(G.steps) - sum(hard[m] for m in left if m in hard)
        if due:  # this seed's own block: in if it fits beside the two reservations
            if b in hard or G.cost(b) <= room:
                G.block(b)
        # an optional block: beside the reservations, room must stay for the seed's blocks still to come, at their present cost - and a
        # switch to watertight = 1 makes each batch block among them dearer by the switch back (3 steps, once)
        elif G.cost(b) + sum(G.cost(m) for m in left if m not in hard) + (3 if b == "watertight" and not G.st["wt"] and {"batch_chain", "table_kept", "batch_frames"} & set(left) else 0) <= room:
            G.block(b)
    if G.pending:
        G.render()
    while len(G.steps) < n:  # fill up: the bounds above are worst cases
        if n - len(G.steps) >= 2 and rng.random() < 0.6:
            G.block(CHANGES[int(rng.integers(0, 4))])
        else:
            G.block("observe")
    assert 8 <= len(G.steps) <= 14 and not G.pending, len(G.steps)
    return dict(seed=seed, family="guide", host_only=bool(host_only), upload=up, steps=G.steps)


class _GuideGen(_Gen):
    def __init__(self, rng, seed, up):
        _Gen.__init__(self, rng, seed, up)
        self.filtered = 0  # filter sizes drawn so far: small, large, small, then anything
        self.bf = 0
        self.pending = False  # a change or a refused call that no step has looked at yet
        self.guide_only = False

    def add(self, step):
        _Gen.add(self, step)
        self.pending = step["op"] not in OBSERVING

    def cost(self, b):
        """The steps block b takes in the present state, the observation a change still needs included."""
        pend, wt = int(self.pending), self.st["wt"]
        wt0 = (2 + pend) if wt else 0  # [what is pending is looked at], the switch, its follow pass
        if b in ("denoise_chain", "filter", "observe"):
            return {"denoise_chain": 3, "filter": 1, "observe": 1}[b]
        if b in ("batch_chain", "table_kept"):
            return wt0 + {"batch_chain": 3, "table_kept": 2}[b]
        if b == "batch_frames":  # a change itself: what is pending is looked at first
            return 4 + (wt0 if wt else pend)
        if b == "between":
            return 3 + (wt0 if BETWEEN[self.seed % 4] == "render_aov_batch" else 0)
        if b == "refused":
            return 2 + pend + (2 if (GUIDE_REFUSED[self.seed % 6] == "aov_batch_watertight" and not wt) else 0)
        return 2 + pend  # a change and what looks at it

    def set_wt(self, v):
        if self.pending:
            self.follow()
        _Gen.set_wt(self, v)

    def form(self):
        """(asynchronous, stream)"""
        dev = bool(self.rng.random() < 0.5)
        return dev, (self.stream() if dev else None)

    def any_size(self):
        return int(self.rng.integers(8, 73)), int(self.rng.integers(6, 57))

    def spp(self, W, H, K=1, filtered=False):
        """A frame that is filtered has bounces: at depth 1 it shows the environment and the emitters only, and a filter leaves a flat frame as it is."""
        spp, depth = _Gen.spp(self, W, H, K, GUIDE_SAMPLE_BUDGET)
        return spp, (int(self.rng.choice(DEPTHS[1:])) if (filtered and depth == 1) else depth)

    def follow_params(self, W, H, K=1):
        rng = self.rng
        n = int(rng.integers(1, 4))
        while n > 1 and W * H * K * n > GUIDE_BUDGET:
            n -= 1
        return dict(n=n, max_follow=int(rng.choice(MAX_FOLLOW)), roughness_max=float(rng.choice(ROUGHNESS_MAX)))

    def filter_params(self, pixels):
        rng = self.rng
        L = int(rng.integers(1, 6))
        while L > 1 and pixels * L > FILTER_BUDGET:
            L -= 1
        p = dict(iterations=L, flags=int(rng.integers(0, 2)))
        for k, v in SIGMAS.items():
            p[k] = float(rng.choice(v))
        if rng.random() < 0.3:
            p[list(SIGMAS)[int(rng.integers(0, 4))]] = float("inf")
        return p

    def frames(self, K):
        rng = self.rng
        null = int(rng.integers(0, K))
        return [(_draw_camera(rng, self.st), None if f == null else _draw_mats(rng, self.st["mats"], guide=True)) for f in range(K)]

    # ---- single steps
    def frame(self, W, H, dev=None, stream=None, filtered=False):
        spp, depth = self.spp(W, H, filtered=filtered)
        if dev is None:
            dev, stream = self.form()
        self.add(dict(op="render_device" if dev else "render", cam=_draw_camera(self.rng, self.st), W=W, H=H, spp=spp, depth=depth, stream=stream))

    def follow(self, cam=None, size=None, form=None):
        W, H = size or self.any_size()
        dev, stream = form or self.form()
        self.add(dict(op=FOLLOW_OPS[dev], cam=cam or _draw_camera(self.rng, self.st), W=W, H=H, stream=stream, **self.follow_params(W, H)))

    aov = follow  # what _Gen.set_wt looks at the switch with: the depth channel is the path length, the sum of the hits' t

    def aov_batch(self, frames=None, size=None, form=None):
        if self.st["wt"]:
            self.set_wt(0)
        W, H = size or self.any_size()
        frames = frames or self.frames(int(self.rng.integers(2, 4)))
        dev, stream = form or self.form()
        self.add(dict(op=AOV_BATCH_OPS[dev], frames=frames, W=W, H=H, stream=stream, **self.follow_params(W, H, len(frames))))

    def filter(self, src=None, chain=False, form=None, batch=None):
        """A filter step.  src: (render step, guide step), the two steps before it (chain) - else a frame and guides of its own draw."""
        rng = self.rng
        if src is None:
            batch = bool(rng.random() < 0.4) if batch is None else batch
            W, H = self.size("filtered")
            if batch:
                frames = self.frames(int(rng.integers(2, 4)))
                spp, depth = self.spp(W, H, len(frames), filtered=True)
                src = (dict(op="render_batch", frames=frames, W=W, H=H, spp=spp, depth=depth, stream=None), dict(op="render_aov_batch", frames=frames, W=W, H=H, stream=None, **self.follow_params(W, H, len(frames))))
            else:
                cam = _draw_camera(rng, self.st)
                spp, depth = self.spp(W, H, filtered=True)
                src = (dict(op="render", cam=cam, W=W, H=H, spp=spp, depth=depth, stream=None), dict(op="render_aov_follow", cam=cam, W=W, H=H, stream=None, **self.follow_params(W, H)))
        batch = "frames" in src[0]
        dev, stream = form or self.form()
        self.add(dict(op=(DENOISE_BATCH_OPS if batch else DENOISE_OPS)[dev], W=src[0]["W"], H=src[0]["H"], K=len(src[0]["frames"]) if batch else 1, params=self.filter_params(src[0]["W"] * src[0]["H"] * (len(src[0]["frames"]) if batch else 1)),
                      in_place=bool(rng.random() < 0.5), want_rgba8=bool(rng.random() < 0.5), stream=stream, chain=chain, src=dict(render=src[0], guides=src[1])))

    def render(self, allow_batch=True, allow_aov=True):
        """One observing step of this family, which is what _Gen's change blocks look at their change with."""
        r = self.rng.random() * (0.8 if self.guide_only else 1.0)
        if r < 0.5 or not allow_aov:
            return self.follow() if allow_aov else self.frame(*self.any_size())
        if r < 0.8:
            return self.aov_batch() if (allow_batch and self.st["wt"] == 0) else self.follow()
        if r < 0.93:
            return self.frame(*self.any_size())
        return self.filter()

    # ---- blocks
    def chain(self, batch, K=None):
        """[render, guides, filter]: all blocking, or all asynchronous - each on a stream of its own draw, nothing in between."""
        rng = self.rng
        if batch and self.st["wt"]:
            self.set_wt(0)
        dev = bool(rng.random() < 0.5)
        form = lambda: (dev, self.stream() if dev else None)
        W, H = self.size("filtered")
        if batch:
            frames = self.frames(K or int(rng.integers(2, 4)))
            spp, depth = self.spp(W, H, len(frames), filtered=True)
            d, stream = form()
            self.add(dict(op="render_batch_device" if d else "render_batch", frames=frames, W=W, H=H, spp=spp, depth=depth, stream=stream))
            first = self.steps[-1]
            self.aov_batch(frames, (W, H), form())
        else:
            self.frame(W, H, *form(), filtered=True)
            first = self.steps[-1]
            self.follow(first["cam"], (W, H), form())
        self.filter((first, self.steps[-1]), chain=True, form=form())

    def block(self, b):
        rng, st = self.rng, self.st
        if b.endswith("!"):
            self.guide_only = True
            self.block(b[:-1])
            self.guide_only = False
            return
        if b == "observe":
            return self.render()
        if b == "filter":
            return self.filter()
        if b == "denoise_chain":
            return self.chain(False)
        if b == "batch_chain":
            return self.chain(True)
        if b == "between":
            x = BETWEEN[self.seed % 4]
            if x == "render_aov_batch" and st["wt"]:
                self.set_wt(0)
            self.frame(*self.any_size())
            first = self.steps[-1]
            if x == "render_aov_follow":
                self.follow(first["cam"], (first["W"], first["H"]))
            elif x == "render_aov_batch":
                self.aov_batch()
            else:
                self.filter(batch=(x == "denoise_batch"))
            return self.add(dict(first))
        if b == "table_kept":
            self.aov_batch()
            return self.follow()
        if st["wt"] and b == "batch_frames":
            self.set_wt(0)
        elif self.pending and b != "watertight":
            self.render()  # one change at a time
        if b == "batch_frames":
            self.bf = 0 if self.bf else (1 if rng.random() < 0.7 else 2)
            self.add(dict(op="set_option", key="batch_frames", value=self.bf))
            return self.chain(True, 3 if self.bf == 1 else None) if rng.random() < 0.8 else self.aov_batch()  # (one frame per launch sequence: three of them)
        if b == "refused":
            what = GUIDE_REFUSED[self.seed % 6]
            if what == "aov_batch_watertight" and not st["wt"]:
                self.set_wt(1)
            dev, stream = self.form()
            step = dict(op="refused", what=what, dev=dev, stream=stream, W=16, H=12)
            if what in ("aov_batch_watertight", "aov_batch_materials"):
                step.update(frames=self.frames(2))
            elif what == "follow_max_follow":
                step.update(cam=_draw_camera(rng, self.st))
            return self.add(step)
        if b == "upload":
            self.k = 0
            self.add(_draw_upload(rng, guide=True))
        elif b == "set_materials":
            self.add(dict(op="set_materials", mats=_draw_mats(rng, st["mats"], guide=True)))
        elif not self.change(b):
            return
        self.render()  # a change is looked at right away, mostly by a guide pass


# ---------------------------------------------------------------------------------------------------------------------
# the third family: one accumulation in the middle of a context's life
# ---------------------------------------------------------------------------------------------------------------------
def default_accum_seeds(n=N_DEFAULT):
    return [ASEED0 + i for i in range(n)]


def draw_accum_sequence(seed, host_only=False):
    """10 to 16 steps around pt_accum_begin / add / read / variance / denoise / reproject / end, pt_denoise_var and pt_upsample (blocking and
    _device forms), on the room of _draw_upload(guide=True).  Every sequence has three accumulations - small, large, small: a growth and a
    shrink of more than 4 x in pixels - and what else it is for goes by j = seed - ASEED0, so that any twelve seeds in a row have all of it:
        [begin small, add]
        [change, add]                  change = ACCUM_CHANGES[j % 4]: watertight (the switch brings its follow pass), update_vertices,
                                       set_materials, set_environment; samples see the state current at their add
        [begin large over the live accumulation, add] and a second add where a selecting add follows
        j % 4:  [knob, selecting add, accum_denoise] | [guides(new camera), reproject, add] |
                [add, guides, accum_denoise, upsample], all blocking or all asynchronous on ONE of the three streams |
                [guides, reproject with a cap, guides, reproject back without, selecting add]
        [set_pixel_shard or (odd j) upload, refused add, begin small, add]; for j % 12 in (4, 11) [refused add (bad parameters), add, begin
        small over the live accumulation, add] instead
        ACCUM_TAILS[j % 12]: read, variance, denoise_var, upsample, [end, refused read], [a call of another family and size, add].
    A selecting add takes the median of the model's finite positive noise as its threshold (the model computes it when its turn comes: the
    call list says "median"; 1.0 where no pixel has finite noise).  Add sizes come from ACCUM_SPP, stepped down until the add fits ACCUM_BUDGET."""
    rng = np.random.default_rng(seed)
    up = _draw_upload(rng, guide=True)
    G = _AccumGen(rng, seed, up)
    j = seed - ASEED0
    G.begin(small=True)
    G.accum_add()
    G.change_add(ACCUM_CHANGES[j % 4])
    G.begin(small=False)
    G.accum_add()
    if j % 4 == 0:
        G.accum_add()
        G.add(dict(op="knob", options=G.knobs[int(rng.integers(0, len(G.knobs)))]))
        G.accum_add(select=True)
        G.accum_denoise(dev=bool(j % 8))
    elif j % 4 == 1:
        G.reproject(cap=0, dev=bool((j // 4) % 2))
        G.accum_add()
    elif j % 4 == 2:
        G.chain(dev=(j % 8 == 2))
    else:
        G.accum_add()
        G.reproject(cap=16, dev=False)
        G.reproject(cap=0, dev=True, back=True)
        G.accum_add(select=True)
    if j % 12 in (4, 11):
        G.refused("accum_bad_params")
        G.accum_add()
    elif j % 2:
        G.k = 0
        G.add(_draw_upload(rng, guide=True))
        G.refused("accum_after_upload")
    else:
        G.add(dict(op="set_pixel_shard", shard=(int(rng.integers(0, 2)), int(rng.integers(2, 4)), int(rng.choice([1, 8, 16])))))
        G.refused("accum_after_shard")
    G.begin(small=True)
    G.accum_add()
    for t in ACCUM_TAILS[j % 12]:
        if t in ("read", "variance"):
            G.add(dict(op="accum_" + t))
        elif t.startswith("denoise_var"):
            G.denoise_var(dev=t.endswith("_device"))
        elif t.startswith("upsample"):
            G.upsample(dev=t.endswith("_device"), stream=G.stream() if t.endswith("_device") else None)
        elif t == "end":
            G.add(dict(op="accum_end"))
            G.live = None
            G.refused("accum_no_accum")
        else:
            assert t == "other", t
            G.other()
            G.accum_add()
    assert 10 <= len(G.steps) <= 16, len(G.steps)
    return dict(seed=seed, family="accum", host_only=bool(host_only), upload=up, steps=G.steps)


class _AccumGen(_GuideGen):
    def __init__(self, rng, seed, up):
        _GuideGen.__init__(self, rng, seed, up)
        self.live = None  # dict(view, W, H, adds) of the accumulation the context holds

    def add(self, step):
        _Gen.add(self, step)  # (nothing is ever pending here: _GuideGen.set_wt puts no extra pass in front of the switch)

    def begin(self, small):
        rng = self.rng
        (w0, w1), (h0, h1) = ACCUM_SMALL if small else ACCUM_LARGE
        W, H = int(rng.integers(w0, w1)), int(rng.integers(h0, h1))
        view = _draw_camera(rng, self.st)
        self.add(dict(op="accum_begin", cam=view, W=W, H=H, depth=int(rng.choice(DEPTHS[1:])), over_live=self.live is not None))
        self.live = dict(view=view, W=W, H=H, adds=0)

    def accum_add(self, select=False, form=None):
        rng, a = self.rng, self.live
        i = int(rng.integers(0, len(ACCUM_SPP)))
        while i > 0 and a["W"] * a["H"] * ACCUM_SPP[i] > ACCUM_BUDGET:
            i -= 1
        dev, stream = form or self.form()
        cap = int(rng.choice([0, 0, 0, 100]))
        self.add(dict(op="accum_add_device" if dev else "accum_add", n=ACCUM_SPP[i], cap=cap, select=bool(select), W=a["W"], H=a["H"], stream=stream,
                      want=bool(rng.random() < 0.7) if dev else True))
        a["adds"] += 1

    def change_add(self, kind):
        if kind == "set_materials":
            self.add(dict(op="set_materials", mats=_draw_mats(self.rng, self.st["mats"], guide=True)))
        else:
            self.change(kind)  # (the watertight switch brings its follow pass)
        self.accum_add()

    def other(self):
        """A call of the first or the second family at a size of its own between two adds."""
        if self.rng.random() < 0.5:
            self.frame(*self.any_size())
        else:
            self.follow()

    def refused(self, what):
        dev, stream = self.form()
        self.add(dict(op="refused", what=what, dev=dev, stream=stream, W=16, H=12))

    def _aov(self, view):
        a = self.live
        return dict(op="render_aov", cam=view, W=a["W"], H=a["H"], n=1, stream=None)

    def _follow(self, view, W, H):
        return dict(op="render_aov_follow", cam=view, W=W, H=H, stream=None, **self.follow_params(W, H))

    def reproject(self, cap, dev, back=False):
        """[guides under the new camera, reproject]: the call gets the buffer the guide pass filled (its host copy in the blocking form) and
        the model's guides under the old camera."""
        rng, a = self.rng, self.live
        old = a["view"]
        a.setdefault("first_view", old)
        new = a["first_view"] if back else _orbit(old, float(rng.choice([-25.0, -15.0, 15.0, 25.0])))
        stream = self.stream() if dev else None
        self.add(dict(self._aov(new), op="render_aov_device" if dev else "render_aov", stream=stream))
        self.add(dict(op="accum_reproject_device" if dev else "accum_reproject", cam=new, W=a["W"], H=a["H"], cap=cap, stream=stream, prev=self._aov(old), cur=self.steps[-1]))
        a["view"] = new

    def accum_denoise(self, dev, guides=None, chain=False, stream=None):
        a = self.live
        stream = stream if chain else (self.stream() if dev else None)
        self.add(dict(op="accum_denoise_device" if dev else "accum_denoise", W=a["W"], H=a["H"], params=self.filter_params(a["W"] * a["H"]), want_rgba8=bool(self.rng.random() < 0.5),
                      stream=stream, chain=bool(chain), guides=guides or self._follow(a["view"], a["W"], a["H"])))

    def chain(self, dev):
        """[add, follow guides, accum_denoise, upsample to 2 x]: all blocking, or all asynchronous on one stream with nothing in between - the
        filter reads the caller buffer the guide pass fills, the upsampling the filter's frame and the same guides."""
        a = self.live
        stream = self.stream() if dev else None
        self.accum_add(form=(dev, stream))
        self.add(dict(self._follow(a["view"], a["W"], a["H"]), op=FOLLOW_OPS[dev], stream=stream))
        g = self.steps[-1]
        self.accum_denoise(dev, guides=g, chain=True, stream=stream)
        self.upsample(dev=dev, stream=stream, chain=True)

    def upsample_params(self):
        rng = self.rng
        return dict(taps=int(rng.choice([2, 4])), flags=int(rng.integers(0, 2)), sigma_normal=float(rng.choice(SIGMAS["sigma_normal"])), sigma_depth=float(rng.choice(SIGMAS["sigma_depth"])),
                    sigma_albedo=float(rng.choice(SIGMAS["sigma_albedo"])))

    def upsample(self, dev=None, stream=None, chain=False):
        """chain: the low frame is the accumulation's filtered frame of the step before, its guides those of the step before that; else a frame and
        guides of the model's own at a small size.  The full size is 2 x the low one."""
        rng = self.rng
        if dev is None:
            dev, stream = self.form()
        if chain:
            a = self.live
            w, h, view = a["W"], a["H"], a["view"]
            lo = (None, self.steps[-2])
        else:
            (w0, w1), (h0, h1) = ACCUM_SMALL
            w, h, view = int(rng.integers(w0, w1)), int(rng.integers(h0, h1)), _draw_camera(rng, self.st)
            spp, depth = self.spp(w, h, filtered=True)
            lo = (dict(op="render", cam=view, W=w, H=h, spp=spp, depth=depth, stream=None), self._follow(view, w, h))
        self.add(dict(op="upsample_device" if dev else "upsample", w=w, h=h, W=2 * w, H=2 * h, params=self.upsample_params(), want_rgba8=bool(rng.random() < 0.5), stream=stream,
                      chain=bool(chain), src=dict(render=lo[0], guides=lo[1], guides_hi=dict(lo[1], op="render_aov_follow", W=2 * w, H=2 * h, stream=None))))

    def denoise_var(self, dev):
        """pt_denoise_var of a frame, a variance map and guides that no call of the sequence made (the model's own)."""
        rng = self.rng
        stream = self.stream() if dev else None
        (w0, w1), (h0, h1) = ACCUM_SMALL if rng.random() < 0.5 else ACCUM_LARGE
        W, H, view = int(rng.integers(w0, w1)), int(rng.integers(h0, h1)), _draw_camera(rng, self.st)
        spp, depth = self.spp(W, H, filtered=True)
        self.add(dict(op="denoise_var_device" if dev else "denoise_var", W=W, H=H, params=self.filter_params(W * H), want_rgba8=bool(rng.random() < 0.5), stream=stream, var_seed=int(rng.integers(0, 1 << 30)),
                      src=dict(render=dict(op="render", cam=view, W=W, H=H, spp=spp, depth=depth, stream=None), guides=self._follow(view, W, H))))


def _orbit(view, deg):
    """The view after an orbit of `deg` degrees about the vertical through look_at."""
    frm, at, up, fov = view
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    x, y, z = (np.asarray(frm, np.float64) - np.asarray(at, np.float64))
    return [float(at[0] + c * x + s * z), float(at[1] + y), float(at[2] - s * x + c * z)], [float(v) for v in at], list(up), fov


def kind_of(step):
    """The kind of change a step is, one of CHANGES, or None."""
    if step["op"] in ("update_vertices", "set_materials", "set_environment", "set_pixel_shard", "upload"):
        return step["op"]
    if step["op"] == "set_option" and step["key"] == "watertight":
        return "watertight"
    return None


def describe(step):
    op = step["op"]
    if op == "upload":
        return "upload %d triangles in %d meshes, builder %d, leaf %d, %s%s" % (sum(m["indices"].shape[0] for m, _ in step["ents"]), len(step["ents"]), step["builder"], step["leaf"],
                                                                            "map" if step["env"].get("use_map") else "auto" if step["env"].get("use_auto") else "colour", ", textured" if step["texs"] else "")
    if op == "update_vertices":
        return "update_vertices k=%d%s%s" % (step["k"], ", normals" if step["with_normals"] else "", "" if step["null_mesh"] is None else ", mesh %d NULL" % step["null_mesh"])
    if op == "set_pixel_shard":
        return "set_pixel_shard %s" % (step["shard"],)
    if op == "set_environment":
        return "set_environment %s" % ("map" if step["env"].get("use_map") else "auto" if step["env"].get("use_auto") else "colour")
    if op == "set_option":
        return "set_option %s=%d" % (step["key"], step["value"])
    if op == "knob":
        return "set_option " + " ".join("%s=%d" % kv for kv in step["options"])
    if op in ACCUM_OPS:
        s = op
        if op == "accum_begin":
            s += " %dx%d depth %d%s" % (step["W"], step["H"], step["depth"], " over a live accumulation" if step["over_live"] else "")
        elif op in ("accum_add", "accum_add_device"):
            s += " %d samples%s%s%s" % (step["n"], ", cap %d" % step["cap"] if step["cap"] else "", ", threshold = the median noise" if step["select"] else "", "" if step["want"] else ", no frame")
        elif op in ("accum_reproject", "accum_reproject_device"):
            s += " max_history %d, guides of the step before" % step["cap"]
        elif op in ("accum_denoise", "accum_denoise_device", "denoise_var", "denoise_var_device"):
            p = step["params"]
            s += " %dx%d L=%d flags=%d sigmas %g %g %g %g%s, guides %s" % (step["W"], step["H"], p["iterations"], p["flags"], p["sigma_color"], p["sigma_normal"], p["sigma_depth"], p["sigma_albedo"],
                                                                        ", RGBA8" if step["want_rgba8"] else "", "of the step before" if step.get("chain") else "[%s]" % describe(step.get("guides") or step["src"]["guides"]))
        elif op in ("upsample", "upsample_device"):
            p = step["params"]
            s += " %dx%d -> %dx%d taps=%d flags=%d sigmas %g %g %g%s of %s" % (step["w"], step["h"], step["W"], step["H"], p["taps"], p["flags"], p["sigma_normal"], p["sigma_depth"], p["sigma_albedo"],
                                                                            ", RGBA8" if step["want_rgba8"] else "", "the two steps before" if step["chain"] else "[%s]" % describe(step["src"]["render"]))
        if op in ACCUM_ASYNC:
            s += " on %s" % _stream_name(step["stream"])
        return s
    if op == "refused":
        return "refused: " + step["what"] + ("" if "dev" not in step else " (blocking)" if not step["dev"] else " (_device on %s)" % _stream_name(step["stream"]))
    if op in OBSERVING:
        s = "%s %dx%d" % (op, step["W"], step["H"])
        if op in AOV_OPS:
            s += " n=%d" % step["n"]
        elif op in FOLLOW_OPS + AOV_BATCH_OPS:
            s += " n=%d max_follow=%d roughness_max=%g" % (step["n"], step["max_follow"], step["roughness_max"])
        elif op in FILTER_OPS:
            p = step["params"]
            s += "%s L=%d flags=%d sigmas %g %g %g %g%s%s of %s" % (" %d frames" % step["K"] if op in DENOISE_BATCH_OPS else "", p["iterations"], p["flags"], p["sigma_color"], p["sigma_normal"],
                                                                p["sigma_depth"], p["sigma_albedo"], ", in place" if step["in_place"] else "", ", RGBA8" if step["want_rgba8"] else "",
                                                                "the two steps before" if step["chain"] else "[%s] and [%s]" % (describe(step["src"]["render"]), describe(step["src"]["guides"])))
        else:
            s += " %d spp depth %d" % (step["spp"], step["depth"])
        if "frames" in step:
            s += " %d frames (table of frame %d NULL)" % (len(step["frames"]), [m is None for _, m in step["frames"]].index(True))
        if op in ASYNC_OPS:
            s += " on %s" % _stream_name(step["stream"])
        return s
    return op


def _stream_name(stream):
    return "the context's stream" if stream is None else "caller stream %d" % stream


def call_list(seq, upto=None):
    lines = ["   upload: " + describe(seq["upload"])]
    for i, s in enumerate(seq["steps"][:upto]):
        lines.append("%5d: %s" % (i, describe(s)))
    return "\n".join(lines)


def coverage(seqs):
    """What the drawn sequences contain between them (the issue's list); the host test asserts it."""
    cov = dict(builder_then_update=set(), batch_then_single=0, aov_between_equal_renders=0, growth=0, shrink=0, shard_change=0, streams=set(), refused=set(), upload_mid=0,
               null_mesh=0, normals=0, spp=set())
    for seq in seqs:
        builder, px = seq["upload"]["builder"], None
        steps = seq["steps"]
        for i, s in enumerate(steps):
            op = s["op"]
            if op == "upload":
                builder = s["builder"]
                cov["upload_mid"] += 1
            if op == "update_vertices":
                cov["builder_then_update"].add(builder)
                cov["null_mesh"] += s["null_mesh"] is not None
                cov["normals"] += bool(s["with_normals"])
            if op in ("render_batch", "render_batch_device") and i + 1 < len(steps) and steps[i + 1]["op"] in ("render", "render_device"):
                cov["batch_then_single"] += 1
            if op == "render_aov" and 0 < i < len(steps) - 1 and steps[i - 1]["op"] in ("render", "render_device") and steps[i + 1] == steps[i - 1]:
                cov["aov_between_equal_renders"] += 1
            if op in RENDER_OPS:
                cov["spp"].add(s["spp"])
                now = s["W"] * s["H"] * len(s.get("frames", [0]))
                if px is not None:
                    cov["growth"] += now >= 4 * px
                    cov["shrink"] += 4 * now <= px
                px = now
            if op in ASYNC_OPS:
                cov["streams"].add(s["stream"])
            if op == "set_pixel_shard":
                cov["shard_change"] += 1
            if op == "refused":
                cov["refused"].add(s["what"])
    return cov


def guide_coverage(seqs):
    """What sequences of the second family contain between them; tests/test_sequences_host.py asserts the issue's conditions on it."""
    cov = dict(ops={o: 0 for o in GUIDE_OPS}, streams={o: set() for o in GUIDE_OPS[1::2]}, async_chains_mixed=0, async_batch_chains=0, in_place={(b, v): 0 for b in (False, True) for v in (False, True)},
               filters=[], growth_and_shrink=0, max_follow=set(), roughness_max=set(), refused=set(), table_kept=0, between=set(), bf1_before_k3_chain=0, followed={k: 0 for k in CHANGES}, upload_mid=0,
               glass_or_metal=0, inf_sigma=0, iterations=set(), demodulate=set(), null_table=0)
    for seq in seqs:
        steps, bf, px, grow, shrink, nf = seq["steps"], 0, None, 0, 0, 0
        m = seq["upload"]["mats"][1]
        cov["glass_or_metal"] += bool(m[4] == 1 or m[14] == 1)
        for i, s in enumerate(steps):
            op = s["op"]
            nxt = steps[i + 1] if i + 1 < len(steps) else None
            if op in GUIDE_OPS:
                cov["ops"][op] += 1
                if op in ASYNC_OPS:
                    cov["streams"][op].add(s["stream"])
            if op in FOLLOW_OPS + AOV_BATCH_OPS:
                cov["max_follow"].add(s["max_follow"])
                cov["roughness_max"].add(s["roughness_max"])
            if op in AOV_BATCH_OPS:
                cov["null_table"] += sum(mats is None for _, mats in s["frames"]) == 1
                cov["table_kept"] += bool(nxt and nxt["op"] in FOLLOW_OPS and any(mats is not None for _, mats in s["frames"]))
            if op == "set_option" and s["key"] == "batch_frames":
                bf = s["value"]
            if op == "upload":
                cov["upload_mid"] += 1
            if op == "refused":
                cov["refused"].add(s["what"])
            if op in GUIDE_OPS and 0 < i and nxt and steps[i - 1]["op"] in ("render", "render_device") and nxt == steps[i - 1] and not s.get("chain"):
                cov["between"].add(BLOCKING_OF.get(op, op))
            if op in FILTER_OPS:
                batch = op in DENOISE_BATCH_OPS
                cov["in_place"][(batch, s["in_place"])] += 1
                cov["inf_sigma"] += any(np.isinf(v) for v in s["params"].values())
                cov["iterations"].add(s["params"]["iterations"])
                cov["demodulate"].add(s["params"]["flags"])
                now = s["K"] * s["W"] * s["H"]
                if px is not None:
                    grow += now >= 4 * px
                    shrink += 4 * now <= px
                px, nf = now, nf + 1
                if s["chain"] and op in ASYNC_OPS:
                    assert steps[i - 1]["op"] in ASYNC_OPS and steps[i - 2]["op"] in ASYNC_OPS
                    if batch:
                        cov["async_batch_chains"] += 1
                    else:
                        cov["async_chains_mixed"] += len({steps[j]["stream"] for j in (i - 2, i - 1, i)}) > 1
                if s["chain"] and batch and s["K"] == 3 and bf == 1:
                    cov["bf1_before_k3_chain"] += 1
            kind = kind_of(s)
            if kind is not None and nxt and nxt["op"] in FOLLOW_OPS + AOV_BATCH_OPS:
                cov["followed"][kind] += 1
        cov["filters"].append((seq["seed"], nf, grow, shrink))
        cov["growth_and_shrink"] += grow >= 1 and shrink >= 1
    return cov


def visibility(seq, model):
    """With the oracle alone: (shown, hidden, frames, flat).  A change is VISIBLE if the oracle's output of the next observing step differs
    from what that step shows in the state before the change (the generator puts nothing but a refused call between the two).  shown:
    visible changes per kind of CHANGES; hidden: [(step, kind)]; frames: observing steps; flat: those whose output is one constant pixel."""
    return _visibility(seq, model)[:4]


def guide_visibility(seq, model):
    """visibility() and, for the second family: follow = (observations of the follow kernels, those whose expected buffer differs from the
    same call with max_follow = 0); filters = [(step, share of the owned pixels in which the filter's output differs from its input)]."""
    return _visibility(seq, model)


def _visibility(seq, model):
    steps, states = seq["steps"], states_of(seq)
    model.forget()
    want = {}

    def expected(j):
        if j not in want:
            want[j] = model.expected(states[j], steps[j])
        return want[j]

    shown, hidden, frames, flat, follow, filters = {k: 0 for k in CHANGES}, [], 0, [], [0, 0], []
    for i, s in enumerate(steps):
        if s["op"] in OBSERVING:
            frames += 1
            a = expected(i)[0]
            if (a == a.reshape(-1, a.shape[-1])[0]).all():
                flat.append(i)
        if s["op"] in FOLLOW_OPS + AOV_BATCH_OPS:
            follow[0] += 1
            follow[1] += bool(same(expected(i)[0], model.expected(states[i], dict(s, max_follow=0))[0]).any())
        if s["op"] in FILTER_OPS:
            own = np.stack([own_mask(states[i], s["W"], s["H"])] * s["K"]).reshape(expected(i)[0].shape[:-1])
            diff = same(expected(i)[0], model.inputs(states[i], s)[0]).any(-1)
            filters.append((i, float((diff & own).sum()) / max(1, int(own.sum()))))
        kind = kind_of(s)
        if kind is None:
            continue
        j = i + 1
        while steps[j]["op"] not in OBSERVING:
            assert steps[j]["op"] == "refused", describe(steps[j])
            j += 1
        if same(expected(j)[0], model.expected(states[i], steps[j])[0]).any():
            shown[kind] += 1
        else:
            hidden.append((i, kind))
    return shown, hidden, frames, flat, tuple(follow), filters


# ---------------------------------------------------------------------------------------------------------------------
# the runner
# ---------------------------------------------------------------------------------------------------------------------
def _bcam(cam, W, H):
    return B.to_camera_data(cam[0], cam[1], cam[2], cam[3], W, H)


def upload(ctx, st, step=None):
    """The state's scene into a context: with `step` (an upload step) its builder options first, else the context's defaults."""
    ctx.set_option("dynamic", 1)
    if step is not None:
        ctx.set_option("bvh_builder", step["builder"])
        ctx.set_option("leaf_size", step["leaf"])
    ctx.upload_scene(entities(st), st["mats"], textures=st["texs"], mesh_textures=st["mesh_tex"], env=B.make_env(**st["env"]))


def collapsed_of(st):
    """Collapsed triangle records by id of a FRESH host-only upload of the state's meshes: the V of refit_common.assert_boxes."""
    h = B.Context(-1)
    try:
        h.upload_scene(entities(st), st["mats"])
        t = RC.tris_by_id(h.export_trees())
        return np.stack([t["p0"], t["p1"], t["p2"]], 1)
    finally:
        h.close()


def same(got, want):
    """Float arrays on raw bits, NaN equal to NaN; integer arrays by value.  Returns the mask of differing elements."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.dtype == np.float32:
        return ~((np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want, F32).view(np.uint32)) | (np.isnan(got) & np.isnan(want)))
    return got != want


def expect_refusal(fn, what):
    """fn must raise PtError with PT_E_INVALID."""
    try:
        fn()
    except B.PtError as e:
        assert "(-1)" in str(e), "%s: refused with another code than PT_E_INVALID: %s" % (what, e)
        return
    raise AssertionError("%s: the call was accepted" % what)


def _follow_params(step, **changes):
    return B.aov_default_params(**dict(dict(n_samples=step.get("n", 1), max_follow=step.get("max_follow", 4), roughness_max=step.get("roughness_max", 0.3)), **changes))


def _filter_params(step, **changes):
    return B.denoise_default_params(**dict(step["params"], **changes))


def _refused_into(ctx, what, call, shape):
    """A blocking guide call that must be refused, through its C entry point with an output array of the caller's: PT_E_INVALID, and the
    array as it was."""
    out = np.full(shape, 0.25, F32)
    rc = int(call(out.ctypes.data_as(C.POINTER(C.c_float))))
    assert rc == -1, "%s: the call returned %d, not PT_E_INVALID (%s)" % (what, rc, B.lib().pt_last_error(ctx._h).decode())
    assert (out == F32(0.25)).all(), "%s: the refused call wrote to its output" % what


def guide_refused_call(ctx, st, step, host_only=False, frame=None, stream=None):
    """The refused calls of the second family: PT_E_INVALID, on a host-only context too (through the twin where the call has one; the batch
    forms check their arguments before they ask for the device).  frame: the caller buffers of the _device form (a DeviceFrame the
    runner reads back at the end: not a byte of it may change); the blocking filters get an in_place frame that must stay as it is."""
    what, W, H = step["what"], step["W"], step["H"]
    dev = step["dev"] and not host_only
    n_mat = st["mats"].shape[0]
    if what in ("aov_batch_watertight", "aov_batch_materials"):
        frames = [(_bcam(cam, W, H), mats) for cam, mats in step["frames"]]
        n_mat += what == "aov_batch_materials"
        if dev:
            return expect_refusal(lambda: ctx.render_aov_batch_device(frames, W, H, frame.rgb, None, stream=stream, n_materials=n_mat), what)
        arr, _, keep = B._marshal_frames(frames)
        return _refused_into(ctx, what, lambda out: B.lib().pt_render_aov_batch(ctx._h, arr, len(frames), n_mat, W, H, None, out), (len(frames), H, W, 8))
    if what == "follow_max_follow":
        cam, p = _bcam(step["cam"], W, H), B.aov_default_params(max_follow=9)
        if dev:
            return expect_refusal(lambda: ctx.render_aov_follow_device(cam, W, H, frame.rgb, p, stream=stream), what)
        if host_only:
            ids = np.arange(W * H, dtype=np.uint32)
            return _refused_into(ctx, what, lambda out: B.lib().pt_debug_aov_follow_host(ctx._h, C.byref(cam), W, H, C.byref(p), ids.ctypes.data_as(C.POINTER(C.c_uint32)), ids.size, out), (H, W, 8))
        return _refused_into(ctx, what, lambda out: B.lib().pt_render_aov_follow(ctx._h, C.byref(cam), W, H, C.byref(p), out), (H, W, 8))
    rgb, aov = np.full((2, H, W, 3), 0.25, F32), np.zeros((2, H, W, 8), F32)
    if what == "denoise_batch_no_frames":
        if dev:
            return expect_refusal(lambda: ctx.denoise_batch_device(frame.rgb, frame.rgb, 0, W, H, frame.rgb, None, d_out_rgba8=frame.rgba8, stream=stream), what)
        expect_refusal(lambda: ctx.denoise_batch(rgb[:0], aov[:0], None, want_rgba8=True, in_place=True), what)
    else:
        p = B.denoise_default_params(iterations=0) if what == "denoise_iterations" else B.denoise_default_params(sigma_normal=float("nan"))
        if dev:
            return expect_refusal(lambda: ctx.denoise_device(frame.rgb, frame.rgb, W, H, frame.rgb, p, d_out_rgba8=frame.rgba8, stream=stream), what)
        expect_refusal(lambda: (ctx.denoise_host if host_only else ctx.denoise)(rgb[0], aov[0], p, want_rgba8=True, in_place=True), what)
        if host_only:  # the batch form: its arguments first, the device last
            expect_refusal(lambda: ctx.denoise_batch(rgb, aov, p, in_place=True), what)
    assert (rgb == F32(0.25)).all(), "%s: the refused call wrote to its frame" % what


def refused_call(ctx, st, step, host_only=False, frame=None, stream=None):
    what = step["what"]
    if what in GUIDE_REFUSED:
        return guide_refused_call(ctx, st, step, host_only, frame, stream)
    if what == "batch_watertight":
        frames = [(_bcam(cam, step["W"], step["H"]), mats) for cam, mats in step["frames"]]
        return expect_refusal(lambda: ctx.render_batch(frames, step["W"], step["H"], step["spp"], step["depth"], n_materials=st["mats"].shape[0]), what)
    if what == "update_count":
        mv = RC.moved(st["scene"], step["k"])
        args = [dict(vertices=m["vertices"]) for m in mv]
        args[step["mesh"]] = dict(args[step["mesh"]], n_vertices=mv[step["mesh"]]["vertices"].shape[0] - 1)
        return expect_refusal(lambda: ctx.update_vertices(args), what)
    if what == "kernel_watertight":
        return expect_refusal(lambda: ctx.set_option("kernel", 1), what)
    assert what == "aov_zero_samples"
    cam = _bcam(step["cam"], step["W"], step["H"])
    if host_only:
        return expect_refusal(lambda: ctx.aov_host(cam, step["W"], step["H"], 0), what)
    return expect_refusal(lambda: ctx.render_aov(cam, step["W"], step["H"], 0), what)


def observe(ctx, step, n_mat, bufs=None, A=None, inputs=None, filter_on=None):
    """The observing call.  Blocking: returns (floats, RGBA8 or None).  Asynchronous: enqueues into bufs (a DeviceFrame) and returns None.
    A filter step - blocking: inputs = (rgb, guide buffers), host arrays that stay as they are; asynchronous: bufs = (d_rgb, d_aov, the
    DeviceFrame of the result).  filter_on: the context that filters (pt_denoise has no group form), default ctx."""
    op, W, H = step["op"], step["W"], step["H"]
    stream = A.stream(step["stream"]) if (A is not None and step.get("stream") is not None) else None
    if op == "render":
        return ctx.render(_bcam(step["cam"], W, H), W, H, step["spp"], step["depth"], want_rgba8=True)
    if op == "render_device":
        return ctx.render_device(_bcam(step["cam"], W, H), W, H, step["spp"], step["depth"], bufs.rgb, bufs.rgba8, stream=stream)
    if op in ("render_batch", "render_batch_device"):
        frames = [(_bcam(cam, W, H), mats) for cam, mats in step["frames"]]
        if op == "render_batch":
            return ctx.render_batch(frames, W, H, step["spp"], step["depth"], want_rgba8=True, n_materials=n_mat)
        return ctx.render_batch_device(frames, W, H, step["spp"], step["depth"], bufs.rgb, bufs.rgba8, stream=stream, n_materials=n_mat)
    if op == "render_aov":
        return ctx.render_aov(_bcam(step["cam"], W, H), W, H, step["n"]), None
    if op == "render_aov_follow":
        return ctx.render_aov_follow(_bcam(step["cam"], W, H), W, H, _follow_params(step)), None
    if op == "render_aov_follow_device":
        return ctx.render_aov_follow_device(_bcam(step["cam"], W, H), W, H, bufs.rgb, _follow_params(step), stream=stream)
    if op in AOV_BATCH_OPS:
        frames = [(_bcam(cam, W, H), mats) for cam, mats in step["frames"]]
        if op == "render_aov_batch":
            return ctx.render_aov_batch(frames, W, H, _follow_params(step), n_materials=n_mat), None
        return ctx.render_aov_batch_device(frames, W, H, bufs.rgb, _follow_params(step), stream=stream, n_materials=n_mat)
    if op in ("denoise", "denoise_batch"):
        rgb = np.array(inputs[0], F32) if step["in_place"] else inputs[0]  # (the model's frame is shared: in place works on a copy)
        out, out8 = getattr(filter_on or ctx, op)(rgb, inputs[1], _filter_params(step), want_rgba8=step["want_rgba8"], in_place=step["in_place"])
        assert not step["in_place"] or out is rgb
        return out, out8
    if op in ("denoise_device", "denoise_batch_device"):
        d_rgb, d_aov, out = bufs
        if op == "denoise_device":
            return ctx.denoise_device(d_rgb, d_aov, W, H, out.rgb, _filter_params(step), d_out_rgba8=out.rgba8 if step["want_rgba8"] else None, stream=stream)
        return ctx.denoise_batch_device(d_rgb, d_aov, step["K"], W, H, out.rgb, _filter_params(step), d_out_rgba8=out.rgba8 if step["want_rgba8"] else None, stream=stream)
    assert op == "render_aov_device", op
    return ctx.render_aov_device(_bcam(step["cam"], W, H), W, H, step["n"], bufs.rgb, stream=stream)


def _device_frame(A, step):
    """The caller buffers a _device step writes (a refused one: must leave alone)."""
    if step["op"] == "refused":
        return A.DeviceFrame(step["W"], step["H"], frames=2, floats=8)
    if step["op"] in ("render_aov_device", "render_aov_follow_device", "render_aov_batch_device"):
        return A.DeviceFrame(step["W"], step["H"], frames=len(step.get("frames", [0])), floats=8)
    return A.DeviceFrame(step["W"], step["H"], frames=step["K"] if step["op"] in FILTER_OPS else len(step.get("frames", [0])))


def expected_launches(st, step):
    """stats()["launches"] after a blocking call of the second family (include/mi355pt.h): the cut is pt_debug_plan_batch's."""
    op = step["op"]
    if op == "render_aov_follow":
        return 1
    if op == "denoise":
        return step["params"]["iterations"] + 2
    seqs = len(B.plan_batch(step["W"], step["H"], step["K"] if op == "denoise_batch" else len(step["frames"]), st.get("batch_frames", 0)))
    return seqs if op == "render_aov_batch" else seqs * (step["params"]["iterations"] + 2)


def fresh_agrees(st, step, want, inputs=None):
    """One more comparison after a mismatch: a fresh context, the model's state, the same call (blocking form of it; a filter gets the
    model's inputs)."""
    ctx = B.Context(0)
    try:
        ctx.set_option("watertight", st["wt"])
        upload(ctx, st)
        if st["shard"]:
            ctx.set_pixel_shard(*st["shard"])
        blocking = dict(step, op=BLOCKING_OF.get(step["op"], step["op"]))
        got = observe(ctx, blocking, st["mats"].shape[0], inputs=inputs)
        return not same(got[0], want[0]).any() and (want[1] is None or not same(got[1], want[1]).any())
    finally:
        ctx.close()


def run(ctx, seq, model, upto=None, A=None, diagnose=True, log=None):
    """Execute seq["steps"][:upto] on ctx (a fresh context) and compare every observation with the model's.  A: tests/async_common (a
    device context); None on a host-only context, where seq["host_only"] must be set.  Returns the list of (step index, floats, RGBA8)
    observed.  Raises AssertionError on the first difference (of the blocking steps at once, of the asynchronous ones after the final
    synchronize)."""
    steps = seq["steps"][:upto]
    host = seq["host_only"]
    model.forget()
    assert host == (A is None)
    where = lambda i: "%ssequence seed=%d, step %d (%s)" % (seq.get("family", "") and seq["family"] + " ", seq["seed"], i, describe(steps[i]))
    bufs, pending, got_all, outs = {}, [], [], {}
    t_gpu = 0.0
    poison = np.uint32(0xA5A5A5A5)
    acc = None

    def check(i, st, got, want):
        bad = same(got[0], want[0])
        bad8 = same(got[1], want[1]) if want[1] is not None else np.zeros(1, bool)
        if not (bad.any() or bad8.any()):
            return
        verdict = ""
        if diagnose and not host:
            ok = fresh_agrees(st, steps[i], want, model.inputs(st, steps[i]) if steps[i]["op"] in FILTER_OPS else None)
            verdict = ("; a FRESH context in the model's state agrees with the oracle: STALE STATE from the sequence" if ok else
                       "; a fresh context in the model's state differs from the oracle as well: a SINGLE-CALL bug")
        first = tuple(np.argwhere(bad)[0]) if bad.any() else None
        raise AssertionError("%s: %d of %d floats%s differ from the oracle%s%s\ncalls:\n%s" % (
            where(i), bad.sum(), bad.size, "" if want[1] is None else " and %d of %d RGBA8 pixels" % (bad8.sum(), bad8.size),
            "" if first is None else "; first at %s: got %r, want %r" % (first, got[0][first], want[0][first]), verdict, call_list(seq, i + 1)))

    try:
        states = states_of(dict(seq, steps=steps))
        if not host:  # every caller buffer before anything is enqueued: an allocation or its fill may wait for the device
            for i, s in enumerate(steps):
                if (s["op"] in ASYNC_OPS and not (s["op"] in FILTER_OPS and s["in_place"])) or (s["op"] == "refused" and s.get("dev") and s["what"] not in ACCUM_REFUSED):  # (in place: the frame it reads)
                    bufs[i] = _device_frame(A, s)
                if s["op"] in ASYNC_OPS and s["op"] in FILTER_OPS and not s["chain"]:  # a filter of the model's own frame and guides: in HBM before the first step
                    rgb, aov = model.inputs(states[i], s)
                    bufs[i, "rgb"], bufs[i, "aov"] = A.DeviceFrame(s["W"], s["H"], frames=s["K"]), A.DeviceFrame(s["W"], s["H"], frames=s["K"], floats=8)
                    A.to_device(bufs[i, "rgb"].rgb, rgb)
                    A.to_device(bufs[i, "aov"].rgb, aov)
        if seq.get("family") == "accum":  # the third family's steps: tests/accum_seq_common.py (imported here: it builds on this module)
            import accum_seq_common

            acc = accum_seq_common.SeqRunner(ctx, model, A, host, seq, steps, states, bufs, where)
            if not host:
                acc.prepare()
        st = states[0]
        t0 = time.time()
        upload(ctx, st, seq["upload"])
        t_gpu += time.time() - t0
        if host:
            _host_handover(ctx, st, seq["upload"])
        for i, s in enumerate(steps):
            op, st = s["op"], states[i]
            if log:
                log("%3d %s" % (i, describe(s)))
            t0 = time.time()
            new = states[i + 1]
            if op == "upload":
                upload(ctx, new, s)
                if host:
                    _host_handover(ctx, new, s)
            elif op == "update_vertices":
                ctx.update_vertices(update_args(st, s))
                exs = [("host", ctx.export_trees())] if host else [("HBM", ctx.export_trees(device=True)), ("lazily refitted host", ctx.export_trees())]
                t_gpu += time.time() - t0
                V = collapsed_of(new)
                for name, ex in exs:
                    RC.assert_boxes(ex, V, where(i) + ": %s arrays against the box definition" % name)
                t0 = time.time()
            elif op == "set_materials":
                ctx.set_materials(s["mats"])
            elif op == "set_environment":
                ctx.set_environment(B.make_env(**s["env"]))
            elif op == "set_pixel_shard":
                ctx.set_pixel_shard(*(s["shard"] or (0, 1, 16)))
            elif op == "set_option":
                ctx.set_option(s["key"], s["value"])
            elif op == "knob":
                for k, v in s["options"]:
                    ctx.set_option(k, v)
            elif op in ACCUM_OPS or (op == "refused" and s["what"] in ACCUM_REFUSED):
                t_gpu += time.time() - t0
                acc.step(i)
                t0 = time.time()
            elif op == "refused":
                refused_call(ctx, st, s, host, bufs.get(i), A.stream(s["stream"]) if (not host and s.get("stream") is not None) else None)
            elif host:
                t_gpu += time.time() - t0
                observe_host(ctx, st, s, model, where(i))
                t0 = time.time()
            elif op in ASYNC_OPS:
                b = bufs.get(i)
                if op in FILTER_OPS:  # from the buffers the two calls before it fill (a chain), or from the model's; in place: into the frame's own
                    src = (bufs[i - 2], bufs[i - 1]) if s["chain"] else (bufs[i, "rgb"], bufs[i, "aov"])
                    if s["in_place"]:
                        outs[i] = i - 2 if s["chain"] else (i, "rgb")
                    b = (src[0].rgb, src[1].rgb, bufs[outs.get(i, i)])
                observe(ctx, s, st["mats"].shape[0], b, A)
                pending.append((i, st))
            else:
                inputs = None
                if op in FILTER_OPS:
                    t_gpu += time.time() - t0
                    inputs = model.inputs(st, s)
                    t0 = time.time()
                got = observe(ctx, s, st["mats"].shape[0], inputs=inputs)
                launches = ctx.stats()["launches"] if op in GUIDE_OPS else None
                t_gpu += time.time() - t0
                got_all.append((i,) + tuple(got))
                check(i, st, got, model.expected(st, s))
                assert launches is None or launches == expected_launches(st, s), "%s: pt_get_stats counts %d launches, the header says %d" % (where(i), launches, expected_launches(st, s))
                t0 = time.time()
            t_gpu += time.time() - t0
        if pending or (acc is not None and acc.pending):
            t0 = time.time()
            ctx.synchronize()  # the one wait of the sequence: everything before it was ordered by the library
            t_gpu += time.time() - t0
            overwritten = {o: i for i, o in outs.items()}  # a frame that a filter after it worked on in place: seen through the filter's result only
            raw = {i: bufs[outs.get(i, i)].read() for i, _ in pending}
            for i, sti in pending:
                s, (rgb, rgba8) = steps[i], raw[i]
                want = model.expected(sti, s)
                got_all.append((i, rgb, rgba8 if want[1] is not None else None))
                if i in overwritten:  # its RGBA8 image is the render's own unless the filter wrote one
                    if not steps[overwritten[i]]["want_rgba8"]:
                        bad8 = same(rgba8, want[1])
                        assert not bad8.any(), "%s: %d of %d RGBA8 pixels differ from the oracle\ncalls:\n%s" % (where(i), bad8.sum(), bad8.size, call_list(seq, i + 1))
                    continue
                if want[1] is None and not (s.get("chain") and i in outs):  # nobody was to write the RGBA8 buffer of this step
                    assert (rgba8 == poison).all(), "%s: the call wrote to a buffer that is not its own (the RGBA8 image beside its result)" % where(i)
                check(i, sti, (rgb, rgba8 if want[1] is not None else None), want)
            for i, s in enumerate(steps):
                if s["op"] == "refused" and i in bufs:
                    rgb, rgba8 = bufs[i].read()
                    assert (rgb.view(np.uint32) == poison).all() and (rgba8 == poison).all(), "%s: the refused call wrote to the caller's buffers" % where(i)
        if acc is not None:
            acc.finish()
            t_gpu += acc.seconds
    finally:
        if not host:
            try:
                if pending or (acc is not None and acc.pending):
                    ctx.synchronize()
            finally:
                for f in list(bufs.values()) + (acc.frames() if acc is not None else []):
                    f.free()
                A.destroy_streams()
    run.seconds = t_gpu
    return sorted(got_all, key=lambda g: g[0])


# ---------------------------------------------------------------------------------------------------------------------
# the host twin
# ---------------------------------------------------------------------------------------------------------------------
def _host_handover(ctx, st, step):
    """Builders 1 and 2 hand over to builder 0 on a host-only context: the arrays are builder 0's, byte for byte."""
    ref = B.Context(-1)
    try:
        upload(ref, st, dict(step, builder=0))
        RC.same_arrays(ref.export_trees(), ctx.export_trees(), "host-only context, bvh_builder %d: the tree is builder 0's" % step["builder"])
    finally:
        ref.close()


def observe_host(ctx, st, step, model, what):
    """What a host-only context can show of the state: the guide buffers of the step's view through pt_debug_aov_host against
    tests/aov_ref.py, closest hits of 200 battery rays inside the domain against the oracle's brute force, the boxes against their
    definition."""
    W, H = step["W"], step["H"]
    if step["op"] in GUIDE_OPS:
        observe_guides_host(ctx, st, step, model, what)
        if step["op"] not in FOLLOW_OPS:
            return
    cams = [c for c, _ in step["frames"]] if "frames" in step else [step["cam"]]
    n = step.get("n", 1 + step.get("spp", 1) % 2)
    S, flat = model.scene(st)
    for cam in cams[:1]:
        got = ctx.aov_host(_bcam(cam, W, H), W, H, n)
        want, _ = model.expected(dict(st, shard=None), dict(op="render_aov", cam=cam, W=W, H=H, n=n))
        bad = same(got, want)
        assert not bad.any(), "%s: pt_debug_aov_host, %d of %d floats differ from aov_ref; first at %s" % (what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))
    tris = RC.soup_of(entities(st))
    rays, cls = rb.make_rays(tris, np.random.default_rng(4242), 200)
    held = rb.bands(rays, rb.scene_measure(tris), cls)[0]
    assert held.sum() > 0.7 * held.size
    t0 = time.time()
    truth = S.intersect_n(rays, use_bvh=False)
    model.seconds += time.time() - t0
    got = ctx.closest_hit_host_n(rays)
    bad = (got[0] != truth[0]) | (got[4] != truth[4])
    for k in (1, 2, 3):
        bad |= truth[0] & (got[k].view(np.uint32) != truth[k].view(np.uint32))
    bad = np.nonzero(bad & held)[0]
    assert bad.size == 0, "%s: %d of %d battery rays inside the domain differ from the oracle's brute force; first: class %d %r" % (what, bad.size, held.sum(), cls[bad[0]], rays[bad[0]].tolist())
    RC.assert_boxes(ctx.export_trees(), collapsed_of(st), what + ": host arrays against the box definition")


def expect_no_device(fn, what):
    """fn must raise PtError with PT_E_NO_DEVICE: a valid call of a device entry point on a host-only context."""
    try:
        fn()
    except B.PtError as e:
        assert "(-2)" in str(e), "%s: a host-only context answers a valid call with another code than PT_E_NO_DEVICE: %s" % (what, e)
        return
    raise AssertionError("%s: a host-only context accepted the call" % what)


def observe_guides_host(ctx, st, step, model, what):
    """The second family on a host-only context: a follow pass through pt_debug_aov_follow_host against tests/aov_follow_ref.py; a guide batch
    is answered with PT_E_NO_DEVICE, and the twin shows its frame with the context's table; a filter through pt_debug_denoise_host on the
    model's inputs against tests/denoise_ref.py, frame by frame, the batch form answered with PT_E_NO_DEVICE."""
    op, W, H = step["op"], step["W"], step["H"]
    whole = dict(st, shard=None)  # (the twin knows no shard)
    if op in FOLLOW_OPS + AOV_BATCH_OPS:
        cam = step["cam"] if op in FOLLOW_OPS else [c for c, mats in step["frames"] if mats is None][0]
        if op in AOV_BATCH_OPS:
            frames = [(_bcam(c, W, H), mats) for c, mats in step["frames"]]
            expect_no_device(lambda: ctx.render_aov_batch(frames, W, H, _follow_params(step), n_materials=st["mats"].shape[0]), what)
        got = ctx.aov_follow_host(_bcam(cam, W, H), W, H, _follow_params(step))
        want, _ = model.expected(whole, dict(step, op="render_aov_follow", cam=cam))
        bad = same(got, want)
        assert not bad.any(), "%s: pt_debug_aov_follow_host, %d of %d floats differ from aov_follow_ref; first at %s" % (what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))
        return
    rgb, aov = model.inputs(whole, step)
    want, want8 = model.expected(whole, step)
    if op in DENOISE_BATCH_OPS:
        expect_no_device(lambda: ctx.denoise_batch(rgb, aov, _filter_params(step)), what)
    else:
        expect_no_device(lambda: ctx.denoise(rgb, aov, _filter_params(step)), what)
        rgb, aov, want, want8 = rgb[None], aov[None], want[None], None if want8 is None else want8[None]
    for f in range(rgb.shape[0]):
        src = np.array(rgb[f], F32) if step["in_place"] else rgb[f]
        got, got8 = ctx.denoise_host(src, aov[f], _filter_params(step), want_rgba8=step["want_rgba8"], in_place=step["in_place"])
        bad = same(got, want[f])
        assert not bad.any(), "%s: pt_debug_denoise_host, frame %d: %d of %d floats differ from denoise_ref; first at %s" % (what, f, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))
        assert want8 is None or (got8 == want8[f]).all(), "%s: pt_debug_denoise_host, frame %d: the RGBA8 image differs from denoise_ref's" % (what, f)


# ---------------------------------------------------------------------------------------------------------------------
# the group path: what pt_group_* can express of a sequence
# ---------------------------------------------------------------------------------------------------------------------
def group_projection(seq):
    """The sequence as a pt_group can run it, with option "watertight" = 1 throughout: uploads, update_vertices, set_materials, box_exact
    and the scheduler knobs stay; every single frame becomes a blocking render, every guide pass (first hit or follow mode) a blocking one,
    and a denoise_chain becomes the group's render, the group's follow pass and pt_denoise of the two on rank 0's context; batches (refused
    with watertight = 1), the other filters, shards (the group's own business), set_environment (no group call), refusals, "batch_frames" and
    the watertight switches go."""
    steps = [dict(op="set_option", key="watertight", value=1)]
    for s in seq["steps"]:
        op = s["op"]
        if op in ("upload", "update_vertices", "set_materials", "knob") or (op == "set_option" and s["key"] == "box_exact"):
            steps.append(s)
        elif op in ("render", "render_device"):
            steps.append(dict(s, op="render", stream=None))
        elif op in AOV_OPS:
            steps.append(dict(s, op="render_aov", stream=None))
        elif op in FOLLOW_OPS:
            steps.append(dict(s, op="render_aov_follow", stream=None))
        elif op in DENOISE_OPS and s["chain"]:  # behind the group's frame and guides: pt_denoise on rank 0's context, as the header prescribes for N GPUs
            render, guides = steps[-2], steps[-1]
            assert render["op"] == "render" and guides["op"] == "render_aov_follow"
            steps.append(dict(s, op="denoise", stream=None, src=dict(render=render, guides=guides)))
    return dict(seed=seq["seed"], family=seq.get("family", ""), host_only=False, upload=seq["upload"], steps=steps)


def run_plain(target, seq):
    """The steps of a projected sequence on `target` (a Context or a Group: the same method names), nothing compared: the observations."""
    st = apply(None, seq["upload"])
    upload(target, st, seq["upload"])
    out = []
    for i, s in enumerate(seq["steps"]):
        op = s["op"]
        if op == "upload":
            upload(target, apply(st, s), s)
        elif op == "update_vertices":
            target.update_vertices(update_args(st, s))
        elif op == "set_materials":
            target.set_materials(s["mats"])
        elif op == "set_option":
            target.set_option(s["key"], s["value"])
        elif op == "knob":
            for k, v in s["options"]:
                target.set_option(k, v)
        elif op == "denoise":  # of the two observations before it, on rank 0's context where target is a group
            out.append((i,) + tuple(observe(target, s, st["mats"].shape[0], inputs=(out[-2][1], out[-1][1]), filter_on=target.ctx(0) if hasattr(target, "ctx") else None)))
        else:
            assert op in ("render", "render_aov", "render_aov_follow"), op
            out.append((i,) + tuple(observe(target, s, st["mats"].shape[0])))
        st = apply(st, s)
    return out
