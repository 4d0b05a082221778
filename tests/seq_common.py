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
"""
import time

import numpy as np

import aov_ref
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
OBSERVING = RENDER_OPS + AOV_OPS
ASYNC_OPS = ("render_device", "render_batch_device", "render_aov_device")
REFUSED = ("batch_watertight", "update_count", "kernel_watertight", "aov_zero_samples")
CHANGES = ("update_vertices", "set_materials", "set_environment", "set_pixel_shard", "watertight", "upload")  # the kinds whose effect must show
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


def _draw_upload(rng):
    scale = float(10.0 ** rng.uniform(-1.0, 1.5))
    offset = rng.uniform(-1.0, 1.0, 3) * scale * (0.0 if rng.random() < 0.3 else float(rng.uniform(0.0, 3.0)))
    n_mesh = int(rng.integers(2, 5))
    n = int(rng.integers(3, 5)) if n_mesh == 2 else int(rng.integers(2, 4))  # 5 * 2 * n^2 wall triangles
    ents = [(_mesh(*_room(n), scale, offset), 0)]
    mats = [scene_io.material(base_color=tuple(rng.uniform(0.3, 0.9, 3)), roughness=float(rng.uniform(0.2, 1.0)))]
    if n_mesh >= 3:
        sub = 2 if (n_mesh == 3 and n == 2 and rng.random() < 0.5) else 1  # 320 or 80 triangles
        radius = float(rng.uniform(0.35, 0.55))
        v, nr, tc = _sphere(sub, radius, (rng.uniform(-0.3, 0.3), -0.95 + radius, rng.uniform(-0.3, 0.3)))
        ents.append((_mesh(v, nr, tc, np.arange(v.shape[0]), scale, offset), 1))
        kind = int(rng.integers(0, 4))
        colour = tuple(rng.uniform(0.2, 1.0, 3))
        mats.append([scene_io.material(base_color=colour, specular_transmission=1.0, ior=1.5, roughness=0.05), scene_io.material(base_color=colour, metallic=1.0, roughness=0.25),
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


def _draw_mats(rng, mats):
    """Another table: the walls' base colour always changes, the other rows half of the time."""
    m = np.array(mats, F32)
    m[0, 0:3] = (m[0, [1, 2, 0]] * F32(0.5) + rng.uniform(0.05, 0.45, 3).astype(F32))
    for r in range(1, m.shape[0]):
        if rng.random() < 0.5:
            if m[r, 16] > 0:
                m[r, 16] = F32(rng.uniform(3.0, 20.0))
            else:
                m[r, 0:3] = rng.uniform(0.1, 1.0, 3).astype(F32)
                m[r, 7] = F32(rng.uniform(0.05, 1.0))
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
                    mesh_tex=step["mesh_tex"], tex_by_mat=step["tex_by_mat"], shard=st["shard"] if st else None, wt=st["wt"] if st else 0, geo=_geo[0],
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
        self.seconds = 0.0

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
            op, W, H = step["op"], step["W"], step["H"]
            if op in ("render", "render_device"):
                return self._frame(st, step["cam"], st["mats"], W, H, step["spp"], step["depth"])
            if op in ("render_batch", "render_batch_device"):
                fr = [self._frame(st, cam, st["mats"] if mats is None else mats, W, H, step["spp"], step["depth"]) for cam, mats in step["frames"]]
                return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr])
            assert op in AOV_OPS, op
            S, flat = self.scene(st)
            cam = step["cam"]
            a = aov_ref.aov(S, flat, st["env"], self.orc.to_camera_data(tuple(cam[0]), tuple(cam[1]), tuple(cam[2]), cam[3], W, H).as_array(), W, H, step["n"], materials=st["mats"])
            return np.where(own_mask(st, W, H)[..., None], a, F32(0.0)), None
        finally:
            self.seconds += time.time() - t0


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

    def size(self):
        rng = self.rng
        (w0, w1), (h0, h1) = (SMALL, LARGE, SMALL)[self.sizes] if self.sizes < 3 else ((8, 73), (6, 57))
        self.sizes += 1
        return int(rng.integers(w0, w1)), int(rng.integers(h0, h1))

    def spp(self, W, H, K=1):
        """Depth 1 shows the environment and the emitters only: it is drawn for one frame in ten."""
        i = int(self.rng.integers(0, len(SPP)))
        while i > 0 and W * H * K * SPP[i] > SAMPLE_BUDGET:
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
            return self.set_wt(1 - st["wt"])
        elif b == "box_exact":
            self.add(dict(op="set_option", key="box_exact", value=int(rng.choice([0, 1]))))
        elif b == "knob":
            self.add(dict(op="knob", options=self.knobs[int(rng.integers(0, len(self.knobs)))]))
        elif b == "upload":
            self.k = 0
            self.add(_draw_upload(rng))
        else:
            raise KeyError(b)
        self.render()


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
    if op == "refused":
        return "refused: " + step["what"]
    if op in OBSERVING:
        s = "%s %dx%d" % (op, step["W"], step["H"])
        if op in AOV_OPS:
            s += " n=%d" % step["n"]
        else:
            s += " %d spp depth %d" % (step["spp"], step["depth"])
        if "frames" in step:
            s += " %d frames (table of frame %d NULL)" % (len(step["frames"]), [m is None for _, m in step["frames"]].index(True))
        if op in ASYNC_OPS:
            s += " on %s" % ("the context's stream" if step["stream"] is None else "caller stream %d" % step["stream"])
        return s
    return op


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


def visibility(seq, model):
    """With the oracle alone: (shown, hidden, frames, flat).  A change is VISIBLE if the oracle's output of the next observing step differs
    from what that step shows in the state before the change (the generator puts nothing but a refused call between the two).  shown:
    visible changes per kind of CHANGES; hidden: [(step, kind)]; frames: observing steps; flat: those whose output is one constant pixel."""
    steps, states = seq["steps"], states_of(seq)
    want = {}

    def expected(j):
        if j not in want:
            want[j] = model.expected(states[j], steps[j])
        return want[j]

    shown, hidden, frames, flat = {k: 0 for k in CHANGES}, [], 0, []
    for i, s in enumerate(steps):
        if s["op"] in OBSERVING:
            frames += 1
            a = expected(i)[0]
            if (a == a.reshape(-1, a.shape[-1])[0]).all():
                flat.append(i)
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
    return shown, hidden, frames, flat


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


def refused_call(ctx, st, step, host_only=False):
    what = step["what"]
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


def observe(ctx, step, n_mat, bufs=None, A=None):
    """The observing call.  Blocking: returns (floats, RGBA8 or None).  Asynchronous: enqueues into bufs (a DeviceFrame) and returns None."""
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
    assert op == "render_aov_device", op
    return ctx.render_aov_device(_bcam(step["cam"], W, H), W, H, step["n"], bufs.rgb, stream=stream)


def _device_frame(A, step):
    if step["op"] == "render_aov_device":
        return A.DeviceFrame(step["W"], step["H"], floats=8)
    return A.DeviceFrame(step["W"], step["H"], frames=len(step.get("frames", [0])))


def fresh_agrees(st, step, want):
    """One more comparison after a mismatch: a fresh context, the model's state, the same call (blocking form of it)."""
    ctx = B.Context(0)
    try:
        ctx.set_option("watertight", st["wt"])
        upload(ctx, st)
        if st["shard"]:
            ctx.set_pixel_shard(*st["shard"])
        blocking = dict(step, op={"render_device": "render", "render_batch_device": "render_batch", "render_aov_device": "render_aov"}.get(step["op"], step["op"]))
        got = observe(ctx, blocking, st["mats"].shape[0])
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
    assert host == (A is None)
    where = lambda i: "sequence seed=%d, step %d (%s)" % (seq["seed"], i, describe(steps[i]))
    bufs, pending, got_all = {}, [], []
    t_gpu = 0.0

    def check(i, st, got, want):
        bad = same(got[0], want[0])
        bad8 = same(got[1], want[1]) if want[1] is not None else np.zeros(1, bool)
        if not (bad.any() or bad8.any()):
            return
        verdict = ""
        if diagnose and not host:
            ok = fresh_agrees(st, steps[i], want)
            verdict = ("; a FRESH context in the model's state agrees with the oracle: STALE STATE from the sequence" if ok else
                       "; a fresh context in the model's state differs from the oracle as well: a SINGLE-CALL bug")
        first = tuple(np.argwhere(bad)[0]) if bad.any() else None
        raise AssertionError("%s: %d of %d floats%s differ from the oracle%s%s\ncalls:\n%s" % (
            where(i), bad.sum(), bad.size, "" if want[1] is None else " and %d of %d RGBA8 pixels" % (bad8.sum(), bad8.size),
            "" if first is None else "; first at %s: got %r, want %r" % (first, got[0][first], want[0][first]), verdict, call_list(seq, i + 1)))

    try:
        if not host:  # every caller buffer before anything is enqueued: an allocation or its fill may wait for the device
            for i, s in enumerate(steps):
                if s["op"] in ASYNC_OPS:
                    bufs[i] = _device_frame(A, s)
        st = apply(None, seq["upload"])
        t0 = time.time()
        upload(ctx, st, seq["upload"])
        t_gpu += time.time() - t0
        if host:
            _host_handover(ctx, st, seq["upload"])
        for i, s in enumerate(steps):
            op = s["op"]
            if log:
                log("%3d %s" % (i, describe(s)))
            t0 = time.time()
            if op == "upload":
                new = apply(st, s)
                upload(ctx, new, s)
                if host:
                    _host_handover(ctx, new, s)
            elif op == "update_vertices":
                ctx.update_vertices(update_args(st, s))
                new = apply(st, s)
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
            elif op == "refused":
                refused_call(ctx, st, s, host)
            elif host:
                t_gpu += time.time() - t0
                observe_host(ctx, st, s, model, where(i))
                t0 = time.time()
            elif op in ASYNC_OPS:
                observe(ctx, s, st["mats"].shape[0], bufs[i], A)
                pending.append((i, st))
            else:
                got = observe(ctx, s, st["mats"].shape[0])
                t_gpu += time.time() - t0
                got_all.append((i,) + tuple(got))
                check(i, st, got, model.expected(st, s))
                t0 = time.time()
            t_gpu += time.time() - t0
            st = apply(st, s)
        if pending:
            t0 = time.time()
            ctx.synchronize()  # the one wait of the sequence: everything before it was ordered by the library
            t_gpu += time.time() - t0
            for i, sti in pending:
                rgb, rgba8 = bufs[i].read()
                got = (rgb, None) if steps[i]["op"] == "render_aov_device" else (rgb, rgba8)
                got_all.append((i,) + got)
            for i, sti in pending:
                got = [g for g in got_all if g[0] == i][0][1:]
                check(i, sti, got, model.expected(sti, steps[i]))
    finally:
        if not host:
            try:
                if pending:
                    ctx.synchronize()
            finally:
                for f in bufs.values():
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


# ---------------------------------------------------------------------------------------------------------------------
# the group path: what pt_group_* can express of a sequence
# ---------------------------------------------------------------------------------------------------------------------
def group_projection(seq):
    """The sequence as a pt_group can run it, with option "watertight" = 1 throughout: uploads, update_vertices, set_materials, box_exact
    and the scheduler knobs stay; every single frame becomes a blocking render, every guide pass a blocking one; batches (refused with
    watertight = 1), shards (the group's own business), set_environment (no group call), refusals and the watertight switches go."""
    steps = [dict(op="set_option", key="watertight", value=1)]
    for s in seq["steps"]:
        op = s["op"]
        if op in ("upload", "update_vertices", "set_materials", "knob") or (op == "set_option" and s["key"] == "box_exact"):
            steps.append(s)
        elif op in ("render", "render_device"):
            steps.append(dict(s, op="render", stream=None))
        elif op in AOV_OPS:
            steps.append(dict(s, op="render_aov", stream=None))
    return dict(seed=seq["seed"], host_only=False, upload=seq["upload"], steps=steps)


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
        else:
            assert op in ("render", "render_aov"), op
            out.append((i,) + tuple(observe(target, s, st["mats"].shape[0])))
        st = apply(st, s)
    return out
