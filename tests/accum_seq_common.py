"""A model of ONE accumulation as it lives on a context (include/mi355pt.h: "progressive accumulation", "variance-guided denoise",
"reprojection", "upsampling"), for the directed legs of tests/accum_changes_common.py and the third family of random sequences
(seq_common.draw_accum_sequence; SeqRunner below is its part of seq_common.run()).  It builds on tests/seq_common.py: a STATE is seq_common's dict (the
uploaded scene, current meshes, table, environment, shard, watertight), and the oracle's scenes come from seq_common.Model.

AccumModel keeps, per pixel and in framebuffer order (row 0 = top, as every output of the header): rng, sum, seen, half, n, n_half,
passes, noise; and the camera, size, depth, owned mask and scene fixed at begin, with adds / active_pixels / samples_total.  Nothing the
library returns reaches it.  It implements the header only:
    begin      noise = +inf on owned pixels, everything else 0
    add        accum_ref.select on the model's noise map; oracle.Scene.accumulate over exactly the active launch ids, in the state
               current at THAT add (meshes after updates, table, environment, triangle test), `first` only for the accumulation's first
               add; accum_ref.resolve
    read / info / state / variance   from the model's arrays (denoise_var_ref.accum_variance)
    denoise    denoise_var_ref.denoise_var(read's rgb, variance, guides)
    reproject  accum_reproject_ref.reproject; rng is untouched, seen = sum, the camera is replaced; before the first add only the camera
    end, and refusal(): the reason the header gives for refusing a call in the present state, or None.  A refused call changes nothing.
guides() are tests/aov_ref.py's (pt_render_aov) or tests/aov_follow_ref.py's (pt_render_aov_follow) in a state; denoise_var() and
upsample() are the stateless calls from the caller's own inputs.  A CAMERA is seq_common's view tuple (look_from, look_at, look_up,
vertical fov): the model makes its camera with the oracle's to_camera_data at the accumulation's size."""
import ctypes as C
import functools
import time

import numpy as np

import accum_ref
import accum_reproject_ref
import aov_follow_ref
import aov_ref
import denoise_var_ref
import seq_common as SC
import upsample_ref
from owl_path_tracer_amd.pyhost import binding as B

F32, U32 = np.float32, np.uint32
STATE = ("sum", "half", "n", "n_half", "passes")
READ = ("rgb", "rgba8", "noise", "samples")
MAX_PIXEL_SAMPLES = 2 ** 31 - 65536
oracle_seconds = [0.0]  # spent in the oracle's accumulate and the numpy restatements here (seq_common.Model.seconds has the frames and guides)


def _timed(f):
    @functools.wraps(f)
    def g(*a, **kw):
        t0 = time.time()
        try:
            return f(*a, **kw)
        finally:
            oracle_seconds[0] += time.time() - t0
    return g


def flip(a):
    """framebuffer order <-> launch order: the rows of an (H, W, ...) array the other way round (a contiguous copy)"""
    return np.ascontiguousarray(a[::-1])


def orbit(view, deg):
    """The view after an orbit of `deg` degrees about the vertical through look_at (accum_reproject_common.pair's "orbit")."""
    from accum_reproject_common import rot_y

    frm, at, up, fov = view
    frm, at = np.asarray(frm, np.float64), np.asarray(at, np.float64)
    return [float(x) for x in at + rot_y(frm - at, deg)], [float(x) for x in at], list(up), fov


class AccumModel:
    def __init__(self, orc, model):
        self.orc, self.model, self.live = orc, model, None

    # ---- the oracle's side of a state ----
    def camera(self, view, W, H):
        return self.orc.to_camera_data(tuple(view[0]), tuple(view[1]), tuple(view[2]), view[3], W, H)

    def guides(self, st, view, W, H, n=1, follow=None):
        """pt_render_aov at n samples in state st; follow = dict(max_follow, roughness_max): pt_render_aov_follow."""
        S, flat = self.model.scene(st)
        cam = self.camera(view, W, H).as_array()
        if follow is None:
            a = aov_ref.aov(S, flat, st["env"], cam, W, H, n, materials=st["mats"])
        else:
            a = aov_follow_ref.aov(S, flat, st["env"], cam, W, H, n, follow["max_follow"], follow["roughness_max"], materials=np.asarray(st["mats"], F32))
        return np.where(SC.own_mask(st, W, H)[..., None], a, F32(0.0)).astype(F32)

    # ---- refusals ----
    def refusal(self, st, call, n_samples=16, cap=0, thr=0.0, reserved=0):
        """Why the header refuses `call` (begin is never refused here; add, read, info, state, variance, denoise, reproject) in state st."""
        a = self.live
        if call == "add" and (not 1 <= n_samples <= 65535 or cap < 0 or not thr >= 0.0 or reserved != 0):
            return "bad parameters"
        if a is None:
            return "no accumulation"
        if call in ("add", "reproject"):
            if tuple(st["shard"] or ()) != a["shard"]:
                return "the pixel shard changed"
            if st["scene"] is not a["scene"]:
                return "a new scene was uploaded"
        if call == "add" and a["n_upper"] + n_samples > MAX_PIXEL_SAMPLES:
            return "sample limit"
        if call == "denoise" and not a["owned"].all():
            return "the shard does not own the whole frame"
        return None

    # ---- the calls ----
    def begin(self, st, view, W, H, depth):
        own = SC.own_mask(st, W, H)
        z3, z = np.zeros((H, W, 3), F32), np.zeros((H, W), U32)
        self.live = dict(view=view, W=W, H=H, depth=depth, owned=own, shard=tuple(st["shard"] or ()), scene=st["scene"], adds=0, active_pixels=0, samples_total=0, n_upper=0,
                         rng=z.copy(), sum=z3.copy(), seen=z3.copy(), half=z3.copy(), n=z.copy(), n_half=z.copy(), passes=z.copy(),
                         noise=np.where(own, F32(np.inf), F32(0.0)).astype(F32), rgb=z3.copy(), rgba8=z.copy())

    def active(self, cap=0, thr=0.0):
        a = self.live
        return accum_ref.select(a["noise"], a["n"], a["owned"], cap, thr).astype(bool)

    @_timed
    def add(self, st, n_samples, cap=0, thr=0.0):
        """-> (rgb, rgba8) of the frame so far"""
        a = self.live
        assert self.refusal(st, "add", n_samples, cap, thr) is None
        W, H = a["W"], a["H"]
        act = self.active(cap, thr)
        ids = np.flatnonzero(flip(act).ravel()).astype(U32)  # launch ids x + W*y of the active set
        rng, sum_ = flip(a["rng"]).reshape(-1), flip(a["sum"]).reshape(-1)
        if ids.size:
            S, _ = self.model.scene(st)
            S.set_materials(np.asarray(st["mats"], F32))
            S.accumulate(self.camera(a["view"], W, H), self.orc.make_env(**st["env"]), W, H, n_samples, a["depth"], rng, sum_, pixel_list=ids, first=a["adds"] == 0)
        a["rng"], a["sum"] = flip(rng.reshape(H, W)), flip(sum_.reshape(H, W, 3))
        r = accum_ref.resolve(a["sum"], a["seen"], a["half"], a["n"], a["n_half"], a["passes"], act, a["owned"], n_samples)
        a.update(r)
        a["adds"] += 1
        a["active_pixels"] = int(act.sum())
        a["samples_total"] += int(act.sum()) * n_samples
        a["n_upper"] += n_samples
        return a["rgb"], a["rgba8"]

    def read(self):
        a = self.live
        return dict(rgb=a["rgb"], rgba8=a["rgba8"], noise=a["noise"], samples=a["n"])

    def state(self):
        """pt_debug_accum_state: +0 outside the shard"""
        a = self.live
        return {k: np.where(a["owned"][..., None] if a[k].ndim == 3 else a["owned"], a[k], a[k].dtype.type(0)) for k in STATE}

    def info(self):
        a = self.live
        return dict(width=a["W"], height=a["H"], max_path_depth=a["depth"], adds=a["adds"], owned_pixels=int(a["owned"].sum()), active_pixels=a["active_pixels"],
                    samples_total=a["samples_total"])

    @_timed
    def variance(self):
        a = self.live
        rgb, var = denoise_var_ref.accum_variance(a["sum"], a["half"], a["n"], a["n_half"], a["owned"])
        return var.reshape(a["H"], a["W"], 3)

    @_timed
    def denoise(self, aov, **params):
        """pt_accum_denoise -> (rgb, rgba8); the state is not touched"""
        a = self.live
        var = denoise_var_ref.accum_variance(a["sum"], a["half"], a["n"], a["n_half"], a["owned"])[1].reshape(a["H"], a["W"], 3)
        out, out8, _ = denoise_var_ref.denoise_var(a["rgb"], var, aov, **params)
        return out, out8

    @_timed
    def reproject(self, st, new_view, aov_prev, aov_cur, **params):
        """-> the share of owned pixels that keep history (None before the first add, which only changes the camera)"""
        a = self.live
        assert self.refusal(st, "reproject") is None
        W, H = a["W"], a["H"]
        if a["adds"] == 0:
            a["view"] = new_view
            return None
        r = accum_reproject_ref.reproject(self.camera(a["view"], W, H).as_array(), self.camera(new_view, W, H).as_array(), aov_prev, aov_cur, {k: a[k] for k in STATE},
                                          None if a["owned"].all() else a["owned"].astype(np.uint8), **params)
        has = r.pop("has")
        a.update(r)
        a["seen"] = a["sum"]
        a["view"] = new_view
        return float(has[a["owned"]].mean())

    def end(self):
        self.live = None


@_timed
def denoise_var(rgb, var, aov, **params):
    """pt_denoise_var from the caller's own inputs -> (rgb, rgba8)"""
    out, out8, _ = denoise_var_ref.denoise_var(rgb, var, aov, **params)
    return out, out8


@_timed
def upsample(rgb_lo, aov_lo, aov_hi, **params):
    """pt_upsample from the caller's own inputs -> (rgb, rgba8)"""
    return upsample_ref.upsample(rgb_lo, aov_lo, aov_hi, **params)


# ---- comparisons with a context ----
def snapshot(ctx):
    """What a context shows of its accumulation: pt_debug_accum_state and pt_accum_read"""
    rd, st = ctx.accum_read(), ctx.accum_state()
    return dict(st, **rd)


def first_difference(ctx, am):
    """The first array of pt_debug_accum_state / pt_accum_read / pt_accum_info_get that differs from the model: (name, how many entries), or None."""
    got = snapshot(ctx)
    want = dict(am.state(), **am.read())
    for k in STATE + READ:
        bad = SC.same(got[k], want[k])
        if bad.any():
            return k, int(bad.sum()), int(bad.size)
    gi, wi = ctx.accum_info(), am.info()
    for k in wi:
        if gi[k] != wi[k]:
            return "info." + k, gi[k], wi[k]
    return None


def assert_accum(ctx, am, what):
    d = first_difference(ctx, am)
    assert d is None, "%s: %s differs from the model (%s of %s)" % (what, d[0], d[1], d[2])


# ---- the same calls on a context and on the model ----
class Both:
    """Every call goes to the model and - where there is one - to a device context, and every blocking call is compared at once: the
    call's own outputs, then pt_debug_accum_state, pt_accum_read and pt_accum_info_get (assert_accum).  ctx None: the model alone, which is
    how the CPU conditions of a leg are checked without a device.  twin: a host-only context; then every step of the model is also held
    through the library's CPU twins applied to the model's arrays BEFORE the step (select, resolve, reproject, variance, denoise_var,
    upsample): twin output must equal the model after the step, bit for bit.  self.st is seq_common's state, self.am the AccumModel."""

    def __init__(self, orc, ctx, up, twin=None, model=None):
        """up: the upload step, which goes to the context; None: the caller has uploaded, and sets self.st before every call (seq_common.run)."""
        self.orc, self.ctx, self.twin = orc, ctx, twin
        self.model = model or SC.Model(orc)
        self.am = AccumModel(orc, self.model)
        self.st = SC.apply(None, up) if up is not None else None
        self.calls = []
        self.last_threshold = 0.0
        if ctx is not None and up is not None:
            ctx.set_option("watertight", 0)
            ctx.set_pixel_shard(0, 1, 16)
            SC.upload(ctx, self.st, up)

    def where(self):
        return "after [" + ", ".join(self.calls) + "]"

    def bcam(self, view):
        return SC._bcam(view, self.am.live["W"], self.am.live["H"])

    def same(self, got, want, what):
        bad = SC.same(got, want)
        assert not bad.any(), "%s %s: %d of %d entries differ from the model" % (what, self.where(), int(bad.sum()), bad.size)

    # -- changes --
    def change(self, step):
        """A change step of seq_common (update_vertices, set_materials, set_environment, set_pixel_shard, set_option, knob, upload)."""
        ctx, st, op = self.ctx, self.st, step["op"]
        self.calls.append(SC.describe(step))
        new = SC.apply(st, step)
        if ctx is not None:
            if op == "upload":
                SC.upload(ctx, new, step)
            elif op == "update_vertices":
                ctx.update_vertices(SC.update_args(st, step))
            elif op == "set_materials":
                ctx.set_materials(step["mats"])
            elif op == "set_environment":
                ctx.set_environment(B.make_env(**step["env"]))
            elif op == "set_pixel_shard":
                ctx.set_pixel_shard(*(step["shard"] or (0, 1, 16)))
            elif op == "set_option":
                ctx.set_option(step["key"], step["value"])
            else:
                assert op == "knob", op
                for k, v in step["options"]:
                    ctx.set_option(k, v)
        self.st = new

    def restore_vertices(self, meshes):
        """pt_update_vertices back to the given meshes (vertices and normals of every mesh)."""
        self.calls.append("update_vertices back")
        if self.ctx is not None:
            self.ctx.update_vertices([dict(vertices=m["vertices"], normals=m["normals"]) for m in meshes])
        SC._geo[0] += 1
        self.st = dict(self.st, meshes=list(meshes), geo=SC._geo[0])

    # -- the accumulation --
    def begin(self, view, W, H, depth):
        self.calls.append("begin %dx%d depth %d" % (W, H, depth))
        self.am.begin(self.st, view, W, H, depth)
        if self.ctx is not None:
            self.ctx.accum_begin(SC._bcam(view, W, H), W, H, depth)
            assert_accum(self.ctx, self.am, self.where())

    def threshold(self):
        """The median of the model's finite positive noise, as a float32"""
        z = self.am.live["noise"]
        z = z[np.isfinite(z) & (z > 0)]
        self.last_threshold = float(F32(np.median(z))) if z.size else 1.0  # (no finite noise, as after a cap that leaves n_half = 0: every pixel is active whatever the threshold)
        return self.last_threshold

    def add(self, n, cap=0, thr=0.0):
        """-> pt_get_stats after the add (None without a context)"""
        am, a = self.am, self.am.live
        self.calls.append("add %d%s%s" % (n, ", cap %d" % cap if cap else "", ", threshold %r" % thr if thr else ""))
        before = {k: a[k] for k in ("seen", "half", "n", "n_half", "passes", "noise")}
        act = am.active(cap, thr)
        rgb, rgba8 = am.add(self.st, n, cap, thr)
        if self.twin is not None:
            prm = B.accum_default_params(n_samples=n, max_pixel_samples=cap, noise_threshold=thr)
            got, count = self.twin.accum_select_host(before["noise"], before["n"], a["owned"], prm)
            assert count == act.sum() and (got.reshape(act.shape) != 0).tolist() == act.tolist(), "pt_debug_accum_select_host " + self.where()
            r = self.twin.accum_resolve_host(a["sum"].reshape(-1, 3), before["seen"].reshape(-1, 3), before["half"].reshape(-1, 3), before["n"].ravel(), before["n_half"].ravel(),
                                             before["passes"].ravel(), act.ravel(), a["owned"].ravel(), n)
            for k in ("seen", "half", "n", "n_half", "passes", "rgb", "rgba8", "noise"):
                self.same(r[k].reshape(a[k].shape), a[k], "pt_debug_accum_resolve_host's " + k)
        if self.ctx is None:
            return None
        got, got8 = self.ctx.accum_add(B.accum_default_params(n_samples=n, max_pixel_samples=cap, noise_threshold=thr), want_rgba8=True)
        stats = self.ctx.stats()
        self.same(got, rgb, "pt_accum_add's image")
        self.same(got8, rgba8, "pt_accum_add's RGBA8 image")
        assert_accum(self.ctx, am, self.where())
        assert (stats["launches"] == 0) == (not act.any()), "%s: %d launches for %d active pixels" % (self.where(), stats["launches"], int(act.sum()))
        return stats

    def guides(self, view, W=None, H=None, n=1, follow=None):
        """The model's guide buffers in the present state; with a context, pt_render_aov / pt_render_aov_follow must return the same."""
        a = self.am.live
        W, H = (a["W"], a["H"]) if W is None else (W, H)
        want = self.am.guides(self.st, view, W, H, n, follow)
        if self.ctx is not None:
            cam = SC._bcam(view, W, H)
            got = self.ctx.render_aov(cam, W, H, n) if follow is None else self.ctx.render_aov_follow(cam, W, H, B.aov_default_params(n_samples=n, **follow))
            self.same(got, want, "the guide pass")
        return want

    def reproject(self, new_view, prev, cur, **params):
        """-> the share of owned pixels that keep history"""
        am, a = self.am, self.am.live
        self.calls.append("reproject %s" % (params or ""))
        before, old_view = {k: a[k] for k in STATE}, a["view"]
        moved = a["adds"] > 0
        share = am.reproject(self.st, new_view, prev, cur, **params)
        prm = B.reproject_default_params(**params)
        if self.twin is not None and moved:
            r = self.twin.accum_reproject_host(self.bcam(old_view), self.bcam(new_view), prev, cur, before, None if a["owned"].all() else a["owned"], prm)
            for k in STATE + ("rgb", "rgba8", "noise"):
                self.same(r[k], a[k], "pt_debug_accum_reproject_host's " + k)
        if self.ctx is not None:
            self.ctx.accum_reproject(self.bcam(new_view), prev, cur, prm)
            assert_accum(self.ctx, am, self.where())
        return share

    def variance(self):
        a = self.am.live
        want = self.am.variance()
        if self.twin is not None:
            rgb, var = self.twin.accum_variance_host(a["sum"], a["half"], a["n"], a["n_half"], a["owned"])
            self.same(var.reshape(want.shape), want, "pt_debug_accum_variance_host")
            self.same(rgb.reshape(want.shape), a["rgb"], "pt_debug_accum_variance_host's image")
        if self.ctx is not None:
            self.same(self.ctx.accum_variance(), want, "pt_accum_variance")
        return want

    def denoise(self, aov, **params):
        self.calls.append("accum_denoise %s" % (params or ""))
        want, want8 = self.am.denoise(aov, **params)
        prm = B.denoise_var_default_params(**params)
        if self.twin is not None:
            got, got8, _ = self.twin.denoise_var_host(self.am.live["rgb"], self.variance(), aov, prm, want_rgba8=True)
            self.same(got, want, "pt_debug_denoise_var_host")
            self.same(got8, want8, "pt_debug_denoise_var_host's RGBA8 image")
        if self.ctx is not None:
            got, got8 = self.ctx.accum_denoise(aov, prm, want_rgba8=True)
            self.same(got, want, "pt_accum_denoise")
            self.same(got8, want8, "pt_accum_denoise's RGBA8 image")
            assert_accum(self.ctx, self.am, self.where())
        return want, want8

    def upsample(self, rgb_lo, aov_lo, aov_hi, **params):
        self.calls.append("upsample %s" % (params or ""))
        want, want8 = upsample(rgb_lo, aov_lo, aov_hi, **params)
        prm = B.upsample_default_params(**params)
        for who, c in (("pt_debug_upsample_host", self.twin), ("pt_upsample", self.ctx)):
            if c is not None:
                got, got8 = (c.upsample_host if c is self.twin else c.upsample)(rgb_lo, aov_lo, aov_hi, prm, want_rgba8=True)
                self.same(got, want, who)
                self.same(got8, want8, who + "'s RGBA8 image")
        return want, want8

    def refused(self, call, fn):
        """fn makes a call on the context that the header refuses in the present state: PT_E_INVALID, and the accumulation as it was."""
        self.calls.append("refused " + call)
        assert self.am.refusal(self.st, call) is not None, call
        if self.ctx is not None:
            SC.expect_refusal(fn, call + " " + self.where())
            if self.am.live is not None:
                assert_accum(self.ctx, self.am, self.where())

    def end(self):
        self.calls.append("end")
        self.am.end()
        if self.ctx is not None:
            self.ctx.accum_end()


# ---- the third family of random sequences (seq_common.draw_accum_sequence) inside seq_common.run() ----
POISON = np.uint32(0xA5A5A5A5)  # async_common.DeviceFrame's fill


def step_inputs(model, st, s):
    """The model's own inputs of a step (host arrays): guides, frames, the variance map."""
    op = SC.BLOCKING_OF_ACCUM.get(s["op"], s["op"])
    e = lambda x: model.expected(st, x)[0]
    if op == "accum_denoise":
        return dict(aov=e(s["guides"]))
    if op == "accum_reproject":
        return dict(prev=e(s["prev"]), cur=e(s["cur"]))
    if op == "denoise_var":
        from denoise_var_common import var_map

        return dict(rgb=e(s["src"]["render"]), var=var_map(s["W"], s["H"], s["var_seed"]), aov=e(s["src"]["guides"]))
    if op == "upsample":
        return dict(rgb_lo=None if s["chain"] else e(s["src"]["render"]), aov_lo=e(s["src"]["guides"]), aov_hi=e(s["src"]["guides_hi"]))
    return {}


def refused_step(b, s, st, host_ctx=None):
    """A refused call of the third family: PT_E_INVALID on a device context and on a host-only one, and the accumulation as it was."""
    what, ctx = s["what"], b.ctx if b.ctx is not None else host_ctx
    am = b.am
    b.calls.append("refused " + what)
    L, fp, byref = B.lib(), lambda a: a.ctypes.data_as(C.POINTER(C.c_float)), C.byref
    if what == "accum_bad_params":
        bad = [dict(n_samples=0), dict(n_samples=65536), dict(max_pixel_samples=-1), dict(noise_threshold=float("nan")), dict(reserved=3)]
        calls = [("pt_accum_add %r" % kw, (lambda kw=kw: L.pt_accum_add(ctx._h, byref(B.accum_default_params(**kw)), None, None))) for kw in bad]
        assert am.refusal(st, "add", n_samples=0) == "bad parameters"
    elif what in ("accum_after_shard", "accum_after_upload"):
        a = am.live
        assert am.refusal(st, "add") in ("the pixel shard changed", "a new scene was uploaded") and am.refusal(st, "reproject") is not None, what
        g = np.zeros((a["H"], a["W"], 8), F32)
        cam = SC._bcam(a["view"], a["W"], a["H"])
        calls = [("pt_accum_add", lambda: L.pt_accum_add(ctx._h, None, None, None)), ("pt_accum_add_device", lambda: L.pt_accum_add_device(ctx._h, None, None, None, None)),
                 ("pt_accum_reproject", lambda: L.pt_accum_reproject(ctx._h, byref(cam), fp(g), fp(g), None))]
    else:
        assert what == "accum_no_accum" and am.live is None and am.refusal(st, "read") == "no accumulation"
        out = np.zeros((4, 4, 3), F32)
        calls = [("pt_accum_add", lambda: L.pt_accum_add(ctx._h, None, None, None)), ("pt_accum_read", lambda: L.pt_accum_read(ctx._h, fp(out), None, None, None)),
                 ("pt_accum_variance", lambda: L.pt_accum_variance(ctx._h, fp(out))), ("pt_accum_denoise", lambda: L.pt_accum_denoise(ctx._h, fp(out), None, fp(out), None))]
    if ctx is None:
        return
    for name, call in calls:
        rc = int(call())
        # (a host-only context holds no accumulation: it judges pt_accum_reproject's arguments alone and answers PT_E_NO_DEVICE to valid ones)
        code = -2 if (b.ctx is None and name == "pt_accum_reproject") else -1
        assert rc == code, "%s %s: returned %d, not %d (%s)" % (name, b.where(), rc, code, L.pt_last_error(ctx._h).decode())
    if b.ctx is not None and am.live is not None:
        assert_accum(b.ctx, am, b.where())


def step_blocking(b, model, s, st, outs, i, host_ctx=None):
    """Step s (an op of seq_common.ACCUM_OPS in its blocking form, or a refused call) on a Both: the model, and its context or twin.  outs[i] =
    the model's output of the step, which a chained step after it reads.  host_ctx: a host-only context, which must answer PT_E_NO_DEVICE
    to valid begin and reproject calls and holds no accumulation."""
    b.st = st
    op = SC.BLOCKING_OF_ACCUM.get(s["op"], s["op"])
    inp = step_inputs(model, st, s)
    if op == "refused":
        return refused_step(b, s, st, host_ctx)
    if op == "accum_begin":
        if host_ctx is not None:
            cam = SC._bcam(s["cam"], s["W"], s["H"])
            rc = B.lib().pt_accum_begin(host_ctx._h, C.byref(cam), s["W"], s["H"], s["depth"])
            assert rc == -2, "pt_accum_begin on a host-only context returned %d, not PT_E_NO_DEVICE" % rc
        return b.begin(s["cam"], s["W"], s["H"], s["depth"])
    if op == "accum_add":
        outs[i] = None
        b.add(s["n"], s["cap"], b.threshold() if s["select"] else 0.0)
        outs[i] = (b.am.live["rgb"], b.am.live["rgba8"])
    elif op == "accum_read":
        b.calls.append("read")
        if b.ctx is not None:
            assert_accum(b.ctx, b.am, b.where())
    elif op == "accum_variance":
        b.calls.append("variance")
        outs[i] = (b.variance(), None)
    elif op == "accum_denoise":
        outs[i] = b.denoise(inp["aov"], **s["params"])
    elif op == "accum_reproject":
        if host_ctx is not None and b.am.live is not None:
            fp = C.POINTER(C.c_float)
            cam = SC._bcam(s["cam"], s["W"], s["H"])
            rc = B.lib().pt_accum_reproject(host_ctx._h, C.byref(cam), inp["prev"].ctypes.data_as(fp), inp["cur"].ctypes.data_as(fp), C.byref(B.reproject_default_params(max_history=s["cap"])))
            assert rc == -2, "pt_accum_reproject on a host-only context returned %d, not PT_E_NO_DEVICE" % rc
        outs[i] = (b.reproject(s["cam"], inp["prev"], inp["cur"], max_history=s["cap"]), None)
    elif op == "accum_end":
        b.end()
    elif op == "denoise_var":
        b.calls.append("denoise_var")
        want = denoise_var(inp["rgb"], inp["var"], inp["aov"], **s["params"])
        prm = B.denoise_var_default_params(**s["params"])
        for who, c in (("pt_debug_denoise_var_host", b.twin), ("pt_denoise_var", b.ctx)):
            if c is not None:
                got = (c.denoise_var_host if c is b.twin else c.denoise_var)(inp["rgb"], inp["var"], inp["aov"], prm, want_rgba8=True)
                b.same(got[0], want[0], who)
                b.same(got[1], want[1], who + "'s RGBA8 image")
        outs[i] = want
    else:
        assert op == "upsample", op
        rgb_lo = outs[i - 1][0] if s["chain"] else inp["rgb_lo"]
        outs[i] = b.upsample(rgb_lo, inp["aov_lo"], inp["aov_hi"], **s["params"])


class SeqRunner:
    """The steps of the third family inside seq_common.run().  Blocking steps go through step_blocking at once (the call's outputs, then
    state, read-back and info).  Asynchronous steps run on the model at once and are enqueued on the context with nothing in between; their
    caller buffers - allocated, and the model's own inputs copied to HBM, before the first step - are read back by finish() after run()'s
    one pt_synchronize, together with a final comparison of the state.  On a host-only context every step is step_blocking's through the
    library's CPU twins."""

    def __init__(self, ctx, model, A, host, seq, steps, states, bufs, where):
        self.ctx, self.model, self.A, self.host, self.seq, self.steps, self.states, self.bufs, self.where = ctx, model, A, host, seq, steps, states, bufs, where
        self.both = Both(model.orc, None if host else ctx, None, twin=ctx if host else None, model=model)
        self.outs, self.pending, self.mine, self.seconds = {}, [], {}, 0.0

    def prepare(self):
        """Every caller buffer of the asynchronous steps, and the model's own inputs in HBM, before anything is enqueued."""
        A = self.A
        for i, s in enumerate(self.steps):
            op = s["op"]
            if op not in SC.ACCUM_ASYNC and not (op == "refused" and s["what"] in SC.ACCUM_REFUSED):
                continue
            m = self.mine[i] = {}
            if op == "refused":
                continue
            W, H = s["W"], s["H"]
            if op != "accum_reproject_device":
                m["out"] = A.DeviceFrame(W, H)
            inp = step_inputs(self.model, self.states[i], s)
            keys = {"accum_denoise_device": () if s.get("chain") else ("aov",), "accum_reproject_device": ("prev",), "denoise_var_device": ("rgb", "var", "aov"),
                    "upsample_device": ("aov_hi",) if s.get("chain") else ("rgb_lo", "aov_lo", "aov_hi")}.get(op, ())
            for k in keys:
                a = inp[k]
                m[k] = A.DeviceFrame(a.shape[1], a.shape[0], floats=a.shape[2])
                A.to_device(m[k].rgb, a)

    def frames(self):
        return [f for m in self.mine.values() for f in m.values()]

    def step(self, i):
        s, st, b = self.steps[i], self.states[i], self.both
        try:
            self._step(i, s, st, b)
        except AssertionError as e:
            verdict = ""
            if not self.host:
                ok = replay_alone(self.model.orc, self.seq, i + 1)
                verdict = ("; a FRESH context given the scene changes and the accumulation calls alone agrees with the model: STALE STATE from the other calls of the sequence" if ok else
                           "; a fresh context given the scene changes and the accumulation calls alone differs from the model as well")
            raise AssertionError("%s: %s%s\ncalls:\n%s" % (self.where(i), e, verdict, SC.call_list(self.seq, i + 1)))

    def _step(self, i, s, st, b):
        op, ctx = s["op"], self.ctx
        if self.host or op not in SC.ACCUM_ASYNC:
            t0, o0 = time.time(), self.model.seconds
            step_blocking(b, self.model, s, st, self.outs, i, host_ctx=ctx if self.host else None)
            self.seconds += time.time() - t0 - (self.model.seconds - o0)
            return
        dev, b.ctx = b.ctx, None  # the model's side of the step first: a blocking call on the context would synchronize
        try:
            step_blocking(b, self.model, s, st, self.outs, i)
        finally:
            b.ctx = dev
        t0 = time.time()
        m, A = self.mine[i], self.A
        stream = A.stream(s["stream"]) if s["stream"] is not None else None
        out8 = lambda: m["out"].rgba8 if s.get("want_rgba8") else None
        if op == "accum_add_device":
            thr = b.last_threshold if s["select"] else 0.0
            prm = B.accum_default_params(n_samples=s["n"], max_pixel_samples=s["cap"], noise_threshold=thr)
            ctx.accum_add_device(prm, m["out"].rgb if s["want"] else None, m["out"].rgba8 if s["want"] else None, stream=stream)
            want = self.outs[i] if s["want"] else (None, None)
        elif op == "accum_denoise_device":
            d_aov = self.bufs[i - 1].rgb if s["chain"] else m["aov"].rgb
            ctx.accum_denoise_device(d_aov, m["out"].rgb, B.denoise_var_default_params(**s["params"]), d_out_rgba8=out8(), stream=stream)
            want = (self.outs[i][0], self.outs[i][1] if s["want_rgba8"] else None)
        elif op == "accum_reproject_device":
            ctx.accum_reproject_device(SC._bcam(s["cam"], s["W"], s["H"]), m["prev"].rgb, self.bufs[i - 1].rgb, B.reproject_default_params(max_history=s["cap"]), stream=stream)
            want = None
        elif op == "denoise_var_device":
            ctx.denoise_var_device(m["rgb"].rgb, m["var"].rgb, m["aov"].rgb, s["W"], s["H"], m["out"].rgb, B.denoise_var_default_params(**s["params"]), d_out_rgba8=out8(), stream=stream)
            want = (self.outs[i][0], self.outs[i][1] if s["want_rgba8"] else None)
        else:
            assert op == "upsample_device", op
            d_lo, d_aov_lo = (self.mine[i - 1]["out"].rgb, self.bufs[i - 2].rgb) if s["chain"] else (m["rgb_lo"].rgb, m["aov_lo"].rgb)
            ctx.upsample_device(d_lo, d_aov_lo, s["w"], s["h"], m["aov_hi"].rgb, s["W"], s["H"], m["out"].rgb, B.upsample_default_params(**s["params"]), d_out_rgba8=out8(), stream=stream)
            want = (self.outs[i][0], self.outs[i][1] if s["want_rgba8"] else None)
        self.seconds += time.time() - t0
        if want is not None:
            self.pending.append((i, want))

    def finish(self):
        """After run()'s pt_synchronize: the asynchronous steps' buffers, the buffers nobody was to write, the final state."""
        for i, (want, want8) in self.pending:
            got, got8 = self.mine[i]["out"].read()
            for g, w, name in ((got, want, "floats"), (got8, want8, "RGBA8 pixels")):
                if w is None:
                    assert (g.view(np.uint32) == POISON).all(), "%s: the call wrote to a buffer that is not its own (%s)" % (self.where(i), name)
                else:
                    bad = SC.same(g, w)
                    assert not bad.any(), "%s: %d of %d %s differ from the model\ncalls:\n%s" % (self.where(i), int(bad.sum()), bad.size, name, SC.call_list(self.seq, i + 1))
        for i, m in self.mine.items():
            for k, f in m.items():
                if k != "out":  # inputs: their RGBA8 halves were never anybody's
                    assert (f.read()[1] == POISON).all(), "%s: a call wrote to the RGBA8 half of an input buffer" % self.where(i)
        if not self.host and self.both.am.live is not None:
            d = first_difference(self.ctx, self.both.am)
            assert d is None, "%ssequence seed=%d, final state: %s differs from the model (%s of %s)\ncalls:\n%s" % (
                self.seq.get("family", "") + " ", self.seq["seed"], d[0], d[1], d[2], SC.call_list(self.seq))


def replay_alone(orc, seq, upto):
    """A fresh context, the scene changes of seq["steps"][:upto] and its accumulation calls alone (blocking forms, the model's own guides):
    True if everything agrees with the model."""
    ctx = B.Context(0)
    try:
        model = SC.Model(orc)
        states = SC.states_of(dict(seq, steps=seq["steps"][:upto]))
        b = Both(orc, ctx, seq["upload"], model=model)
        outs = {}
        for i, s in enumerate(seq["steps"][:upto]):
            if s["op"] in SC.ACCUM_OPS[:10]:
                step_blocking(b, model, s, states[i], outs, i)
            elif s["op"] not in SC.OBSERVING and s["op"] != "refused":
                b.st = states[i]
                b.change(s)
        return True
    except (AssertionError, B.PtError):
        return False
    finally:
        ctx.close()


def model_run(seq, model, skip=None):
    """The sequence on the model alone (no context, no twin); skip: the index of a step that is left out.  -> dict(sums = {index of an add:
    the model's sums after it}, shares = [(index of a reproject, share of the owned pixels that keep history)])."""
    steps = [dict(op="knob", options=()) if i == skip else s for i, s in enumerate(seq["steps"])]
    states = SC.states_of(dict(seq, steps=steps))
    b = Both(model.orc, None, None, model=model)
    outs, sums, shares = {}, {}, []
    for i, s in enumerate(steps):
        if s["op"] in SC.ACCUM_OPS:
            step_blocking(b, model, s, states[i], outs, i)
            if s["op"] in ("accum_add", "accum_add_device"):
                sums[i] = b.am.live["sum"]
            if s["op"] in ("accum_reproject", "accum_reproject_device"):
                shares.append((i, outs[i][0]))
    return dict(sums=sums, shares=shares)


def visibility(seq, model):
    """With the oracle alone: (shown, hidden, shares).  A change between two adds of an accumulation is VISIBLE if the model's sums after the
    next add differ from those of the same sequence without the change.  shown: visible changes per kind; hidden: [(step, kind)]; shares: model_run's."""
    base = model_run(seq, model)
    shown, hidden = {k: 0 for k in SC.ACCUM_CHANGES}, []
    steps = seq["steps"]
    for i, s in enumerate(steps):
        kind = SC.kind_of(s)
        if kind not in SC.ACCUM_CHANGES:
            continue
        k = next(j for j in range(i + 1, len(steps)) if steps[j]["op"] in ("accum_add", "accum_add_device", "accum_begin"))
        if steps[k]["op"] == "accum_begin":
            continue  # (not between two adds of one accumulation)
        alt = model_run(seq, model, skip=i)
        if SC.same(base["sums"][k], alt["sums"][k]).any():
            shown[kind] += 1
        else:
            hidden.append((i, kind))
    return shown, hidden, base["shares"]


def coverage(seqs):
    """What sequences of the third family contain between them; tests/test_sequences_host.py asserts the issue's conditions on it."""
    cov = dict(ops={o: 0 for o in SC.ACCUM_OPS}, streams=set(), change_then_add={k: 0 for k in SC.ACCUM_CHANGES}, knob_then_selecting_add=0, caps=set(), reprojects_in_one=0, async_chains=0,
               blocking_chains=0, add_sizes=set(), refused=set(), begin_over_live=0, growth_and_shrink=0, between=0, selecting=0)
    for seq in seqs:
        steps, px, grow, shrink, reprojects, adds = seq["steps"], None, 0, 0, 0, 0
        for i, s in enumerate(steps):
            op = s["op"]
            nxt = [t["op"] for t in steps[i + 1:i + 4]]
            if op in SC.ACCUM_OPS:
                cov["ops"][op] += 1
            if op in SC.ACCUM_ASYNC:
                cov["streams"].add(s["stream"])
            kind = SC.kind_of(s)
            if kind in SC.ACCUM_CHANGES and (nxt[:1] in (["accum_add"], ["accum_add_device"]) or (kind == "watertight" and nxt[0] in SC.FOLLOW_OPS and nxt[1] in ("accum_add", "accum_add_device"))):
                cov["change_then_add"][kind] += 1
            if op == "knob" and nxt and nxt[0] in ("accum_add", "accum_add_device") and steps[i + 1]["select"]:
                cov["knob_then_selecting_add"] += 1
            if op == "accum_begin":
                now = s["W"] * s["H"]
                if px is not None:
                    grow += now >= 4 * px
                    shrink += 4 * now <= px
                px, reprojects, adds = now, 0, 0
                cov["begin_over_live"] += bool(s["over_live"])
            if op in ("accum_reproject", "accum_reproject_device"):
                cov["caps"].add(s["cap"])
                reprojects += 1
                cov["reprojects_in_one"] += reprojects == 2
            if op in ("accum_add", "accum_add_device"):
                cov["add_sizes"].add(s["n"])
                cov["selecting"] += bool(s["select"])
                if steps[i - 1]["op"] in SC.OBSERVING and adds:  # a call of another family right before an add that continues
                    cov["between"] += 1
                adds += 1
            if op in ("upsample", "upsample_device") and s["chain"]:
                chain = steps[i - 3:i + 1]
                assert [c["op"] in SC.ASYNC_OPS + SC.ACCUM_ASYNC for c in chain] in ([True] * 4, [False] * 4) and len({c["stream"] for c in chain}) == 1, (seq["seed"], i)
                cov["async_chains" if op == "upsample_device" else "blocking_chains"] += 1
            if op == "refused":
                cov["refused"].add(s["what"])
        cov["growth_and_shrink"] += grow >= 1 and shrink >= 1
    return cov
