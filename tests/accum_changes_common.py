"""The legs of tests/test_gpu_accum_changes.py (a device context) and tests/test_accum_changes_host.py (the model alone, held through the
library's CPU twins): an accumulation that lives through scene changes, scheduler knobs, camera moves and refusals, every step on the
model of tests/accum_seq_common.py and - where there is one - on the context, compared bit for bit after every blocking call.

SCENES are the sequence generator's lit room with its sphere and the sliver mesh (seq_common._draw_upload(guide=True)): MAIN has a metal
sphere under an environment map, at scale 1.9 away from the origin; GLASS a glass sphere under the automatic sky at scale 0.16.  The VIEW
looks at the sphere from 1.2 scene units: it fills about a third of the frame, which is where the two triangle tests differ (flat walls
give the same frame under both).  Frames are 37 x 23 (partial 8 x 8 blocks on both axes, more than one wave) and 9 x 6 (less than one
wave), depth 4.  Add sizes are 5 and 40: the sorted schedule starts at 4 x prepass_spp samples, 32 with the automatic pre-pass of 8; the
GPU test reads the value in force from pt_get_stats.

Every leg asserts, on the model alone and before the context sees the call that matters, that it can show something: a change alters the
sums of the next add in at least a quarter of the owned pixels, a selecting add takes between a quarter and three quarters of the frame,
an orbit keeps the history of between a quarter and three quarters of the pixels."""
import numpy as np

import accum_seq_common as AQ
import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B

W, H, DEPTH = 37, 23, 4
SMALL = (9, 6)
MAIN, GLASS = 1, 3          # seeds of the two scenes
ORBIT = 20.0                # degrees: keeps 0.60 of the 37 x 23 pixels in MAIN, 0.63 in GLASS (measured on the model; asserted in the legs)
CHANGES = ("set_materials", "update_vertices", "set_environment", "watertight")
_cache = {}


def scene(seed, builder=None):
    """(upload step, state, view) of a scene"""
    if seed not in _cache:
        rng = np.random.default_rng(seed)
        up = SC._draw_upload(rng, guide=True)
        st = SC.apply(None, up)
        assert up["env"]["intensity"] >= 0.3 and len(up["ents"]) >= 3
        c, s = st["meshes"][1]["vertices"].astype(np.float64).mean(0), up["scale"]  # the sphere
        view = ([float(x) for x in c + np.array([0.3, 0.3, 1.2]) * s], [float(x) for x in c], [0.0, 1.0, 0.0], 45.0)
        _cache[seed] = (up, st, view)
    up, st, view = _cache[seed]
    return (up if builder is None else dict(up, builder=builder)), st, view


def change_steps(kind, st, seed=MAIN):
    """(the change, the change back; None = restore_vertices) of a kind in state st"""
    rng = np.random.default_rng(seed + 100)
    if kind == "set_materials":
        return dict(op="set_materials", mats=SC._draw_mats(rng, st["mats"], guide=True)), dict(op="set_materials", mats=st["mats"])
    if kind == "update_vertices":
        return dict(op="update_vertices", k=3, with_normals=True, null_mesh=None), None
    if kind == "set_environment":
        return dict(op="set_environment", env=SC._draw_env(rng, 1)), dict(op="set_environment", env=st["env"])
    assert kind == "watertight", kind
    return dict(op="set_option", key="watertight", value=1), dict(op="set_option", key="watertight", value=0)


def sorted_as_planned(stats, n, uniform_full_frame):
    """pt_get_stats after an add of n samples: the pre-pass in force decides the schedule.  A uniform add of the 37 x 23 frame at default
    knobs sorts from 4 x prepass_spp samples on (include/mi355pt.h, option "schedule"); the value itself is read, not assumed."""
    if stats is None or not uniform_full_frame:
        return
    pre = stats["prepass_spp"]
    if n == 5:
        assert pre == 0, "an add of 5 samples took the sorted schedule (prepass_spp %d)" % pre
    else:
        assert pre > 0 and 5 < 4 * pre <= n, "an add of %d samples at default knobs: prepass_spp %d" % (n, pre)


def _unchanged_sums(orc, seed, w, h, adds):
    key = ("base", seed, w, h, adds)
    if key not in _cache:
        up, _, view = scene(seed)
        b = AQ.Both(orc, None, up)
        b.begin(view, w, h, DEPTH)
        for n in adds:
            b.add(n)
        _cache[key] = b.am.live["sum"]
    return _cache[key]


def leg_change(orc, ctx, twin, kind, builder=0):
    """add 5, the change, add 40, the change back, add 5"""
    up, st0, view = scene(MAIN, builder)
    b = AQ.Both(orc, ctx, up, twin)
    there, back = change_steps(kind, st0)
    try:
        b.begin(view, W, H, DEPTH)
        sorted_as_planned(b.add(5), 5, True)
        b.change(there)
        # the model alone, before the context's add: with the change the second add must give other sums in a quarter of the pixels
        probe = AQ.Both(orc, None, up)
        probe.begin(view, W, H, DEPTH)
        probe.add(5)
        probe.change(there)
        probe.add(40)
        share = float(SC.same(probe.am.live["sum"], _unchanged_sums(orc, MAIN, W, H, (5, 40))).any(-1)[probe.am.live["owned"]].mean())
        print("%s: the change alters the sums of the next add in %.3f of the owned pixels" % (kind, share))
        assert share >= 0.25, (kind, share)
        sorted_as_planned(b.add(40), 40, True)
        b.same(b.am.live["sum"], probe.am.live["sum"], "the two models")
        if back is None:
            b.restore_vertices(st0["meshes"])
        else:
            b.change(back)
        sorted_as_planned(b.add(5), 5, True)
    finally:
        b.end()
        if ctx is not None:
            ctx.set_option("watertight", 0)


def knob_defaults(options):
    from test_gpu_fuzz import DEFAULTS

    return tuple((k, DEFAULTS[k]) for k, _ in options)


def leg_knob(orc, ctx, twin, options):
    """8 + 8 at default knobs, the knob, then a uniform and a selecting add on either side of the sort threshold (40, 40, 5, 5).  The model
    ignores knobs."""
    up, _, view = scene(MAIN)
    b = AQ.Both(orc, ctx, up, twin)
    try:
        b.begin(view, W, H, DEPTH)
        b.add(8)
        b.add(8)
        b.change(dict(op="knob", options=options))
        for n in (40, 5):
            b.add(n)
            thr = b.threshold()
            share = float(b.am.active(0, thr).mean())
            assert 0.25 <= share <= 0.75, (options, n, share)
            st = b.add(n, thr=thr)
            if st is not None:
                print("%s: selecting add of %d over %.3f of the frame: %d launches, prepass_spp %d" % (options, n, share, st["launches"], st["prepass_spp"]))
    finally:
        b.end()
        if ctx is not None:
            for k, v in knob_defaults(options):
                ctx.set_option(k, v)


def _history(share, what):
    print("%s: %.3f of the pixels keep history" % (what, share))
    assert 0.25 <= share <= 0.75, (what, share)


def leg_orbit(orc, ctx, twin, cap):
    """5 + 40, an orbit, a uniform add, a selecting add"""
    up, _, view = scene(MAIN)
    b = AQ.Both(orc, ctx, up, twin)
    there = AQ.orbit(view, ORBIT)
    try:
        b.begin(view, W, H, DEPTH)
        b.add(5)
        b.add(40)
        _history(b.reproject(there, b.guides(view), b.guides(there), max_history=cap), "orbit, max_history %d" % cap)
        a = b.am.live
        assert (a["n"] == 0).any() and (a["n"] == (cap or 45)).any(), "both kinds of pixel: reset ones and ones with history"
        b.add(5)
        b.add(40, thr=b.threshold())
        assert len(np.unique(a["n"])) >= 3, np.unique(a["n"])
    finally:
        b.end()


def leg_orbit_and_back(orc, ctx, twin):
    """Two reprojects in a row - the two sets of state buffers swap twice - then adds"""
    up, _, view = scene(MAIN)
    b = AQ.Both(orc, ctx, up, twin)
    there = AQ.orbit(view, ORBIT)
    try:
        b.begin(view, W, H, DEPTH)
        b.add(5)
        b.add(40)
        g_here, g_there = b.guides(view), b.guides(there)
        _history(b.reproject(there, g_here, g_there), "orbit")
        share = b.reproject(view, g_there, g_here, max_history=4)
        print("and back: %.3f of the pixels keep history" % share)
        assert 0 < share < 1, share
        b.add(40)
        b.add(5, thr=b.threshold())
    finally:
        b.end()


def leg_orbit_after_update(orc, ctx, twin):
    """A reproject after pt_update_vertices: the samples from before the update are carried along, the guides are the moved scene's"""
    up, st0, view = scene(MAIN)
    b = AQ.Both(orc, ctx, up, twin)
    there = AQ.orbit(view, 30.0)  # (in the moved scene 20 degrees keep 0.78 of the pixels)
    try:
        b.begin(view, W, H, DEPTH)
        b.add(5)
        b.add(40)
        b.change(change_steps("update_vertices", st0)[0])
        _history(b.reproject(there, b.guides(view), b.guides(there), max_history=0), "orbit after update_vertices")
        b.add(5)
        b.add(40, thr=b.threshold())
    finally:
        b.end()


def leg_small(orc, ctx, twin):
    """9 x 6, the glass scene: every active set is smaller than one wave"""
    up, st0, view = scene(GLASS)
    w, h = SMALL
    b = AQ.Both(orc, ctx, up, twin)
    there = AQ.orbit(view, ORBIT)
    try:
        b.begin(view, w, h, DEPTH)
        b.add(5)
        b.change(change_steps("set_materials", st0, GLASS)[0])
        b.add(40)
        share = float(SC.same(b.am.live["sum"], _unchanged_sums(orc, GLASS, w, h, (5, 40))).any(-1).mean())
        assert share >= 0.25, share
        thr = b.threshold()
        assert 0.25 <= b.am.active(0, thr).mean() <= 0.75
        b.add(40, thr=thr)
        share = b.reproject(there, b.guides(view), b.guides(there), max_history=4)
        print("9 x 6: %.3f of the pixels keep history" % share)
        assert 0 < share < 1, share
        b.add(5)
        b.add(5, thr=b.threshold())
        b.add(40, cap=50)
    finally:
        b.end()


def leg_refusals(orc, ctx, twin):
    """Refused in place: after a shard change and after an upload the accumulation stays as it was and stays readable; without an
    accumulation every call is refused; bad parameters."""
    up, st0, view = scene(MAIN)
    b = AQ.Both(orc, ctx, up, twin)
    P = lambda **kw: B.accum_default_params(**kw)
    there = AQ.orbit(view, ORBIT)
    try:
        if ctx is not None:
            ctx.accum_end()
        b.refused("info", lambda: ctx.accum_info())  # no accumulation yet
        assert ctx is None or B.lib().pt_accum_add(ctx._h, None, None, None) == -1
        b.begin(view, W, H, DEPTH)
        b.add(5)
        b.add(5)
        g_here, g_there = b.guides(view), b.guides(there)
        for kw in (dict(n_samples=0), dict(n_samples=65536), dict(max_pixel_samples=-1), dict(noise_threshold=-1.0), dict(noise_threshold=float("nan")), dict(reserved=1)):
            assert b.am.refusal(b.st, "add", kw.get("n_samples", 16), kw.get("max_pixel_samples", 0), kw.get("noise_threshold", 0.0), kw.get("reserved", 0)) == "bad parameters"
            b.calls.append("refused add %r" % kw)
            if ctx is not None:
                SC.expect_refusal(lambda: ctx.accum_add(P(**kw)), "add %r" % kw)
                AQ.assert_accum(ctx, b.am, b.where())
        b.change(dict(op="set_pixel_shard", shard=(1, 3, 8)))
        b.refused("add", lambda: ctx.accum_add(P(n_samples=5)))
        b.refused("reproject", lambda: ctx.accum_reproject(b.bcam(there), g_here, g_there))
        b.variance()
        b.denoise(g_here)  # the accumulation owns its whole frame, whatever the context's shard is now
        b.change(dict(op="set_pixel_shard", shard=None))
        b.add(5)  # the shard it was begun with: goes on
        b.change(dict(up))  # the same scene again is a new scene all the same
        b.refused("add", lambda: ctx.accum_add(P(n_samples=5)))
        b.refused("reproject", lambda: ctx.accum_reproject(b.bcam(there), g_here, g_there))
        b.variance()
        b.denoise(g_here)
        b.begin(view, W, H, DEPTH)
        b.add(5)
        b.end()
        for call, fn in (("add", lambda: ctx.accum_add(P(n_samples=5))), ("read", lambda: ctx.accum_read()), ("state", lambda: ctx.accum_state()),
                         ("variance", lambda: ctx.accum_variance()), ("denoise", lambda: ctx.accum_denoise(g_here)),
                         ("reproject", lambda: ctx.accum_reproject(SC._bcam(there, W, H), g_here, g_there))):
            b.refused(call, fn)
    finally:
        b.end()
        if ctx is not None:
            ctx.set_pixel_shard(0, 1, 16)


CHAIN_ROUNDS = (SMALL, (W, H), SMALL)  # the work buffers of the filters grow, then shrink
FOLLOW = dict(max_follow=4, roughness_max=0.3)


POISON = np.uint32(0xA5A5A5A5)  # async_common.DeviceFrame's fill


def leg_chain(orc, ctx, twin, A=None):
    """The interactive chain, three rounds: blocking adds of 8 + 8 and a pt_set_materials, then on ONE caller stream with no synchronize
    pt_accum_add_device(40), pt_render_aov_follow_device at the accumulation's size and at 2 x the size, pt_accum_denoise_device with the
    first guides, pt_upsample_device of the filtered frame to 2 x the size.  One pt_synchronize, then every caller buffer and the state
    must equal the model's chain.  A: tests/async_common (None without a context)."""
    up, _, view = scene(GLASS)
    b = AQ.Both(orc, ctx, up, twin)
    rng = np.random.default_rng(GLASS + 200)
    frames = []
    try:
        for w, h in CHAIN_ROUNDS:
            W2, H2 = 2 * w, 2 * h
            b.begin(view, w, h, DEPTH)
            b.add(8)
            b.add(8)
            if ctx is not None:  # every caller buffer before the chain: an allocation or its fill may wait for the device
                frames = [A.DeviceFrame(w, h), A.DeviceFrame(w, h, floats=8), A.DeviceFrame(W2, H2, floats=8), A.DeviceFrame(w, h), A.DeviceFrame(W2, H2)]
            b.change(dict(op="set_materials", mats=SC._draw_mats(rng, b.st["mats"], guide=True)))
            dev, b.ctx = b.ctx, None  # the model's chain (and the twins'): blocking calls on the context would synchronize
            try:
                b.add(40)
                want_add = (b.am.live["rgb"], b.am.live["rgba8"])
                g_lo, g_hi = b.guides(view, w, h, 1, FOLLOW), b.guides(view, W2, H2, 1, FOLLOW)
                want_dn = b.denoise(g_lo)
                want_up = b.upsample(want_dn[0], g_lo, g_hi)
            finally:
                b.ctx = dev
            assert SC.same(want_dn[0], want_add[0]).any() and np.isfinite(want_up[0]).all(), "the filter must change the frame"
            if ctx is None:
                b.end()
                continue
            f_add, f_lo, f_hi, f_dn, f_up = frames
            s, fp = A.stream(0), B.aov_default_params(n_samples=1, **FOLLOW)
            ctx.accum_add_device(B.accum_default_params(n_samples=40), f_add.rgb, f_add.rgba8, stream=s)
            ctx.render_aov_follow_device(SC._bcam(view, w, h), w, h, f_lo.rgb, fp, stream=s)
            ctx.render_aov_follow_device(SC._bcam(view, W2, H2), W2, H2, f_hi.rgb, fp, stream=s)
            ctx.accum_denoise_device(f_lo.rgb, f_dn.rgb, None, d_out_rgba8=f_dn.rgba8, stream=s)
            ctx.upsample_device(f_dn.rgb, f_lo.rgb, w, h, f_hi.rgb, W2, H2, f_up.rgb, None, d_out_rgba8=f_up.rgba8, stream=s)
            ctx.synchronize()  # the one wait of the round
            what = "%d x %d: " % (w, h)
            for f, want, name in ((f_add, want_add, "pt_accum_add_device"), (f_lo, (g_lo, None), "pt_render_aov_follow_device"), (f_hi, (g_hi, None), "pt_render_aov_follow_device at 2 x"),
                                  (f_dn, want_dn, "pt_accum_denoise_device"), (f_up, want_up, "pt_upsample_device")):
                got, got8 = f.read()
                b.same(got, want[0], what + name)
                if want[1] is None:
                    assert (got8 == POISON).all(), what + name + " wrote to a buffer that is not its own"
                else:
                    b.same(got8, want[1], what + name + "'s RGBA8 image")
            AQ.assert_accum(ctx, b.am, what + b.where())
            b.end()
            for f in frames:
                f.free()
            frames = []
    finally:
        b.end()
        if ctx is not None:
            ctx.synchronize()
            for f in frames:
                f.free()
