"""The legs of tests/test_gpu_accum_changes.py without a device: the model of tests/accum_seq_common.py alone, every step held through the
library's CPU twins on a host-only context (pt_debug_accum_select_host, _resolve_host, _reproject_host, pt_debug_accum_variance_host,
pt_debug_denoise_var_host, pt_debug_upsample_host) applied to the model's arrays before the step.  This proves the model, and the
conditions the legs assert on it (a change shows in a quarter of the pixels, a selecting add takes a quarter to three quarters of the
frame, an orbit keeps the history of a quarter to three quarters of the pixels), before a GPU is involved.  A host-only context refuses
the accumulation itself with PT_E_NO_DEVICE."""
import numpy as np
import pytest

import accum_changes_common as AC
import accum_seq_common as AQ
import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B


@pytest.fixture(scope="module")
def twin():
    ctx = B.Context(-1)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("kind", AC.CHANGES)
def test_change_between_adds(orc, twin, kind):
    AC.leg_change(orc, None, twin, kind)


def test_knob_between_adds(orc, twin):
    AC.leg_knob(orc, None, twin, SC.knobs()[0])  # (the model ignores knobs: one stands for all)
    assert len(SC.knobs()) >= 20
    for options in SC.knobs():
        assert [k for k, _ in AC.knob_defaults(options)] == [k for k, _ in options]


@pytest.mark.parametrize("cap", [0, 4])
def test_orbit(orc, twin, cap):
    AC.leg_orbit(orc, None, twin, cap)


def test_orbit_and_back(orc, twin):
    AC.leg_orbit_and_back(orc, None, twin)


def test_orbit_after_update_vertices(orc, twin):
    AC.leg_orbit_after_update(orc, None, twin)


def test_small_frame(orc, twin):
    AC.leg_small(orc, None, twin)


def test_refusals(orc, twin):
    AC.leg_refusals(orc, None, twin)


def test_chain(orc, twin):
    AC.leg_chain(orc, None, twin)


def test_host_only_context_has_no_accumulation(twin):
    up, st, view = AC.scene(AC.MAIN)
    SC.upload(twin, st, up)
    with pytest.raises(B.PtError, match=r"pt_accum_begin failed \(-2\)"):  # PT_E_NO_DEVICE
        twin.accum_begin(SC._bcam(view, AC.W, AC.H), AC.W, AC.H, AC.DEPTH)


def test_the_model_equals_render_without_changes(orc):
    """The model's own anchor: uniform adds of 5 + 40 + 5 without a change are seq_common.Model's render at 50 samples, RGBA8 included."""
    up, st, view = AC.scene(AC.MAIN)
    b = AQ.Both(orc, None, up)
    b.begin(view, AC.W, AC.H, AC.DEPTH)
    for n in (5, 40, 5):
        b.add(n)
    want, want8 = b.model.expected(st, dict(op="render", cam=view, W=AC.W, H=AC.H, spp=50, depth=AC.DEPTH))
    assert not SC.same(b.am.live["rgb"], want).any() and (b.am.live["rgba8"] == want8).all()
    assert (np.asarray(want) > 0).mean() > 0.9
