"""An accumulation as it lives on a context, held to the oracle bit for bit (uint32 view, NaN equals NaN): the legs of
tests/accum_changes_common.py on the GPU.  The reference is the model of tests/accum_seq_common.py - the oracle continues every active
pixel from its stored stream in the scene state current at that add (oracle.Scene.accumulate), the restatements accum_ref,
accum_reproject_ref, denoise_var_ref, upsample_ref, aov_ref and aov_follow_ref do the rest - and nothing the library returns reaches it.
After every blocking call pt_debug_accum_state, pt_accum_read (rgb, RGBA8, noise, samples) and pt_accum_info_get are compared with it.

1. One change between two adds - pt_set_materials, pt_update_vertices (on the trees of builders 0, 1 and 2), pt_set_environment, option
   "watertight" - as add 5, change, add 40, change back, add 5: samples see the state current at their add.
2. Every scheduler path of seq_common.knobs() set between two adds: a uniform continuing add and a selecting add over about half of the
   frame, at 40 and at 5 samples.
3. An orbit of 20 degrees with max_history 0 and 4, then a uniform and a selecting add under the new camera; an orbit and back; an orbit
   after pt_update_vertices.
4. A 9 x 6 frame: every active set is smaller than one wave.
5. The interactive chain on one caller stream without a synchronize, three rounds whose sizes grow and shrink.
6. Refusals in place, with the accumulation's readable state as it was.
ONE context for the module and one caller stream."""
import pytest

import accum_changes_common as AC
import async_common as AS
import seq_common as SC
from owl_path_tracer_amd.pyhost import binding as B

pytestmark = pytest.mark.gpu

_ctx = {}


def gpu():
    if "ctx" not in _ctx:
        _ctx["ctx"] = B.Context(0)
        _ctx["twin"] = B.Context(-1)
    return _ctx["ctx"], _ctx["twin"]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    AS.destroy_streams()
    for k in ("ctx", "twin"):
        if k in _ctx:
            _ctx[k].close()
    _ctx.clear()


@pytest.mark.parametrize("kind,builder", [("set_materials", 0), ("update_vertices", 0), ("update_vertices", 1), ("update_vertices", 2), ("set_environment", 0), ("watertight", 0)])
def test_change_between_adds(orc, kind, builder):
    AC.leg_change(orc, *gpu(), kind, builder)


@pytest.mark.parametrize("k", range(len(SC.knobs())))
def test_knob_between_adds(orc, k):
    AC.leg_knob(orc, *gpu(), SC.knobs()[k])


@pytest.mark.parametrize("cap", [0, 4])
def test_orbit(orc, cap):
    AC.leg_orbit(orc, *gpu(), cap)


def test_orbit_and_back(orc):
    AC.leg_orbit_and_back(orc, *gpu())


def test_orbit_after_update_vertices(orc):
    AC.leg_orbit_after_update(orc, *gpu())


def test_small_frame(orc):
    AC.leg_small(orc, *gpu())


def test_chain_on_one_stream(orc):
    AC.leg_chain(orc, *gpu(), AS)


def test_refusals_in_place(orc):
    AC.leg_refusals(orc, *gpu())
