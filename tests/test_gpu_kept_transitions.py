"""The transitions of a kept trace (KeptState of csrc/kept_state.h) on one context, each state read through what the calls return:
the listener bit dropped between a trace and a relisten leaves that trace's listener records in use; the next trace, made for
materials alone, refuses a relisten and still re-shades; keeping switched off refuses both.  Every result against the CPU oracle's
trace — records, direct slot, image candidates, merged images.  The constructed room of tests/image_edges.py at its smallest shape,
64 rays x 2 reflections, one pair."""
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_image_edges import assert_equal, case_of, new_context, room, states_of
from test_gpu_reshade import AIR_B

pytestmark = pytest.mark.gpu

SHAPE = (64, 2)


def refused(call, what):
    from parallel_reverb_raytracer_amd import capi
    with pytest.raises(capi.RvbError) as e:
        call()
    assert e.value.code == capi.ERR_STATE, what + ": " + str(e.value)
    return str(e.value)


def test_listener_bit_dropped_then_materials_only_then_keeping_off(oracle):
    (mic, source), other_mic = E.PAIRS[0], E.PAIRS[1][0]
    traced, heard, traced_b = (case_of(oracle, mic, source, SHAPE), case_of(oracle, other_mic, source, SHAPE),
                               case_of(oracle, mic, source, SHAPE, "B"))
    # the ground: the second microphone and the other table each change the results
    assert all(traced[k].tobytes() != x[k].tobytes() for x in (heard, traced_b) for k in ("diffuse", "image"))
    c = new_context(room(), "listener")
    try:
        c.set_directions(traced["dirs"])
        c.trace(mic, source, SHAPE[1], AIR_COEFFICIENTS)
        assert_equal(oracle, states_of(c)[0], traced, "kept trace")
        c.keep_paths(True)                                       # the listener bit dropped: the last trace's listener records stay
        c.relisten(other_mic)
        assert_equal(oracle, states_of(c)[0], heard, "relistened behind keep_paths(True)")
        c.trace(mic, source, SHAPE[1], AIR_COEFFICIENTS)         # kept for materials only
        assert "path_keep_kernel" in [k for k, _ in c.last_timings()]
        assert "RVB_KEEP_LISTENER" in refused(lambda: c.relisten(other_mic), "relisten behind a trace kept for materials")
        assert_equal(oracle, states_of(c)[0], traced, "behind the refused relisten")
        c.reshade(E.table_b(), AIR_B)
        assert_equal(oracle, states_of(c)[0], traced_b, "re-shaded to B")
        c.keep_paths(False)
        assert "rvb_keep_paths" in refused(lambda: c.reshade(None, AIR_COEFFICIENTS), "reshade behind keep_paths(False)")
        refused(lambda: c.relisten(other_mic), "relisten behind keep_paths(False)")
        assert_equal(oracle, states_of(c)[0], traced_b, "behind the refused reshade")
    finally:
        c.close()
