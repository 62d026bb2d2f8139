"""The selected pair's results of a launch of several pairs (TraceStage of csrc/ctx.h: direct path, direct slot on the device, diffuse
time range, live count) behind the calls that rewrite the records: pair 1 of a two-pair launch after rvb_relisten and after rvb_reshade,
every quantity against the CPU oracle's trace of that pair — the direct path, the speaker time range, the merged-image configuration
(which gathers from the device direct slot) and an RVB_IR_EXACT accumulate, bit for bit.  The constructed room of tests/image_edges.py at
the smallest two-pair shape of tests/test_gpu_live_list.py."""
import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_image_edges import case_of
from test_gpu_live_list import RATES, TRACE_SHAPES, check_against_oracle, live_rows, make_ctx
from test_gpu_reshade import AIR_B, SPEAKERS
from test_gpu_source_pattern import oracle_range, same_records

pytestmark = pytest.mark.gpu

SHAPE = TRACE_SHAPES[0]
# traced as (microphone 1, source 1) and (microphone 2, source 0); the relisten moves pair 1 to microphone 0, which sees its source
TRACED_MICS, SOURCES, HEARD_MICS = E.MICS[[1, 2]], E.SOURCES[[1, 0]], E.MICS[[2, 0]]


def assert_pair_1(c, oracle, want, other, what):
    from parallel_reverb_raytracer_amd import capi
    mic, diffuse, images = want["mic"], want["diffuse"], want["images"]
    # the ground: a direct path, images beside it, live and dead records, and nothing that pair 0 would give as well
    assert want["direct"]["volume"].any() and images.shape[0] >= 2 and 0 < live_rows(diffuse) < diffuse.shape[0], what
    assert not same_records(other["direct"], want["direct"]) and oracle_range(other["diffuse"]) != oracle_range(diffuse), what
    assert other["images"].shape != images.shape or not same_records(other["images"], images), what
    with pytest.raises(capi.RvbError) as e:             # the call before has voided the configuration ... and selected pair 0:
        c.ir_time_range()
    assert e.value.code == capi.ERR_STATE, what
    assert same_records(c.get_direct(), other["direct"]), what
    c.select_pair(1)
    assert same_records(c.get_direct(), want["direct"]), what
    c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    assert c.ir_time_range() == oracle_range(diffuse), what
    assert c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False) == images.shape[0], what
    attenuate = lambda r: [oracle.attenuate_speaker(mic, r, d, k) for d, k in zip(*SPEAKERS)]
    check_against_oracle(c, oracle, attenuate, np.concatenate([diffuse, images]), what, RATES[:1])
    # a replay counts nothing: every impulse of the pair is listed
    assert c.ir_exact_list_info() == (diffuse.shape[0] + images.shape[0], live_rows(diffuse) + live_rows(images), False), what


def test_pair_1_of_two_after_a_relisten_and_after_a_reshade(oracle):
    nrays, nrefl = SHAPE
    c = make_ctx(keep=True)
    try:
        c.set_directions(E.directions(nrays))
        c.trace_pairs(TRACED_MICS, SOURCES, nrefl, AIR_COEFFICIENTS)
        c.select_pair(1)
        c.relisten(HEARD_MICS)
        assert_pair_1(c, oracle, case_of(oracle, HEARD_MICS[1], SOURCES[1], SHAPE), case_of(oracle, HEARD_MICS[0], SOURCES[0], SHAPE), "after the relisten")
        c.reshade(E.table_b(), AIR_B)
        assert_pair_1(c, oracle, case_of(oracle, HEARD_MICS[1], SOURCES[1], SHAPE, "B"), case_of(oracle, HEARD_MICS[0], SOURCES[0], SHAPE, "B"),
                      "after the re-shade")
    finally:
        c.close()
