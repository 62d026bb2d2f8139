"""The host half of the impulse-response stage (csrc/ir_state.h) alone: tests/cpp/ir_state.cpp, which includes nothing else of the
library, is compiled as host code with AddressSanitizer and UndefinedBehaviorSanitizer into a temporary directory and run once; what it
printed is held against the values below, which are written out from the rules of include/rvb_capi.h (rvb_ir_configure_*,
rvb_ir_time_range_begin, rvb_ir_exact_prepare, rvb_attenuate_hrtf*, rvb_flatten).  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from parallel_reverb_raytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"

NOTHING, FLATTEN_QUERY, EXACT_LIST = 0, 1, 2                # what the sort buffers hold
QUERY = {"query_a": 1, "query_n": 300, "query_rate": 44100, "query_bins": 12345}
SPEAKERS = {"hrtf_combined": 0, "nbins": 4096, "n": 700, "ndiffuse": 660, "exact_nimages": 40}
EARS = {"hrtf_combined": 1, "nbins": 512, "n": 1400, "ndiffuse": 1320, "exact_nimages": 80}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tool = os.path.join(str(tmp_path_factory.mktemp("ir_state")), "ir_state")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", SANITIZE, "-fno-sanitize-recover=all", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "ir_state.cpp"), "-o", tool])
    done = subprocess.run([tool], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0 and done.stderr == "", done.stderr           # a sanitizer report goes to stderr and ends the program
    return done.stdout.splitlines()


def of_kind(lines, kind):
    got = {}
    for line in lines:
        words = line.split()
        if words[0] == kind:
            assert words[1] not in got, line
            got[words[1]] = {k: int(v) for k, v in (item.split("=", 1) for item in words[2:])}
    return got


def state(configured=0, which=capi.IR_ALL, nimages=0, merged=0, stale=0, range_pending=0, table_ears=0, tenant=NOTHING, **payload):
    """every reader of IrState; the payload of the tenant is printed only while there is one"""
    want = {"configured": configured, "which": which, "nimages": nimages, "merged": merged, "stale": stale, "range_pending": range_pending,
            "table_ears": table_ears, "tenant": tenant, "prepared": int(tenant == EXACT_LIST)}
    want.update(payload)
    return want


def test_the_program_includes_the_state_header_alone():
    with open(os.path.join(ROOT, "tests", "cpp", "ir_state.cpp")) as f:
        local = [l.split('"')[1] for l in f if l.startswith('#include "')]
    assert local == ["ir_state.h"]
    with open(os.path.join(CSRC, "ir_state.h")) as f:
        assert not [l for l in f if l.startswith('#include "') or "hip/" in l]


def test_transitions(lines):
    # the last configuration of the walk: rvb_ir_configure_* with which == RVB_IR_IMAGES and three images, behind a one-ear table
    cfg = dict(configured=1, which=capi.IR_IMAGES, nimages=3, table_ears=1)
    assert of_kind(lines, "step") == {
        # a new context: nothing configured (which is RVB_IR_ALL until a configure says otherwise), no table, nothing in the sort buffers
        "initial": state(),
        # "Every successful rvb_ir_configure_* replaces the previous configuration as a whole"
        "configure": state(configured=1, which=capi.IR_DIFFUSE, nimages=40),
        # rvb_ir_configure_*_merged: the list is the gather of the merged list; its host copy comes down when a reader asks, once
        "configure_gathered": state(configured=1, which=capi.IR_ALL, nimages=7, merged=1, stale=1),
        "images_fetched": state(configured=1, which=capi.IR_ALL, nimages=7, merged=1),
        # a trace, rvb_reshade, rvb_relisten, rvb_ir_select_pair: "voids the IR configuration and a prepared exact list"
        "drop": state(which=capi.IR_ALL, nimages=7),
        "two_ear_table_prepared": state(configured=1, which=capi.IR_ALL, nimages=40, table_ears=2, tenant=EXACT_LIST, **EARS),
        # rvb_attenuate_hrtf*: "void the IR configuration (whichever model it names) and a prepared exact list, and a following
        # rvb_ir_configure_hrtf with table == NULL returns RVB_ERR_STATE"
        "one_ear_table": state(which=capi.IR_ALL, nimages=40, table_ears=1),
        # rvb_ir_time_range_begin enqueues the pass of the CURRENT configuration; rvb_ir_time_range takes it; a new configuration voids it
        "range_enqueued": state(range_pending=1, **cfg),
        "range_taken": state(**cfg),
        "range_voided_by_configure": state(**cfg),
        # rvb_flatten with out == NULL is remembered for the fill; the fill's sort consumes the keys
        "flatten_query": state(tenant=FLATTEN_QUERY, **cfg, **QUERY),
        "flatten_fill": state(**cfg),
        # whoever rewrites the sort buffers claims them: neither a query's keys nor a prepared list outlive that
        "query_then_claimed": state(**cfg),
        "prepare": state(tenant=EXACT_LIST, **cfg, **SPEAKERS),
        "prepare_then_claimed": state(**cfg),
        # rvb_ir_exact_prepare: "rvb_ir_accumulate in either mode and with any nbins ... voids it" — RVB_IR_FAST with up to 8 speakers does
        # not touch the sort buffers, so the keys of a size query stay
        "prepare_then_accumulate": state(**cfg),
        "query_then_accumulate": state(tenant=FLATTEN_QUERY, **cfg, **QUERY),
        "prepare_then_drop": state(which=capi.IR_IMAGES, nimages=3, table_ears=1),
        # a configure voids a prepared list and nothing else of the sort buffers
        "query_then_configure": state(configured=1, which=capi.IR_DIFFUSE, nimages=0, table_ears=1, tenant=FLATTEN_QUERY, **QUERY),
    }


def test_a_fill_finds_exactly_its_own_query(lines):
    """the same (pointer, n, sample_rate) and nothing else — never a null pointer —, and only while the query's keys are in the sort buffers"""
    no = {"same": 0, "other_pointer": 0, "other_n": 0, "other_rate": 0, "null": 0}
    yes = dict(no, same=1)
    assert of_kind(lines, "resident") == {
        "initial": no, "flatten_query": yes, "flatten_fill": no, "flatten_query_null": no, "query_then_claimed": no,
        "query_then_accumulate": yes, "query_then_prepare": no, "query_then_configure": yes,
    }


def test_a_fold_finds_exactly_the_prepared_nbins(lines):
    void = {"nbins": 0, "nbins_plus_1": 0}
    assert of_kind(lines, "prepared_for") == {
        "initial": void, "prepare": {"nbins": 1, "nbins_plus_1": 0}, "prepare_then_claimed": void, "prepare_then_accumulate": void,
        "prepare_then_drop": void,
    }
