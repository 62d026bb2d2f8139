"""The host half of the trace stage (csrc/trace_state.h) alone: tests/cpp/trace_state.cpp, which includes nothing else of the library,
is compiled as host code with AddressSanitizer and UndefinedBehaviorSanitizer into a temporary directory and run once; what it printed
is held against the values below, which are written out from the rules of include/rvb_capi.h (rvb_trace*, rvb_reshade, rvb_relisten,
rvb_ir_select_pair, rvb_set_scene, rvb_set_directions*) and include/rvb_capi_live.h (*count_valid).  No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"

# the trace the walk fetches: two pairs, 128 rays in all, 5 reflections, ray_offset 1000 — and the one behind a scene change
TRACE = {"npairs": 2, "rays": 128, "nreflections": 5, "ray_offset": 1000}
OTHER = {"npairs": 3, "rays": 21, "nreflections": 9, "ray_offset": 77}


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    tool = os.path.join(str(tmp_path_factory.mktemp("trace_state")), "trace_state")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", SANITIZE, "-fno-sanitize-recover=all", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "cpp", "trace_state.cpp"), "-o", tool])
    done = subprocess.run([tool], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0 and done.stderr == "", done.stderr           # a sanitizer report goes to stderr and ends the program
    got = {}
    for line in done.stdout.splitlines():
        words = line.split()
        assert words[0] == "step" and words[1] not in got, line
        got[words[1]] = {k: int(v) for k, v in (item.split("=", 1) for item in words[2:])}
    return got


def state(traced=0, npairs=1, rays=0, nreflections=0, ray_offset=0, pair=0, fetched=0, count_holds=0):
    """every reader of TraceState"""
    return {"traced": traced, "npairs": npairs, "rays": rays, "nreflections": nreflections, "ray_offset": ray_offset, "pair": pair,
            "fetched": fetched, "count_holds": count_holds}


def test_the_program_includes_the_state_header_alone():
    with open(os.path.join(ROOT, "tests", "cpp", "trace_state.cpp")) as f:
        local = [l.split('"')[1] for l in f if l.startswith('#include "')]
    assert local == ["trace_state.h"]
    with open(os.path.join(CSRC, "trace_state.h")) as f:
        assert not [l for l in f if l.startswith('#include "') or "hip/" in l]


def test_transitions(steps):
    assert steps == {
        # a new context: nothing traced ("rvb_ir_select_pair ... return RVB_ERR_STATE"), one pair, pair 0, nothing fetched, no count
        "initial": state(),
        # a trace that begins: until it has finished there are no results
        "begin": state(),
        # a finished trace: every reader reports the launch; nothing of it is fetched; "pair 0 after a trace"; the count holds
        # exactly where the caller says that the shadow stage wrote the final records
        "finished": state(traced=1, count_holds=1, **TRACE),
        "fetched": state(traced=1, fetched=1, count_holds=1, **TRACE),
        # "*count_valid 0: ... a source directivity ... had rewritten the records behind it"
        "finished_count_does_not_hold": state(traced=1, npairs=1, rays=64, nreflections=5),
        # rvb_reshade, rvb_relisten: "like a trace ... rvb_ir_select_pair is back at 0"; the block is the old records', and
        # "*count_valid 0: ... a re-shade or a relisten had rewritten the records"; the trace and its sizes stand
        "fetched_then_rewritten": state(traced=1, **TRACE),
        # rvb_ir_select_pair chooses among results that are already down: the block and the count stay
        "fetched_then_select_1": state(traced=1, pair=1, fetched=1, count_holds=1, **TRACE),
        "select_1_then_rewritten": state(traced=1, **TRACE),
        # the next trace begins: not traced, and its kernels count anew (the sizes are read by nothing until it has finished)
        "fetched_then_begin": state(pair=1, fetched=1, **TRACE),
        "select_1_then_next_trace": state(traced=1, **TRACE),
        # rvb_set_scene, rvb_share_scene, rvb_set_directions*: nothing traced until the next trace, of which then everything is new
        "inputs_changed": state(pair=1, fetched=1, count_holds=1, **TRACE),
        "inputs_changed_then_finished": state(traced=1, count_holds=1, **OTHER),
    }


def test_nothing_of_the_old_trace_survives_the_next(steps):
    """behind a scene or direction change a finished trace reports the new launch alone: the old one had other sizes, pair 1 selected
    and its block fetched"""
    old, new = steps["inputs_changed"], steps["inputs_changed_then_finished"]
    assert old["traced"] == 0 and new["traced"] == 1
    assert all(new[k] == OTHER[k] != TRACE[k] for k in OTHER)
    assert (old["pair"], old["fetched"]) == (1, 1) and (new["pair"], new["fetched"]) == (0, 0)
