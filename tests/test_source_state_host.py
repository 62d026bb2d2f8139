"""The host half of the source directivity (csrc/source_state.h, csrc/source_state.hip) and the staging block of a launch of several
pairs (PairBlock, PairLaunch of csrc/ctx.h) alone: tests/cpp/source_state.cpp is compiled as host code together with source_state.hip,
with AddressSanitizer and UndefinedBehaviorSanitizer, into a temporary directory and run once; what it printed is held against the
values below, which are written out from the rules of include/rvb_capi.h and the texts of the entry points.  No GPU, nothing loaded
into Python."""
import os
import struct
import subprocess

import pytest

from parallel_reverb_raytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SANITIZE = "-fsanitize=address,undefined"

ZERO_LENGTH = "rvb_set_source_pattern: pattern 1 has a direction of zero length (or one binary32 cannot normalise)"
REFUSALS = {
    "pattern_nan_shape": "rvb_set_source_pattern: pattern 1 holds a value that is not finite",
    "pattern_zero": ZERO_LENGTH,
    "pattern_tiny": ZERO_LENGTH,
    "pattern_huge": ZERO_LENGTH,
    "table_inf": "rvb_set_source_table: row 64799 of the table holds a value that is not finite",
    "no_orientations": "rvb_set_source_table: a table without orientations",
    "up_parallel": "rvb_set_source_table: orientation 1: normalize3(cross3(up, facing)) is zero or not finite",
}
TABLE_FLOATS = 64800 * 8


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    directory = str(tmp_path_factory.mktemp("source_state"))
    objects = []
    for src in (os.path.join(CSRC, "source_state.hip"), os.path.join(ROOT, "tests", "cpp", "source_state.cpp")):
        obj = os.path.join(directory, os.path.basename(src) + ".o")
        subprocess.check_call([HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off", SANITIZE, "-fno-sanitize-recover=all",
                               "-I" + CSRC, "-c", src, "-o", obj])
        objects.append(obj)
    tool = os.path.join(directory, "source_state")
    subprocess.check_call([HIPCC, SANITIZE, "-o", tool] + objects)
    done = subprocess.run([tool], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(done.stdout)
    assert done.returncode == 0 and done.stderr == "", done.stderr           # a sanitizer report goes to stderr and ends the program
    return done.stdout.splitlines()


def fields(line):
    return dict(item.split("=", 1) for item in line.split()[2:])


def test_refusals_give_their_texts_and_leave_the_state_as_it_was(lines):
    got = [l for l in lines if l.startswith("refusal ")]
    assert len(got) == 3 * len(REFUSALS)
    seen = set()
    for line in got:
        head, text = line.split(" text=", 1)
        _, base, name, code, unchanged = head.split()
        assert text == REFUSALS[name], line
        assert code == "code=%d" % capi.ERR_INVALID and unchanged == "unchanged=1", line
        seen.add((base, name))
    assert seen == {(base, name) for base in ("off", "patterns", "table") for name in REFUSALS}


def test_transitions(lines):
    steps = {l.split()[1]: {k: int(v) for k, v in fields(l).items()} for l in lines if l.startswith("step ")}

    def state(patterns=0, orientations=0, patterns_upload=0, table_upload=0):
        return {"rc": capi.OK, "patterns": patterns, "orientations": orientations, "table_floats": TABLE_FLOATS if orientations else 0,
                "patterns_upload": patterns_upload, "table_upload": table_upload, "off": int(patterns == 0 and orientations == 0)}

    want = {
        "initial": state(),
        "off_to_patterns": state(patterns=1, patterns_upload=1),
        "uploaded": state(patterns=1),
        "same_patterns_again": state(patterns=1),
        "other_patterns": state(patterns=1, patterns_upload=1),
        "patterns_to_table": state(orientations=2, table_upload=1),
        "table_uploaded": state(orientations=2),
        "same_table_again": state(orientations=2, table_upload=1),
        "table_to_patterns": state(patterns=1, patterns_upload=1),
        "null_table_while_patterns_on": state(patterns=1),
        "null_patterns": state(),
        "null_table_while_table_on": state(),
    }
    assert steps == want
    # the accepted values themselves: the direction normalised with w = 0 whatever direction[3] held, the table's first and last float read
    assert "form direction=0,1,0,0 shape0=0.25" in lines
    assert "table first=0.25 last=15.75 basis0=1,0,0" in lines


def test_count_check(lines):
    got = {tuple(l.split()[1:3]): l.split(" ", 3)[3] for l in lines if l.startswith("counts ")}
    assert got == {
        ("patterns", "1_for_3"): "code=0 text=",
        ("patterns", "3_for_3"): "code=0 text=",
        ("patterns", "2_for_3"): "code=1 text=rvb_trace: 2 source patterns for 3 pair(s): one for all pairs, or one per pair (rvb_set_source_pattern)",
        ("orientations", "1_for_3"): "code=0 text=",
        ("orientations", "3_for_3"): "code=0 text=",
        ("orientations", "2_for_3"): "code=1 text=rvb_reshade: 2 source orientations for 3 pair(s): one for all pairs, or one per pair (rvb_set_source_table)",
    }


def test_pair_block(lines):
    blocks = {l.split()[1]: bytes.fromhex(l.split()[2]) for l in lines if l.startswith("block ")}
    assert "block_bytes 120 40" in lines and "block_ranges_offset 96" in lines
    sources_and_ranges = struct.pack("<12f", -1, -2, -3, 0, -4, -5, -6, 0, -7, -8, -9, 0) + bytes.fromhex("FFFFFFFF00000000") * 3
    staged = struct.pack("<12f", 1, 2, 3, 0, 4, 5, 6, 0, 7, 8, 9, 0) + sources_and_ranges
    assert len(staged) == 120 and blocks["staged"] == staged
    restaged = struct.pack("<12f", 10, 11, 12, 0, 13, 14, 15, 0, 16, 17, 18, 0) + sources_and_ranges
    assert blocks["restaged"][:48] == restaged[:48] and blocks["restaged"][48:] == staged[48:] and len(blocks["restaged"]) == 120
    # one pair: nothing allocated, no event, no pointer of the launch moved — and no HIP call was needed for it
    assert "one_pair error=0 block=0 geom=0 direct=0 range=0 event=0 pointers=0" in lines
