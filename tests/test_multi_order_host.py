"""The call order of the multi-GPU layer (rvb_multi_*, csrc/multi.hip): multi.hip is compiled as host code together with
tests/cpp/multi_order.cpp, which stands in for the HIP runtime, for the add launcher and for the C-ABI below rvb_multi_*, logs every
call with the integer arguments that define the schedule, really copies and adds, and checks the chain's invariants (an event is
recorded before a wait names it; every block is folded once per device, in order, behind its arrival; the blocks tile the
histogram; streams and buffers are used under their own device; no copy leaves its allocation) and csrc/bin_blocks.h.  Two builds —
AddressSanitizer + UndefinedBehaviorSanitizer, and ThreadSanitizer — are run once each; stdout must equal
tests/golden/multi_call_order.txt line for line.  The enqueued device work is a function of that sequence, so a change of multi.hip
that keeps it has changed no device work.  No GPU, nothing loaded into Python.

    python tests/test_multi_order_host.py --write [--sources <files>]

records the fixture anew (only when the schedule is changed on purpose), after 25 runs that must print the same bytes.  With
`--sources` alone the program is built from those translation units instead (e.g. an earlier commit's multi.hip, copied to where
its relative includes resolve; the current headers are on the include path) and held against the fixture."""
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "parallel-reverb-raytracer_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CLANGXX = os.environ.get("ROCM_CLANGXX", "/opt/rocm/llvm/bin/clang++")
FIXTURE = os.path.join(ROOT, "tests", "golden", "multi_call_order.txt")
HARNESS = os.path.join(ROOT, "tests", "cpp", "multi_order.cpp")
SOURCES = [os.path.join(CSRC, "multi.hip")]
BUILDS = {"address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "thread": ["-fsanitize=thread"]}


def build(directory, sanitize, sources=SOURCES):
    objects = []
    for src in list(sources) + [HARNESS]:
        obj = os.path.join(directory, os.path.basename(src) + ".o")
        subprocess.check_call([HIPCC, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + [a for f in sanitize for a in ("-Xarch_host", f)]
                              + ["-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", obj])
        objects.append(obj)
    # multi.hip holds no device code: a host-only object of it must not ask for a fat binary or a kernel registration
    for obj in objects[:-1]:
        undefined = subprocess.check_output(["nm", "-u", obj], universal_newlines=True)
        assert "__hip" not in undefined, undefined
    tool = os.path.join(directory, "multi_order")
    subprocess.check_call([CLANGXX] + sanitize + ["-pthread", "-o", tool] + objects + ["-ldl"])
    return tool


def run(tool):
    done = subprocess.run([tool], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert done.returncode == 0 and done.stderr == "", done.stderr      # a sanitizer report or a broken invariant goes to stderr
    return done.stdout


def compare(got):
    with open(FIXTURE) as f:
        want = f.read().splitlines()
    got = got.splitlines()
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, "line %d: %r, recorded %r" % (k + 1, a, b)
    assert len(got) == len(want)


@pytest.mark.parametrize("sanitizer", sorted(BUILDS))
def test_call_order_equals_the_recorded_one(tmp_path, sanitizer):
    compare(run(build(str(tmp_path), BUILDS[sanitizer])))


if __name__ == "__main__":
    args = sys.argv[1:]
    write = "--write" in args
    if write:
        args.remove("--write")
    assert not args or args[0] == "--sources" and len(args) > 1, __doc__
    sources = [os.path.abspath(a) for a in args[1:]] or SOURCES
    with tempfile.TemporaryDirectory() as tmp:
        outputs = {}
        for name in sorted(BUILDS):
            os.mkdir(os.path.join(tmp, name))
            tool = build(os.path.join(tmp, name), BUILDS[name], sources)
            outputs[name] = {run(tool) for _ in range(25 if write else 1)}
    got = set.union(*outputs.values())
    assert len(got) == 1, "the runs print different bytes: %s" % {k: len(v) for k, v in outputs.items()}
    got = got.pop()
    if write:
        with open(FIXTURE, "w") as f:
            f.write(got)
        print("%s: %d lines, 25 runs of each build printed the same bytes" % (FIXTURE, len(got.splitlines())))
    else:
        compare(got)
        print("%s reproduced byte for byte by %s" % (os.path.relpath(FIXTURE, ROOT), " ".join(os.path.relpath(s, ROOT) if s.startswith(ROOT) else s for s in sources)))
