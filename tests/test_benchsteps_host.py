"""tools/benchsteps.py on the host: the command string of the step chain, what the chain does when a step fails or runs out of time
(over a stub script that touches no GPU), and the sample store."""
import json
import os
import shlex
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import benchsteps  # noqa: E402

STUB = """import argparse, sys, time
p = argparse.ArgumentParser()
for name in ("--log", "--step", "--out"):
    p.add_argument(name)
args = p.parse_args()
with open(args.log, "a") as f:
    f.write(args.step + "\\n")
if args.step == "fails":
    sys.exit(3)
if args.step == "hangs":
    time.sleep(30)
if args.step == "report" and args.out:
    open(args.out, "w").write("table\\n")
"""


def test_command_string():
    lib = "/some where/librvb_hip.so"
    command = benchsteps.chain_command(["python", "tools/x_bench.py"], ["--rays", "2000"], benchsteps.in_turn(2, lib), 77, out="a table.txt")
    parts = command.split(" && ")
    assert [part.split()[-1] for part in parts[:4]] == ["this", "parent", "this", "parent"]
    limited = "timeout -k 10 77 python tools/x_bench.py --rays 2000 --step "
    assert parts[0] == parts[2] == limited + "this"
    assert parts[1] == parts[3] == "RVB_LIB=" + shlex.quote(lib) + " " + limited + "parent"
    assert parts[4] == "python tools/x_bench.py --rays 2000 --step report --out 'a table.txt'"
    assert len(parts) == 5 and "timeout" not in parts[4] and command.count("RVB_LIB=") == 2
    assert shlex.split(parts[1])[0] == "RVB_LIB=" + lib


def test_in_turn_without_a_parent_library():
    assert benchsteps.in_turn(2, None) == [("this", [], None)] * 2


def test_extra_arguments_and_a_relative_library():
    command = benchsteps.chain_command(["x"], [], [("gpu", ["--nrows", "16"], "lib.so")], 5)
    assert command == "RVB_LIB=%s timeout -k 10 5 x --nrows 16 --step gpu && x --step report" % shlex.quote(os.path.abspath("lib.so"))


def run_stub(tmp_path, names, step_timeout):
    stub, log, out = tmp_path / "stub.py", tmp_path / "log", tmp_path / "out.txt"
    stub.write_text(STUB)
    status = benchsteps.chain([sys.executable, str(stub)], ["--log", str(log)], [(name, [], None) for name in names], step_timeout, str(out))
    return status, log.read_text().split(), out


def test_all_steps_then_the_report(tmp_path):
    status, ran, out = run_stub(tmp_path, ["first", "second"], 20)
    assert status == 0 and ran == ["first", "second", "report"] and out.read_text() == "table\n"


def test_a_failing_step_ends_the_chain(tmp_path):
    status, ran, out = run_stub(tmp_path, ["first", "fails", "third"], 20)
    assert status == 3 and ran == ["first", "fails"] and not out.exists()


def test_a_step_past_its_time_limit_ends_the_chain(tmp_path):
    status, ran, out = run_stub(tmp_path, ["hangs", "second"], 1)
    assert status == 124 and ran == ["hangs"] and not out.exists()


def test_samples(tmp_path):
    s, waited = benchsteps.Samples(), []
    for rep in s.repetitions(1, 2):
        s.timed("call", lambda: None, lambda: waited.append(rep), lambda: [("kernel_a", 0.5), ("kernel_b", 0.25)])
        s.timed("plain", lambda: None, lambda: None)
        s.note("noted", rep)
    assert waited == [0, 1, 2]
    assert sorted(s.samples) == ["call", "call:kernel_a", "call:kernel_b", "noted", "plain"]
    assert s.samples["call:kernel_a"] == [0.5, 0.5] and s.samples["noted"] == [1.0, 2.0]          # the warm-up repetition dropped
    assert len(s.samples["call"]) == 2 and all(v >= 0 for v in s.samples["call"])
    s.restart()
    assert s.samples == {}
    s.note("x", 1)
    work = tmp_path / "work.jsonl"
    work.write_text('{"earlier": true}\n')
    s.dump(str(work), step="this", nbins=7)
    lines = work.read_text().splitlines()
    assert len(lines) == 2 and json.loads(lines[1]) == {"step": "this", "nbins": 7, "samples": {"x": [1.0]}}


def test_table_rows():
    t = benchsteps.Table(benchsteps.merge([{"step": "this", "samples": {"a": [1, 3], "a:k2": [2], "a:k1": [4]}}, {"step": "this", "samples": {"a": [2]}},
                                           {"step": "parent", "samples": {"a": [5]}}]))
    assert t.row("label", ("this", "a")) == 2 and t.row("other", ("parent", "b")) is None
    t.kernel_rows("this", "a")
    assert t.lines == ["  %-58s %8.3f [%.3f .. %.3f] (%d)" % ("label", 2, 1, 3, 3), "  %-58s not measured" % "other",
                       "  %-58s %8.3f [%.3f .. %.3f] (%d)" % ("      k1", 4, 4, 4, 1), "  %-58s %8.3f [%.3f .. %.3f] (%d)" % ("      k2", 2, 2, 2, 1)]
    assert t.med(("parent", "a")) == 5 and t.med(("parent", "b")) is None and t.spread(("this", "a")) == 2
