"""What the feature benches (tools/*_bench.py with GPU steps) share: the step chain, the sample store, the report table and a few inputs.

The rule of the chain: every GPU step is a child process of its own under its own `timeout -k 10`, the steps are joined with &&, so a
step that fails or runs out of time starts nothing after it, and the report step, which opens no GPU and has no time limit, comes last:
the table is printed and written (--out) only when every step ended well.

Plain Python: neither torch nor the library is imported here, so a machine without a GPU can import and test it."""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HELP = {"parent_lib": "librvb_hip.so built from the commit before the feature"}


def chain_command(me, shape, steps, step_timeout, out=None):
    """The shell command of a bench.  me: the words that start the tool; shape: the arguments every step and the report get;
    steps: (name, extra arguments, library or None) per GPU step, a library being the librvb_hip.so the step loads through RVB_LIB."""
    def words(*more):
        return " ".join(shlex.quote(x) for x in [*me, *shape, *more])
    parts = ["%stimeout -k 10 %d %s" % ("RVB_LIB=%s " % shlex.quote(os.path.abspath(lib)) if lib else "", step_timeout, words(*extra, "--step", name))
             for name, extra, lib in steps]
    return " && ".join(parts + [words("--step", "report", *(["--out", out] if out else []))])


def chain(me, shape, steps, step_timeout, out=None):
    return subprocess.call(["bash", "-c", chain_command(me, shape, steps, step_timeout, out)])


def in_turn(rounds, parent_lib):
    """this, parent, this, parent, ... for so many rounds, so that both libraries see the same drift; this alone without a parent library."""
    return [step for _ in range(rounds) for step in [("this", [], None)] + ([("parent", [], parent_lib)] if parent_lib else [])]


def add_common_arguments(parser, repeats, warmup, step_timeout, parent_lib=False, rounds=None, help=HELP):
    """The options every feature bench has, visible and hidden; help: texts by destination."""
    parser.add_argument("--repeats", type=int, default=repeats, help=help.get("repeats"))
    parser.add_argument("--warmup", type=int, default=warmup)
    if rounds is not None:
        parser.add_argument("--rounds", type=int, default=rounds, help=help.get("rounds"))
    if parent_lib:
        parser.add_argument("--parent-lib", default=None, help=help.get("parent_lib"))
    parser.add_argument("--step-timeout", type=int, default=step_timeout)
    parser.add_argument("--out", default=None)
    parser.add_argument("--step", default=None, help=argparse.SUPPRESS)
    parser.add_argument("--work", default=None, help=argparse.SUPPRESS)


def shape(args, *names):
    """The named options as words, with the values they have in args: what a tool hands on to its steps and its report."""
    return [word for name in names for word in ("--" + name.replace("_", "-"), str(getattr(args, name)))]


def run(args, step_fns, report_fn, build_steps):
    """What every main() ends in.  --step report: the report; --step NAME: step_fns[NAME]; neither: a work file of its own and the chain of
    build_steps(args) = (shape, steps), with --work appended to the shape."""
    if args.step == "report":
        return report_fn(args)
    if args.step:
        return step_fns[args.step](args)
    me = os.path.abspath(sys.argv[0])
    work = os.path.join(tempfile.mkdtemp(prefix=os.path.splitext(os.path.basename(me))[0] + "_"), "samples.jsonl")
    shape, steps = build_steps(args)
    return chain([sys.executable, me], shape + ["--work", work], steps, args.step_timeout, args.out)


class Samples:
    """The raw samples of one GPU step: milliseconds by name."""

    def __init__(self):
        self.samples = {}

    def note(self, name, value):
        self.samples.setdefault(name, []).append(float(value))

    def timed(self, name, call, wait, timings=None):
        """The host clock from the call to the end of wait(); then the (kernel, ms) pairs of timings() as name:kernel."""
        t0 = time.perf_counter()
        call()
        wait()
        self.note(name, (time.perf_counter() - t0) * 1e3)
        for k, v in timings() if timings else ():
            self.note(name + ":" + k, v)

    def restart(self):
        """The end of the warm-up: what was recorded so far does not count."""
        self.samples.clear()

    def repetitions(self, warmup, repeats):
        for rep in range(warmup + repeats):
            if rep == warmup:
                self.restart()
            yield rep

    def dump(self, path, **fields):
        """One more JSON line in the work file: the fields and the samples."""
        with open(path, "a") as f:
            f.write(json.dumps(dict(fields, samples=self.samples)) + "\n")


def records(path):
    return [json.loads(line) for line in open(path).read().splitlines()]


def merge(recs, key=lambda rec, name: (rec["step"], name)):
    """The samples of several work-file lines pooled under key(record, name); a key of None leaves a sample list out."""
    merged = {}
    for rec in recs:
        for name, values in rec["samples"].items():
            if key(rec, name) is not None:
                merged.setdefault(key(rec, name), []).extend(values)
    return merged


class Table:
    """The report: lines of text, and rows over a dict of sample lists (self.samples; a tool with several sections sets it per section).
    Keys are (step, name) where `step` is given, as merge() makes them, and plain names where it is None."""

    def __init__(self, samples=None, label=58, value=8):
        self.samples, self.lines = samples or {}, []
        self.measured, self.missing = "  %%-%ds %%%d.3f [%%.3f .. %%.3f] (%%d)%%s" % (label, value), "  %%-%ds not measured" % label

    @classmethod
    def load(cls, path, key=None, **widths):
        return cls(merge(records(path), *([key] if key else [])), **widths)

    def line(self, text):
        self.lines.append(text)

    def med(self, key):
        return statistics.median(self.samples[key]) if key in self.samples else None

    def spread(self, key):
        return max(self.samples[key]) - min(self.samples[key])

    def row(self, label, key, tail=""):
        """One row, median [min .. max] (n); returns the median, or None where nothing was measured."""
        if key not in self.samples:
            return self.line(self.missing % label)
        v = self.samples[key]
        self.line(self.measured % (label, statistics.median(v), min(v), max(v), len(v), tail))
        return statistics.median(v)

    def kernels(self, step, prefix):
        """The sorted kernel names of a timed call: the part after `prefix:` of the keys that start with it."""
        names = (k for s, k in self.samples if s == step) if step is not None else self.samples
        return sorted(k[len(prefix) + 1:] for k in names if k.startswith(prefix + ":"))

    def kernel_rows(self, step, prefix, indent="      "):
        for k in self.kernels(step, prefix):
            self.row(indent + k, prefix + ":" + k if step is None else (step, prefix + ":" + k))

    def emit(self, out=None, notes=""):
        """Prints the table and, with out, writes it there (notes: text to keep below it); returns it."""
        text = "\n".join(self.lines)
        print(text, flush=True)
        if out:
            with open(out, "w") as f:
                f.write(text + "\n" + notes)
        return text


def load_library():
    """The prologue of a GPU step: the package importable from this tree, before torch or the package is imported."""
    import rvb_import
    rvb_import.load()


def other_surfaces(surfaces):
    """Another material table for the same scene, seeded."""
    import numpy as np
    rng = np.random.default_rng(11)
    b = surfaces.copy()
    b["specular"] = rng.uniform(0.3, 0.9, b["specular"].shape).astype(np.float32)
    b["diffuse"] = rng.uniform(0.3, 0.9, b["diffuse"].shape).astype(np.float32)
    return b


def tolerate_an_older_library():
    """The binding is strict: it sets the argument types of every entry point when it loads the library, and a parent commit's
    library lacks the newest ones.  For the parent's process alone, the loader hands out a stand-in for an rvb_* symbol that the
    library does not export; the step never calls it."""
    import ctypes

    class Missing:
        restype = argtypes = None

    class Older(ctypes.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if not name.startswith("rvb_"):
                    raise
                return Missing()

    ctypes.CDLL = Older
