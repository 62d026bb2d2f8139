#!/usr/bin/env python3
"""Developer tool: what keeping a trace for new microphones costs and what a relisten (RVB_KEEP_LISTENER / rvb_relisten,
csrc/relisten_kernels.hip) takes, against the only other way to the same result, rvb_trace with the new microphone.  At workload C2 by
default (100 000 rays x 128 reflections in the 75 000-triangle cathedral, one context) it records, as medians over all repetitions with
their spread,

  (a) rvb_trace with keeping off               this library, and the parent's with --parent-lib (a build of the commit before the feature)
  (b) rvb_trace with RVB_KEEP_MATERIALS        this library
  (c) rvb_trace with RVB_KEEP_LISTENER too     this library; (c) - (b) is the cost of the 8 more bytes per record
  (d) rvb_relisten, its kernels broken out     this library, alternating between two microphones
  (n) rvb_relisten in natural order            this library with RVB_RELISTEN_ORDER=0: the kept grouping order ignored (a process of its own)

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  The
libraries are measured in processes of their own, `--rounds` times in turn (this, natural, parent, this, ...), so that all see the same
drift; within a process the variants alternate repetition by repetition.  Every GPU step is a child process under its own
`timeout -k 10`, the steps are chained with &&, and the table is written (--out) only when all of them ended well.

    python tools/relisten_bench.py [--parent-lib PATH] [--rays N] [--reflections K] [--triangles T] [--repeats R] [--rounds M] [--out FILE]
"""
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

OTHER_MIC = (-10.28, 3.85, -2.24)


def step(args):
    """One GPU process: --step this | natural | parent.  Appends one JSON line of raw samples to the work file."""
    import rvb_import
    rvb_import.load()
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    samples = {}

    def note(name, value):
        samples.setdefault(name, []).append(float(value))

    def timed(ctx, prefix, call):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        note(prefix, (time.perf_counter() - t0) * 1e3)
        for k, v in ctx.last_timings():
            note(prefix + ":" + k, v)

    off = capi.Context(0)
    off.set_scene(scene)
    off.set_directions(dirs)
    if args.step == "parent":
        for rep in range(args.warmup + args.repeats):
            if rep == args.warmup:
                samples.clear()
            timed(off, "a", lambda: off.trace(mic, src, args.reflections, air))
            timed(off, "a2", lambda: off.trace(OTHER_MIC, src, args.reflections, air))
    else:
        materials, listener = capi.Context(0), capi.Context(0)
        for c in (materials, listener):
            c.share_scene(off)
            c.set_directions(dirs)
        materials.keep_paths(True)
        listener.keep_paths(True, listener=True)
        for rep in range(args.warmup + args.repeats):
            if rep == args.warmup:
                samples.clear()
            if args.step == "this":
                timed(off, "a", lambda: off.trace(mic, src, args.reflections, air))
                timed(off, "a2", lambda: off.trace(OTHER_MIC, src, args.reflections, air))
                timed(materials, "b", lambda: materials.trace(mic, src, args.reflections, air))
            if args.step == "this" or rep == 0:
                timed(listener, "c", lambda: listener.trace(mic, src, args.reflections, air))
            name = "d" if args.step == "this" else "n"
            for m in (OTHER_MIC, mic):                               # to the other microphone and back
                timed(listener, name, lambda: listener.relisten(m))
        materials.close()
        listener.close()
    off.close()
    with open(args.work, "a") as f:
        f.write(json.dumps({"step": args.step, "lib": capi.LIB_PATH, "samples": samples}) + "\n")


def report(args):
    merged = {}
    for line in open(args.work):
        rec = json.loads(line)
        for k, v in rec["samples"].items():
            if rec["step"] == "natural" and not k.startswith("n"):
                continue
            merged.setdefault(("this" if rec["step"] == "natural" else rec["step"], k), []).extend(v)
    nrecords = args.rays * args.reflections
    lines = ["relisten bench: %d rays x %d reflections = %d records (%.0f MB of records, %.0f MB kept for re-shading, %.0f MB more for listeners), "
             "cathedral %d triangles, one context" % (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, nrecords * 16 / 1e6, nrecords * 8 / 1e6, args.triangles),
             "median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings"]

    def med(key):
        return statistics.median(merged[key]) if key in merged else None

    def row(label, key):
        if key not in merged:
            lines.append("  %-58s not measured" % label)
            return
        v = merged[key]
        lines.append("  %-58s %8.3f [%.3f .. %.3f] (%d)" % (label, statistics.median(v), min(v), max(v), len(v)))

    def kernels(prefix, indent="      "):
        for k in sorted(k for s, k in merged if s == "this" and k.startswith(prefix + ":")):
            row(indent + k[len(prefix) + 1:], ("this", k))

    row("(a) rvb_trace, keeping off, this library", ("this", "a"))
    row("(a) rvb_trace, keeping off, parent library", ("parent", "a"))
    row("(a) the same with the other microphone, this library", ("this", "a2"))
    row("(a) the same with the other microphone, parent library", ("parent", "a2"))
    for k in sorted(k for s, k in merged if s == "this" and k.startswith("a:")):
        row("      " + k[2:] + " (this)", ("this", k))
        row("      " + k[2:] + " (parent)", ("parent", k))
    row("(b) rvb_trace, RVB_KEEP_MATERIALS", ("this", "b"))
    kernels("b")
    row("(c) rvb_trace, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER", ("this", "c"))
    kernels("c")
    row("(d) rvb_relisten", ("this", "d"))
    kernels("d")
    row("(n) rvb_relisten, natural order (RVB_RELISTEN_ORDER=0)", ("this", "n"))
    kernels("n")
    lines.append("bars:")
    a, ap, b, c, d, n = (med(k) for k in (("this", "a"), ("parent", "a"), ("this", "b"), ("this", "c"), ("this", "d"), ("this", "n")))
    if a is not None and ap is not None:
        spread = max(merged[("parent", "a")]) - min(merged[("parent", "a")])
        lines.append("  keeping off against the parent: %.3f ms against %.3f ms, difference %+.3f ms; spread of the parent's repetitions %.3f ms (max - min)" %
                     (a, ap, a - ap, spread))
        if d is not None:
            both = merged[("parent", "a")] + merged.get(("parent", "a2"), [])
            ref = statistics.median(both)
            lines.append("  a new microphone: rvb_relisten %.3f ms against the parent's rvb_trace %.3f ms (both microphones): %.3f ms less, %s the spread; ratio %.2f" %
                         (d, ref, ref - d, "more than" if ref - d > spread else "NOT more than", ref / d))
    if b is not None and c is not None:
        kb, kc = med(("this", "b:path_keep_kernel")), med(("this", "c:path_keep_kernel"))
        lines.append("  cost of keeping for listeners: (c) - (b) = %+.3f ms; path_keep_kernel %.3f -> %.3f ms" % (c - b, kb, kc))
    rk = med(("this", "d:relisten_records_kernel"))
    if rk is not None:
        lines.append("  relisten_records_kernel moves 104 B per record (16 + 8 + 16 read, 64 written): %.2f TB/s" % (nrecords * 104 / (rk * 1e-3) / 1e12))
    if d is not None and n is not None:
        lines.append("  kept grouping order against natural order: %.3f ms against %.3f ms per relisten: the kept order is %s" %
                     (d, n, "faster" if d < n else "NOT faster"))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    p.add_argument("--repeats", type=int, default=12, help="per round and library (>= 20 in all with the default two rounds)")
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--parent-lib", default=None, help="librvb_hip.so built from the commit before the feature")
    p.add_argument("--step-timeout", type=int, default=240)
    p.add_argument("--out", default=None)
    p.add_argument("--step", default=None, help=argparse.SUPPRESS)
    p.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.step == "report":
        return report(args)
    if args.step:
        return step(args)
    work = os.path.join(tempfile.mkdtemp(prefix="relisten_bench_"), "samples.jsonl")
    shape = ["--rays", str(args.rays), "--reflections", str(args.reflections), "--triangles", str(args.triangles),
             "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    steps = []
    for _ in range(args.rounds):
        steps.append(("", "this"))
        steps.append(("RVB_RELISTEN_ORDER=0 ", "natural"))
        if args.parent_lib:
            steps.append(("RVB_LIB=%s " % shlex.quote(os.path.abspath(args.parent_lib)), "parent"))
    parts = []
    for env, name in steps:      # every GPU step under a time limit of its own; a step that fails ends the chain
        parts.append("%stimeout -k 10 %d %s" % (env, args.step_timeout, " ".join(shlex.quote(x) for x in me + shape + ["--step", name])))
    parts.append(" ".join(shlex.quote(x) for x in me + shape + ["--step", "report"] + (["--out", args.out] if args.out else [])))
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
