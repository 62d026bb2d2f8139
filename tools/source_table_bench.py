#!/usr/bin/env python3
"""Developer tool: what a directivity at the source end costs a trace — the first-order polar pattern (rvb_set_source_pattern) against
the gain table (rvb_set_source_table, csrc/source_kernels.hip).  At workload C2 by default (100 000 rays x 128 reflections in the
75 000-triangle cathedral, one context per variant, one shared scene) it records, as medians over all repetitions with their spread,

  (a) rvb_trace with the directivity off       this library, and the parent's with --parent-lib (a build of the commit before the feature)
  (p) rvb_trace with a polar pattern           this library; source_pattern_kernel broken out
  (t) rvb_trace with a table                   this library; source_table_rays_kernel and source_table_kernel broken out

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  The three
variants alternate repetition by repetition inside one process, so the three kernels are measured in the same run; the libraries are
measured in processes of their own, `--rounds` times in turn (this, parent, this, ...), so that both see the same drift.  Every GPU step
is a child process under its own `timeout -k 10`, the steps are chained with &&, and the table is written (--out) only when all of
them ended well.

    python tools/source_table_bench.py [--parent-lib PATH] [--rays N] [--reflections K] [--triangles T] [--repeats R] [--rounds M] [--out FILE]
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

FACING, UP = (0.6, 0.0, 0.8), (0.0, 1.0, 0.0)


def step(args):
    """One GPU process: --step this | parent.  Appends one JSON line of raw samples to the work file."""
    import numpy as np
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

    def timed(ctx, prefix):
        t0 = time.perf_counter()
        ctx.trace(mic, src, args.reflections, air)
        ctx.synchronize()
        note(prefix, (time.perf_counter() - t0) * 1e3)
        for k, v in ctx.last_timings():
            note(prefix + ":" + k, v)

    off = capi.Context(0)
    off.set_scene(scene)
    off.set_directions(dirs)
    variants = [("a", off)]
    if args.step == "this":
        from parallel_reverb_raytracer_amd import directivity
        shape = np.linspace(0.0, 1.0, 8)
        pattern, table = capi.Context(0), capi.Context(0)
        for c in (pattern, table):
            c.share_scene(off)
            c.set_directions(dirs)
        pattern.set_source_pattern(FACING, shape)
        table.set_source_table(directivity.table_from_function(directivity.polar_pattern(shape)), FACING, UP)
        variants += [("p", pattern), ("t", table)]
    for rep in range(args.warmup + args.repeats):
        if rep == args.warmup:
            samples.clear()
        for name, c in variants:
            timed(c, name)
    for _, c in reversed(variants):
        c.close()
    with open(args.work, "a") as f:
        f.write(json.dumps({"step": args.step, "lib": capi.LIB_PATH, "samples": samples}) + "\n")


def report(args):
    merged = {}
    for line in open(args.work):
        rec = json.loads(line)
        for k, v in rec["samples"].items():
            merged.setdefault((rec["step"], k), []).extend(v)
    nrecords = args.rays * args.reflections
    lines = ["source table bench: %d rays x %d reflections = %d records (%.0f MB of records, %.1f MB of per-ray gains), cathedral %d triangles, "
             "one context per variant" % (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, args.rays * 32 / 1e6, args.triangles),
             "median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings"]

    def med(key):
        return statistics.median(merged[key]) if key in merged else None

    def spread(key):
        return max(merged[key]) - min(merged[key])

    def row(label, key):
        if key not in merged:
            lines.append("  %-58s not measured" % label)
            return
        v = merged[key]
        lines.append("  %-58s %8.3f [%.3f .. %.3f] (%d)" % (label, statistics.median(v), min(v), max(v), len(v)))

    row("(a) rvb_trace, directivity off, this library", ("this", "a"))
    row("(a) rvb_trace, directivity off, parent library", ("parent", "a"))
    for k in sorted(k for s, k in merged if s == "this" and k.startswith("a:")):
        row("      " + k[2:] + " (this)", ("this", k))
        row("      " + k[2:] + " (parent)", ("parent", k))
    row("(p) rvb_trace, polar pattern", ("this", "p"))
    row("      source_pattern_kernel", ("this", "p:source_pattern_kernel"))
    row("(t) rvb_trace, table", ("this", "t"))
    row("      source_table_rays_kernel", ("this", "t:source_table_rays_kernel"))
    row("      source_table_kernel", ("this", "t:source_table_kernel"))
    lines.append("bars:")
    a, ap = med(("this", "a")), med(("parent", "a"))
    if a is not None and ap is not None:
        s = spread(("parent", "a"))
        lines.append("  directivity off against the parent: %.3f ms against %.3f ms, difference %+.3f ms, %s the spread of the parent's repetitions, "
                     "%.3f ms (max - min)" % (a, ap, a - ap, "within" if abs(a - ap) <= s else "OUTSIDE", s))
    kp, kt, kr = med(("this", "p:source_pattern_kernel")), med(("this", "t:source_table_kernel")), med(("this", "t:source_table_rays_kernel"))
    if kp is not None and kt is not None:
        s = spread(("this", "p:source_pattern_kernel"))
        lines.append("  source_table_kernel against source_pattern_kernel: %.3f ms against %.3f ms, difference %+.3f ms; spread of the pattern kernel "
                     "%.3f ms (max - min): the table pass is %s" % (kt, kp, kt - kp, s, "SLOWER by more than the spread" if kt - kp > s else "not slower by more than the spread"))
        lines.append("  both move 128 B per record (64 read, 64 written): pattern %.2f TB/s, table %.2f TB/s; the row selections of all rays take %.3f ms" %
                     (nrecords * 128 / (kp * 1e-3) / 1e12, nrecords * 128 / (kt * 1e-3) / 1e12, kr))
    p, t = med(("this", "p")), med(("this", "t"))
    if a is not None and p is not None and t is not None:
        lines.append("  a directivity costs a trace: pattern %+.3f ms, table %+.3f ms" % (p - a, t - a))
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
    work = os.path.join(tempfile.mkdtemp(prefix="source_table_bench_"), "samples.jsonl")
    shape = ["--rays", str(args.rays), "--reflections", str(args.reflections), "--triangles", str(args.triangles),
             "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    steps = []
    for _ in range(args.rounds):
        steps.append(("", "this"))
        if args.parent_lib:
            steps.append(("RVB_LIB=%s " % shlex.quote(os.path.abspath(args.parent_lib)), "parent"))
    parts = []
    for env, name in steps:      # every GPU step under a time limit of its own; a step that fails ends the chain
        parts.append("%stimeout -k 10 %d %s" % (env, args.step_timeout, " ".join(shlex.quote(x) for x in me + shape + ["--step", name])))
    parts.append(" ".join(shlex.quote(x) for x in me + shape + ["--step", "report"] + (["--out", args.out] if args.out else [])))
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
