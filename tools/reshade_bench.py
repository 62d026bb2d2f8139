#!/usr/bin/env python3
"""Developer tool: what keeping the paths of a trace costs and what a re-shade (rvb_keep_paths / rvb_reshade, csrc/reshade_kernels.hip)
takes, against the only other way to the same result, rvb_set_scene + rvb_trace.  At workload C2 by default (100 000 rays x 128
reflections in the 75 000-triangle cathedral, one context) it records, as medians over all repetitions with their spread,

  (a) rvb_trace with keeping off             this library, and the parent's with --parent-lib (a build of the commit before the feature)
  (b) rvb_trace with keeping on              this library
  (c) path_keep_kernel alone                 this library (from the traces of (b))
  (d) rvb_reshade, its kernels broken out    this library; the shadow kernel of the same traces beside it
  (e) rvb_set_scene + rvb_trace              the parent's library (today's only way to the same result)

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  The two
libraries are measured in processes of their own, `--rounds` times in turn (this, parent, this, parent, ...), so that both see the same
drift; within a process the variants alternate repetition by repetition.  Every GPU step is a child process under its own
`timeout -k 10`, the steps are chained with &&, and the table is written (--out) only when all of them ended well.

    python tools/reshade_bench.py [--parent-lib PATH] [--rays N] [--reflections K] [--triangles T] [--repeats R] [--rounds M] [--out FILE]
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RECORD_FLOOR_TBS = 6.6          # what attenuate_kernel reaches (README): the floor of a streaming pass is its bytes at this rate


def other_surfaces(surfaces):
    rng = np.random.default_rng(7)
    b = surfaces.copy()
    b["specular"] = rng.uniform(0.55, 0.9, b["specular"].shape).astype(np.float32)
    b["diffuse"] = rng.uniform(0.3, 0.85, b["diffuse"].shape).astype(np.float32)
    return b


def step(args):
    """One GPU process: --step this | parent.  Appends one JSON line of raw samples to the work file."""
    import rvb_import
    rvb_import.load()
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air_a = dtypes.AIR_COEFFICIENTS
    air_b = (air_a * np.float32(1.7) - np.float32(1e-4)).astype(np.float32)
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    samples = {}

    def note(name, value):
        samples.setdefault(name, []).append(float(value))

    def timed_trace(ctx, prefix):
        t0 = time.perf_counter()
        ctx.trace(mic, src, args.reflections, air_a)
        ctx.synchronize()
        note(prefix, (time.perf_counter() - t0) * 1e3)
        for k, v in ctx.last_timings():
            note(prefix + ":" + k, v)

    off = capi.Context(0)
    off.set_scene(scene)
    off.set_directions(dirs)
    if args.step == "this":
        on = capi.Context(0)
        on.share_scene(off)
        on.set_directions(dirs)
        on.keep_paths(True)
        table_b = other_surfaces(scene[2])
        for rep in range(args.warmup + args.repeats):
            if rep == args.warmup:
                samples.clear()
            timed_trace(off, "a")
            timed_trace(on, "b")
            for name, table, air in (("d", table_b, air_b), ("d", None, air_a)):      # to the other materials and back
                t0 = time.perf_counter()
                on.reshade(table, air)
                on.synchronize()
                note(name, (time.perf_counter() - t0) * 1e3)
                for k, v in on.last_timings():
                    note(name + ":" + k, v)
        on.close()
    else:
        for rep in range(args.warmup + args.repeats):
            if rep == args.warmup:
                samples.clear()
            timed_trace(off, "a")
            if rep % 2 == 0:            # (a host BVH build each: half as many)
                t0 = time.perf_counter()
                off.set_scene(scene)
                off.trace(mic, src, args.reflections, air_a)
                off.synchronize()
                note("e", (time.perf_counter() - t0) * 1e3)
    off.close()
    with open(args.work, "a") as f:
        f.write(json.dumps({"step": args.step, "lib": capi.LIB_PATH, "samples": samples}) + "\n")


def report(args):
    merged = {}
    for line in open(args.work):
        rec = json.loads(line)
        for k, v in rec["samples"].items():
            merged.setdefault((rec["step"], k), []).extend(v)
    nrecords = args.rays * args.reflections
    lines = ["reshade bench: %d rays x %d reflections = %d records (%.0f MB of records, %.0f MB kept), cathedral %d triangles, one context" %
             (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, nrecords * 16 / 1e6, args.triangles),
             "median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings"]

    def med(key):
        return statistics.median(merged[key]) if key in merged else None

    def row(label, key):
        if key not in merged:
            lines.append("  %-58s not measured" % label)
            return
        v = merged[key]
        lines.append("  %-58s %8.3f [%.3f .. %.3f] (%d)" % (label, statistics.median(v), min(v), max(v), len(v)))

    row("(a) rvb_trace, keeping off, this library", ("this", "a"))
    row("(a) rvb_trace, keeping off, parent library", ("parent", "a"))
    for k in sorted(k for s, k in merged if s == "this" and k.startswith("a:")):
        row("      " + k[2:] + " (this)", ("this", k))
        row("      " + k[2:] + " (parent)", ("parent", k))
    row("(b) rvb_trace, keeping on", ("this", "b"))
    for k in sorted(k for s, k in merged if s == "this" and k.startswith("b:")):
        row("      " + k[2:], ("this", k))
    row("(c) path_keep_kernel", ("this", "b:path_keep_kernel"))
    row("(d) rvb_reshade", ("this", "d"))
    for k in sorted(k for s, k in merged if s == "this" and k.startswith("d:")):
        row("      " + k[2:], ("this", k))
    row("(e) rvb_set_scene + rvb_trace, parent library", ("parent", "e"))
    a, ap, b, c, d, e = med(("this", "a")), med(("parent", "a")), med(("this", "b")), med(("this", "b:path_keep_kernel")), med(("this", "d")), med(("parent", "e"))
    shadow = [med(("this", k)) for s, k in merged if s == "this" and k.startswith("b:shadow")]
    rk = med(("this", "d:reshade_kernel"))
    lines.append("bars:")
    if rk is not None and shadow:
        lines.append("  reshade_kernel %.3f ms against the shadow kernel of the same traces %.3f ms: %s" % (rk, shadow[0], "below" if rk < shadow[0] else "NOT below"))
        lines.append("    reshade_kernel moves 80 B per record (16 + 32 read, 32 written): %.2f TB/s" % (nrecords * 80 / (rk * 1e-3) / 1e12))
    if a is not None and ap is not None:
        spread = max(merged[("parent", "a")]) - min(merged[("parent", "a")])
        lines.append("  keeping off against the parent: %.3f ms against %.3f ms, difference %+.3f ms; spread of the parent's repetitions %.3f ms (max - min)" %
                     (a, ap, a - ap, spread))
    if a is not None and b is not None and c is not None:
        floor = nrecords * 48 / (RECORD_FLOOR_TBS * 1e12) * 1e3
        lines.append("  cost of keeping: (b) - (a) = %.3f ms, path_keep_kernel %.3f ms; floor (32 B read + 16 B written per record at %.1f TB/s) %.3f ms: %.2f x the floor" %
                     (b - a, c, RECORD_FLOOR_TBS, floor, c / floor))
    if d is not None and e is not None:
        lines.append("  a new material set: rvb_reshade %.3f ms against rvb_set_scene + rvb_trace %.3f ms (%.0f x)" % (d, e, e / d))
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
    work = os.path.join(tempfile.mkdtemp(prefix="reshade_bench_"), "samples.jsonl")
    shape = ["--rays", str(args.rays), "--reflections", str(args.reflections), "--triangles", str(args.triangles),
             "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    steps = []
    for _ in range(args.rounds):
        steps.append((None, "this"))
        if args.parent_lib:
            steps.append((os.path.abspath(args.parent_lib), "parent"))
    parts = []
    for lib, name in steps:      # every GPU step under a time limit of its own; a step that fails ends the chain
        env = "RVB_LIB=%s " % shlex.quote(lib) if lib else ""
        parts.append("%stimeout -k 10 %d %s" % (env, args.step_timeout, " ".join(shlex.quote(x) for x in me + shape + ["--step", name])))
    parts.append(" ".join(shlex.quote(x) for x in me + shape + ["--step", "report"] + (["--out", args.out] if args.out else [])))
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
