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
import sys

import numpy as np

import benchsteps
from benchsteps import Samples, Table

RECORD_FLOOR_TBS = 6.6          # what attenuate_kernel reaches (README): the floor of a streaming pass is its bytes at this rate


def other_surfaces(surfaces):
    rng = np.random.default_rng(7)
    b = surfaces.copy()
    b["specular"] = rng.uniform(0.55, 0.9, b["specular"].shape).astype(np.float32)
    b["diffuse"] = rng.uniform(0.3, 0.85, b["diffuse"].shape).astype(np.float32)
    return b


def step(args):
    """One GPU process: --step this | parent.  Appends one JSON line of raw samples to the work file."""
    benchsteps.load_library()
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air_a = dtypes.AIR_COEFFICIENTS
    air_b = (air_a * np.float32(1.7) - np.float32(1e-4)).astype(np.float32)
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    s = Samples()

    def timed(ctx, name, call):
        s.timed(name, call, ctx.synchronize, ctx.last_timings)

    def timed_trace(ctx, name):
        timed(ctx, name, lambda: ctx.trace(mic, src, args.reflections, air_a))

    off = capi.Context(0)
    off.set_scene(scene)
    off.set_directions(dirs)
    if args.step == "this":
        on = capi.Context(0)
        on.share_scene(off)
        on.set_directions(dirs)
        on.keep_paths(True)
        table_b = other_surfaces(scene[2])
        for rep in s.repetitions(args.warmup, args.repeats):
            timed_trace(off, "a")
            timed_trace(on, "b")
            for table, air in ((table_b, air_b), (None, air_a)):      # to the other materials and back
                timed(on, "d", lambda: on.reshade(table, air))
        on.close()
    else:
        def set_scene_and_trace():
            off.set_scene(scene)
            off.trace(mic, src, args.reflections, air_a)
        for rep in s.repetitions(args.warmup, args.repeats):
            timed_trace(off, "a")
            if rep % 2 == 0:            # (a host BVH build each: half as many)
                s.timed("e", set_scene_and_trace, off.synchronize)
    off.close()
    s.dump(args.work, step=args.step, lib=capi.LIB_PATH)


def report(args):
    t = Table.load(args.work)
    nrecords = args.rays * args.reflections
    t.line("reshade bench: %d rays x %d reflections = %d records (%.0f MB of records, %.0f MB kept), cathedral %d triangles, one context" %
           (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, nrecords * 16 / 1e6, args.triangles))
    t.line("median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings")
    t.row("(a) rvb_trace, keeping off, this library", ("this", "a"))
    t.row("(a) rvb_trace, keeping off, parent library", ("parent", "a"))
    for k in t.kernels("this", "a"):
        t.row("      " + k + " (this)", ("this", "a:" + k))
        t.row("      " + k + " (parent)", ("parent", "a:" + k))
    t.row("(b) rvb_trace, keeping on", ("this", "b"))
    t.kernel_rows("this", "b")
    t.row("(c) path_keep_kernel", ("this", "b:path_keep_kernel"))
    t.row("(d) rvb_reshade", ("this", "d"))
    t.kernel_rows("this", "d")
    t.row("(e) rvb_set_scene + rvb_trace, parent library", ("parent", "e"))
    a, ap, b, c, d, e = (t.med(k) for k in (("this", "a"), ("parent", "a"), ("this", "b"), ("this", "b:path_keep_kernel"), ("this", "d"), ("parent", "e")))
    shadow = [t.med(("this", k)) for s, k in t.samples if s == "this" and k.startswith("b:shadow")]
    rk = t.med(("this", "d:reshade_kernel"))
    t.line("bars:")
    if rk is not None and shadow:
        t.line("  reshade_kernel %.3f ms against the shadow kernel of the same traces %.3f ms: %s" % (rk, shadow[0], "below" if rk < shadow[0] else "NOT below"))
        t.line("    reshade_kernel moves 80 B per record (16 + 32 read, 32 written): %.2f TB/s" % (nrecords * 80 / (rk * 1e-3) / 1e12))
    if a is not None and ap is not None:
        t.line("  keeping off against the parent: %.3f ms against %.3f ms, difference %+.3f ms; spread of the parent's repetitions %.3f ms (max - min)" %
               (a, ap, a - ap, t.spread(("parent", "a"))))
    if a is not None and b is not None and c is not None:
        floor = nrecords * 48 / (RECORD_FLOOR_TBS * 1e12) * 1e3
        t.line("  cost of keeping: (b) - (a) = %.3f ms, path_keep_kernel %.3f ms; floor (32 B read + 16 B written per record at %.1f TB/s) %.3f ms: %.2f x the floor" %
               (b - a, c, RECORD_FLOOR_TBS, floor, c / floor))
    if d is not None and e is not None:
        t.line("  a new material set: rvb_reshade %.3f ms against rvb_set_scene + rvb_trace %.3f ms (%.0f x)" % (d, e, e / d))
    t.emit(args.out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    benchsteps.add_common_arguments(p, repeats=12, warmup=3, step_timeout=240, parent_lib=True, rounds=2,
                                    help=dict(benchsteps.HELP, repeats="per round and library (>= 20 in all with the default two rounds)"))
    args = p.parse_args()
    return benchsteps.run(args, dict.fromkeys(("this", "parent"), step), report, lambda args: (
        benchsteps.shape(args, "rays", "reflections", "triangles", "repeats", "warmup"), benchsteps.in_turn(args.rounds, args.parent_lib)))


if __name__ == "__main__":
    sys.exit(main())
