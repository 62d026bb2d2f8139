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
import sys

import benchsteps
from benchsteps import Samples, Table

FACING, UP = (0.6, 0.0, 0.8), (0.0, 1.0, 0.0)


def step(args):
    """One GPU process: --step this | parent.  Appends one JSON line of raw samples to the work file."""
    import numpy as np
    benchsteps.load_library()
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    s = Samples()

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
    for rep in s.repetitions(args.warmup, args.repeats):
        for name, c in variants:
            s.timed(name, lambda: c.trace(mic, src, args.reflections, air), c.synchronize, c.last_timings)
    for _, c in reversed(variants):
        c.close()
    s.dump(args.work, step=args.step, lib=capi.LIB_PATH)


def report(args):
    t = Table.load(args.work)
    nrecords = args.rays * args.reflections
    t.line("source table bench: %d rays x %d reflections = %d records (%.0f MB of records, %.1f MB of per-ray gains), cathedral %d triangles, "
           "one context per variant" % (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, args.rays * 32 / 1e6, args.triangles))
    t.line("median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings")
    t.row("(a) rvb_trace, directivity off, this library", ("this", "a"))
    t.row("(a) rvb_trace, directivity off, parent library", ("parent", "a"))
    for k in t.kernels("this", "a"):
        t.row("      " + k + " (this)", ("this", "a:" + k))
        t.row("      " + k + " (parent)", ("parent", "a:" + k))
    t.row("(p) rvb_trace, polar pattern", ("this", "p"))
    t.row("      source_pattern_kernel", ("this", "p:source_pattern_kernel"))
    t.row("(t) rvb_trace, table", ("this", "t"))
    t.row("      source_table_rays_kernel", ("this", "t:source_table_rays_kernel"))
    t.row("      source_table_kernel", ("this", "t:source_table_kernel"))
    t.line("bars:")
    a, ap = t.med(("this", "a")), t.med(("parent", "a"))
    if a is not None and ap is not None:
        s = t.spread(("parent", "a"))
        t.line("  directivity off against the parent: %.3f ms against %.3f ms, difference %+.3f ms, %s the spread of the parent's repetitions, "
               "%.3f ms (max - min)" % (a, ap, a - ap, "within" if abs(a - ap) <= s else "OUTSIDE", s))
    kp, kt, kr = (t.med(("this", k)) for k in ("p:source_pattern_kernel", "t:source_table_kernel", "t:source_table_rays_kernel"))
    if kp is not None and kt is not None:
        s = t.spread(("this", "p:source_pattern_kernel"))
        t.line("  source_table_kernel against source_pattern_kernel: %.3f ms against %.3f ms, difference %+.3f ms; spread of the pattern kernel "
               "%.3f ms (max - min): the table pass is %s" % (kt, kp, kt - kp, s, "SLOWER by more than the spread" if kt - kp > s else "not slower by more than the spread"))
        t.line("  both move 128 B per record (64 read, 64 written): pattern %.2f TB/s, table %.2f TB/s; the row selections of all rays take %.3f ms" %
               (nrecords * 128 / (kp * 1e-3) / 1e12, nrecords * 128 / (kt * 1e-3) / 1e12, kr))
    p, tb = t.med(("this", "p")), t.med(("this", "t"))
    if a is not None and p is not None and tb is not None:
        t.line("  a directivity costs a trace: pattern %+.3f ms, table %+.3f ms" % (p - a, tb - a))
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
