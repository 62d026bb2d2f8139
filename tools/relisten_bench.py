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
import os
import statistics
import sys

import benchsteps
from benchsteps import Samples, Table

OTHER_MIC = (-10.28, 3.85, -2.24)


def step(args):
    """One GPU process: --step this | natural | parent.  Appends one JSON line of raw samples to the work file."""
    if args.step == "natural":
        os.environ["RVB_RELISTEN_ORDER"] = "0"          # read once per process, at the first relisten
    benchsteps.load_library()
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    s = Samples()

    def timed(ctx, name, call):
        s.timed(name, call, ctx.synchronize, ctx.last_timings)

    off = capi.Context(0)
    off.set_scene(scene)
    off.set_directions(dirs)
    if args.step == "parent":
        for rep in s.repetitions(args.warmup, args.repeats):
            timed(off, "a", lambda: off.trace(mic, src, args.reflections, air))
            timed(off, "a2", lambda: off.trace(OTHER_MIC, src, args.reflections, air))
    else:
        materials, listener = capi.Context(0), capi.Context(0)
        for c in (materials, listener):
            c.share_scene(off)
            c.set_directions(dirs)
        materials.keep_paths(True)
        listener.keep_paths(True, listener=True)
        for rep in s.repetitions(args.warmup, args.repeats):
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
    s.dump(args.work, step=args.step, lib=capi.LIB_PATH)


def report(args):
    # the natural-order process counts as this library's, with its relisten samples alone
    t = Table.load(args.work, key=lambda rec, k: (rec["step"], k) if rec["step"] != "natural" else ("this", k) if k.startswith("n") else None)
    nrecords = args.rays * args.reflections
    t.line("relisten bench: %d rays x %d reflections = %d records (%.0f MB of records, %.0f MB kept for re-shading, %.0f MB more for listeners), "
           "cathedral %d triangles, one context" % (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, nrecords * 16 / 1e6, nrecords * 8 / 1e6, args.triangles))
    t.line("median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings")
    t.row("(a) rvb_trace, keeping off, this library", ("this", "a"))
    t.row("(a) rvb_trace, keeping off, parent library", ("parent", "a"))
    t.row("(a) the same with the other microphone, this library", ("this", "a2"))
    t.row("(a) the same with the other microphone, parent library", ("parent", "a2"))
    for k in t.kernels("this", "a"):
        t.row("      " + k + " (this)", ("this", "a:" + k))
        t.row("      " + k + " (parent)", ("parent", "a:" + k))
    for name, label in (("b", "(b) rvb_trace, RVB_KEEP_MATERIALS"), ("c", "(c) rvb_trace, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER"), ("d", "(d) rvb_relisten"),
                        ("n", "(n) rvb_relisten, natural order (RVB_RELISTEN_ORDER=0)")):
        t.row(label, ("this", name))
        t.kernel_rows("this", name)
    t.line("bars:")
    a, ap, b, c, d, n = (t.med(k) for k in (("this", "a"), ("parent", "a"), ("this", "b"), ("this", "c"), ("this", "d"), ("this", "n")))
    if a is not None and ap is not None:
        spread = t.spread(("parent", "a"))
        t.line("  keeping off against the parent: %.3f ms against %.3f ms, difference %+.3f ms; spread of the parent's repetitions %.3f ms (max - min)" %
               (a, ap, a - ap, spread))
        if d is not None:
            ref = statistics.median(t.samples[("parent", "a")] + t.samples.get(("parent", "a2"), []))
            t.line("  a new microphone: rvb_relisten %.3f ms against the parent's rvb_trace %.3f ms (both microphones): %.3f ms less, %s the spread; ratio %.2f" %
                   (d, ref, ref - d, "more than" if ref - d > spread else "NOT more than", ref / d))
    if b is not None and c is not None:
        kb, kc = t.med(("this", "b:path_keep_kernel")), t.med(("this", "c:path_keep_kernel"))
        t.line("  cost of keeping for listeners: (c) - (b) = %+.3f ms; path_keep_kernel %.3f -> %.3f ms" % (c - b, kb, kc))
    rk = t.med(("this", "d:relisten_records_kernel"))
    if rk is not None:
        t.line("  relisten_records_kernel moves 104 B per record (16 + 8 + 16 read, 64 written): %.2f TB/s" % (nrecords * 104 / (rk * 1e-3) / 1e12))
    if d is not None and n is not None:
        t.line("  kept grouping order against natural order: %.3f ms against %.3f ms per relisten: the kept order is %s" %
               (d, n, "faster" if d < n else "NOT faster"))
    t.emit(args.out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    benchsteps.add_common_arguments(p, repeats=12, warmup=3, step_timeout=240, parent_lib=True, rounds=2,
                                    help=dict(benchsteps.HELP, repeats="per round and library (>= 20 in all with the default two rounds)"))
    args = p.parse_args()
    # this, natural, parent, this, ...: the natural-order process sets RVB_RELISTEN_ORDER=0 for itself
    a_round = [("this", [], None), ("natural", [], None)] + ([("parent", [], args.parent_lib)] if args.parent_lib else [])
    return benchsteps.run(args, dict.fromkeys(("this", "natural", "parent"), step), report, lambda args: (
        benchsteps.shape(args, "rays", "reflections", "triangles", "repeats", "warmup"), a_round * args.rounds))


if __name__ == "__main__":
    sys.exit(main())
