#!/usr/bin/env python3
"""Developer tool: what the sensitivity map (rvb_reshade_grad_map, csrc/reshade_grad_map_kernels.hip) takes against the only other way
to the same numbers, rvb_reshade_grad on the scene relabelled with one surface per triangle (a sweep of the kept trace per 64
triangles).  At 100 000 rays x 128 reflections, two cardioid speakers, 44.1 kHz, the workload's own predelay and bin count, in the
cathedral at every size of --triangles (75 000 and 3 000 by default), one process per size and library, it records as medians with
their spread

  rvb_trace, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER     this library and, with --parent-lib, the library of the commit before
  rvb_reshade_grad (the scene's own surfaces)           both libraries alike
  rvb_reshade_grad_map                                  its kernels broken out, against their byte floors
  rvb_reshade_grad, one surface per triangle            --relabelled-repeats calls in full (ntriangles / 64 sweeps each)

--rounds processes per size and library, the two libraries in turn and the parent's first in every other round.

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  Every GPU
step is a child process under its own `timeout -k 10`, chained with &&; the table is written (--out) only when all of them ended well.
In an --out file that exists it replaces what stands above the line "---- notes" and keeps the rest.

    python tools/reshade_grad_map_bench.py [--rays N] [--reflections K] [--triangles T ...] [--parent-lib SO] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

import benchsteps
from benchsteps import Samples, Table

SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])
NOTES_MARK = "---- notes"          # in the --out file: what follows is kept when the table above it is written again
PEAK_TBS = 6.6          # a streaming pass on this device (profiles/reshade_grad_n1.txt)


def step(args):
    """The GPU process of one (library, size): appends one JSON line of raw samples to the work file."""
    benchsteps.load_library()
    has_map = args.step != "parent"
    if not has_map:
        benchsteps.tolerate_an_older_library()          # (the parent commit's library lacks rvb_reshade_grad_map)
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    triangles = args.triangles[0]
    scene, info = scenes.cathedral(triangles)
    mic, src = info["mic"], info["source"]
    table = benchsteps.other_surfaces(scene[2])
    s = Samples()

    def timed(ctx, name, call):
        s.timed(name, call, ctx.synchronize, ctx.last_timings)

    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
    ctx.keep_paths(True, listener=True)
    ctx.trace(mic, src, args.reflections, air)
    ctx.reshade(table, air)
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, args.sample_rate)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out = torch.empty((scene[0].shape[0], 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for rep in s.repetitions(args.warmup, args.repeats):
        timed(ctx, "trace", lambda: ctx.trace(mic, src, args.reflections, air))
        ctx.reshade(table, air)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        ctx.synchronize()
        timed(ctx, "grad", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()))
        if has_map:
            timed(ctx, "map", lambda: ctx.reshade_grad_map(predelay, args.sample_rate, nbins, weights.data_ptr(), out=out))
    live = None
    if has_map:
        live = int((out != 0).any(dim=1).sum().item())
    ctx.close()
    if has_map and args.relabelled_repeats:
        # the same numbers through rvb_reshade_grad: every triangle a surface of its own with its surface's coefficients
        relabelled = scene[0].copy()
        relabelled["surface"] = np.arange(relabelled.shape[0])
        own = np.ascontiguousarray(table[scene[0]["surface"].astype(np.int64)])
        ctx = capi.Context(0)
        ctx.set_scene((relabelled, scene[1], np.ascontiguousarray(scene[2][scene[0]["surface"].astype(np.int64)])))
        ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
        ctx.keep_paths(True)
        ctx.trace(mic, src, args.reflections, air)
        ctx.reshade(own, air)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        for rep in range(args.relabelled_repeats):
            timed(ctx, "relabelled", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()))
        ctx.close()
    s.dump(args.work, step=args.step, triangles=int(scene[0].shape[0]), asked=triangles, nbins=nbins, live=live)


def report(args):
    recs = benchsteps.records(args.work)
    nrecords = args.rays * args.reflections
    t = Table(label=66, value=9)
    t.line("reshade_grad_map bench: %d rays x %d reflections = %d records, 2 speakers, %.0f Hz, one context" %
           (args.rays, args.reflections, nrecords, args.sample_rate))
    t.line("median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings")
    for asked in args.triangles:
        mine = [r for r in recs if r["asked"] == asked]
        if not mine:
            continue
        ntri = mine[0]["triangles"]
        t.samples = benchsteps.merge(mine)
        t.line("")
        t.line("cathedral, %d triangles, %d bins; triangles with a non-zero row: %s" % (ntri, mine[0]["nbins"], next((r["live"] for r in mine if r["live"] is not None), "?")))
        for name, label in (("trace", "rvb_trace, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER"), ("grad", "rvb_reshade_grad, the scene's own surfaces")):
            a, b = t.row(label + ", this library", ("this", name)), t.row(label + ", parent library", ("parent", name))
            if a is not None and b is not None:
                spread = t.spread(("parent", name))
                t.line("      difference of the medians %+.3f ms; spread of the parent's repetitions %.3f ms (max - min): %s" %
                       (a - b, spread, "inside" if abs(a - b) <= spread else "OUTSIDE"))
        m = t.row("rvb_reshade_grad_map", ("this", "map"))
        t.kernel_rows("this", "map")
        rel = t.row("rvb_reshade_grad, one surface per triangle (%d sweeps)" % ((ntri + 63) // 64), ("this", "relabelled"))
        if m is not None and rel is not None:
            t.line("  the map against the relabelled path: %.3f ms against %.3f ms, %.0f times %s" % (m, rel, rel / m, "faster" if m < rel else "SLOWER"))
        floors = (("reshade_grad_map_terms_kernel", 48 + 8 + 64 + 8, "48 B of records, 8 B listener record read; 64 B row, 8 B sort entry written"),
                  ("reshade_grad_map_sort", 0, None),
                  ("reshade_grad_map_fold_kernel", 8 + 64, "8 B sort entry, 64 B row gathered"))
        parts = {kernel: t.med(("this", "map:" + kernel)) for kernel, _, _ in floors}
        for kernel, per_record, what in floors:
            if parts[kernel] is None:
                continue
            if per_record:
                tbs = nrecords * per_record / (parts[kernel] * 1e-3) / 1e12
                t.line("  %s: %d B per record (%s): %.2f TB/s, floor %.3f ms at %.1f TB/s" %
                       (kernel, per_record, what, tbs, nrecords * per_record / (PEAK_TBS * 1e12) * 1e3, PEAK_TBS))
            else:
                bits = max(1, int(ntri).bit_length())
                passes = (bits + 7) // 8
                t.line("  %s: %d key bits, at least %d passes of 16 B per entry (8 read, 8 written): floor %.3f ms at %.1f TB/s" %
                       (kernel, bits, passes, passes * nrecords * 16 / (PEAK_TBS * 1e12) * 1e3, PEAK_TBS))
        if all(v is not None for v in parts.values()):
            t.line("  the largest of the three: %s" % max(parts, key=parts.get))
    # the table replaces what stands above the line that starts with NOTES_MARK; the notes from there on are kept
    notes = ""
    if args.out and os.path.exists(args.out):
        old = open(args.out).read()
        at = old.find("\n" + NOTES_MARK)
        notes = old[at:] if at >= 0 else ""
    t.emit(args.out, notes)


def build_steps(args):
    steps = []
    for triangles in args.triangles:
        for r in range(args.rounds):
            # the libraries in turn, the parent's first in every other round: two processes differ by more than two repetitions of one,
            # so either library gets both places.  The relabelled path once, in this library's first process.
            for name, _, lib in benchsteps.in_turn(1, args.parent_lib)[::-1 if r % 2 else 1]:
                relabelled = args.relabelled_repeats if name == "this" and r == 0 else 0
                steps.append((name, ["--relabelled-repeats", str(relabelled), "--triangles", str(triangles)], lib))
    return (benchsteps.shape(args, "rays", "reflections", "sample_rate", "repeats", "warmup", "relabelled_repeats")
            + ["--triangles"] + [str(t) for t in args.triangles], steps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, nargs="+", default=[75000, 3000])
    p.add_argument("--sample-rate", type=float, default=44100.0)
    p.add_argument("--relabelled-repeats", type=int, default=1, help="full calls of the relabelled path per size (0: skip it)")
    benchsteps.add_common_arguments(p, repeats=11, warmup=2, step_timeout=400, parent_lib=True, rounds=2,
                                    help=dict(benchsteps.HELP, rounds="processes per size and library"))
    args = p.parse_args()
    return benchsteps.run(args, dict.fromkeys(("this", "parent"), step), report, build_steps)


if __name__ == "__main__":
    sys.exit(main())
