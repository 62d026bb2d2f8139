#!/usr/bin/env python3
"""Developer tool: what the early reflections cost a material fit (include/rvb_capi_images.h).  Two workloads — 100 000 rays x 128
reflections in the 75 000-triangle cathedral, and the constructed room of tests/image_edges.py at 100 000 x 12 —, one context, two
cardioid speakers, 44.1 kHz, the workload's own predelay and bin count under RVB_IR_ALL.  Per workload it records in ONE process,
repetition by repetition in turn, as medians with their spread,

  (a) one forward evaluation with RVB_IR_ALL: rvb_reshade + configure + rvb_ir_accumulate(RVB_IR_EXACT)
        through the host merge (rvb_get_image_candidates, rvb_get_direct, rvb_merge_images, rvb_ir_configure_speakers): the baseline,
        the path of earlier versions;
        through rvb_ir_configure_speakers_merged, the FIRST call after the list was voided (a relisten to the same microphone, outside
        the clock) and a LATER call (the cached list: the gather alone); the configure step of each on its own;
  (b) rvb_reshade_grad_images and its two kernels beside rvb_reshade_grad;

and with --parent-lib, a build of the parent commit (the same ABI, loaded through RVB_LIB),

  (c) rvb_trace with keeping on, rvb_reshade and rvb_reshade_grad with this build and with the parent's in child processes that take
      turns (--turns each): their device code is unchanged, so the differences must lie inside the parent's own spread.

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  Every GPU
step is a child process under its own `timeout -k 10`; the table is written (--out) only when all ended well.

    python tools/early_fit_bench.py [--rays N] [--repeats R] [--parent-lib FILE] [--out FILE]
"""
import argparse
import os
import sys
import time

import benchsteps
from benchsteps import Samples, Table

SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])
WORKLOADS = {"cathedral": 128, "room": 12}


def workload(args, name):
    """(scene, mic, source, reflections)"""
    from parallel_reverb_raytracer_amd import scenes
    if name == "cathedral":
        scene, info = scenes.cathedral(args.triangles)
        return scene, info["mic"], info["source"], WORKLOADS[name]
    sys.path.insert(0, os.path.join(benchsteps.ROOT, "tests"))
    import image_edges
    return image_edges.room(), image_edges.PAIRS[0][0], image_edges.PAIRS[0][1], WORKLOADS[name]


def step_forward(args):
    """(a) and (b) for one workload: writes one JSON line of raw samples to that workload's work file."""
    benchsteps.load_library()
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    scene, mic, src, nrefl = workload(args, args.workload)
    table = benchsteps.other_surfaces(scene[2])
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
    ctx.keep_paths(True, listener=True)
    ctx.trace(mic, src, nrefl, air)
    ctx.reshade(table, air)
    nimages = ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    ncandidates = int(ctx.get_image_candidates().shape[0])
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, args.sample_rate)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = Samples()
    sr = args.sample_rate

    def timed(name, call, kernels=True):
        s.timed(name, call, ctx.synchronize, ctx.last_timings if kernels else None)

    def configure_host():
        t0 = time.perf_counter()
        images = ctx.get_raw_images(False)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, images)
        return (time.perf_counter() - t0) * 1e3

    def configure_merged():
        t0 = time.perf_counter()
        ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        return (time.perf_counter() - t0) * 1e3

    def forward(name, configure):
        def call():
            ctx.reshade(table, air)
            s.note(name + ":configure (host clock, not synchronised)", configure())
            ctx.ir_accumulate(predelay, sr, nbins, capi.IR_EXACT, hist.data_ptr())
        timed(name, call, kernels=False)

    for rep in s.repetitions(args.warmup, args.repeats):
        forward("host", configure_host)
        ctx.relisten(mic)                                   # the same microphone: the same results, the list void
        ctx.synchronize()
        forward("merged_first", configure_merged)
        forward("merged_later", configure_merged)
        timed("grad_images", lambda: ctx.reshade_grad_images(predelay, sr, nbins, weights.data_ptr()))
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        timed("grad", lambda: ctx.reshade_grad(predelay, sr, nbins, weights.data_ptr()))
    ctx.close()
    s.dump(args.work + "." + args.workload, nbins=nbins, nsurfaces=int(scene[2].shape[0]), nimages=int(nimages), ncandidates=ncandidates,
           reflections=nrefl, triangles=int(scene[0].shape[0]))


def step_turn(args):
    """(c), one turn of one library (RVB_LIB decides which): appends one JSON line of raw samples to the work file of the turns."""
    benchsteps.load_library()
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    if args.label == "parent":
        capi._IMAGE_SIGNATURES.clear()          # the parent's library has no entry point of rvb_capi_images.h: nothing of that table to apply
    scene, mic, src, nrefl = workload(args, "cathedral")
    table = benchsteps.other_surfaces(scene[2])
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
    ctx.keep_paths(True)
    ctx.trace(mic, src, nrefl, air)
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, args.sample_rate)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    torch.cuda.synchronize()
    s = Samples()
    for rep in s.repetitions(args.warmup, args.repeats):
        s.timed("trace", lambda: ctx.trace(mic, src, nrefl, air), ctx.synchronize)
        s.timed("reshade", lambda: ctx.reshade(table, air), ctx.synchronize)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        s.timed("grad", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()), ctx.synchronize)
    ctx.close()
    s.dump(args.work + ".turns", lib=args.label)


def report(args):
    t = Table()          # (rows a level deeper than the other benches': two more spaces in front of every label)
    t.line("early fit bench: %d rays, 2 speakers, %.0f Hz, one context; median ms [min .. max] (n); calls: host clock to rvb_synchronize; "
           "kernels: HIP events of rvb_last_timings" % (args.rays, args.sample_rate))
    for name in WORKLOADS:
        rec, = benchsteps.records(args.work + "." + name)
        t.samples = rec["samples"]
        t.line("%s: %d triangles, %d surfaces, %d rays x %d reflections, %d candidates -> %d images, %d bins" %
               (name, rec["triangles"], rec["nsurfaces"], args.rays, rec["reflections"], rec["ncandidates"], rec["nimages"], rec["nbins"]))
        t.line("  (a) one forward evaluation, RVB_IR_ALL: rvb_reshade + configure + rvb_ir_accumulate(RVB_IR_EXACT)")
        for key, label in (("host", "through the host merge (baseline)"), ("merged_first", "rvb_ir_configure_speakers_merged, first call"),
                           ("merged_later", "rvb_ir_configure_speakers_merged, later calls")):
            t.row("  " + label, key)
            t.row("        its configure step", key + ":configure (host clock, not synchronised)")
        host, later, first = (t.med(k) for k in ("host", "merged_later", "merged_first"))
        spread = t.spread("host")
        t.line("    host / later = %.2f x, host / first = %.2f x; host - later = %.3f ms, the host path's repetitions spread over %.3f ms: %s" %
               (host / later, host / first, host - later, spread,
                "later calls are faster beyond that spread" if host - later > spread else
                "NOT faster beyond that spread (the evaluation is bound by the re-shade and the exact binning of the diffuse records)"))
        t.line("  (b) the gradients")
        for key, label in (("grad_images", "rvb_reshade_grad_images"), ("grad", "rvb_reshade_grad")):
            t.row("  " + label, key)
            t.kernel_rows(None, key, indent="        ")
    if args.parent_lib:
        t.samples = benchsteps.merge(benchsteps.records(args.work + ".turns"), key=lambda rec, k: (rec["lib"], k))
        t.line("(c) cathedral, this build and the parent commit's in processes that take turns (%d turns each, every sample of a library pooled)" % args.turns)
        for key, label in (("trace", "rvb_trace, keeping on"), ("reshade", "rvb_reshade"), ("grad", "rvb_reshade_grad")):
            parent, this = (t.row("  %s, %s" % (label, lib), (lib, key)) for lib in ("parent", "this"))
            diff, spread = this - parent, t.spread(("parent", key))
            t.line("      this - parent = %+.3f ms, the parent's own spread %.3f ms: %s" % (diff, spread, "inside" if abs(diff) <= spread else "OUTSIDE"))
    t.emit(args.out)


def build_steps(args):
    steps = [("forward", ["--workload", name], None) for name in WORKLOADS]
    if args.parent_lib:
        steps += [("turn", ["--label", "parent"], args.parent_lib), ("turn", ["--label", "this"], None)] * args.turns
    return (benchsteps.shape(args, "rays", "triangles", "sample_rate", "repeats", "warmup", "turns") +
            (["--parent-lib", args.parent_lib] if args.parent_lib else []), steps)          # (the report asks whether there were turns)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--triangles", type=int, default=75000)
    p.add_argument("--sample-rate", type=float, default=44100.0)
    p.add_argument("--turns", type=int, default=3)
    benchsteps.add_common_arguments(p, repeats=21, warmup=3, step_timeout=240, parent_lib=True, help={})
    p.add_argument("--workload", default=None, help=argparse.SUPPRESS)
    p.add_argument("--label", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    return benchsteps.run(args, {"forward": step_forward, "turn": step_turn}, report, build_steps)


if __name__ == "__main__":
    sys.exit(main())
