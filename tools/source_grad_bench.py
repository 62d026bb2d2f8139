#!/usr/bin/env python3
"""Developer tool: what the source-end gradients cost (include/rvb_capi_source_grad.h).  100 000 rays x 128 reflections in the
75 000-triangle cathedral, one context, two cardioid speakers, 44.1 kHz, a polar pattern on the source, the workload's own predelay and
bin count.  In ONE process, repetition by repetition in turn, as medians with their spread,

  (a) rvb_source_grad (per-ray gradient and pattern gradient) and its kernels, beside rvb_reshade_grad in the same run — the new sweep
      does strictly less work — and the floor: the kept side records, the records' two chunks and the weights read once at 6.6 TB/s;
      rvb_source_grad_images under the merged RVB_IR_ALL configuration;
  (b) one aim-gradient evaluation of the STI loss (fitting.aim_loss_and_grad) against what it replaces: two loss evaluations
      (set_source_pattern + rvb_reshade + rvb_ir_accumulate + analysis: fitting.aim_loss) per free parameter of a central difference;

and with --parent-lib, a build of the parent commit (the same ABI, loaded through RVB_LIB),

  (c) rvb_trace with keeping on, rvb_reshade and rvb_reshade_grad with this build and with the parent's in child processes that take
      turns (--turns each): their device code is unchanged, so the differences must lie inside the parent's own spread.

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  Every GPU
step is a child process under its own `timeout -k 10`; the table is written (--out) only when all ended well.  No counter run is made.

    python tools/source_grad_bench.py [--rays N] [--repeats R] [--parent-lib FILE] [--out FILE]
"""
import argparse
import sys

import benchsteps
from benchsteps import Samples, Table

SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])
REFLECTIONS = 128
FACING, SHAPE = (0.8, 0.35, -0.5), 0.5
HBM_TBS = 6.6                       # the streaming rate the project measured on one MI355X (tools/copy_probe.hip)


def context(args, capi, scenes, dtypes, listener):
    scene, info = scenes.cathedral(args.triangles)
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
    ctx.keep_paths(True, listener=listener)
    return ctx, scene, info["mic"], info["source"]


def step_grads(args):
    """(a) and (b): writes one JSON line of raw samples to the work file."""
    benchsteps.load_library()
    import numpy as np
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, fitting, scenes
    air, sr = dtypes.AIR_COEFFICIENTS, args.sample_rate
    ctx, scene, mic, src = context(args, capi, scenes, dtypes, True)
    table = benchsteps.other_surfaces(scene[2])
    ctx.set_source_pattern(FACING, SHAPE)
    ctx.trace(mic, src, REFLECTIONS, air)
    ctx.reshade(table, air)
    nimages = ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, sr)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    torch.cuda.synchronize()
    s = Samples()

    def timed(name, call, kernels=True):
        s.timed(name, call, ctx.synchronize, ctx.last_timings if kernels else None)

    target = (np.array([0.9, 0.9]), np.ones(2), None)
    aim_args = (table, air, mic, SPEAKERS, target, sr, predelay, nbins)
    for rep in s.repetitions(args.warmup, args.repeats):
        ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        timed("source_grad_images", lambda: ctx.source_grad_images(predelay, sr, nbins, weights.data_ptr(), want_depart=True, want_pattern=True))
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        timed("source_grad", lambda: ctx.source_grad(predelay, sr, nbins, weights.data_ptr(), want_pattern=True))
        timed("source_grad_rays_only", lambda: ctx.source_grad(predelay, sr, nbins, weights.data_ptr()))
        timed("reshade_grad", lambda: ctx.reshade_grad(predelay, sr, nbins, weights.data_ptr()))
        timed("aim_gradient", lambda: fitting.aim_loss_and_grad(ctx, "sti", FACING, SHAPE, *aim_args), kernels=False)
        timed("aim_loss", lambda: fitting.aim_loss(ctx, "sti", FACING, SHAPE, *aim_args), kernels=False)
    ctx.close()
    s.dump(args.work + ".grads", nbins=nbins, nimages=int(nimages), triangles=int(scene[0].shape[0]))


def step_turn(args):
    """(c), one turn of one library (RVB_LIB decides which): appends one JSON line of raw samples to the work file of the turns."""
    benchsteps.load_library()
    if args.label == "parent":
        benchsteps.tolerate_an_older_library()          # the parent's library has no entry point of rvb_capi_source_grad.h
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    ctx, scene, mic, src = context(args, capi, scenes, dtypes, False)
    table = benchsteps.other_surfaces(scene[2])
    ctx.trace(mic, src, REFLECTIONS, air)
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, args.sample_rate)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    torch.cuda.synchronize()
    s = Samples()
    for rep in s.repetitions(args.warmup, args.repeats):
        s.timed("trace", lambda: ctx.trace(mic, src, REFLECTIONS, air), ctx.synchronize)
        s.timed("reshade", lambda: ctx.reshade(table, air), ctx.synchronize)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        s.timed("grad", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()), ctx.synchronize)
    ctx.close()
    s.dump(args.work + ".turns", lib=args.label)


def report(args):
    t = Table()
    rec, = benchsteps.records(args.work + ".grads")
    t.samples = rec["samples"]
    t.line("source grad bench: cathedral, %d triangles, %d rays x %d reflections, 2 speakers, %.0f Hz, %d bins, %d images, one context; median ms "
           "[min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings"
           % (rec["triangles"], args.rays, REFLECTIONS, args.sample_rate, rec["nbins"], rec["nimages"]))
    t.line("(a) the gradients")
    for key, label in (("source_grad", "rvb_source_grad, d_ray_grad and pattern_grad"), ("source_grad_rays_only", "rvb_source_grad, d_ray_grad alone"),
                       ("reshade_grad", "rvb_reshade_grad, the same run"), ("source_grad_images", "rvb_source_grad_images, everything asked for")):
        t.row(label, key)
        t.kernel_rows(None, key)
    records = args.rays * REFLECTIONS
    floor_bytes = records * (16 + 32) + rec["nbins"] * 2 * 8 * 4
    sweep, old = t.med("source_grad:source_grad_rays_kernel"), t.med("reshade_grad:reshade_grad_kernel")
    t.line("  floor of source_grad_rays_kernel: %d records x (16 B side record + 32 B of the record) + %d B of weights = %.1f MB, %.3f ms at %.1f TB/s; "
           "the kernel takes %.2f x that, and %.2f x reshade_grad_kernel (%s)"
           % (records, rec["nbins"] * 64, floor_bytes / 1e6, floor_bytes / (HBM_TBS * 1e9), HBM_TBS, sweep / (floor_bytes / (HBM_TBS * 1e9)), sweep / old,
              "not slower" if sweep <= old else "SLOWER than the sweep it does less than"))
    t.line("(b) aiming: the STI loss and its gradient with respect to direction and shapes")
    grad, loss = t.row("one aim-gradient evaluation (fitting.aim_loss_and_grad)", "aim_gradient"), t.row("one loss evaluation (fitting.aim_loss)", "aim_loss")
    for free, label in ((2, "the direction (two tangent coordinates)"), (10, "direction and eight shapes")):
        t.line("  central differences for %s: %d loss evaluations = %.3f ms, %.1f x the gradient evaluation" % (label, 2 * free, 2 * free * loss, 2 * free * loss / grad))
    if args.parent_lib:
        t.samples = benchsteps.merge(benchsteps.records(args.work + ".turns"), key=lambda rec, k: (rec["lib"], k))
        t.line("(c) this build and the parent commit's in processes that take turns (%d turns each, every sample of a library pooled)" % args.turns)
        for key, label in (("trace", "rvb_trace, keeping on"), ("reshade", "rvb_reshade"), ("grad", "rvb_reshade_grad")):
            parent, this = (t.row("%s, %s" % (label, lib), (lib, key)) for lib in ("parent", "this"))
            diff, spread = this - parent, t.spread(("parent", key))
            t.line("      this - parent = %+.3f ms, the parent's own spread %.3f ms: %s" % (diff, spread, "inside" if abs(diff) <= spread else "OUTSIDE"))
    else:
        t.line("(c) not measured: no --parent-lib")
    t.line("not measured: hardware counters (no counter run was made), more than one GPU, other ray counts")
    t.emit(args.out)


def build_steps(args):
    steps = [("grads", [], None)]
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
    p.add_argument("--label", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    return benchsteps.run(args, {"grads": step_grads, "turn": step_turn}, report, build_steps)


if __name__ == "__main__":
    sys.exit(main())
