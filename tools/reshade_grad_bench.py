#!/usr/bin/env python3
"""Developer tool: what a material gradient (rvb_reshade_grad, csrc/reshade_grad_kernels.hip) takes against the forward evaluations a
finite-difference gradient is made of.  At workload C2 by default (100 000 rays x 128 reflections in the 75 000-triangle cathedral, one
context, two cardioid speakers, 44.1 kHz, the workload's own predelay and bin count) it records in ONE process, repetition by
repetition in turn, as medians with their spread,

  rvb_reshade                      one forward re-shade (its kernels broken out)
  rvb_ir_accumulate, RVB_IR_FAST   one forward binning (its kernels broken out)
  rvb_reshade_grad                 the gradient (its kernels broken out)

and what 16 x nsurfaces + 8 forward evaluations (a re-shade and a binning each) would cost from those medians.  Call times are host
clocks around work that ends in rvb_synchronize (rvb_reshade_grad is synchronous by itself); kernel times are the HIP events of
rvb_last_timings.  The GPU step is a child process under its own `timeout -k 10`; the table is written (--out) only when it ended well.

    python tools/reshade_grad_bench.py [--rays N] [--reflections K] [--triangles T] [--repeats R] [--out FILE]
"""
import argparse
import sys

import benchsteps
from benchsteps import Samples, Table

SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])


def step(args):
    """The GPU process: writes one JSON line of raw samples to the work file."""
    benchsteps.load_library()
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    table = benchsteps.other_surfaces(scene[2])
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
    ctx.keep_paths(True)
    ctx.trace(mic, src, args.reflections, air)
    ctx.reshade(table, air)
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, args.sample_rate)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = Samples()

    def timed(name, call):
        s.timed(name, call, ctx.synchronize, ctx.last_timings)

    for rep in s.repetitions(args.warmup, args.repeats):
        timed("reshade", lambda: ctx.reshade(table, air))
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        timed("accumulate", lambda: ctx.ir_accumulate(predelay, args.sample_rate, nbins, capi.IR_FAST, hist.data_ptr()))
        timed("grad", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()))
    ctx.close()
    s.dump(args.work, nbins=nbins, nsurfaces=int(scene[2].shape[0]))


def report(args):
    rec, = benchsteps.records(args.work)
    t, nsurfaces, nbins = Table(rec["samples"]), rec["nsurfaces"], rec["nbins"]
    nrecords = args.rays * args.reflections
    t.line("reshade_grad bench: %d rays x %d reflections = %d records, cathedral %d triangles, %d surfaces, 2 speakers, %.0f Hz, %d bins, one context" %
           (args.rays, args.reflections, nrecords, args.triangles, nsurfaces, args.sample_rate, nbins))
    t.line("median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings")
    for name, label in (("reshade", "rvb_reshade"), ("accumulate", "rvb_ir_accumulate, RVB_IR_FAST"), ("grad", "rvb_reshade_grad")):
        t.row(label, name)
        t.kernel_rows(None, name)
    forward = t.med("reshade") + t.med("accumulate")
    grad = t.med("grad")
    evaluations = 16 * nsurfaces + 8
    t.line("a finite-difference gradient: %d forward evaluations x (%.3f + %.3f) ms = %.1f ms; rvb_reshade_grad %.3f ms = %.2f forward evaluations" %
           (evaluations, t.med("reshade"), t.med("accumulate"), evaluations * forward, grad, grad / forward))
    t.line("reshade_grad_kernel reads 48 B per record (16 side + 32 position and time) and gathers 32 B per live record and channel: "
           "%.2f TB/s of record bytes" % (nrecords * 48 / (t.med("grad:reshade_grad_kernel") * 1e-3) / 1e12))
    t.emit(args.out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    p.add_argument("--sample-rate", type=float, default=44100.0)
    benchsteps.add_common_arguments(p, repeats=21, warmup=3, step_timeout=240)
    args = p.parse_args()
    return benchsteps.run(args, {"gpu": step}, report, lambda args: (
        benchsteps.shape(args, "rays", "reflections", "triangles", "sample_rate", "repeats", "warmup"), [("gpu", [], None)]))


if __name__ == "__main__":
    sys.exit(main())
