#!/usr/bin/env python3
"""Developer tool: what rvb_decay_params and rvb_decay_params_loss (csrc/decay_params_kernels.hip) take on nrows rows of nbins floats — by
default at workload C2's stereo histogram, 16 x 846 741, and at 512 x 846 741 (64 channels) — against what a user has without them.  In
ONE process per shape, repetition by repetition in turn, as medians with their spread:

  rvb_decay_params                      (its kernels broken out, each against its byte floor)
  three rvb_decay_times calls           EDT, T20, T30 one after the other
  pinned download of the curve          what a host-side C80 / D50 / Ts needs on top of the three calls
  rvb_decay_params_loss with weights    (its kernels broken out, each against its byte floor)
  rvb_decay_params_loss, loss only
  rvb_decay_loss with weights / loss only       the loss against a full target curve, for scale
  rvb_decay_curve, rvb_decay_times (T30), rvb_decay_loss     with --parent ROOT: these three alone, from this build and from a build of
                                        another commit (a directory with rvb_import.py and the built package), in processes that take
                                        turns and run the same loop: their device code is meant to be the same, so the difference must
                                        lie inside the spread of the repetitions

Call times are host clocks around work that ends in a synchronisation; kernel times are the HIP events of rvb_last_timings.  Byte floors
at 6.6 TB/s: params, E read twice (find, sums); adjoint, E read twice (sums, scan), H read and w written once (scan).  The inputs are a
seeded decaying histogram and its curve; the targets are the curve's own parameters x 1.25, the weights 1 / target^2.  Every GPU step is a
child process under its own `timeout -k 10`; the table is written (--out) only when all of them ended well.

    python tools/decay_params_bench.py [--rows 16,512] [--bins N] [--repeats R] [--parent ROOT] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import benchsteps
from benchsteps import Samples, Table

HBM_TBS = 6.6
LEVELS = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))


def step(args):
    """The GPU process of one shape and one build: appends one JSON line of raw samples to the work file."""
    sys.path.insert(0, args.root)          # the build under test: this checkout's, or the one of --parent
    benchsteps.load_library()
    import numpy as np
    import torch
    from parallel_reverb_raytracer_amd import capi
    nrows, nbins, sr = args.nrows, args.bins, 44100.0
    new = args.step == "new"                                 # "new": the new calls (and rvb_decay_loss for scale); "this" / "parent": the three old calls
    ctx = capi.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    envelope = torch.exp(torch.arange(nbins, device="cuda", dtype=torch.float32) * (-6.9 / nbins))

    def histogram():
        h = torch.randn((nrows, nbins), dtype=torch.float32, device="cuda", generator=gen) * envelope
        h[torch.rand((nrows, nbins), device="cuda", generator=gen) < 0.35] = 0.0
        return h

    hist = histogram()
    curve, weights = torch.empty_like(hist), torch.empty_like(hist)
    target = ctx.decay_curve_tensor(histogram())
    ctx.synchronize()
    level = 10.0 * torch.log10(target.double() / target[:, :1].double())
    mask = ((level <= -5.0) & (level >= -35.0)).float().contiguous()
    del level
    pinned = torch.empty((nrows, nbins), dtype=torch.float32).pin_memory()
    torch.cuda.synchronize()
    s = Samples()

    def timed(name, call, kernels=True, wait=ctx.synchronize):
        s.timed(name, call, wait, ctx.last_timings if kernels else None)

    h, e, t, m, w = (x.data_ptr() for x in (hist, curve, target, mask, weights))
    ctx.decay_curve(h, nrows, nbins, e)
    ctx.synchronize()
    checks = {}
    if new:
        params = ctx.decay_params(e, nrows, nbins, sr)
        has = np.isfinite(params) & (params != 0)
        safe = np.where(has, params, 1.0).astype(np.float64)
        targets, pweights = (safe * 1.25).astype(np.float32), np.where(has, 1.0 / (safe * safe), 0.0).astype(np.float32)
    for rep in s.repetitions(args.warmup, args.repeats):
        if not new:
            timed("curve", lambda: ctx.decay_curve(h, nrows, nbins, e))
            timed("times", lambda: ctx.decay_times(e, nrows, nbins, sr, -5.0, -35.0))
        timed("loss", lambda: checks.__setitem__("loss", ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, w)))
        if not new:
            continue
        timed("loss_only", lambda: ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, None))
        timed("params", lambda: checks.__setitem__("params", ctx.decay_params(e, nrows, nbins, sr)))
        timed("three_times", lambda: checks.__setitem__("three", [ctx.decay_times(e, nrows, nbins, sr, a, b) for a, b in LEVELS]), kernels=False)
        timed("download", lambda: pinned.copy_(curve, non_blocking=True), kernels=False, wait=torch.cuda.synchronize)
        timed("params_loss", lambda: checks.__setitem__("ploss", ctx.decay_params_loss(h, e, nrows, nbins, sr, targets, pweights, w)[0]))
        timed("params_loss_only", lambda: checks.__setitem__("ploss_only", ctx.decay_params_loss(h, e, nrows, nbins, sr, targets, pweights, None)[0]))
    rec = {"side": args.step, "nrows": nrows, "nbins": nbins, "loss": float(checks["loss"].sum())}
    if new:
        assert all(checks["params"][:, p].tobytes() == checks["three"][p].tobytes() for p in range(3)), "the times differ from rvb_decay_times"
        assert checks["ploss"].tobytes() == checks["ploss_only"].tobytes()
        rec.update(params0=[float(x) for x in checks["params"][0]], params_loss=float(checks["ploss"].sum()))
    ctx.close()
    s.dump(args.work, **rec)


def report(args):
    t = Table()
    t.line("decay params bench: rows x %d bins of float32, one context, one MI355X; median ms [min .. max] (n)" % args.bins)
    t.line("calls: host clock to the synchronisation; kernels: HIP events of rvb_last_timings; floors at %.1f TB/s" % HBM_TBS)
    records = benchsteps.records(args.work)
    for nrows in sorted({r["nrows"] for r in records}):
        mine = [r for r in records if r["nrows"] == nrows]
        t.samples = benchsteps.merge(mine, key=lambda rec, k: (rec["side"], k))
        first = next(r for r in mine if r["side"] == "new")
        array = nrows * args.bins * 4
        floor = array / (HBM_TBS * 1e12) * 1e3
        med = lambda key, side="new": t.med((side, key))
        t.line("%d x %d (%.1f MB per array); EDT T20 T30 C50 C80 D50 Ts of row 0: %s; params loss %.6g, decay loss %.6g" %
               (nrows, args.bins, array / 1e6, " ".join("%.4g" % x for x in first["params0"]), first["params_loss"], first["loss"]))
        floors = {"decay_params_find_kernel": floor, "decay_params_sums_kernel": floor, "decay_params_adjoint_sums_kernel": floor,
                  "decay_params_adjoint_scan_kernel": 3 * floor}
        for name, label in (("params", "rvb_decay_params"), ("params_loss", "rvb_decay_params_loss with weights"),
                            ("params_loss_only", "rvb_decay_params_loss, loss only")):
            t.row(label, ("new", name))
            for k in t.kernels("new", name):
                t.row("      " + k, ("new", name + ":" + k), tail="   floor %.3f ms: %.2f x" % (floors[k], med(name + ":" + k) / floors[k]) if k in floors else "")
        t.row("three rvb_decay_times calls (EDT, T20, T30)", ("new", "three_times"))
        t.row("pinned download of the curve", ("new", "download"))
        t.row("rvb_decay_loss with weights", ("new", "loss"))
        t.row("rvb_decay_loss, loss only", ("new", "loss_only"))
        kernels = lambda name, start="": sum(med(name + ":" + k) for k in t.kernels("new", name) if k.startswith(start))
        t.line("  params: %.3f ms against %.3f ms for the three calls and the download (%.1f x); kernels %.3f ms against a floor of %.3f ms "
               "(E twice)" % (med("params"), med("three_times") + med("download"), (med("three_times") + med("download")) / med("params"),
                              kernels("params"), 2 * floor))
        t.line("  params loss with weights: %.3f ms against rvb_decay_loss' %.3f ms; loss only %.3f ms against %.3f ms; adjoint kernels %.3f ms "
               "against a floor of %.3f ms (E twice, H once, w once)" %
               (med("params_loss"), med("loss"), med("params_loss_only"), med("loss_only"), kernels("params_loss", "decay_params_adjoint"), 4 * floor))
        if any(r["side"] == "parent" for r in mine):
            t.line("  this build against the parent build, the same three calls in alternating processes:")
            for name, label in (("curve", "rvb_decay_curve"), ("times", "rvb_decay_times, -5 .. -35 dB"), ("loss", "rvb_decay_loss with weights")):
                t.row("    %s, this build" % label, ("this", name))
                t.row("    %s, parent" % label, ("parent", name))
                runs = [statistics.median(r["samples"][name]) for r in mine if r["side"] == "parent"]
                t.line("      difference of the medians %+.4f ms; the parent's own processes: medians %s, samples %.3f .. %.3f" %
                       (med(name, "this") - med(name, "parent"), " / ".join("%.4f" % x for x in runs), min(t.samples[("parent", name)]), max(t.samples[("parent", name)])))
    t.emit(args.out)


def build_steps(args):
    sides = [("new", benchsteps.ROOT)] + ([("this", benchsteps.ROOT), ("parent", os.path.abspath(args.parent))] * 2 if args.parent else [])
    return (benchsteps.shape(args, "bins", "repeats", "warmup"),
            [(side, ["--root", root, "--nrows", str(int(n))], None) for n in args.rows.split(",") for side, root in sides])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="16,512")
    p.add_argument("--bins", type=int, default=846741)
    benchsteps.add_common_arguments(p, repeats=21, warmup=3, step_timeout=240)
    p.add_argument("--parent", default=None, help="root of a built checkout of the commit to compare the unchanged calls with")
    p.add_argument("--root", default=benchsteps.ROOT, help=argparse.SUPPRESS)
    p.add_argument("--nrows", type=int, default=0, help=argparse.SUPPRESS)
    args = p.parse_args()
    return benchsteps.run(args, dict.fromkeys(("new", "this", "parent"), step), report, build_steps)


if __name__ == "__main__":
    sys.exit(main())
