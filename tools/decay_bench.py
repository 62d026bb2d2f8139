#!/usr/bin/env python3
"""Developer tool: what the decay calls (rvb_decay_curve, rvb_decay_times, rvb_decay_loss; csrc/decay_kernels.hip) take on nrows rows of
nbins floats — by default at workload C2's stereo histogram, 16 x 846 741, and at 512 x 846 741 (64 channels) — against what a user has
without them.  In ONE process per shape, repetition by repetition in turn, as medians with their spread:

  rvb_decay_curve                       (its kernels broken out)
  rvb_decay_times, -5 .. -35 dB         (its kernels broken out)
  rvb_decay_loss with weights           (its kernels broken out)
  rvb_decay_loss, loss only
  torch float64 flip-cumsum-flip        what a user writes for the curve: flip(cumsum(flip(h.double() ** 2))).float() on the same GPU
  pinned download of the histogram      what a C caller needs before it can compute anything on the host

Call times are host clocks around work that ends in a synchronisation; kernel times are the HIP events of rvb_last_timings.  The inputs
are a seeded decaying histogram, the curve of another as the target, and the mask of the target's -5 .. -35 dB range.  Every GPU step
is a child process under its own `timeout -k 10`; the table is written (--out) only when all of them ended well.

    python tools/decay_bench.py [--rows 16,512] [--bins N] [--repeats R] [--out FILE]
"""
import argparse
import sys

import benchsteps
from benchsteps import Samples, Table

HBM_TBS = 6.6


def step(args):
    """The GPU process of one shape: writes one JSON line of raw samples to the work file."""
    benchsteps.load_library()
    import torch
    from parallel_reverb_raytracer_amd import capi
    nrows, nbins = args.nrows, args.bins
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

    def timed(name, call):
        s.timed(name, call, ctx.synchronize, ctx.last_timings)

    h, e, t, m, w = (x.data_ptr() for x in (hist, curve, target, mask, weights))
    checks = {}
    for rep in s.repetitions(args.warmup, args.repeats):
        timed("curve", lambda: ctx.decay_curve(h, nrows, nbins, e))
        timed("times", lambda: checks.__setitem__("seconds", ctx.decay_times(e, nrows, nbins, 44100.0, -5.0, -35.0)))
        timed("loss", lambda: checks.__setitem__("loss", ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, w)))
        timed("loss_only", lambda: ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, None))
        s.timed("torch", lambda: checks.__setitem__("torch", torch.flip(torch.cumsum(torch.flip(hist.double() ** 2, (1,)), 1), (1,)).float()),
                torch.cuda.synchronize)
        s.timed("download", lambda: pinned.copy_(hist, non_blocking=True), torch.cuda.synchronize)
    agree = float(((checks["torch"] - curve).abs() / curve.abs().clamp_min(1e-30)).max())
    ctx.close()
    s.dump(args.work, nrows=nrows, nbins=nbins, agree=agree, seconds0=float(checks["seconds"][0]), loss=float(checks["loss"].sum()))


def report(args):
    t = Table()
    t.line("decay bench: rows x %d bins of float32, one context, one MI355X; median ms [min .. max] (n)" % args.bins)
    t.line("calls: host clock to the synchronisation; kernels: HIP events of rvb_last_timings; floors at %.1f TB/s" % HBM_TBS)
    for rec in benchsteps.records(args.work):          # a shape per line, each with a section of its own
        t.samples, nrows, nbins = rec["samples"], rec["nrows"], rec["nbins"]
        array = nrows * nbins * 4
        t.line("%d x %d (%.1f MB per array); T30 of row 0 %.4f s, loss %.6g, max |torch - curve| / curve %.2g" %
               (nrows, nbins, array / 1e6, rec["seconds0"], rec["loss"], rec["agree"]))
        for name, label in (("curve", "rvb_decay_curve"), ("times", "rvb_decay_times, -5 .. -35 dB"), ("loss", "rvb_decay_loss with weights"),
                            ("loss_only", "rvb_decay_loss, loss only")):
            t.row(label, name)
            t.kernel_rows(None, name)
        t.row("torch float64 flip-cumsum-flip of the squares", "torch")
        t.row("pinned download of the histogram", "download")
        kernels = lambda name: sum(t.med(name + ":" + k) for k in t.kernels(None, name))
        curve_floor, loss_floor = 3 * array / (HBM_TBS * 1e12) * 1e3, (3 + 4 + 1) * array / (HBM_TBS * 1e12) * 1e3
        t.line("  curve: kernels %.3f ms against a floor of %.3f ms (H twice, E once); the torch expression takes %.2f x the call" %
               (kernels("curve"), curve_floor, t.med("torch") / t.med("curve")))
        t.line("  loss with weights: kernels %.3f ms against a floor of %.3f ms (E, T, m twice, H once, w once)" % (kernels("loss"), loss_floor))
    t.emit(args.out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="16,512")
    p.add_argument("--bins", type=int, default=846741)
    benchsteps.add_common_arguments(p, repeats=21, warmup=3, step_timeout=240)
    p.add_argument("--nrows", type=int, default=0, help=argparse.SUPPRESS)
    args = p.parse_args()
    return benchsteps.run(args, {"gpu": step}, report, lambda args: (
        benchsteps.shape(args, "bins", "repeats", "warmup"), [("gpu", ["--nrows", str(int(n))], None) for n in args.rows.split(",")]))


if __name__ == "__main__":
    sys.exit(main())
