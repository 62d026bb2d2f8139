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
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.6


def step(args):
    """The GPU process of one shape: writes one JSON line of raw samples to the work file."""
    import rvb_import
    rvb_import.load()
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
    samples = {}

    def note(name, value):
        samples.setdefault(name, []).append(float(value))

    def timed(name, call, kernels=True, wait=ctx.synchronize):
        t0 = time.perf_counter()
        call()
        wait()
        note(name, (time.perf_counter() - t0) * 1e3)
        if kernels:
            for k, v in ctx.last_timings():
                note(name + ":" + k, v)

    h, e, t, m, w = (x.data_ptr() for x in (hist, curve, target, mask, weights))
    checks = {}
    for rep in range(args.warmup + args.repeats):
        if rep == args.warmup:
            samples.clear()
        timed("curve", lambda: ctx.decay_curve(h, nrows, nbins, e))
        timed("times", lambda: checks.__setitem__("seconds", ctx.decay_times(e, nrows, nbins, 44100.0, -5.0, -35.0)))
        timed("loss", lambda: checks.__setitem__("loss", ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, w)))
        timed("loss_only", lambda: ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, None))
        timed("torch", lambda: checks.__setitem__("torch", torch.flip(torch.cumsum(torch.flip(hist.double() ** 2, (1,)), 1), (1,)).float()),
              kernels=False, wait=torch.cuda.synchronize)
        timed("download", lambda: pinned.copy_(hist, non_blocking=True), kernels=False, wait=torch.cuda.synchronize)
    agree = float(((checks["torch"] - curve).abs() / curve.abs().clamp_min(1e-30)).max())
    ctx.close()
    with open(args.work, "a") as f:
        f.write(json.dumps({"nrows": nrows, "nbins": nbins, "samples": samples, "agree": agree,
                            "seconds0": float(checks["seconds"][0]), "loss": float(checks["loss"].sum())}) + "\n")


def report(args):
    lines = ["decay bench: rows x %d bins of float32, one context, one MI355X; median ms [min .. max] (n)" % args.bins,
             "calls: host clock to the synchronisation; kernels: HIP events of rvb_last_timings; floors at %.1f TB/s" % HBM_TBS]
    for raw in open(args.work).read().splitlines():
        rec = json.loads(raw)
        s, nrows, nbins = rec["samples"], rec["nrows"], rec["nbins"]
        array = nrows * nbins * 4
        lines.append("%d x %d (%.1f MB per array); T30 of row 0 %.4f s, loss %.6g, max |torch - curve| / curve %.2g" %
                     (nrows, nbins, array / 1e6, rec["seconds0"], rec["loss"], rec["agree"]))

        def row(label, key):
            v = s[key]
            lines.append("  %-58s %8.3f [%.3f .. %.3f] (%d)" % (label, statistics.median(v), min(v), max(v), len(v)))

        for name, label in (("curve", "rvb_decay_curve"), ("times", "rvb_decay_times, -5 .. -35 dB"), ("loss", "rvb_decay_loss with weights"),
                            ("loss_only", "rvb_decay_loss, loss only")):
            row(label, name)
            for k in sorted(k for k in s if k.startswith(name + ":")):
                row("      " + k.split(":", 1)[1], k)
        row("torch float64 flip-cumsum-flip of the squares", "torch")
        row("pinned download of the histogram", "download")
        kernels = lambda name: sum(statistics.median(s[k]) for k in s if k.startswith(name + ":"))
        curve_floor, loss_floor = 3 * array / (HBM_TBS * 1e12) * 1e3, (3 + 4 + 1) * array / (HBM_TBS * 1e12) * 1e3
        lines.append("  curve: kernels %.3f ms against a floor of %.3f ms (H twice, E once); the torch expression takes %.2f x the call" %
                     (kernels("curve"), curve_floor, statistics.median(s["torch"]) / statistics.median(s["curve"])))
        lines.append("  loss with weights: kernels %.3f ms against a floor of %.3f ms (E, T, m twice, H once, w once)" % (kernels("loss"), loss_floor))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="16,512")
    p.add_argument("--bins", type=int, default=846741)
    p.add_argument("--repeats", type=int, default=21)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--step-timeout", type=int, default=240)
    p.add_argument("--out", default=None)
    p.add_argument("--step", default=None, help=argparse.SUPPRESS)
    p.add_argument("--nrows", type=int, default=0, help=argparse.SUPPRESS)
    p.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.step == "report":
        return report(args)
    if args.step:
        return step(args)
    work = os.path.join(tempfile.mkdtemp(prefix="decay_bench_"), "samples.json")
    shape = ["--bins", str(args.bins), "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    parts = ["timeout -k 10 %d %s" % (args.step_timeout, " ".join(shlex.quote(x) for x in me + shape + ["--step", "gpu", "--nrows", str(int(n))]))
             for n in args.rows.split(",")]
    parts.append(" ".join(shlex.quote(x) for x in me + shape + ["--step", "report"] + (["--out", args.out] if args.out else [])))
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
