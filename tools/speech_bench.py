#!/usr/bin/env python3
"""Developer tool: what rvb_mtf and rvb_mtf_adjoint (include/rvb_capi_speech.h, csrc/speech_kernels.hip) take on nrows rows of nbins
floats — by default at workload C2's stereo histogram, 16 x 846 741, and at 512 x 846 741 (64 channels) — against what a user has
without them.  In ONE process per shape, as medians with their spread:

  rvb_mtf, 14 frequencies               (its kernels broken out; the streaming floor is H read once)
  rvb_mtf_adjoint                       (its kernels broken out; the floor is H read twice and w written once)
  pinned download of the histogram      what the host needs before it can start
  numpy on the host                     the same transfer values in binary64 from the downloaded histogram: the cos / sin tables of the 14
                                        frequencies (once per shape of histogram) and, per histogram, the squares and one matrix product
                                        per block of 16 rows, on --host-threads BLAS threads; fewer repetitions (--host-repeats)
  rvb_decay_curve, rvb_decay_times (T30), rvb_decay_loss     with --parent-lib: these three alone, from this build and from a library built
                                        from the commit before, in processes that take turns and run the same loop: their device code is
                                        meant to be the same, so the difference must lie inside the spread of the repetitions

Call times are host clocks around work that ends in a synchronisation; kernel times are the HIP events of rvb_last_timings.  Byte floors
at 6.6 TB/s.  The input is a seeded decaying histogram with 35 % zeros, the coefficients dL/dm seeded normal values.  Every GPU step is a
child process under its own `timeout -k 10`; the table is written (--out) only when all of them ended well.

    python tools/speech_bench.py [--rows 16,512] [--bins N] [--repeats R] [--parent-lib LIB] [--out FILE]
"""
import argparse
import os
import sys

import benchsteps
from benchsteps import Samples, Table

HBM_TBS = 6.6
FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
SR = 44100.0


def step(args):
    """The GPU process of one shape and one build: appends one JSON line of raw samples to the work file."""
    os.environ["OMP_NUM_THREADS"] = os.environ["OPENBLAS_NUM_THREADS"] = os.environ["MKL_NUM_THREADS"] = str(args.host_threads)
    if args.step == "parent":
        benchsteps.tolerate_an_older_library()          # (the parent commit's library lacks the speech calls)
    benchsteps.load_library()
    import numpy as np
    import torch
    from parallel_reverb_raytracer_amd import capi
    nrows, nbins = args.nrows, args.bins
    new = args.step == "new"
    ctx = capi.Context(0)
    gen = torch.Generator(device="cuda").manual_seed(5)
    envelope = torch.exp(torch.arange(nbins, device="cuda", dtype=torch.float32) * (-6.9 / nbins))

    def histogram():
        h = torch.randn((nrows, nbins), dtype=torch.float32, device="cuda", generator=gen) * envelope
        h[torch.rand((nrows, nbins), device="cuda", generator=gen) < 0.35] = 0.0
        return h

    hist = histogram()
    weights = torch.empty_like(hist)
    torch.cuda.synchronize()
    s = Samples()
    checks = {}

    def timed(name, call, kernels=True, wait=ctx.synchronize):
        s.timed(name, call, wait, ctx.last_timings if kernels else None)

    h, w = hist.data_ptr(), weights.data_ptr()
    if new:
        coeffs = np.random.default_rng(9).standard_normal((nrows, len(FREQS)))
        pinned = torch.empty((nrows, nbins), dtype=torch.float32).pin_memory()
        for rep in s.repetitions(args.warmup, args.repeats):
            timed("mtf", lambda: checks.__setitem__("m", ctx.mtf(h, nrows, nbins, SR, FREQS)))
            timed("adjoint", lambda: ctx.mtf_adjoint(h, nrows, nbins, SR, FREQS, coeffs, w))
            timed("download", lambda: pinned.copy_(hist, non_blocking=True), kernels=False, wait=torch.cuda.synchronize)
        host = pinned.numpy()
        tables = {}

        def make_tables():
            phase = 2 * np.pi * np.outer(np.arange(nbins, dtype=np.float64), np.asarray(FREQS) / SR)
            tables["cs"] = np.concatenate([np.cos(phase), np.sin(phase)], axis=1)          # [nbins][28]

        def on_host():
            out = np.empty((nrows, len(FREQS)))
            for r in range(0, nrows, 16):
                e = host[r:r + 16].astype(np.float64) ** 2
                ab = e @ tables["cs"]
                out[r:r + 16] = np.hypot(ab[:, :len(FREQS)], ab[:, len(FREQS):]) / e.sum(axis=1)[:, None]
            checks["host"] = out

        for rep in range(args.host_repeats):
            timed("host_tables", make_tables, kernels=False, wait=lambda: None)
            timed("host_mtf", on_host, kernels=False, wait=lambda: None)
        rec = {"largest_difference": float(np.abs(checks["m"] - checks["host"]).max()), "m0": [float(x) for x in checks["m"][0]]}
    else:
        curve = torch.empty_like(hist)
        target = ctx.decay_curve_tensor(histogram())
        ctx.synchronize()
        level = 10.0 * torch.log10(target.double() / target[:, :1].double())
        mask = ((level <= -5.0) & (level >= -35.0)).float().contiguous()
        del level
        torch.cuda.synchronize()
        e, t, m = curve.data_ptr(), target.data_ptr(), mask.data_ptr()
        for rep in s.repetitions(args.warmup, args.repeats):
            timed("curve", lambda: ctx.decay_curve(h, nrows, nbins, e))
            timed("times", lambda: ctx.decay_times(e, nrows, nbins, SR, -5.0, -35.0))
            timed("loss", lambda: checks.__setitem__("loss", ctx.decay_loss(h, e, t, m, nrows, nbins, capi.DECAY_NORMALISED, w)))
        rec = {"loss": float(checks["loss"].sum())}
    ctx.close()
    s.dump(args.work, side=args.step, nrows=nrows, nbins=nbins, **rec)


def report(args):
    t = Table()
    t.line("speech bench: rows x %d bins of float32, %d modulation frequencies, one context, one MI355X; median ms [min .. max] (n)" % (args.bins, len(FREQS)))
    t.line("calls: host clock to the synchronisation; kernels: HIP events of rvb_last_timings; floors at %.1f TB/s; host: %d threads" % (HBM_TBS, args.host_threads))
    records = benchsteps.records(args.work)
    for nrows in sorted({r["nrows"] for r in records}):
        mine = [r for r in records if r["nrows"] == nrows]
        t.samples = benchsteps.merge(mine, key=lambda rec, k: (rec["side"], k))
        first = next(r for r in mine if r["side"] == "new")
        array = nrows * args.bins * 4
        floor = array / (HBM_TBS * 1e12) * 1e3
        med = lambda key, side="new": t.med((side, key))
        t.line("%d x %d (%.1f MB); m of row 0 at 0.63 and 12.5 Hz: %.6f %.6f; largest |device - numpy| %.3e" %
               (nrows, args.bins, array / 1e6, first["m0"][0], first["m0"][-1], first["largest_difference"]))
        floors = {"mtf_sums_kernel": floor, "mtf_adjoint_kernel": 2 * floor}
        for name, label, call_floor in (("mtf", "rvb_mtf", floor), ("adjoint", "rvb_mtf_adjoint", 3 * floor)):
            t.row(label, ("new", name), tail="   floor %.3f ms: %.1f x" % (call_floor, med(name) / call_floor))
            for k in t.kernels("new", name):
                t.row("      " + k, ("new", name + ":" + k), tail="   floor %.3f ms: %.1f x" % (floors[k], med(name + ":" + k) / floors[k]) if k in floors else "")
        t.row("pinned download of the histogram", ("new", "download"))
        t.row("numpy: cos / sin tables of the shape", ("new", "host_tables"))
        t.row("numpy: transfer values of one histogram", ("new", "host_mtf"))
        t.line("  rvb_mtf %.3f ms against %.3f ms for the download and numpy with the tables at hand (%.0f x), %.3f ms with the tables made (%.0f x)" %
               (med("mtf"), med("download") + med("host_mtf"), (med("download") + med("host_mtf")) / med("mtf"),
                med("download") + med("host_mtf") + med("host_tables"), (med("download") + med("host_mtf") + med("host_tables")) / med("mtf")))
        if any(r["side"] == "parent" for r in mine):
            t.line("  this build against the parent's library, the same three calls in alternating processes:")
            for name, label in (("curve", "rvb_decay_curve"), ("times", "rvb_decay_times, -5 .. -35 dB"), ("loss", "rvb_decay_loss with weights")):
                t.row("    %s, this build" % label, ("this", name))
                t.row("    %s, parent" % label, ("parent", name))
                t.line("      difference of the medians %+.4f ms; the parent's own spread %.4f ms" %
                       (med(name, "this") - med(name, "parent"), t.spread(("parent", name))))
    t.emit(args.out)


def build_steps(args):
    turns = benchsteps.in_turn(args.rounds, args.parent_lib) if args.parent_lib else []
    return (benchsteps.shape(args, "bins", "repeats", "warmup", "host_repeats", "host_threads"),
            [(side, ["--nrows", str(int(n))], lib) for n in args.rows.split(",") for side, _, lib in [("new", [], None)] + turns])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", default="16,512")
    p.add_argument("--bins", type=int, default=846741)
    p.add_argument("--host-repeats", type=int, default=3)
    p.add_argument("--host-threads", type=int, default=16)
    benchsteps.add_common_arguments(p, repeats=21, warmup=3, step_timeout=240, parent_lib=True, rounds=2)
    p.add_argument("--nrows", type=int, default=0, help=argparse.SUPPRESS)
    args = p.parse_args()
    return benchsteps.run(args, dict.fromkeys(("new", "this", "parent"), step), report, build_steps)


if __name__ == "__main__":
    sys.exit(main())
