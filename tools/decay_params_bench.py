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
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.6
LEVELS = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))


def step(args):
    """The GPU process of one shape and one build: appends one JSON line of raw samples to the work file."""
    sys.path.insert(0, args.root)
    import rvb_import
    rvb_import.load()
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
    ctx.decay_curve(h, nrows, nbins, e)
    ctx.synchronize()
    checks = {}
    if new:
        params = ctx.decay_params(e, nrows, nbins, sr)
        has = np.isfinite(params) & (params != 0)
        safe = np.where(has, params, 1.0).astype(np.float64)
        targets, pweights = (safe * 1.25).astype(np.float32), np.where(has, 1.0 / (safe * safe), 0.0).astype(np.float32)
    for rep in range(args.warmup + args.repeats):
        if rep == args.warmup:
            samples.clear()
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
    rec = {"side": args.step, "nrows": nrows, "nbins": nbins, "samples": samples, "loss": float(checks["loss"].sum())}
    if new:
        assert all(checks["params"][:, p].tobytes() == checks["three"][p].tobytes() for p in range(3)), "the times differ from rvb_decay_times"
        assert checks["ploss"].tobytes() == checks["ploss_only"].tobytes()
        rec.update(params0=[float(x) for x in checks["params"][0]], params_loss=float(checks["ploss"].sum()))
    ctx.close()
    with open(args.work, "a") as f:
        f.write(json.dumps(rec) + "\n")


def report(args):
    lines = ["decay params bench: rows x %d bins of float32, one context, one MI355X; median ms [min .. max] (n)" % args.bins,
             "calls: host clock to the synchronisation; kernels: HIP events of rvb_last_timings; floors at %.1f TB/s" % HBM_TBS]
    records = [json.loads(raw) for raw in open(args.work).read().splitlines()]
    for nrows in sorted({r["nrows"] for r in records}):
        merged = {"new": {}, "this": {}, "parent": {}}
        for r in records:
            if r["nrows"] == nrows:
                for k, v in r["samples"].items():
                    merged[r["side"]].setdefault(k, []).extend(v)
        first = next(r for r in records if r["nrows"] == nrows and r["side"] == "new")
        s, array = merged["new"], nrows * args.bins * 4
        floor = array / (HBM_TBS * 1e12) * 1e3
        med = lambda key, side="new": statistics.median(merged[side][key])
        lines.append("%d x %d (%.1f MB per array); EDT T20 T30 C50 C80 D50 Ts of row 0: %s; params loss %.6g, decay loss %.6g" %
                     (nrows, args.bins, array / 1e6, " ".join("%.4g" % x for x in first["params0"]), first["params_loss"], first["loss"]))

        def row(label, key, side="new", floor_ms=None):
            v = merged[side][key]
            tail = "" if floor_ms is None else "   floor %.3f ms: %.2f x" % (floor_ms, statistics.median(v) / floor_ms)
            lines.append("  %-58s %8.3f [%.3f .. %.3f] (%d)%s" % (label, statistics.median(v), min(v), max(v), len(v), tail))

        floors = {"decay_params_find_kernel": floor, "decay_params_sums_kernel": floor, "decay_params_adjoint_sums_kernel": floor,
                  "decay_params_adjoint_scan_kernel": 3 * floor}
        for name, label in (("params", "rvb_decay_params"), ("params_loss", "rvb_decay_params_loss with weights"),
                            ("params_loss_only", "rvb_decay_params_loss, loss only")):
            row(label, name)
            for k in sorted(k for k in s if k.startswith(name + ":")):
                row("      " + k.split(":", 1)[1], k, floor_ms=floors.get(k.split(":", 1)[1]))
        row("three rvb_decay_times calls (EDT, T20, T30)", "three_times")
        row("pinned download of the curve", "download")
        row("rvb_decay_loss with weights", "loss")
        row("rvb_decay_loss, loss only", "loss_only")
        kernels = lambda name: sum(statistics.median(s[k]) for k in s if k.startswith(name + ":"))
        lines.append("  params: %.3f ms against %.3f ms for the three calls and the download (%.1f x); kernels %.3f ms against a floor of %.3f ms "
                     "(E twice)" % (med("params"), med("three_times") + med("download"), (med("three_times") + med("download")) / med("params"),
                                    kernels("params"), 2 * floor))
        lines.append("  params loss with weights: %.3f ms against rvb_decay_loss' %.3f ms; loss only %.3f ms against %.3f ms; adjoint kernels %.3f ms "
                     "against a floor of %.3f ms (E twice, H once, w once)" %
                     (med("params_loss"), med("loss"), med("params_loss_only"), med("loss_only"), sum(statistics.median(v) for k, v in s.items() if k.startswith("params_loss:decay_params_adjoint")),
                      4 * floor))
        if merged["parent"]:
            lines.append("  this build against the parent build, the same three calls in alternating processes:")
            for name, label in (("curve", "rvb_decay_curve"), ("times", "rvb_decay_times, -5 .. -35 dB"), ("loss", "rvb_decay_loss with weights")):
                row("    %s, this build" % label, name, side="this")
                row("    %s, parent" % label, name, side="parent")
                runs = [statistics.median(r["samples"][name]) for r in records if r["nrows"] == nrows and r["side"] == "parent"]
                lines.append("      difference of the medians %+.4f ms; the parent's own processes: medians %s, samples %.3f .. %.3f" %
                             (med(name, "this") - med(name, "parent"), " / ".join("%.4f" % x for x in runs), min(merged["parent"][name]), max(merged["parent"][name])))
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
    p.add_argument("--parent", default=None, help="root of a built checkout of the commit to compare the unchanged calls with")
    p.add_argument("--out", default=None)
    p.add_argument("--step", default=None, help=argparse.SUPPRESS)
    p.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    p.add_argument("--nrows", type=int, default=0, help=argparse.SUPPRESS)
    p.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.step == "report":
        return report(args)
    if args.step:
        return step(args)
    work = os.path.join(tempfile.mkdtemp(prefix="decay_params_bench_"), "samples.json")
    shape = ["--bins", str(args.bins), "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    sides = [("new", ROOT)] + ([("this", ROOT), ("parent", os.path.abspath(args.parent))] * 2 if args.parent else [])
    parts = ["timeout -k 10 %d %s && echo 'decay_params_bench: %s rows, %s build done' >&2" %
             (args.step_timeout, " ".join(shlex.quote(x) for x in me + shape + ["--step", side, "--root", root, "--nrows", str(int(n))]), int(n), side)
             for n in args.rows.split(",") for side, root in sides]
    parts.append(" ".join(shlex.quote(x) for x in me + shape + ["--step", "report"] + (["--out", args.out] if args.out else [])))
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
