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
import json
import os
import shlex
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])


def other_surfaces(surfaces):
    rng = np.random.default_rng(11)
    b = surfaces.copy()
    b["specular"] = rng.uniform(0.3, 0.9, b["specular"].shape).astype(np.float32)
    b["diffuse"] = rng.uniform(0.3, 0.9, b["diffuse"].shape).astype(np.float32)
    return b


def step(args):
    """The GPU process: writes one JSON line of raw samples to the work file."""
    import rvb_import
    rvb_import.load()
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    table = other_surfaces(scene[2])
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
    samples = {}

    def note(name, value):
        samples.setdefault(name, []).append(float(value))

    def timed(name, call):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        note(name, (time.perf_counter() - t0) * 1e3)
        for k, v in ctx.last_timings():
            note(name + ":" + k, v)

    for rep in range(args.warmup + args.repeats):
        if rep == args.warmup:
            samples.clear()
        timed("reshade", lambda: ctx.reshade(table, air))
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        timed("accumulate", lambda: ctx.ir_accumulate(predelay, args.sample_rate, nbins, capi.IR_FAST, hist.data_ptr()))
        timed("grad", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()))
    ctx.close()
    with open(args.work, "w") as f:
        f.write(json.dumps({"samples": samples, "nbins": nbins, "nsurfaces": int(scene[2].shape[0])}) + "\n")


def report(args):
    rec = json.loads(open(args.work).read())
    s, nsurfaces, nbins = rec["samples"], rec["nsurfaces"], rec["nbins"]
    nrecords = args.rays * args.reflections
    lines = ["reshade_grad bench: %d rays x %d reflections = %d records, cathedral %d triangles, %d surfaces, 2 speakers, %.0f Hz, %d bins, one context" %
             (args.rays, args.reflections, nrecords, args.triangles, nsurfaces, args.sample_rate, nbins),
             "median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings"]

    def row(label, key):
        v = s[key]
        lines.append("  %-58s %8.3f [%.3f .. %.3f] (%d)" % (label, statistics.median(v), min(v), max(v), len(v)))

    for name, label in (("reshade", "rvb_reshade"), ("accumulate", "rvb_ir_accumulate, RVB_IR_FAST"), ("grad", "rvb_reshade_grad")):
        row(label, name)
        for k in sorted(k for k in s if k.startswith(name + ":")):
            row("      " + k.split(":", 1)[1], k)
    forward = statistics.median(s["reshade"]) + statistics.median(s["accumulate"])
    grad = statistics.median(s["grad"])
    evaluations = 16 * nsurfaces + 8
    lines.append("a finite-difference gradient: %d forward evaluations x (%.3f + %.3f) ms = %.1f ms; rvb_reshade_grad %.3f ms = %.2f forward evaluations" %
                 (evaluations, statistics.median(s["reshade"]), statistics.median(s["accumulate"]), evaluations * forward, grad, grad / forward))
    kernel = statistics.median(s["grad:reshade_grad_kernel"])
    lines.append("reshade_grad_kernel reads 48 B per record (16 side + 32 position and time) and gathers 32 B per live record and channel: "
                 "%.2f TB/s of record bytes" % (nrecords * 48 / (kernel * 1e-3) / 1e12))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    p.add_argument("--sample-rate", type=float, default=44100.0)
    p.add_argument("--repeats", type=int, default=21)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--step-timeout", type=int, default=240)
    p.add_argument("--out", default=None)
    p.add_argument("--step", default=None, help=argparse.SUPPRESS)
    p.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.step == "report":
        return report(args)
    if args.step:
        return step(args)
    work = os.path.join(tempfile.mkdtemp(prefix="reshade_grad_bench_"), "samples.json")
    shape = ["--rays", str(args.rays), "--reflections", str(args.reflections), "--triangles", str(args.triangles),
             "--sample-rate", str(args.sample_rate), "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    parts = ["timeout -k 10 %d %s" % (args.step_timeout, " ".join(shlex.quote(x) for x in me + shape + ["--step", "gpu"])),
             " ".join(shlex.quote(x) for x in me + shape + ["--step", "report"] + (["--out", args.out] if args.out else []))]
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
