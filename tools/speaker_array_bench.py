#!/usr/bin/env python3
"""Developer tool: duration of the binning stage at workload C2 for speaker arrays of 8, 16, 24, 32 and 64 channels, both modes, two arms
alternated in one process on ONE trace (HIP events around the stage, rvb_last_timings):
    wide      one ir_configure_speakers(C) + ir_accumulate_tensor                       (above 8 channels: ordered_sum_wide_kernel)
    by hand   ceil(C / 8) x (ir_configure_speakers of eight + ir_accumulate_tensor into that slice of the histogram): what a caller
              had to do while the fused path stopped at eight channels — the eight-channel kernels only
Every shape is warmed first; min / median / max over the repeats per cell.
    python tools/speaker_array_bench.py [--repeats 6] [--channels 8,16,24,32,64] [--only wide|byhand] [--modes exact,fast] [--out FILE]
--only runs one arm alone (for a rocprofv3 --pmc pass of its own)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rvb_import  # noqa: E402

rvb_import.load()
from parallel_reverb_raytracer_amd import capi, dtypes, scenes  # noqa: E402


def main():
    import torch
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=6)
    p.add_argument("--channels", default="8,16,24,32,64")
    p.add_argument("--modes", default="exact,fast")
    p.add_argument("--only", choices=["wide", "byhand"])
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    p.add_argument("--out")
    args = p.parse_args()
    sr = 44100.0
    scene, info = scenes.cathedral(args.triangles)
    mic = info["mic"]
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.raytrace(mic, info["source"], scenes.sphere_directions(args.rays, seed=1), args.reflections, dtypes.AIR_COEFFICIENTS)
    images = ctx.get_raw_images(False)
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def stage(directions, coefficients, mode, hist):
        ctx.ir_configure_speakers(mic, directions, coefficients, capi.IR_ALL, images)
        ctx.ir_accumulate_tensor(lo, sr, nbins, mode, hist)
        ctx.synchronize()
        return sum(v for _, v in ctx.last_timings())

    def wide(directions, coefficients, mode, hist):
        return stage(directions, coefficients, mode, hist)

    def byhand(directions, coefficients, mode, hist):
        return sum(stage(directions[g:g + 8], coefficients[g:g + 8], mode, hist[g:g + 8]) for g in range(0, len(coefficients), 8))

    ctx.ir_configure_speakers(mic, [(1, 0, 0)], [0.5], capi.IR_ALL, images)
    lo, hi = ctx.ir_time_range()
    nbins = ctx.ir_bins(hi, lo, sr)
    say("workload: %d triangles, %d rays x %d, %.0f Hz, %d bins, %d image impulses; %d repeats per cell, arms alternated; ms, min / median / max"
        % (args.triangles, args.rays, args.reflections, sr, nbins, images.shape[0], args.repeats))
    say("%-9s %-6s %-26s %-26s %s" % ("channels", "mode", "wide", "by hand (eights)", "by hand / wide (medians)"))
    arms = [("wide", wide), ("byhand", byhand)]
    if args.only:
        arms = [a for a in arms if a[0] == args.only]
    for nch in [int(x) for x in args.channels.split(",")]:
        directions = scenes.sphere_directions(nch, seed=101)[:, :3]
        coefficients = np.linspace(0.0, 1.0, nch).astype(np.float32)
        hists = {name: torch.zeros((nch, 8, nbins), device="cuda", dtype=torch.float32) for name, _ in arms}
        for mode_name in args.modes.split(","):
            mode = capi.IR_EXACT if mode_name == "exact" else capi.IR_FAST
            times = {name: [] for name, _ in arms}
            for rep in range(args.repeats + 1):                 # repeat 0 warms the shape
                for name, arm in arms:
                    hists[name].zero_()
                    torch.cuda.synchronize()
                    t = arm(directions, coefficients, mode, hists[name])
                    if rep:
                        times[name].append(t)
            cells = {name: "%8.3f /%8.3f /%8.3f" % (min(v), float(np.median(v)), max(v)) for name, v in times.items()}
            ratio = ""
            if len(arms) == 2:
                ratio = "%.2f" % (float(np.median(times["byhand"])) / float(np.median(times["wide"])))
                if mode == capi.IR_EXACT:
                    ratio += "   same bytes: %s" % bool(torch.equal(hists["wide"], hists["byhand"]))
            say("%-9d %-6s %-26s %-26s %s" % (nch, mode_name, cells.get("wide", "-"), cells.get("byhand", "-"), ratio))
        del hists
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
