#!/usr/bin/env python3
"""Developer tool: what the sensitivity map (rvb_reshade_grad_map, csrc/reshade_grad_map_kernels.hip) takes against the only other way
to the same numbers, rvb_reshade_grad on the scene relabelled with one surface per triangle (a sweep of the kept trace per 64
triangles).  At 100 000 rays x 128 reflections, two cardioid speakers, 44.1 kHz, the workload's own predelay and bin count, in the
cathedral at every size of --triangles (75 000 and 3 000 by default), one process per size and library, it records as medians with
their spread

  rvb_trace, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER     this library and, with --parent-lib, the library of the commit before
  rvb_reshade_grad (the scene's own surfaces)           both libraries alike
  rvb_reshade_grad_map                                  its kernels broken out, against their byte floors
  rvb_reshade_grad, one surface per triangle            --relabelled-repeats calls in full (ntriangles / 64 sweeps each)

--rounds processes per size and library, the two libraries in turn and the parent's first in every other round.

Call times are host clocks around work that ends in rvb_synchronize; kernel times are the HIP events of rvb_last_timings.  Every GPU
step is a child process under its own `timeout -k 10`, chained with &&; the table is written (--out) only when all of them ended well.
In an --out file that exists it replaces what stands above the line "---- notes" and keeps the rest.

    python tools/reshade_grad_map_bench.py [--rays N] [--reflections K] [--triangles T ...] [--parent-lib SO] [--out FILE]
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
NOTES_MARK = "---- notes"          # in the --out file: what follows is kept when the table above it is written again
PEAK_TBS = 6.6          # a streaming pass on this device (profiles/reshade_grad_n1.txt)


def other_surfaces(surfaces):
    rng = np.random.default_rng(11)
    b = surfaces.copy()
    b["specular"] = rng.uniform(0.3, 0.9, b["specular"].shape).astype(np.float32)
    b["diffuse"] = rng.uniform(0.3, 0.9, b["diffuse"].shape).astype(np.float32)
    return b


def tolerate_an_older_library():
    """The binding is strict: it sets the argument types of every entry point when it loads the library, and the parent commit's
    library lacks rvb_reshade_grad_map.  For the parent's process alone, the loader hands out a stand-in for an rvb_* symbol that the
    library does not export; the step never calls it."""
    import ctypes

    class Missing:
        restype = argtypes = None

    class Older(ctypes.CDLL):
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if not name.startswith("rvb_"):
                    raise
                return Missing()

    ctypes.CDLL = Older


def step(args):
    """The GPU process of one (library, size): appends one JSON line of raw samples to the work file."""
    import rvb_import
    rvb_import.load()
    has_map = args.step != "parent"
    if not has_map:
        tolerate_an_older_library()
    import torch
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    air = dtypes.AIR_COEFFICIENTS
    triangles = args.triangles[0]
    scene, info = scenes.cathedral(triangles)
    mic, src = info["mic"], info["source"]
    table = other_surfaces(scene[2])
    samples = {}

    def note(name, value):
        samples.setdefault(name, []).append(float(value))

    def timed(ctx, name, call):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        note(name, (time.perf_counter() - t0) * 1e3)
        for k, v in ctx.last_timings():
            note(name + ":" + k, v)

    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
    ctx.keep_paths(True, listener=True)
    ctx.trace(mic, src, args.reflections, air)
    ctx.reshade(table, air)
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, args.sample_rate)
    weights = torch.randn((2, 8, nbins), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    out = torch.empty((scene[0].shape[0], 16), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for rep in range(args.warmup + args.repeats):
        if rep == args.warmup:
            samples.clear()
        timed(ctx, "trace", lambda: ctx.trace(mic, src, args.reflections, air))
        ctx.reshade(table, air)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        ctx.synchronize()
        timed(ctx, "grad", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()))
        if has_map:
            timed(ctx, "map", lambda: ctx.reshade_grad_map(predelay, args.sample_rate, nbins, weights.data_ptr(), out=out))
    live = None
    if has_map:
        live = int((out != 0).any(dim=1).sum().item())
    ctx.close()
    if has_map and args.relabelled_repeats:
        # the same numbers through rvb_reshade_grad: every triangle a surface of its own with its surface's coefficients
        relabelled = scene[0].copy()
        relabelled["surface"] = np.arange(relabelled.shape[0])
        own = np.ascontiguousarray(table[scene[0]["surface"].astype(np.int64)])
        ctx = capi.Context(0)
        ctx.set_scene((relabelled, scene[1], np.ascontiguousarray(scene[2][scene[0]["surface"].astype(np.int64)])))
        ctx.set_directions(scenes.sphere_directions(args.rays, seed=1))
        ctx.keep_paths(True)
        ctx.trace(mic, src, args.reflections, air)
        ctx.reshade(own, air)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        for rep in range(args.relabelled_repeats):
            timed(ctx, "relabelled", lambda: ctx.reshade_grad(predelay, args.sample_rate, nbins, weights.data_ptr()))
        ctx.close()
    with open(args.work, "a") as f:
        f.write(json.dumps({"step": args.step, "triangles": int(scene[0].shape[0]), "asked": triangles, "samples": samples, "nbins": nbins,
                            "live": live}) + "\n")


def report(args):
    recs = [json.loads(line) for line in open(args.work)]
    nrecords = args.rays * args.reflections
    lines = ["reshade_grad_map bench: %d rays x %d reflections = %d records, 2 speakers, %.0f Hz, one context" %
             (args.rays, args.reflections, nrecords, args.sample_rate),
             "median ms [min .. max] (n); calls: host clock to rvb_synchronize; kernels: HIP events of rvb_last_timings"]
    for asked in args.triangles:
        mine = [r for r in recs if r["asked"] == asked]
        if not mine:
            continue
        ntri = mine[0]["triangles"]
        merged = {}
        for r in mine:
            for k, v in r["samples"].items():
                merged.setdefault((r["step"], k), []).extend(v)
        lines.append("")
        lines.append("cathedral, %d triangles, %d bins; triangles with a non-zero row: %s" % (ntri, mine[0]["nbins"], next((r["live"] for r in mine if r["live"] is not None), "?")))

        def med(key):
            return statistics.median(merged[key]) if key in merged else None

        def row(label, key):
            if key not in merged:
                lines.append("  %-66s not measured" % label)
                return
            v = merged[key]
            lines.append("  %-66s %9.3f [%.3f .. %.3f] (%d)" % (label, statistics.median(v), min(v), max(v), len(v)))

        for name, label in (("trace", "rvb_trace, RVB_KEEP_MATERIALS | RVB_KEEP_LISTENER"), ("grad", "rvb_reshade_grad, the scene's own surfaces")):
            row(label + ", this library", ("this", name))
            row(label + ", parent library", ("parent", name))
            a, b = med(("this", name)), med(("parent", name))
            if a is not None and b is not None:
                v = merged[("parent", name)]
                lines.append("      difference of the medians %+.3f ms; spread of the parent's repetitions %.3f ms (max - min): %s" %
                             (a - b, max(v) - min(v), "inside" if abs(a - b) <= max(v) - min(v) else "OUTSIDE"))
        row("rvb_reshade_grad_map", ("this", "map"))
        for k in sorted(k for s, k in merged if s == "this" and k.startswith("map:")):
            row("      " + k[4:], ("this", k))
        row("rvb_reshade_grad, one surface per triangle (%d sweeps)" % ((ntri + 63) // 64), ("this", "relabelled"))
        m, rel = med(("this", "map")), med(("this", "relabelled"))
        if m is not None and rel is not None:
            lines.append("  the map against the relabelled path: %.3f ms against %.3f ms, %.0f times %s" % (m, rel, rel / m, "faster" if m < rel else "SLOWER"))
        floors = (("map:reshade_grad_map_terms_kernel", 48 + 8 + 64 + 8, "48 B of records, 8 B listener record read; 64 B row, 8 B sort entry written"),
                  ("map:reshade_grad_map_sort", 0, None),
                  ("map:reshade_grad_map_fold_kernel", 8 + 64, "8 B sort entry, 64 B row gathered"))
        for key, per_record, what in floors:
            t = med(("this", key))
            if t is None:
                continue
            if per_record:
                tbs = nrecords * per_record / (t * 1e-3) / 1e12
                lines.append("  %s: %d B per record (%s): %.2f TB/s, floor %.3f ms at %.1f TB/s" %
                             (key[4:], per_record, what, tbs, nrecords * per_record / (PEAK_TBS * 1e12) * 1e3, PEAK_TBS))
            else:
                bits = max(1, int(ntri).bit_length())
                passes = (bits + 7) // 8
                lines.append("  %s: %d key bits, at least %d passes of 16 B per entry (8 read, 8 written): floor %.3f ms at %.1f TB/s" %
                             (key[4:], bits, passes, passes * nrecords * 16 / (PEAK_TBS * 1e12) * 1e3, PEAK_TBS))
        parts = {k: med(("this", "map:" + k)) for k in ("reshade_grad_map_terms_kernel", "reshade_grad_map_sort", "reshade_grad_map_fold_kernel")}
        if all(v is not None for v in parts.values()):
            lines.append("  the largest of the three: %s" % max(parts, key=parts.get))
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        # the table replaces what stands above the line that starts with NOTES_MARK; the notes from there on are kept
        notes = ""
        if os.path.exists(args.out):
            old = open(args.out).read()
            at = old.find("\n" + NOTES_MARK)
            notes = old[at:] if at >= 0 else ""
        with open(args.out, "w") as f:
            f.write(text + "\n" + notes)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, nargs="+", default=[75000, 3000])
    p.add_argument("--sample-rate", type=float, default=44100.0)
    p.add_argument("--repeats", type=int, default=11)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--relabelled-repeats", type=int, default=1, help="full calls of the relabelled path per size (0: skip it)")
    p.add_argument("--rounds", type=int, default=2, help="processes per size and library")
    p.add_argument("--parent-lib", default=None, help="librvb_hip.so built from the commit before the feature")
    p.add_argument("--step-timeout", type=int, default=400)
    p.add_argument("--out", default=None)
    p.add_argument("--step", default=None, help=argparse.SUPPRESS)
    p.add_argument("--work", default=None, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.step == "report":
        return report(args)
    if args.step:
        return step(args)
    work = os.path.join(tempfile.mkdtemp(prefix="reshade_grad_map_bench_"), "samples.jsonl")
    common = ["--rays", str(args.rays), "--reflections", str(args.reflections), "--sample-rate", str(args.sample_rate), "--repeats", str(args.repeats),
              "--warmup", str(args.warmup), "--work", work]
    me = [sys.executable, os.path.abspath(__file__)]
    parts = []
    for triangles in args.triangles:      # every GPU step under a time limit of its own; a step that fails ends the chain
        for r in range(args.rounds):
            # the libraries in turn, the parent's first in every other round: two processes differ by more than two repetitions of one,
            # so either library gets both places.  The relabelled path once, in this library's first process.
            steps = [("", "this")] + ([("RVB_LIB=%s " % shlex.quote(os.path.abspath(args.parent_lib)), "parent")] if args.parent_lib else [])
            for env, name in steps[::-1] if r % 2 else steps:
                relabelled = args.relabelled_repeats if name == "this" and r == 0 else 0
                parts.append("%stimeout -k 10 %d %s" % (env, args.step_timeout, " ".join(shlex.quote(x) for x in me + common +
                             ["--relabelled-repeats", str(relabelled), "--triangles", str(triangles), "--step", name])))
    parts.append(" ".join(shlex.quote(x) for x in me + common + ["--relabelled-repeats", str(args.relabelled_repeats), "--triangles"] + [str(t) for t in args.triangles] + ["--step", "report"]
                          + (["--out", args.out] if args.out else [])))
    return subprocess.call(["bash", "-c", " && ".join(parts)])


if __name__ == "__main__":
    sys.exit(main())
