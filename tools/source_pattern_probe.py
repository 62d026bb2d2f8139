#!/usr/bin/env python3
"""Developer tool: what the directional-source pass (csrc/source_kernels.hip) costs.  At workload C2 by default (100 000 rays x 128
reflections in the 75 000-triangle cathedral) it prints, and with --out appends to a file,

  A. source_pattern_kernel from rvb_last_timings for each store form (RVB_SOURCE_STORE = record | record_nt | volumes | volumes_nt)
     and attenuate_kernel on the same records in the same session: milliseconds (median of --repeats) and achieved bytes per second
     (the pass reads 64 B per record and writes 64 B or 32 B; attenuate_kernel reads 64 B and writes 64 B);
  B. milliseconds per impulse response through rvb_pipeline_* (4 contexts, exact mode, two speakers) without and with a pattern,
     alternating runs.

    python tools/source_pattern_probe.py [--rays N] [--reflections K] [--triangles T] [--repeats R] [--jobs J] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rvb_import  # noqa: E402

rvb_import.load()
from parallel_reverb_raytracer_amd import capi, dtypes, scenes  # noqa: E402

FACING, SHAPES = (0.8, 0.35, -0.5), np.linspace(0.0, 1.0, 8).astype(np.float32)
SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--jobs", type=int, default=32)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import torch

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    nrecords = args.rays * args.reflections
    say("source pattern probe: %d rays x %d reflections = %d records (%.0f MB), cathedral %d" %
        (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, args.triangles))

    # ---- A: the pass per store form, attenuate_kernel beside it -------------------------------------------------------------
    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(dirs)
    d_out = torch.empty(nrecords * 16, dtype=torch.float32, device="cuda")
    forms = ["record", "record_nt", "volumes", "volumes_nt"]
    taken = {f: [] for f in forms}
    taken["attenuate_kernel"] = []
    shadow = {"with": [], "without": []}
    ctx.set_source_pattern(None)
    for _ in range(2):                                      # warm-up, and the shadow kernel without the pass behind it
        ctx.trace(mic, src, args.reflections, dtypes.AIR_COEFFICIENTS)
        shadow["without"] += [v for k, v in ctx.last_timings() if k.startswith("shadow")]
    ctx.set_source_pattern(FACING, SHAPES)
    for _ in range(args.repeats):
        for form in forms:                                  # alternating: every form sees the same drift
            os.environ["RVB_SOURCE_STORE"] = form
            ctx.trace(mic, src, args.reflections, dtypes.AIR_COEFFICIENTS)
            t = dict(ctx.last_timings())
            taken[form].append(t["source_pattern_kernel"])
            shadow["with"] += [v for k, v in t.items() if k.startswith("shadow")]
            d_in, n = ctx.diffuse_device()
            ctx.attenuate_speaker_device(mic, d_in, n, SPEAKERS[0][0], SPEAKERS[1][0], d_out.data_ptr())
            taken["attenuate_kernel"].append(dict(ctx.last_timings())["attenuate_kernel"])
    os.environ.pop("RVB_SOURCE_STORE", None)
    moved = {"record": 128, "record_nt": 128, "volumes": 96, "volumes_nt": 96, "attenuate_kernel": 128}
    for name in forms + ["attenuate_kernel"]:
        ms = statistics.median(taken[name])
        say("  %-32s %.3f ms (min %.3f, max %.3f, n %d)  %3d B/record  %.2f TB/s" %
            (name if name == "attenuate_kernel" else "source_pattern_kernel[%s]" % name, ms, min(taken[name]), max(taken[name]), len(taken[name]),
             moved[name], nrecords * moved[name] / (ms * 1e-3) / 1e12))
    say("  (source_pattern_kernel covers the streaming pass AND the small launch over candidates and direct slot)")
    say("  shadow kernel: %.3f ms without the pass behind it, %.3f ms with" % (statistics.median(shadow["without"]), statistics.median(shadow["with"])))
    ctx.set_source_pattern(None)
    ctx.close()
    del d_out
    torch.cuda.empty_cache()

    # ---- B: the pipeline with and without a pattern, alternating --------------------------------------------------------------
    contexts = [capi.Context(0) for _ in range(4)]
    contexts[0].set_scene(scene)
    for c in contexts:
        if c is not contexts[0]:
            c.share_scene(contexts[0])
        c.set_directions(dirs)
    pipe = capi.Pipeline(contexts)
    pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], args.reflections, dtypes.AIR_COEFFICIENTS)
    rng = np.random.default_rng(3)

    def run(njobs):
        sent = got = 0
        t0 = time.perf_counter()
        while got < njobs:
            while sent < njobs and pipe.pending() < pipe.limit:
                jitter = rng.uniform(-0.5, 0.5, 3)
                pipe.submit(np.asarray(mic) + jitter, src)
                sent += 1
            pipe.next(copy=False)
            got += 1
        return (time.perf_counter() - t0) * 1e3 / njobs

    run(8)
    per_ir = {"without": [], "with": []}
    for _ in range(3):
        for which in ("without", "with"):
            pipe.set_source_pattern(FACING if which == "with" else None, SHAPES)
            run(4)
            per_ir[which].append(run(args.jobs))
    for which in ("without", "with"):
        say("  pipeline, 4 contexts, exact mode, %s a pattern: %s ms per IR (alternating runs of %d jobs), median %.3f" %
            (which, " / ".join("%.3f" % v for v in per_ir[which]), args.jobs, statistics.median(per_ir[which])))
    pipe.close()
    for c in contexts:
        c.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
