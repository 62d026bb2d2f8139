#!/usr/bin/env python3
"""Developer tool: what the echo finder costs (rvb_window_paths of include/rvb_capi_window.h, csrc/window_kernels.hip) and what the
same query costs without it.  At workload C2 by default (100 000 rays x 128 reflections in the 75 000-triangle cathedral, one context,
the trace kept with RVB_KEEP_LISTENER) it records, as medians over all repetitions with their spread,

  (w) rvb_window_paths, max_hits = nreflections, for three windows — 50 ms from the first arrival, [q25, q75) of the live times, the
      whole response — at max_paths 64 and 1024, with its kernels by name
  (t) torch: the score of every record from a float32 view of the records, the window mask, torch.topk(1024)
  (h) rvb_get_diffuse plus numpy: the 64-byte records to the host, the score, np.argpartition and a sort of the 1024 winners
  (a) with --parent-lib: rvb_trace with keeping on, rvb_reshade and rvb_relisten of this library and of a build of the commit before
      the feature, in processes that take turns

Call times are host clocks around calls that return when the work is done (the window calls are synchronous; the others end in
rvb_synchronize); kernel times are the HIP events of rvb_last_timings.  Every GPU step is a child process under its own `timeout -k 10`,
the steps are chained with &&, and the table is written (--out) only when all of them ended well.

    python tools/window_bench.py [--parent-lib PATH] [--rays N] [--reflections K] [--triangles T] [--repeats R] [--rounds M] [--out FILE]
"""
import argparse
import ctypes
import json
import sys
import time

import benchsteps
from benchsteps import Samples, Table

OTHER_MIC = (-10.28, 3.85, -2.24)
HBM_TBS = 6.6                 # the streaming rate the floor of the score pass is taken at


def step(args):
    """One GPU process: --step window | routes | this | parent.  Appends one JSON line of raw samples to the work file."""
    import numpy as np
    benchsteps.load_library()
    from parallel_reverb_raytracer_amd import capi, dtypes, scenes
    if args.step == "parent":
        capi._WINDOW_SIGNATURES.clear()                                     # (the parent's library does not export them)
    air = dtypes.AIR_COEFFICIENTS
    scene, info = scenes.cathedral(args.triangles)
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(args.rays, seed=1)
    s, facts = Samples(), {}
    note = s.note

    ctx = capi.Context(0)
    ctx.set_scene(scene)
    ctx.set_directions(dirs)
    ctx.keep_paths(True, listener=True)

    def timed(name, call):
        s.timed(name, call, ctx.synchronize, ctx.last_timings)

    if args.step in ("this", "parent"):
        for rep in s.repetitions(args.warmup, args.repeats):
            timed("trace", lambda: ctx.trace(mic, src, args.reflections, air))
            timed("reshade", lambda: ctx.reshade(None, air))
            timed("relisten", lambda: ctx.relisten(OTHER_MIC))
            timed("relisten", lambda: ctx.relisten(mic))
    else:
        ctx.trace(mic, src, args.reflections, air)
        ctx.synchronize()
        records = ctx.get_raw_diffuse()
        live = (records["volume"] != 0).any(axis=1)
        times = records["time"][live]
        first = float(times[times > 0].min())
        q25, q75 = (float(np.float32(q)) for q in np.quantile(times.astype(np.float64), [0.25, 0.75]))
        windows = {"50ms": (first, float(np.float32(first + 0.05))), "q25_q75": (q25, q75), "whole": (0.0, float(np.float32(times.max() * 2 + 1)))}
        facts.update(records=int(records.shape[0]), live=int(live.sum()), windows=windows)
        n = records.shape[0]
        if args.step == "window":
            def block(nbytes):
                p = ctypes.c_void_p()
                ctx._check(ctx.lib.rvb_device_alloc(ctx.handle, nbytes, ctypes.byref(p)))
                return p
            d_paths = block(capi.WINDOW_MAX_PATHS * capi.WINDOW_PATH.itemsize)
            d_hits = block(capi.WINDOW_MAX_PATHS * args.reflections * capi.WINDOW_HIT.itemsize)
            count, inside = ctypes.c_uint64(0), ctypes.c_uint64(0)
            for name, (t0, t1) in windows.items():
                for k in (64, 1024):
                    part = Samples()                                        # a warm-up per window and list length; the call is synchronous
                    for rep in part.repetitions(args.warmup, args.repeats):
                        part.timed("w %s %d" % (name, k), lambda: ctx._check(ctx.lib.rvb_window_paths(
                            ctx.handle, t0, t1, None, k, args.reflections, d_paths, d_hits, ctypes.byref(count), ctypes.byref(inside))),
                            lambda: None, ctx.last_timings)
                    s.samples.update(part.samples)
                    facts["in_window %s" % name] = inside.value
                    facts["count %s %d" % (name, k)] = count.value
                    if (name, k) == ("q25_q75", 1024):                      # the list the routes step makes on the host
                        paths = np.zeros(count.value, dtype=capi.WINDOW_PATH)
                        ctx._check(ctx.lib.rvb_copy_to_host(ctx.handle, paths.ctypes.data, d_paths, paths.nbytes))
                        facts["gpu_top"] = [int(r) * args.reflections + int(b) for r, b in zip(paths["ray"], paths["bounce"])]
        else:
            t0w, t1w = windows["q25_q75"]

            def numpy_route():
                t = time.perf_counter()
                rec = ctx.get_raw_diffuse()
                note("h copy", (time.perf_counter() - t) * 1e3)
                x = rec["volume"]
                score = np.zeros(n, np.float32)
                for b in range(8):
                    score += x[:, b] * x[:, b]
                score[~((rec["time"] >= np.float32(t0w)) & (rec["time"] < np.float32(t1w)))] = 0
                top = np.argpartition(score, n - 1024)[n - 1024:]
                top = top[np.lexsort((top, -score[top].view(np.uint32).astype(np.int64)))]
                note("h", (time.perf_counter() - t) * 1e3)
                return top
            for rep in range(3):
                top = numpy_route()
            facts["host_top"] = [int(i) for i in top]
            import torch
            d_in, count = ctx.diffuse_device()

            class View:                                                     # the records where they are, as torch sees foreign device memory
                __cuda_array_interface__ = {"shape": (n, 16), "typestr": "<f4", "data": (int(d_in), True), "version": 2, "strides": None}
            try:
                view = torch.as_tensor(View(), device="cuda")
                _ = float(view[0, 0])
                facts["torch_input"] = "the rvb_diffuse_device view"
            except Exception as e:                                          # (the library and torch each bring a HIP runtime)
                view = torch.from_numpy(records.view(np.float32).reshape(n, 16).copy()).cuda()
                facts["torch_input"] = "a copy of the records in a torch tensor (torch refused the foreign pointer: %s)" % type(e).__name__

            def torch_route():
                v = view[:, :8]
                score = (v * v).sum(dim=1)
                t = view[:, 12]
                score = torch.where((t >= t0w) & (t < t1w), score, torch.zeros_like(score))
                return torch.topk(score, 1024)
            for rep in range(args.warmup + args.repeats):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = torch_route()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    note("t", (time.perf_counter() - t) * 1e3)
            facts["torch_top_set_equals_host"] = sorted(int(i) for i in out.indices.cpu()) == sorted(facts["host_top"])
    ctx.close()
    s.dump(args.work, step=args.step, lib=capi.LIB_PATH, facts=facts)


def report(args):
    recs, facts = benchsteps.records(args.work), {}
    for rec in recs:
        facts.setdefault(rec["step"], {}).update(rec["facts"])
    t = Table(benchsteps.merge(recs), label=66, value=9)
    nrecords = args.rays * args.reflections
    t.line("window bench: %d rays x %d reflections = %d records (%.0f MB), cathedral %d triangles, one context, trace kept with RVB_KEEP_LISTENER"
           % (args.rays, args.reflections, nrecords, nrecords * 64 / 1e6, args.triangles))
    t.line("median ms [min .. max] (n); calls: host clock around the call (window calls are synchronous, the others run to rvb_synchronize); "
           "kernels: HIP events of rvb_last_timings")
    t.line("floor of the score pass: %.0f MB at %.1f TB/s = %.3f ms" % (nrecords * 64 / 1e6, HBM_TBS, nrecords * 64 / (HBM_TBS * 1e12) * 1e3))
    w = facts.get("window", {})
    if w:
        t.line("records %d, live %d; windows %s" % (w["records"], w["live"], json.dumps(w["windows"])))
    for name in ("50ms", "q25_q75", "whole"):
        for k in (64, 1024):
            prefix = "w %s %d" % (name, k)
            if ("window", prefix) not in t.samples:
                continue
            t.row("(w) rvb_window_paths, %s, max_paths %d (in window %s, listed %s)" % (name, k, w.get("in_window %s" % name), w.get("count %s %d" % (name, k))),
                  ("window", prefix))
            kernels = sorted(t.kernels("window", prefix), key=lambda kernel: -t.med(("window", prefix + ":" + kernel)))       # the longest first
            for kernel in kernels:
                t.row("      " + kernel, ("window", prefix + ":" + kernel))
            if kernels:
                t.line("      bound by %s; the score pass streams %.2f TB/s" %
                       (kernels[0], nrecords * 64 / (t.med(("window", prefix + ":window_score_kernel")) * 1e-3) / 1e12))
    r = facts.get("routes", {})
    if r:
        t.line("the same query ([q25, q75), 1024 entries) without the feature:")
        t.row("(t) torch: score, mask, torch.topk over %s" % r.get("torch_input"), ("routes", "t"))
        t.row("(h) rvb_get_diffuse + numpy (argpartition, sort of the winners)", ("routes", "h"))
        t.row("      of which the copy of the records to the host", ("routes", "h copy"))
        t.line("  torch's 1024 are the host's 1024 as a set: %s" % r.get("torch_top_set_equals_host"))
        if "gpu_top" in w and "host_top" in r:
            t.line("  rvb_window_paths' 1024 are the host's 1024, in the same order: %s" % (w["gpu_top"] == r["host_top"]))
    if any(step_ == "parent" for step_, _ in t.samples):
        t.line("unchanged paths against a build of the parent commit (processes in turn):")
        for call in ("trace", "reshade", "relisten"):
            a, b = t.row("(a) rvb_%s, this library" % call, ("this", call)), t.row("(a) rvb_%s, parent library" % call, ("parent", call))
            if a is not None and b is not None:
                spread = t.spread(("parent", call))
                t.line("      %.3f against %.3f ms, difference %+.3f ms; spread of the parent's repetitions %.3f ms (max - min): %s" %
                       (a, b, a - b, spread, "inside" if abs(a - b) <= spread else "OUTSIDE"))
    t.emit(args.out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rays", type=int, default=100000)
    p.add_argument("--reflections", type=int, default=128)
    p.add_argument("--triangles", type=int, default=75000)
    benchsteps.add_common_arguments(p, repeats=21, warmup=3, step_timeout=240, parent_lib=True, rounds=2)
    args = p.parse_args()
    return benchsteps.run(args, dict.fromkeys(("window", "routes", "this", "parent"), step), report, lambda args: (
        benchsteps.shape(args, "rays", "reflections", "triangles", "repeats", "warmup"),
        [("window", [], None), ("routes", [], None)] + (benchsteps.in_turn(args.rounds, args.parent_lib) if args.parent_lib else [])))


if __name__ == "__main__":
    sys.exit(main())
