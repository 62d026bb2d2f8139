"""The contract of parallel_reverb_raytracer_amd.distributed, per rank: the ORDER of the calls it makes on its tracer(s) and the
order of its collectives.  A recording stand-in (tests/oracle_tracer.py, CPU oracle, gloo) logs every call with the integer arguments
that define the schedule — never arrays or floats —, together with the `on_stage` names, the `host_out` and `on_result` calls and
the `torch.distributed` collectives (peer only); the logs must equal tests/golden/distributed_call_order.json entry for entry.
The enqueued device work of a GPU context is a function of that sequence, so an orchestration change that keeps it has changed
no device work.

    python tests/test_distributed_call_order.py --write

records the fixture anew (only when a schedule is changed on purpose)."""
import contextlib
import inspect
import json
import os
import socket
import subprocess
import sys

import numpy as np

from conftest import ROOT

from oracle_tracer import OracleTracer
from parallel_reverb_raytracer_amd import capi, distributed, dtypes, scenes

FIXTURE = os.path.join(ROOT, "tests", "golden", "distributed_call_order.json")
SPEAKERS = dict(speakers_dir=[(-1, 0, -1), (1, 0, -1)], speakers_coeff=[0.5, 0.5])
RAYS, NREFL = 64, 8                                      # generate_ir / IrPipeline: scenes.cathedral(1200)
PAIRS, PAIR_RAYS, PAIR_NREFL = 5, 40, 6                  # generate_pair_irs: scenes.concert_hall(900)

# logged per tracer method: the integer arguments that define the schedule ("images", "mics": their number)
LOGGED = {"set_concurrent_traces": ("traces",), "trace": ("nreflections", "ray_offset"),
          "trace_pairs": ("mics", "nreflections", "ray_offset"), "select_pair": ("pair",), "get_image_candidates": (),
          "get_pair_candidates": ("pair",), "get_direct": (), "ir_configure_speakers": ("which", "images"),
          "ir_configure_hrtf": ("which", "images"), "ir_time_range": (), "ir_bins": (), "ir_accumulate_tensor": ("nbins", "mode"),
          "ir_accumulate_export_tensor": ("nbins", "mode"), "ir_accumulate_wait_for_torch": (), "export_tensor_to_host": (),
          "synchronize_exports": (), "ir_exact_prepare": ("nbins",), "ir_exact_fold_tensor": ("nbins", "bin_begin", "bin_end"),
          "synchronize": ()}
COLLECTIVES = {"all_gather": None, "all_reduce": None, "send": "dst", "recv": "src", "broadcast": "src"}     # name -> its peer argument


def _logged(name, keep):
    base = getattr(OracleTracer, name)
    signature = inspect.signature(base)

    def method(self, *args, **kwargs):
        given = signature.bind(self, *args, **kwargs)
        given.apply_defaults()
        shown = ["%s=%d" % (k, 0 if given.arguments[k] is None else len(given.arguments[k]) if k in ("images", "mics") else given.arguments[k])
                 for k in keep]
        result = base(self, *args, **kwargs)
        if name == "ir_bins":
            shown.append("-> %d" % result)
        self.log.append(" ".join(["t%d.%s" % (self.slot, name)] + shown))
        return result
    return method


class RecordingTracer(OracleTracer):
    def __init__(self, log, index, *args):
        super().__init__(*args)
        self.log, self.slot = log, index

    @staticmethod
    def trace_group(tracers, mics, sources, nreflections, air, ray_offsets=None):
        tracers[0].log.append("trace_group %s nreflections=%d ray_offsets=%s" % (",".join("t%d" % t.slot for t in tracers), nreflections,
                                                                                 ",".join("%d" % o for o in ray_offsets or ())))
        OracleTracer.trace_group(tracers, mics, sources, nreflections, air, ray_offsets)


for _name, _keep in LOGGED.items():
    setattr(RecordingTracer, _name, _logged(_name, _keep))


class Recorder:
    """One scenario's log, its tracers, and the callbacks that write to the log besides them."""

    def __init__(self, oracle, scene, directions, ntracers=1):
        self.log = []
        self.tracers = [RecordingTracer(self.log, k, oracle, scene, directions) for k in range(ntracers)]

    def on_stage(self, name, tracer):
        self.log.append("stage %s t%d" % (name, tracer.slot))

    def host_out(self, shape):
        import torch
        self.log.append("host_out")
        return torch.empty(shape, dtype=torch.float32)

    def on_result(self, hist, info, tracer):
        self.log.append("result t%d" % tracer.slot)

    @contextlib.contextmanager
    def collectives(self):
        """torch.distributed's collectives log themselves (the peer only) while this is open."""
        import torch.distributed as dist
        saved = {name: getattr(dist, name) for name in COLLECTIVES}

        def logged(name, peer):
            signature = inspect.signature(saved[name])

            def call(*args, **kwargs):
                self.log.append("dist.%s" % name + (" %s=%d" % (peer, signature.bind(*args, **kwargs).arguments[peer]) if peer else ""))
                return saved[name](*args, **kwargs)
            return call
        try:
            for name, peer in COLLECTIVES.items():
                setattr(dist, name, logged(name, peer))
            yield
        finally:
            for name, call in saved.items():
                setattr(dist, name, call)


@contextlib.contextmanager
def _environment(**switches):
    saved = {k: os.environ.get(k) for k in switches}
    os.environ.update(switches)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _hrtf_model():
    return distributed.HrtfModel(scenes.hrtf_synthetic_table(), (1.0, 0.0, 0.2), (0.0, 1.0, 0.0))


def _ir_scenarios(oracle, rank, world):
    """generate_ir on this rank's shard of the cathedral's rays: {scenario: log}."""
    scene, where = scenes.cathedral(1200)
    first, count = distributed.shard_range(RAYS, rank, world)
    directions = scenes.sphere_directions(count, seed=9, first=first)
    logs = {}

    def run(name, host=True, begin=False, defer=False, **kwargs):
        rec = Recorder(oracle, scene, directions)
        args = dict(SPEAKERS, sample_rate=44100.0, trim_predelay=True, mode=capi.IR_EXACT, rank=rank, world=world, ray_offset=first,
                    device="cpu", on_stage=rec.on_stage, host_out=rec.host_out if host else None, defer=defer, begun=begin)
        args.update(kwargs)
        with rec.collectives():
            if begin:
                distributed.begin_ir(rec.tracers[0], where["mic"], where["source"], NREFL, dtypes.AIR_COEFFICIENTS, first)
                rec.log.append("begun")
            got = distributed.generate_ir(rec.tracers[0], where["mic"], where["source"], NREFL, dtypes.AIR_COEFFICIENTS, **args)
            if defer:
                rec.log.append("deferred")
                got[2]()
        assert ("host" in got[1]) == host
        logs[name] = rec.log

    if world == 1:
        for which_name, which in (("all", capi.IR_ALL), ("diffuse", capi.IR_DIFFUSE), ("images", capi.IR_IMAGES)):
            for host in (False, True):
                run("exact_%s%s" % (which_name, "_host" if host else ""), host, which=which)
        run("fast", False, mode=capi.IR_FAST)
        run("fast_host", mode=capi.IR_FAST)
        run("defer", defer=True)
        run("defer_no_host", False, defer=True)
        run("begun", begin=True)
        run("rehearsed_collectives_host", collectives=True)              # (the caller has made a one-rank process group)
        run("rehearsed_collectives_host_images", collectives=True, which=capi.IR_IMAGES)
    else:
        run("all_reduce_host")
        run("all_reduce_images", which=capi.IR_IMAGES)                  # the rank that does not add the images contributes nothing
        run("all_reduce_defer", False, defer=True)
        run("chain_hrtf_3_blocks", chain_exact=True, chain_blocks=3, model=_hrtf_model())
        run("chain_images_only", chain_exact=True, which=capi.IR_IMAGES)
        run("chain_asked_for_in_fast_mode", chain_exact=True, mode=capi.IR_FAST)     # (no chain: the all-reduce)
        saved, distributed.EXCHANGE_CAPACITY = distributed.EXCHANGE_CAPACITY, 0     # forces the second exchange round
        try:
            run("exchange_overflow")
        finally:
            distributed.EXCHANGE_CAPACITY = saved
    return logs


def _pipeline_scenarios(oracle):
    """IrPipeline with 1, 2 and 4 tracers under each RVB_PIPELINE_* switch: run(5) then run(2) on the same pipeline."""
    scene, where = scenes.cathedral(1200)
    directions = scenes.sphere_directions(RAYS, seed=9)
    trace_args = (where["mic"], where["source"], NREFL, dtypes.AIR_COEFFICIENTS)
    logs = {}

    def kwargs(rec):
        return dict(SPEAKERS, sample_rate=44100.0, trim_predelay=True, mode=capi.IR_EXACT, device="cpu", host_out=rec.host_out)

    for ntracers in (1, 2, 4):
        for switch in ({}, {"RVB_PIPELINE_AHEAD": "1"}, {"RVB_PIPELINE_FUSE": "0"}, {"RVB_PIPELINE_GROUP": "1"}):
            rec = Recorder(oracle, scene, directions, ntracers)
            with _environment(**switch):
                pipe = distributed.IrPipeline(rec.tracers)
                pipe.run(5, trace_args, kwargs(rec), rec.on_result)
                rec.log.append("second run")
                pipe.run(2, trace_args, kwargs(rec), rec.on_result)
            logs["%d_tracers%s" % (ntracers, "".join("_%s=%s" % kv for kv in switch.items()))] = rec.log
    # two jobs of a group differ in reflection count: the group falls back to separate traces
    rec = Recorder(oracle, scene, directions, 4)
    jobs = [((where["mic"], where["source"], 6 if k == 1 else NREFL, dtypes.AIR_COEFFICIENTS), kwargs(rec)) for k in range(4)]
    distributed.IrPipeline(rec.tracers).run_jobs(jobs, rec.on_result)
    logs["4_tracers_mixed_reflection_counts"] = rec.log
    return logs


def _pair_scenarios(oracle, rank, world, cases):
    """generate_pair_irs over five pairs of the concert hall: cases = [(pairs_per_launch, ntracers)]."""
    scene, _ = scenes.concert_hall(900)
    src, mic = scenes.source_mic_pairs(PAIRS, seed=2)
    table = scenes.hrtf_synthetic_table()
    directions = scenes.sphere_directions(PAIR_RAYS, seed=4)

    def model(i):
        facing = src[i] - mic[i]
        return distributed.HrtfModel(table, facing / np.linalg.norm(facing), (0, 1, 0))

    logs = {}
    for per_launch, ntracers in cases:
        rec = Recorder(oracle, scene, directions, ntracers)
        with rec.collectives():
            got = distributed.generate_pair_irs(rec.tracers, [(mic[i], src[i]) for i in range(PAIRS)], PAIR_NREFL, dtypes.AIR_COEFFICIENTS, model,
                                                44100.0, rank=rank, world=world, mode=capi.IR_EXACT, pairs_per_launch=per_launch)
        rec.log.append("pairs %s" % ",".join("%d" % i for i in got))
        logs["%d_per_launch_%d_tracers" % (per_launch, ntracers)] = rec.log
    return logs


def _world2_worker(rank, port, out_dir):
    import pyoracle
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=2)
    oracle = pyoracle.Oracle("port")
    logs = {"generate_ir": _ir_scenarios(oracle, rank, 2), "generate_pair_irs": _pair_scenarios(oracle, rank, 2, [(2, 2)])}
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(logs, f)
    dist.barrier()
    dist.destroy_process_group()


def record(oracle, tmp_dir):
    """Every scenario's log: {"world1" | "world2_rank0" | "world2_rank1": {family: {scenario: log}}}."""
    import torch.distributed as dist
    import torch.multiprocessing as mp
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0, world_size=1)   # for collectives=True on one rank
    try:
        world1 = {"generate_ir": _ir_scenarios(oracle, 0, 1)}
    finally:
        dist.destroy_process_group()
    world1["IrPipeline"] = _pipeline_scenarios(oracle)
    world1["generate_pair_irs"] = _pair_scenarios(oracle, 0, 1, [(1, 1), (1, 2), (2, 1), (2, 2)])
    mp.spawn(_world2_worker, args=(_free_port(), str(tmp_dir)), nprocs=2, join=True)         # ONE spawn for all two-rank scenarios
    logs = {"world1": world1}
    for rank in (0, 1):
        with open(os.path.join(str(tmp_dir), "rank%d.json" % rank)) as f:
            logs["world2_rank%d" % rank] = json.load(f)
    return logs


def test_call_order_and_collectives_equal_the_recorded_contract(tmp_path, oracle):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = record(oracle, tmp_path)
    flat = lambda logs: {(w, f, s): logs[w][f][s] for w in logs for f in logs[w] for s in logs[w][f]}      # noqa: E731
    got, want = flat(got), flat(want)
    assert sorted(got) == sorted(want)
    for scenario in sorted(want):
        for k, (a, b) in enumerate(zip(got[scenario], want[scenario])):
            assert a == b, "%s, entry %d: %r, recorded %r" % ("/".join(scenario), k, a, b)
        assert len(got[scenario]) == len(want[scenario]), "/".join(scenario)


if __name__ == "__main__":
    import tempfile
    assert sys.argv[1:] == ["--write"], __doc__
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_build/librvb_oracle.so"])
    import pyoracle
    with tempfile.TemporaryDirectory() as tmp:
        logs = record(pyoracle.Oracle("port"), tmp)
    with open(FIXTURE, "w") as f:
        json.dump(logs, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%s: %d entries" % (FIXTURE, sum(len(logs[w][f][s]) for w in logs for f in logs[w] for s in logs[w][f])))
