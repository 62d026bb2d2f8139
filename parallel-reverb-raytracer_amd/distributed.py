"""Multi-GPU impulse-response generation: one process per GPU, `torch.distributed` (backend "nccl" = RCCL over xGMI on ROCm; "gloo" in
the CPU tests).

The path shards by rays: the scene is replicated, rank r traces the contiguous ray range [r*n, (r+1)*n) of one seeded
global ray set, and the only data-path collective is ONE all-reduce(sum) of the [channels][8][nbins] histograms.  ONE small control
collective makes the shards agree on the binning: an all-gather of a few-KB block per rank holding the shard's diffuse time range — the
inputs of findPredelay (reference rayverb.h:49-74) and MAX_SAMPLE (rayverb.cpp:57) — and its few valid image-source candidates.  Every
rank merges the candidates itself with the reference's "lowest ray index wins" rule (rayverb.cpp:654-676), so all ranks know the global
time range without a second exchange; rank 0 alone adds the merged image impulses to its histogram.

`tracer` is a capi.Context (GPU) or any object with the same methods (the CPU tests drive this module
with an oracle-backed stand-in, tests/oracle_tracer.py).  The TRACER PROTOCOL, as capi.Context defines it:
  tracing: trace, trace_group (static), trace_pairs, select_pair, set_concurrent_traces, `nrays`;
  small results on the host: get_image_candidates, get_pair_candidates, get_direct;
  binning: ir_configure_speakers, ir_configure_hrtf, ir_time_range, ir_bins, ir_accumulate_tensor,
  ir_accumulate_export_tensor, ir_exact_prepare, ir_exact_fold_tensor;
  order and the way to the host: synchronize, ir_accumulate_wait_for_torch, export_tensor_to_host, and
  synchronize_exports for the caller who reads info["host"].
This module's contract, per rank, is the ORDER of these calls and of the collectives
(tests/test_distributed_call_order.py holds it against a recorded log).
"""
import os
import types

import numpy as np

from . import capi
from .dtypes import IMPULSE

_EMPTY = np.zeros(0, dtype=IMPULSE)


def shard_range(total_rays, rank, world):
    """Contiguous ray range of `rank`; ranges differ by at most one ray."""
    base, extra = divmod(int(total_rays), int(world))
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


EXCHANGE_CAPACITY = 64          # image-source candidates per rank carried by the first (normally only) exchange
_HEADER_BYTES = 16              # u64 candidate count, f32 min non-zero time, f32 max time


def _pack_block(candidates, lo, hi, capacity):
    block = np.zeros(_HEADER_BYTES + capacity * capi.IMAGE_CANDIDATE.itemsize, dtype=np.uint8)
    block[:8] = np.frombuffer(np.uint64(candidates.shape[0]).tobytes(), dtype=np.uint8)
    block[8:16] = np.frombuffer(np.array([lo, hi], dtype=np.float32).tobytes(), dtype=np.uint8)
    n = min(int(candidates.shape[0]), capacity)
    if n:
        block[_HEADER_BYTES:_HEADER_BYTES + n * capi.IMAGE_CANDIDATE.itemsize] = \
            np.frombuffer(np.ascontiguousarray(candidates[:n]).tobytes(), dtype=np.uint8)
    return block


def _unpack_block(block, capacity):
    count = int(np.frombuffer(block[:8].tobytes(), dtype=np.uint64)[0])
    lo, hi = (float(x) for x in np.frombuffer(block[8:16].tobytes(), dtype=np.float32))
    n = min(count, capacity)
    cand = np.frombuffer(block[_HEADER_BYTES:_HEADER_BYTES + n * capi.IMAGE_CANDIDATE.itemsize].tobytes(),
                         dtype=capi.IMAGE_CANDIDATE).copy()
    return count, lo, hi, cand


def exchange_shard_summaries(candidates, lo, hi, world, device, capacity=None):
    """The ONE control collective of a multi-GPU impulse response: an all-gather of a small fixed-size
    block per rank = (number of valid image-source candidates, min non-zero / max diffuse time of the
    shard, the candidates themselves).  Returns (all candidates in rank order, [(lo, hi)] per rank).
    A shard with more than `capacity` candidates (rare: a few per 100k rays are typical) triggers one
    more all-gather sized for the largest shard; every rank sees the same counts, so all ranks agree
    on whether that second round happens."""
    import torch
    import torch.distributed as dist
    capacity = EXCHANGE_CAPACITY if capacity is None else capacity
    while True:
        mine = torch.from_numpy(_pack_block(candidates, lo, hi, capacity)).to(device)
        blocks = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(blocks, mine)
        parts = [_unpack_block(b.cpu().numpy(), capacity) for b in blocks]
        worst = max(p[0] for p in parts)
        if worst <= capacity:
            return np.concatenate([p[3] for p in parts]), [(p[1], p[2]) for p in parts]
        capacity = worst


def combine_time_ranges(ranges):
    """(min non-zero, max) over (lo, hi) pairs in which lo == 0 means "no non-zero time"."""
    los = [lo for lo, _ in ranges if lo > 0]
    return (min(los) if los else 0.0), max([hi for _, hi in ranges] + [0.0])


class SpeakerModel:
    """Microphone model of reference kernel `attenuate` (cardioid-family speakers, config.h AttenuationModel::SPEAKER)."""

    def __init__(self, directions, coefficients):
        self.directions, self.coefficients = directions, coefficients
        self.nchannels = len(coefficients)

    def configure(self, tracer, mic, which, images):
        tracer.ir_configure_speakers(mic, self.directions, self.coefficients, which, images)


class HrtfModel:
    """Listener model of reference kernel `hrtf` (AttenuationModel::HRTF): table [2][360][180][8], facing and up vectors."""

    def __init__(self, table, facing, up):
        self.table, self.facing, self.up = table, facing, up
        self.nchannels = 2

    def configure(self, tracer, mic, which, images):
        tracer.ir_configure_hrtf(mic, self.table, self.facing, self.up, which, images)


def _p2p_staged(t):
    """gloo carries point-to-point messages for CPU tensors only: a CUDA block goes through host memory there (RCCL takes it as it is)."""
    import torch.distributed as dist
    return t.is_cuda and dist.get_backend() == "gloo"


def _send_block(view, dst):
    import torch.distributed as dist
    block = view.contiguous()
    dist.send(block.cpu() if _p2p_staged(block) else block, dst=dst)


def _recv_block(view, src):
    import torch
    import torch.distributed as dist
    staged = _p2p_staged(view)
    block = torch.empty(view.shape, dtype=view.dtype, device="cpu" if staged else view.device)
    dist.recv(block, src=src)
    return block.to(view.device) if staged else block


def begin_ir(tracer, mic, source, nreflections, air, ray_offset=0):
    """First half of generate_ir: enqueues the trace of the rays already set on `tracer` (asynchronous on a GPU context)."""
    tracer.trace(mic, source, nreflections, air, ray_offset=ray_offset)


class _Ir:
    """One rank's part in one impulse response: the plain record that the phases _plan -> _enqueue -> _finish hand on."""

    def __init__(self, tracer, model, mic, which, mode, sample_rate, device, rank=0, world=1, chain_blocks=8, on_stage=None):
        self.tracer, self.model, self.mic, self.mode, self.sample_rate, self.device = tracer, model, mic, mode, sample_rate, device
        self.which, self.rank, self.world = which, rank, world       # (`which`: the caller's selection for the WHOLE impulse response)
        self.chain_blocks, self.on_stage = chain_blocks, on_stage
        self.reduce = None                               # fixed by _plan from here on: _reduce_none | _reduce_sum | _reduce_chain
        self.bins_now = True                             # _enqueue bins what _plan configured (a chain folds in _finish; a rank may have nothing to add)
        self.images = _EMPTY                             # merged image impulses that this rank adds (all-reduce: rank 0) or, in a chain, the last rank will
        self.predelay, self.max_time, self.nbins = 0.0, 0.0, 0
        self.hist, self.host, self.export_behind_reduce = None, None, False      # fixed by _enqueue (the last: _finish sends hist to host)

    def stage(self, name):
        if self.on_stage:
            self.on_stage(name, self.tracer)


def _plan(p, candidates, direct, remove_direct, trim_predelay, collectives=False, chain_exact=False):
    """Phase 1, host work on the trace's small results: merges the image sources, fixes predelay and nbins, and decides ONCE which reduce
    path applies and what this rank bins.  candidates() / direct() -> this trace's image-source candidates / direct impulse; a rank on
    its own asks for them only when images are wanted.  Leaves the tracer configured for what _enqueue bins."""
    tracer, model, want_images = p.tracer, p.model, bool(p.which & capi.IR_IMAGES)
    if not collectives:                                      # no other rank: everything asked for, images from this trace's candidates
        p.reduce = _reduce_none
        p.images = capi.merge_images(candidates(), direct(), remove_direct) if want_images else _EMPTY
        model.configure(tracer, p.mic, p.which, p.images)
        lo, hi = tracer.ir_time_range()
        p.stage("time_range")
    else:
        lo = hi = 0.0
        if p.which & capi.IR_DIFFUSE:                        # this shard's diffuse impulses alone
            model.configure(tracer, p.mic, capi.IR_DIFFUSE, _EMPTY)
            lo, hi = tracer.ir_time_range()
            p.stage("time_range")
        everyones, ranges = exchange_shard_summaries(candidates(), lo, hi, p.world, p.device)
        p.images = capi.merge_images(everyones, direct(), remove_direct) if want_images else _EMPTY
        if p.images.shape[0]:                                # the merged images' own range, the same on every rank
            model.configure(tracer, p.mic, capi.IR_IMAGES, p.images)
            ranges.append(tracer.ir_time_range())
        lo, hi = combine_time_ranges(ranges)
        if chain_exact and p.mode == capi.IR_EXACT and p.world > 1:
            p.reduce, p.bins_now = _reduce_chain, False      # (its last rank adds the merged images, after the folds)
        else:
            p.reduce = _reduce_sum                           # rank 0 adds the merged images to its own sum
            mine = p.which if p.rank == 0 else p.which & capi.IR_DIFFUSE
            p.bins_now = mine != 0
            p.images = p.images if p.rank == 0 else _EMPTY
            if p.bins_now:
                model.configure(tracer, p.mic, mine, p.images)
    p.predelay, p.max_time = (lo if trim_predelay else 0.0), hi
    p.nbins = tracer.ir_bins(hi, p.predelay, p.sample_rate)


def _enqueue(p, host_out=None):
    """Phase 2: the zeroed histogram, the caller's host tensor, the binning (asynchronous on a GPU context: the tracer's stream waits for
    torch's zero fill by an event).  Returns generate_ir's (hist, info).  HOW THE HISTOGRAM REACHES THE HOST is decided here and nowhere else:
      - no reduction: FUSED with the binning, one call (rvb_ir_accumulate_export: in exact mode the bin ranges leave as they become final);
      - a reduction: BEHIND THE COLLECTIVE, in _finish — the collective runs on torch's stream, so the tracer's stream first waits for it by
        an event (ir_accumulate_wait_for_torch), then export_tensor_to_host on the tracer's export stream.
    (A copy in stream order behind a separate binning call has no user: without a reduction a rank always bins, and the fused call does both.)"""
    import torch
    p.hist = torch.zeros((p.model.nchannels, 8, p.nbins), device=p.device, dtype=torch.float32)
    info = {"nbins": p.nbins, "predelay": p.predelay, "images": int(p.images.shape[0]), "max_time": p.max_time}
    if host_out is not None:
        p.host = info["host"] = host_out(tuple(p.hist.shape))
        p.export_behind_reduce = p.reduce is not _reduce_none
    if p.host is not None and not p.export_behind_reduce:
        p.tracer.ir_accumulate_export_tensor(p.predelay, p.sample_rate, p.nbins, p.mode, p.hist, p.host)
    elif p.bins_now:
        p.tracer.ir_accumulate_tensor(p.predelay, p.sample_rate, p.nbins, p.mode, p.hist)
    return p.hist, info


def _finish(p):
    """Phase 3: waits for the binning, reduces over the ranks, sends the reduced histogram to the host."""
    p.stage("accumulate")
    p.reduce(p)
    if p.export_behind_reduce:
        p.tracer.ir_accumulate_wait_for_torch()
        p.tracer.export_tensor_to_host(p.hist, p.host)


def _reduce_none(p):
    p.tracer.synchronize()


def _reduce_sum(p):
    """All-reduce of the ranks' own sums: the single-GPU histogram up to float re-association."""
    import torch.distributed as dist
    p.tracer.synchronize()
    dist.all_reduce(p.hist, op=dist.ReduceOp.SUM)            # RCCL over xGMI: [channels][8][nbins] floats


def _reduce_chain(p):
    """One serial sum over all ranks, in ray order (generate_ir's docstring) — SYSTOLIC: the histogram travels in bin-range blocks, rank r
    folds block k while rank r + 1 folds block k - 1; a rank keys and sorts its impulses (ir_exact_prepare) before the first block arrives."""
    import torch.distributed as dist
    tracer, hist, nbins, last = p.tracer, p.hist, p.nbins, p.world - 1
    blocks = max(1, min(int(p.chain_blocks), (nbins + 15) // 16))
    per = ((nbins + blocks - 1) // blocks + 15) & ~15
    folds = bool(p.which & capi.IR_DIFFUSE)
    if folds:
        p.model.configure(tracer, p.mic, capi.IR_DIFFUSE, _EMPTY)
        tracer.ir_exact_prepare(p.predelay, p.sample_rate, nbins)
    for b0 in range(0, nbins, per):
        b1 = min(nbins, b0 + per)
        if p.rank > 0:
            hist[:, :, b0:b1] = _recv_block(hist[:, :, b0:b1], p.rank - 1)
        if folds:
            tracer.ir_exact_fold_tensor(nbins, b0, b1, hist)
            tracer.synchronize()
        if p.rank < last:
            _send_block(hist[:, :, b0:b1], p.rank + 1)
    if p.rank == last and (p.which & capi.IR_IMAGES) and p.images.shape[0]:
        p.model.configure(tracer, p.mic, capi.IR_IMAGES, p.images)
        tracer.ir_accumulate_tensor(p.predelay, p.sample_rate, nbins, p.mode, hist)
        tracer.synchronize()
    dist.broadcast(hist, src=last)


def generate_ir(tracer, mic, source, nreflections, air, speakers_dir=None, speakers_coeff=None, sample_rate=44100.0,
                trim_predelay=True, mode=capi.IR_FAST, rank=0, world=1, ray_offset=0, device="cpu",
                which=capi.IR_ALL, remove_direct=False, on_stage=None, begun=False, model=None, collectives=None, defer=False,
                host_out=None, chain_exact=False, chain_blocks=8):
    """One impulse response from the rays already set on `tracer`.  Returns (hist tensor [nchannels][8][nbins] — identical on every
    rank —, info dict).  A short driver over three phases: _plan (host), _enqueue (binning), _finish (wait, reduce, export).

    world == 1: trace -> merge image sources -> time range -> bin.
    world > 1: two collectives in all.  (1) exchange_shard_summaries: every rank learns every shard's image-source candidates and
    diffuse time range, merges the candidates itself (deterministic, a few dozen records) and so knows the global predelay / length
    without a further exchange; (2) the all-reduce(sum) of the histograms.  Only rank 0 adds the merged image impulses to its histogram.

    begun=True: begin_ir(tracer, ...) has already enqueued this IR's trace.  A caller with two contexts per GPU calls begin_ir on the
    second before generate_ir(..., begun=True) on the first, so that one IR's trace (VALU-bound) runs beside the other's record
    grouping, binning, host work and collectives (IrPipeline below).

    chain_exact=True (several ranks, exact mode): instead of all-reducing the ranks' serial sums — which is the single-GPU histogram
    only up to float re-association — the ranks continue ONE serial sum in ray order: rank r receives the histogram from rank r-1,
    folds its own diffuse impulses on top (rvb_ir_accumulate in exact mode adds to what the histogram holds), hands it to rank r+1;
    the last rank adds the merged image sources (the reference's order: diffuse, then images — rayverb.cpp:708-714) and broadcasts.
    Bit-identical to one GPU and to flattenImpulses.  The traces, and every rank's keying and sorting, run side by side; only the
    fold is a chain, and the histogram travels through it in `chain_blocks` bin-range blocks (rank r folds block k while rank r + 1
    folds block k - 1: (world + blocks - 1) / blocks folds and hops instead of world).

    host_out(shape) -> pinned host tensor: the finished histogram is also copied there (info["host"]) — enqueued behind the binning
    (behind the all-reduce with collectives) on the tracer's export stream, so neither the host nor the tracer's next trace waits for
    the link; info["host"] is complete after tracer.synchronize_exports() (or a device-wide synchronisation), and the caller keeps
    `hist` alive until then.

    defer=True: returns (hist, info, finish) as soon as the binning is ENQUEUED; finish() waits for it (and runs the all-reduce).
    A caller that finishes several IRs enqueues all their binning stages first, so that they run side by side instead of each
    waiting for the one before (IrPipeline: the stages of a group)."""
    if collectives is None:                              # True with world == 1 rehearses the multi-rank code path on one rank
        collectives = world > 1
    if model is None:                                    # the two-list form: speakers (what bench.py and the reference demo configs use)
        model = SpeakerModel(speakers_dir, speakers_coeff)
    if not begun:
        begin_ir(tracer, mic, source, nreflections, air, ray_offset)
    p = _Ir(tracer, model, mic, which, mode, sample_rate, device, rank, world, chain_blocks, on_stage)
    candidates = tracer.get_image_candidates()           # small: valid image-source paths only
    p.stage("trace")
    direct = tracer.get_direct()                         # (a host wait on a GPU context: here, whether or not images are wanted)
    _plan(p, lambda: candidates, lambda: direct, remove_direct, trim_predelay, collectives, chain_exact)
    hist, info = _enqueue(p, host_out)
    if defer:
        return hist, info, lambda: _finish(p)
    _finish(p)
    return hist, info


class IrPipeline:
    """Impulse responses back to back with TWO contexts per GPU: the trace of IR i+1 is enqueued on the other context before IR i is
    finished, so its VALU-bound path kernel runs beside IR i's bandwidth-, atomic- and host-bound stages (record grouping, binning,
    candidate merge, collectives).  Single host thread, collectives in program order: safe with any world size.  Measured on one
    MI355X at workload C2: 6.45 -> 5.6 ms per IR."""

    def __init__(self, tracers):
        assert len(tracers) >= 1
        self.tracers = list(tracers)
        self.next_slot, self.begun = 0, [False] * len(self.tracers)
        self.fuse_groups = os.environ.get("RVB_PIPELINE_FUSE", "1") != "0"       # one path-kernel launch per group
        # the traces of a group run side by side (run_jobs): tell the contexts, so that the path kernel is sized for the rays in flight
        for t in self.tracers:
            t.set_concurrent_traces(self.group_size(len(self.tracers)))

    @staticmethod
    def group_size(n):
        group = max(1, n // 2) if n > 1 else 1
        return min(group, int(os.environ.get("RVB_PIPELINE_GROUP", group)))       # (an override may only shrink it)

    def run(self, count, trace_args, ir_kwargs, on_result=None):
        """`count` IRs with the same arguments (bench) — trace_args = (mic, source, nreflections, air), ir_kwargs as
        generate_ir takes them.  on_result(hist, info, tracer) is called per IR in order."""
        self.run_jobs([(trace_args, ir_kwargs)] * count, on_result)

    def _begin(self, run, k):
        trace_args, ir_kwargs = run.jobs[k]
        begin_ir(self.tracers[run.slots[k]], *trace_args, ray_offset=ir_kwargs.get("ray_offset", 0))
        self.begun[run.slots[k]] = True

    def _begin_group(self, run, ks):
        """The traces of a group in ONE path-kernel launch (Context.trace_group) when the jobs agree in reflection count and air
        coefficients (and RVB_PIPELINE_FUSE allows it); one after the other otherwise."""
        args = [run.jobs[k][0] for k in ks]
        same = all(a[2] == args[0][2] and tuple(a[3]) == tuple(args[0][3]) for a in args)
        if len(ks) > 1 and same and self.fuse_groups:
            tracers = [self.tracers[run.slots[k]] for k in ks]
            tracers[0].trace_group(tracers, [a[0] for a in args], [a[1] for a in args], args[0][2], args[0][3],
                                   [run.jobs[k][1].get("ray_offset", 0) for k in ks])
            for k in ks:
                self.begun[run.slots[k]] = True
        else:
            for k in ks:
                self._begin(run, k)

    def _begin_upto(self, run, k):
        """Begins the traces of jobs [run.begun_upto, k): group by group in the default schedule, else one by one."""
        grouped = len(self.tracers) > 1 and run.ahead <= 0 and run.group > 1
        while run.begun_upto < min(k, len(run.jobs)):        # (group boundaries: begun_upto is a multiple of group here)
            ks = list(range(run.begun_upto, min(run.begun_upto + (run.group if grouped else 1), k, len(run.jobs))))
            self._begin_group(run, ks)
            run.begun_upto += len(ks)

    def _enqueue(self, run, i):
        """generate_ir of job i up to its enqueued binning: (hist, info, finish, tracer)."""
        slot = run.slots[i]
        trace_args, ir_kwargs = run.jobs[i]
        began, self.begun[slot] = self.begun[slot], False
        return generate_ir(self.tracers[slot], *trace_args, begun=began, defer=True, **ir_kwargs) + (self.tracers[slot],)

    def run_jobs(self, jobs, on_result=None):
        """One IR per job = (trace_args, ir_kwargs), e.g. the source / listener pairs of a hall (BASELINE config C5): every
        context must hold the same scene and rays.  Results arrive in job order.

        Default schedule: jobs are enqueued in GROUPS of `group` traces (their path kernels then run side by side: more waves per SIMD,
        see DESIGN.md "rays per launch"), and group j+1 is enqueued before group j is finished: the traces of the group after next are
        enqueued, then the binning stages of ALL IRs of this group (each needs its own trace's image-source candidates on the host
        first), and only then the host waits for them — the stages of a group run side by side, beside the next group's path kernels.
        group = len(tracers) // 2; two contexts: group 1 = the plain alternation.  RVB_PIPELINE_AHEAD=k (and a single context) instead
        finishes the IRs one by one and keeps k traces enqueued ahead of the one being finished (k < len(tracers))."""
        n = len(self.tracers)
        if not jobs:
            return
        run = types.SimpleNamespace(jobs=jobs, slots=[(self.next_slot + k) % n for k in range(len(jobs))], begun_upto=0,       # (jobs [0, begun_upto) are begun)
                                    group=self.group_size(n), ahead=min(n - 1, int(os.environ.get("RVB_PIPELINE_AHEAD", 0))))
        by_groups = n > 1 and run.ahead <= 0
        step = run.group if by_groups else 1                 # IRs whose binning stages are enqueued before the host waits for the first
        in_flight = max(2, n // run.group)                   # groups whose traces are enqueued at a time (each context holds one IR)
        self._begin_upto(run, run.group if run.ahead <= 0 else 1 + run.ahead)
        for g0 in range(0, len(jobs), step):
            self._begin_upto(run, (g0 // step + in_flight) * step if by_groups else g0 + 1 + max(0, run.ahead))
            pending = [self._enqueue(run, i) for i in range(g0, min(g0 + step, len(jobs)))]
            for hist, info, finish, tracer in pending:
                finish()
                if on_result:
                    on_result(hist, info, tracer)
        self.next_slot = (self.next_slot + len(jobs)) % n


def generate_pair_irs(tracers, pairs, nreflections, air, model_for_pair, sample_rate, rank=0, world=1, device="cpu",
                      trim_predelay=True, mode=capi.IR_FAST, which=capi.IR_ALL, remove_direct=False, pairs_per_launch=1):
    """BASELINE config C5: many (source, listener) pairs in one scene.  The PAIRS shard over the ranks (contiguous blocks, shard_range)
    and every rank traces its own pairs with all of its rays — no collective at all.  `pairs` = [(mic, source)],
    `model_for_pair(i)` -> SpeakerModel / HrtfModel of pair i; `tracers` = this rank's contexts (same scene and rays on each).
    Returns {pair index: (hist, info)} for this rank's pairs.

    pairs_per_launch == 1: the pairs are jobs of the two-context pipeline, one trace each.
    pairs_per_launch > 1: that many pairs are traced in ONE launch (Context.trace_pairs: the path kernel runs with more waves per
    SIMD), the next launch is enqueued on the other context before this launch's pairs are binned."""
    first, count = shard_range(len(pairs), rank, world)
    out = {}
    if pairs_per_launch <= 1:
        kwargs = dict(sample_rate=sample_rate, trim_predelay=trim_predelay, mode=mode, device=device, which=which,
                      remove_direct=remove_direct)                  # rank 0 / world 1 inside generate_ir: a pair is not sharded
        jobs = [((*pairs[i], nreflections, air), dict(kwargs, model=model_for_pair(i))) for i in range(first, first + count)]
        order = iter(range(first, first + count))
        IrPipeline(tracers).run_jobs(jobs, lambda hist, info, _tracer: out.__setitem__(next(order), (hist, info)))
        return out

    batches = [list(range(b, min(first + count, b + pairs_per_launch))) for b in range(first, first + count, pairs_per_launch)]
    n = len(tracers)

    def begin(j):
        tracers[j % n].trace_pairs([pairs[i][0] for i in batches[j]], [pairs[i][1] for i in batches[j]], nreflections, air)

    if batches:
        begin(0)
    for j, batch in enumerate(batches):
        if j + 1 < len(batches) and n > 1:
            begin(j + 1)
        tracer = tracers[j % n]
        candidates = tracer.get_image_candidates()           # all pairs of the launch, global ray numbers
        for k, i in enumerate(batch):                        # generate_ir's single-rank staging, pair by pair; ONE wait for the launch
            tracer.select_pair(k)
            p = _Ir(tracer, model_for_pair(i), pairs[i][0], which, mode, sample_rate, device)
            _plan(p, lambda: tracer.get_pair_candidates(k, candidates), tracer.get_direct, remove_direct, trim_predelay)
            out[i] = _enqueue(p)
        tracer.synchronize()
        if n == 1 and j + 1 < len(batches):
            begin(j + 1)                                     # (only now: the next launch reuses this context's buffers)
    return out

