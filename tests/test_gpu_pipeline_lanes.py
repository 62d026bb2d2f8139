"""The pipeline over lanes and with several pairs per path-kernel launch (rvb_pipeline_create_lanes, csrc/pipeline.hip) through its ctypes
binding, against distributed.generate_ir on a solo context: lane layouts with one and several pairs per launch (incomplete last units
included), the HRTF model with a facing per job, float atomics, reconfiguration between batches, results taken late, the pending limit,
the refusals, a failing lane — and C5's per-GPU share at full size (8 HRTF pairs of the 30 000-triangle hall at 100 000 rays x 128)."""
import ctypes

import numpy as np
import pytest

from parallel_reverb_raytracer_amd import dtypes, scenes

pytestmark = pytest.mark.gpu

SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])
NREFL = 24
UP = (0.0, 1.0, 0.0)


@pytest.fixture(scope="module")
def rig():
    from parallel_reverb_raytracer_amd import capi
    scene, _ = scenes.concert_hall(6000)
    dirs = scenes.sphere_directions(9000, seed=31)
    ctxs = [capi.Context(0) for _ in range(5)]
    for k, c in enumerate(ctxs):
        if k in (1, 2, 3):
            c.share_scene(ctxs[0])          # the lane contexts read ONE copy of the scene; the solo context has its own
        else:
            c.set_scene(scene)
        c.set_directions(dirs)
    src, mic = scenes.source_mic_pairs(16, seed=5)
    pairs = [(tuple(float(x) for x in m), tuple(float(x) for x in s)) for s, m in zip(src, mic)]      # (microphone, source)
    yield ctxs[:4], ctxs[4], pairs, {}
    for c in ctxs:
        c.close()


def _solo(rig, k, mode=None, which=None, trim=True, hrtf=None, remove_direct=False):
    """Job k's impulse response generated alone on the solo context (cached per rig)."""
    import torch
    from parallel_reverb_raytracer_amd import capi, distributed
    _, solo, pairs, cache = rig
    mode = capi.IR_EXACT if mode is None else mode
    which = capi.IR_ALL if which is None else which
    key = (k, mode, which, trim, hrtf is not None, remove_direct)
    if key not in cache:
        mic, src = pairs[k]
        model = distributed.HrtfModel(hrtf, _facing(mic, src), UP) if hrtf is not None else None
        hist, info = distributed.generate_ir(solo, mic, src, NREFL, dtypes.AIR_COEFFICIENTS, SPEAKERS[0], SPEAKERS[1], 44100.0, trim_predelay=trim,
                                             mode=mode, which=which, remove_direct=remove_direct, device=torch.device("cuda", 0), model=model)
        solo.synchronize()
        cache[key] = (hist.cpu().numpy(), info)
    return cache[key]


def _facing(mic, src):
    d = np.array(src, np.float64) - np.array(mic, np.float64)
    d[1] = 0.0
    return tuple(float(x) for x in d / np.linalg.norm(d))


def _lanes(ctxs, sizes):
    out, first = [], 0
    for s in sizes:
        out.append(ctxs[first:first + s])
        first += s
    return out


def _run(pipe, jobs, submit):
    """Submits jobs as the pending limit allows, takes every result in order: [(histogram copy, info)]."""
    got, sent = [], 0
    while len(got) < len(jobs):
        while sent < len(jobs) and pipe.pending() < pipe.limit:
            submit(jobs[sent])
            sent += 1
        got.append(pipe.next())
    assert pipe.pending() == 0
    return got


def _check_exact(got, info, k, want, winfo):
    assert info["job"] == k and info["nbins"] == winfo["nbins"] and info["images"] == winfo["images"]
    assert np.float32(info["predelay"]) == np.float32(winfo["predelay"])
    assert got.shape == want.shape and np.array_equal(got, want) and got.any(), "job %d differs from the solo impulse response" % k


@pytest.mark.parametrize("sizes,ppl,njobs", [([2, 2], 1, 9), ([2, 2], 4, 16), ([2, 2], 3, 10), ([1, 1, 1, 1], 2, 7), ([4], 4, 9), ([1], 1, 3),
                                             ([4], 1, 9)])     # (the last: a lane that traces groups of two contexts per launch)
def test_lane_layouts_equal_one_context_bit_for_bit(rig, sizes, ppl, njobs):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, pairs, _ = rig
    pipe = capi.Pipeline(None, lanes=_lanes(ctxs, sizes), pairs_per_launch=ppl)
    try:
        pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        got = _run(pipe, list(range(njobs)), lambda k: pipe.submit(*pairs[k]))
        for k, (hist, info) in enumerate(got):
            want, winfo = _solo(rig, k)
            _check_exact(hist, info, k, want, winfo)
        with pytest.raises(capi.RvbError):
            pipe.next()
    finally:
        pipe.close()


def test_hrtf_with_a_facing_per_job_equals_one_context_bit_for_bit(rig):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, pairs, _ = rig
    table = scenes.hrtf_synthetic_table()
    pipe = capi.Pipeline(None, lanes=_lanes(ctxs, [2, 2]), pairs_per_launch=4)
    try:
        pipe.configure_hrtf(table, (0.0, 0.0, 1.0), UP, NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        got = _run(pipe, list(range(12)), lambda k: pipe.submit(pairs[k][0], pairs[k][1], _facing(*pairs[k]), UP))
        for k, (hist, info) in enumerate(got):
            want, winfo = _solo(rig, k, hrtf=table)
            _check_exact(hist, info, k, want, winfo)
    finally:
        pipe.close()


def test_fast_mode_diffuse_only_within_float_atomic_tolerance(rig):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, pairs, _ = rig
    pipe = capi.Pipeline(None, lanes=_lanes(ctxs, [2, 2]), pairs_per_launch=4)
    try:
        pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_FAST, which=capi.IR_DIFFUSE)
        got = _run(pipe, list(range(8)), lambda k: pipe.submit(*pairs[k]))
        for k, (hist, info) in enumerate(got):
            want, winfo = _solo(rig, k, which=capi.IR_DIFFUSE)
            band_max = np.abs(want).max(axis=2, keepdims=True)
            assert info["job"] == k and info["images"] == 0 and info["nbins"] == winfo["nbins"]
            assert hist.shape == want.shape and hist.any()
            assert (np.abs(hist.astype(np.float64) - want) <= 1e-5 * band_max).all(), "job %d" % k
    finally:
        pipe.close()


def test_reconfigured_between_batches_and_results_taken_late(rig):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, pairs, _ = rig
    table = scenes.hrtf_synthetic_table()
    pipe = capi.Pipeline(None, lanes=_lanes(ctxs, [2, 2]), pairs_per_launch=2)
    try:
        # image sources only, the direct path removed, no predelay trimming
        pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, False, capi.IR_EXACT, which=capi.IR_IMAGES, remove_direct=True)
        got = _run(pipe, list(range(5)), lambda k: pipe.submit(*pairs[k]))
        for k, (hist, info) in enumerate(got):
            want, winfo = _solo(rig, k, which=capi.IR_IMAGES, trim=False, remove_direct=True)
            assert info["predelay"] == 0.0 and info["images"] == winfo["images"] and np.array_equal(hist, want)
        # HRTF, every job facing its source
        pipe.configure_hrtf(table, (0.0, 0.0, 1.0), UP, NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        got = _run(pipe, list(range(3, 9)), lambda k: pipe.submit(pairs[k][0], pairs[k][1], _facing(*pairs[k]), UP))
        for k, (hist, info) in zip(range(3, 9), got):
            want, winfo = _solo(rig, k, hrtf=table)
            assert info["nbins"] == winfo["nbins"] and np.array_equal(hist, want)
        # speakers again after HRTF, taken late: fill to the pending limit, then take all; every view keeps its values while `valid_for`
        # further results are taken
        pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        assert pipe.limit == 16 and pipe.valid_for == 8
        jobs = [k % len(pairs) for k in range(pipe.limit)]
        for k in jobs:
            pipe.submit(*pairs[k])
        assert pipe.pending() == pipe.limit
        views, copies = [], []
        for t, k in enumerate(jobs):
            view, info = pipe.next(copy=False)
            want, winfo = _solo(rig, k)
            assert info["job"] == 11 + t and info["nbins"] == winfo["nbins"] and np.array_equal(np.asarray(view), want)
            views.append(view)
            copies.append(np.array(view))
            for i in range(max(0, t - pipe.valid_for), t + 1):
                assert np.array_equal(np.asarray(views[i]), copies[i]), "result %d overwritten after %d further results" % (i, t - i)
    finally:
        pipe.close()


def test_submit_past_the_pending_limit_is_refused_and_the_pipeline_goes_on(rig):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, pairs, _ = rig
    pipe = capi.Pipeline(None, lanes=_lanes(ctxs, [2, 2]), pairs_per_launch=2)
    try:
        pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        for t in range(pipe.limit):
            pipe.submit(*pairs[t % len(pairs)])
        with pytest.raises(capi.RvbError) as e:
            pipe.submit(*pairs[0])
        assert e.value.code == 5
        for t in range(pipe.limit):
            hist, info = pipe.next()
            want, _ = _solo(rig, t % len(pairs))
            assert info["job"] == t and np.array_equal(hist, want)
        for k in (5, 6, 7):                     # and afterwards
            pipe.submit(*pairs[k])
        for t, k in enumerate((5, 6, 7)):
            hist, info = pipe.next()
            assert info["job"] == pipe.limit + t and np.array_equal(hist, _solo(rig, k)[0])
    finally:
        pipe.close()


def test_refusals(rig):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, _, _ = rig
    for kwargs in (dict(lanes=[ctxs[:2], ctxs[1:3]]),                      # a context in two lanes
                   dict(lanes=[ctxs[:2], ctxs[2:4]], pairs_per_launch=0),
                   dict(lanes=[ctxs[:2], ctxs[2:4]], pairs_per_launch=capi.PIPELINE_MAX_PAIRS + 1),
                   dict(lanes=[ctxs[:2], ctxs[2:4]], pairs_per_launch=2, group=2)):
        with pytest.raises(capi.RvbError) as e:
            capi.Pipeline(None, **kwargs)
        assert e.value.code == 1, kwargs
    # lane sizes that do not add up to the context count
    lib = capi.load_library()
    handle = ctypes.c_void_p()
    handles = (ctypes.c_void_p * 4)(*[c.handle for c in ctxs])
    opts = capi.PipelineOptions(0, 2)
    for sizes in ((2, 1), (2, 3), (4, 0)):
        arr = (ctypes.c_uint64 * len(sizes))(*sizes)
        assert lib.rvb_pipeline_create_lanes(ctypes.byref(handle), handles, ctypes.c_uint64(4), arr, ctypes.c_uint64(len(sizes)), ctypes.byref(opts)) == 1, sizes
        assert not handle.value


def test_a_failing_lane_fails_its_jobs_and_names_itself(rig):
    from parallel_reverb_raytracer_amd import capi
    ctxs, _, pairs, _ = rig
    bad = capi.Context(0)                       # rays, no scene: rvb_trace refuses with RVB_ERR_STATE
    try:
        bad.set_directions(scenes.sphere_directions(9000, seed=31))
        pipe = capi.Pipeline(None, lanes=[[ctxs[0]], [bad]])
        try:
            pipe.configure_speakers(SPEAKERS[0], SPEAKERS[1], NREFL, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
            pipe.submit(*pairs[0])
            pipe.submit(*pairs[1])
            hist, info = pipe.next()
            want, winfo = _solo(rig, 0)
            _check_exact(hist, info, 0, want, winfo)
            with pytest.raises(capi.RvbError) as e:
                pipe.next()
            assert e.value.code == 4 and "lane 1" in str(e.value) and "trace" in str(e.value), str(e.value)
            assert pipe.pending() == 0
        finally:
            pipe.close()                         # joins the lane threads after the failure
    finally:
        bad.close()


def test_c5_per_gpu_share_full_size_hrtf_lanes_of_two_four_pairs_per_launch():
    """C5's per-GPU share with the real histogram sizes: the first 8 of the 64 (source, listener) pairs of the 30 000-triangle hall at
    100 000 rays x 128 bounces, HRTF with each listener facing its source, exact mode, lanes [2, 2] with 4 pairs per launch.  Every
    histogram must equal, bit for bit, that pair traced and binned alone on a fifth context."""
    import torch
    from parallel_reverb_raytracer_amd import capi, distributed
    scene, _ = scenes.concert_hall(30000)
    src, mic = scenes.source_mic_pairs(64, seed=0)
    table = scenes.hrtf_synthetic_table()
    nrays, nrefl = 100000, 128
    dirs = scenes.sphere_directions(nrays, seed=1)
    ctxs = [capi.Context(0) for _ in range(5)]
    pipe = None
    try:
        for k, c in enumerate(ctxs):
            if k in (1, 2, 3):
                c.share_scene(ctxs[0])
            else:
                c.set_scene(scene)
            c.set_directions(dirs)
        solo = ctxs[4]
        facings = [tuple(float(x) for x in (src[p] - mic[p]) / np.linalg.norm(src[p] - mic[p])) for p in range(8)]
        pipe = capi.Pipeline(None, lanes=[ctxs[:2], ctxs[2:4]], pairs_per_launch=4)
        pipe.configure_hrtf(table, (0.0, 0.0, 1.0), UP, nrefl, dtypes.AIR_COEFFICIENTS, 44100.0, True, capi.IR_EXACT)
        for p in range(8):
            pipe.submit(mic[p], src[p], facings[p], UP)
        got = [pipe.next() for _ in range(8)]
        pipe.close()
        pipe = None
        for p, (hist, info) in enumerate(got):
            want, winfo = distributed.generate_ir(solo, mic[p], src[p], nrefl, dtypes.AIR_COEFFICIENTS,
                                                  model=distributed.HrtfModel(table, facings[p], UP), sample_rate=44100.0, trim_predelay=True,
                                                  mode=capi.IR_EXACT, device=torch.device("cuda", 0))
            solo.synchronize()
            want = want.cpu().numpy()
            assert info["job"] == p and info["nbins"] == winfo["nbins"] and info["images"] == winfo["images"]
            assert np.float32(info["predelay"]) == np.float32(winfo["predelay"])
            assert hist.shape == want.shape and np.array_equal(hist, want) and hist.any(), "pair %d differs from the pair alone" % p
    finally:
        if pipe is not None:
            pipe.close()
        for c in ctxs:
            c.close()
