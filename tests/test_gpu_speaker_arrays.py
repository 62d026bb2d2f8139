"""Speaker arrays of more than eight channels (up to capi.MAX_SPEAKERS = 64) through the fused impulse-response path: one key pass,
one sort and one fold for all channels (ordered_sum_wide_kernel, csrc/exact_kernels.hip) against the CPU oracle's per-channel chain
attenuate -> findPredelay / fixPredelay -> flattenImpulses, against the eight-channel path on slices of the same layout, and through the
step-wise entry points (exact_prepare / exact_fold, two contexts folding one after the other, the export to pinned memory).

Bars:
  * RVB_IR_EXACT: every channel bit for bit the oracle's serial sum, and bit for bit what the <= 8-channel kernels return;
  * RVB_IR_FAST: |fast - exact| <= 1e-5 * |exact| + n_bin * 2^-23 * sum|terms| per band-bin (the bound of tests/test_gpu_parity.py)."""
import hashlib

import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

pytestmark = pytest.mark.gpu

NRAYS, NREFL = 512, 24


@pytest.fixture(scope="module")
def ctx():
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    yield c
    c.close()


@pytest.fixture(scope="module")
def traced(ctx):
    """The common input: one trace of the 3 000-triangle cathedral, its merged image sources, all raw impulses in reference order."""
    scene, info = scenes.cathedral(3000)
    mic, src = info["mic"], info["source"]
    ctx.set_scene(scene)
    ctx.raytrace(mic, src, scenes.sphere_directions(NRAYS, seed=23), NREFL, AIR_COEFFICIENTS)
    images = ctx.get_raw_images(False)
    all_raw = np.concatenate([ctx.get_raw_diffuse(), images])
    assert all_raw.shape[0] == NRAYS * NREFL + images.shape[0]
    return {"scene": scene, "mic": mic, "source": src, "images": images, "all_raw": all_raw}


def speakers_for(nchannels):
    """Omni (k = 0) to figure-of-eight (k = 1): gains of both signs and exact zeros occur."""
    return scenes.sphere_directions(nchannels, seed=101)[:, :3], np.linspace(0.0, 1.0, nchannels).astype(np.float32)


def oracle_ir(oracle, mic, impulses, directions, coefficients, trim, sr):
    """The chain of tests/test_gpu_parity.py (_oracle_ir), speaker model."""
    chans = [oracle.attenuate_speaker(mic, impulses, d, c) for d, c in zip(directions, coefficients)]
    if trim:
        pd = oracle.find_predelay(chans)
        for c in chans:
            oracle.fix_predelay(c, pd)
    flat = [oracle.flatten(c, sr) for c in chans]
    return flat, max(f.shape[1] for f in flat), chans


def fast_bound(exact, chans, sr):
    """Rounding bound of a re-ordered float sum per band-bin: 1e-5 * |exact| + n_bin * 2^-23 * sum|terms|."""
    bound = np.empty(exact.shape, np.float64)
    for ch, att in enumerate(chans):
        bins = np.round(att["time"] * np.float32(sr)).astype(np.int64)
        count = np.zeros(exact.shape[2], np.float64)
        np.add.at(count, bins, 1.0)
        absum = np.zeros((8, exact.shape[2]), np.float64)
        for b in range(8):
            np.add.at(absum[b], bins, np.abs(att["volume"][:, b].astype(np.float64)))
        bound[ch] = 1e-5 * np.abs(exact[ch]) + count[None, :] * 2.0 ** -23 * absum + 1e-30
    return bound


def configure(ctx, traced, directions, coefficients, which=None, images="all"):
    from parallel_reverb_raytracer_amd import capi
    ctx.ir_configure_speakers(traced["mic"], directions, coefficients, capi.IR_ALL if which is None else which,
                              traced["images"] if isinstance(images, str) else images)


@pytest.mark.parametrize("sr", [44100.0, 1000.0])
@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("nchannels", [9, 16, 33, 64])
def test_exact_mode_equals_the_oracle_bit_for_bit(ctx, oracle, traced, nchannels, trim, sr):
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(nchannels)
    flat, nb, chans = oracle_ir(oracle, traced["mic"], traced["all_raw"], directions, coefficients, trim, sr)
    # the oracle's data must put the summation under test before the GPU is compared
    live = (traced["all_raw"]["volume"] != 0).any(axis=1)
    assert 0.6 < live.mean() < 0.8
    per_bin = np.bincount(np.round(chans[0]["time"][live] * np.float32(sr)).astype(np.int64))
    if sr == 1000.0:
        assert (per_bin >= 8).sum() >= 300, "too few crowded bins: the summation ORDER would not be under test"
    else:
        for ch in range(nchannels):
            assert np.count_nonzero(flat[ch].any(axis=0)) >= 8000, ch
    assert len({(f.shape, hashlib.sha1(f.tobytes()).digest()) for f in flat}) == nchannels, "two channels' oracle histograms are equal"
    configure(ctx, traced, directions, coefficients)
    exact = ctx.ir_download(trim, sr, capi.IR_EXACT)
    assert exact.shape == (nchannels, 8, nb)
    for ch in range(nchannels):
        n = flat[ch].shape[1]                     # the reference bins every channel on its own maxtime
        assert np.array_equal(exact[ch][:, :n], flat[ch]), (nchannels, trim, sr, ch)
        assert not exact[ch][:, n:].any()


def test_wide_equals_the_eight_channel_path_on_slices_of_the_layout(ctx, traced):
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(16)
    configure(ctx, traced, directions, coefficients)
    wide = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
    assert wide.shape[0] == 16 and wide.any()
    for g in range(2):
        configure(ctx, traced, directions[8 * g:8 * g + 8], coefficients[8 * g:8 * g + 8])
        narrow = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
        assert narrow.shape == (8,) + wide.shape[1:]
        assert np.array_equal(wide[8 * g:8 * g + 8], narrow), g


@pytest.mark.parametrize("nchannels", [9, 33])
def test_fast_mode_within_the_reordered_sum_bound(ctx, oracle, traced, nchannels):
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(nchannels)
    _, nb, chans = oracle_ir(oracle, traced["mic"], traced["all_raw"], directions, coefficients, True, 44100.0)
    configure(ctx, traced, directions, coefficients)
    exact = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
    fast = ctx.ir_download(True, 44100.0, capi.IR_FAST)
    assert fast.shape == exact.shape == (nchannels, 8, nb) and fast.any()
    bound = fast_bound(exact, chans, 44100.0)
    assert (np.abs(fast.astype(np.float64) - exact) <= bound).all()


def test_prepare_and_fold_over_three_unequal_bin_ranges_equal_accumulate(ctx, traced):
    import torch
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(33)
    configure(ctx, traced, directions, coefficients)
    lo, hi = ctx.ir_time_range()
    nbins = ctx.ir_bins(hi, lo, 44100.0)
    whole = torch.zeros((33, 8, nbins), device="cuda", dtype=torch.float32)
    ctx.ir_accumulate_tensor(lo, 44100.0, nbins, capi.IR_EXACT, whole)
    ctx.synchronize()
    parts = torch.zeros((33, 8, nbins), device="cuda", dtype=torch.float32)
    ctx.ir_exact_prepare(lo, 44100.0, nbins)
    cuts = [0, 1000, nbins // 3 + 7, nbins]
    for b0, b1 in zip(cuts[:-1], cuts[1:]):
        ctx.ir_exact_fold_tensor(nbins, b0, b1, parts)
    ctx.synchronize()
    assert whole.any() and torch.equal(whole, parts)


def test_two_contexts_with_consecutive_ray_halves_fold_into_one_histogram(ctx, traced):
    """Diffuse shards first, the merged images last (tests/test_gpu_decomposition.py does it for C3): equals one context."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(33)
    dirs = scenes.sphere_directions(NRAYS, seed=23)
    configure(ctx, traced, directions, coefficients)
    lo, hi = ctx.ir_time_range()
    nbins = ctx.ir_bins(hi, lo, 44100.0)
    whole = torch.zeros((33, 8, nbins), device="cuda", dtype=torch.float32)
    ctx.ir_accumulate_tensor(lo, 44100.0, nbins, capi.IR_EXACT, whole)
    ctx.synchronize()
    halves = [capi.Context(0) for _ in range(2)]
    try:
        chain = torch.zeros((33, 8, nbins), device="cuda", dtype=torch.float32)
        first = 0
        for c, n in zip(halves, (NRAYS // 2 - 40, NRAYS - (NRAYS // 2 - 40))):
            c.set_scene(traced["scene"])
            c.set_directions(dirs[first:first + n])
            c.trace(traced["mic"], traced["source"], NREFL, AIR_COEFFICIENTS, ray_offset=first)
            c.ir_configure_speakers(traced["mic"], directions, coefficients, capi.IR_DIFFUSE, None)
            c.ir_accumulate_tensor(lo, 44100.0, nbins, capi.IR_EXACT, chain)
            c.synchronize()
            first += n
        halves[1].ir_configure_speakers(traced["mic"], directions, coefficients, capi.IR_IMAGES, traced["images"])
        halves[1].ir_accumulate_tensor(lo, 44100.0, nbins, capi.IR_EXACT, chain)
        halves[1].synchronize()
        assert whole.any() and torch.equal(whole, chain)
    finally:
        for c in halves:
            c.close()


def test_export_to_pinned_memory_equals_download(ctx, traced):
    import torch
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers_for(16)
    configure(ctx, traced, directions, coefficients)
    want = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
    lo, hi = ctx.ir_time_range()
    nbins = ctx.ir_bins(hi, lo, 44100.0)
    assert want.shape == (16, 8, nbins)
    for slices in (0, 3):
        hist = torch.zeros((16, 8, nbins), device="cuda", dtype=torch.float32)
        landed = torch.full((16, 8, nbins), float("nan"), dtype=torch.float32).pin_memory()
        ctx.ir_accumulate_export_tensor(lo, 44100.0, nbins, capi.IR_EXACT, hist, landed, slices=slices)
        ctx.synchronize_exports()
        assert np.array_equal(landed.numpy(), want), slices
        ctx.synchronize()


def test_speaker_count_limits(ctx, traced):
    from parallel_reverb_raytracer_amd import capi

    def refused(call):
        with pytest.raises(capi.RvbError) as e:
            call()
        assert e.value.code == 1 and "64" in str(e.value), str(e.value)      # RVB_ERR_INVALID, and the text names the limit

    lanes = [capi.Context(0)]
    multi = capi.MultiContext([0, 0])
    try:
        lanes[0].set_scene(traced["scene"])
        lanes[0].set_directions(scenes.sphere_directions(64, seed=23))
        pipe = capi.Pipeline(None, lanes=[lanes])
        try:
            multi.set_scene(traced["scene"])
            multi.raytrace(traced["mic"], traced["source"], scenes.sphere_directions(64, seed=23), 8, AIR_COEFFICIENTS)
            for n in (0, capi.MAX_SPEAKERS + 1):
                d, k = np.zeros((n, 3), np.float32) + np.float32(1.0), np.full(n, 0.5, np.float32)
                refused(lambda: ctx.ir_configure_speakers(traced["mic"], d, k, capi.IR_ALL, traced["images"]))
                refused(lambda: pipe.configure_speakers(d, k, 8, AIR_COEFFICIENTS))
                refused(lambda: multi.ir_speakers(traced["mic"], d, k, True, 44100.0, capi.IR_EXACT))
            d, k = speakers_for(9)
            ctx.ir_configure_speakers(traced["mic"], d, k, capi.IR_ALL, traced["images"])
            pipe.configure_speakers(d, k, 8, AIR_COEFFICIENTS)
            assert multi.ir_speakers(traced["mic"], d, k, True, 44100.0, capi.IR_EXACT).shape[0] == 9
        finally:
            pipe.close()
    finally:
        multi.close()
        lanes[0].close()
