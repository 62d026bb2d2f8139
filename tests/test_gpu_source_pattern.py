"""Directional sources (rvb_set_source_pattern, csrc/source_kernels.hip): a per-band polar pattern applied to the final records of a
trace.  Expected values come from the CPU oracle only: the gain of a record with departure vector v is the oracle's own
attenuate_speaker on a fake unit-volume impulse — diffuse records: fake microphone 0, fake position = the ray's direction; image-source
and direct impulses: fake microphone = the impulse's position, fake position = the real microphone, so that the subtraction is the
contract's mic - position —, expected records are the oracle's impulse volumes times those gains in numpy float32, and expected impulse
responses the usual oracle chain (attenuate -> find_predelay / fix_predelay -> flatten) on those records.

Bars: records, time ranges and RVB_IR_EXACT histograms bit for bit; RVB_IR_FAST within fast_bound of tests/test_gpu_speaker_arrays.py."""
import functools

import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, aligned_zeros

from test_gpu_speaker_arrays import fast_bound

pytestmark = pytest.mark.gpu

NRAYS, NREFL = 512, 24
SHAPES = np.linspace(0.0, 1.0, 8).astype(np.float32)
FACING = (0.8, 0.35, -0.5)          # not a unit vector: the host normalises it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gains_of(oracle, fake_mics, fake_positions, direction, shapes):
    """[n][8] gains: oracle.attenuate_speaker on unit-volume impulses, one call per distinct shape (and per distinct fake microphone)."""
    fake_mics = np.asarray(fake_mics, np.float32).reshape(-1, 3)
    fake_positions = np.asarray(fake_positions, np.float32).reshape(-1, 3)
    n = fake_positions.shape[0]
    gains = np.zeros((n, 8), np.float32)
    fake = aligned_zeros(n, IMPULSE)
    fake["volume"] = 1.0
    fake["position"][:, :3] = fake_positions
    for shape in sorted(set(float(s) for s in shapes)):
        if fake_mics.shape[0] == 1:
            g = oracle.attenuate_speaker(fake_mics[0], fake, direction, shape)["volume"][:, 0]
        else:
            g = np.array([oracle.attenuate_speaker(fake_mics[i], fake[i:i + 1], direction, shape)["volume"][0, 0] for i in range(n)], np.float32)
        for b in range(8):
            if float(shapes[b]) == shape:
                gains[:, b] = g
    return gains


def expected_records(oracle, case, direction, shapes):
    """The oracle's trace of `case`, scaled: (diffuse, merged images with the direct one first, diffuse gains, image gains)."""
    nrefl = case["nrefl"]
    g_rays = gains_of(oracle, [(0.0, 0.0, 0.0)], case["dirs"][:, :3], direction, shapes)
    g_diffuse = np.repeat(g_rays, nrefl, axis=0)
    diffuse = case["diffuse"].copy()
    diffuse["volume"] = diffuse["volume"] * g_diffuse
    images = case["images"].copy()
    g_images = gains_of(oracle, images["position"][:, :3], np.tile(np.asarray(case["mic"], np.float32), (images.shape[0], 1)), direction, shapes)
    images["volume"] = images["volume"] * g_images
    return diffuse, images, g_diffuse, g_images


def oracle_case(oracle, scene, mic, src, dirs, nrefl):
    diffuse, image, index = oracle.raytrace(scene, mic, src, dirs, nrefl, AIR_COEFFICIENTS)
    return {"scene": scene, "mic": mic, "source": src, "dirs": dirs, "nrefl": nrefl, "diffuse": diffuse,
            "images": oracle.collect_images(image, index, False)}


@pytest.fixture(scope="module")
def cathedral():
    return scenes.cathedral(3000)


@pytest.fixture(scope="module")
def ctx(cathedral):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(cathedral[0])
    yield c
    c.close()


@pytest.fixture(scope="module")
def main_case(oracle, cathedral):
    """512 rays x 24 reflections from the scene's own source to its own microphone: the input of the impulse-response tests."""
    scene, info = cathedral
    return oracle_case(oracle, scene, info["mic"], info["source"], scenes.sphere_directions(NRAYS, seed=23), NREFL)


def same_records(got, want):
    return all(np.array_equal(bits(got[f]), bits(want[f])) for f in ("volume", "position", "time"))


@pytest.mark.parametrize("nrays,nrefl", [(509, 24), (5, 70)])
def test_raw_records_equal_the_oracle_records_times_the_oracle_gain(ctx, oracle, cathedral, nrays, nrefl):
    """509 x 24 = 12 216 records: a partial last workgroup and wave, several rays per wave; 5 x 70: a ray longer than a wave."""
    scene, info = cathedral
    case = oracle_case(oracle, scene, info["mic"], info["source"], scenes.sphere_directions(nrays, seed=23), nrefl)
    diffuse, images, g_diffuse, g_images = expected_records(oracle, case, FACING, SHAPES)
    # the oracle's data must put the feature under test
    assert (g_diffuse < 0).any() and (g_diffuse > 0).any(), "gains of one sign only"
    if nrays == 509:
        assert case["images"].shape[0] >= 2, "no image-source impulse besides the direct one"
    assert case["images"].shape[0] >= 1 and (case["images"]["volume"][0] != 0).any(), "the direct path is hidden"
    live = (case["diffuse"]["volume"] != 0).any(axis=1)
    assert live.any() and not live.all()
    for b in range(1, 8):
        assert (diffuse["volume"][live, b] != case["diffuse"]["volume"][live, b]).any(), b
        assert (images["volume"][:, b] != case["images"]["volume"][:, b]).any(), b

    ctx.set_source_pattern(None)
    ctx.raytrace(case["mic"], case["source"], case["dirs"], nrefl, AIR_COEFFICIENTS)
    plain_diffuse, plain_direct, plain_images = ctx.get_raw_diffuse(), ctx.get_direct(), ctx.get_raw_images(False)
    assert same_records(plain_diffuse, case["diffuse"]) and same_records(plain_images, case["images"])
    ctx.set_source_pattern(FACING, SHAPES)
    try:
        ctx.raytrace(case["mic"], case["source"], case["dirs"], nrefl, AIR_COEFFICIENTS)
        got_diffuse, got_direct, got_images = ctx.get_raw_diffuse(), ctx.get_direct(), ctx.get_raw_images(False)
        assert "source_pattern_kernel" in [k for k, _ in ctx.last_timings()]
    finally:
        ctx.set_source_pattern(None)
    assert same_records(got_diffuse, diffuse)
    assert same_records(got_direct, images[:1])            # std::map order: the direct path's key {0} comes first
    assert got_images.shape == images.shape and same_records(got_images, images)
    # band 0 has shape 0: gain exactly 1, the unscaled trace bit for bit; every other band differs from it
    assert np.array_equal(bits(got_diffuse["volume"][:, 0]), bits(plain_diffuse["volume"][:, 0]))
    assert np.array_equal(bits(got_images["volume"][:, 0]), bits(plain_images["volume"][:, 0]))
    assert np.array_equal(bits(got_direct["volume"][:, 0]), bits(plain_direct["volume"][:, 0]))
    for b in range(1, 8):
        assert not np.array_equal(bits(got_diffuse["volume"][:, b]), bits(plain_diffuse["volume"][:, b])), b
        assert not np.array_equal(bits(got_images["volume"][:, b]), bits(plain_images["volume"][:, b])), b


def oracle_range(records):
    """findPredelay's and MAX_SAMPLE's inputs: earliest non-zero and latest time of the impulses that carry volume."""
    live = (records["volume"] != 0).any(axis=1)
    t = records["time"][live]
    return float(t[t != 0].min()), float(t.max())


def test_a_null_of_the_pattern_moves_the_time_range(ctx, oracle, cathedral):
    """Figure-of-eight facing +x in every band; the second half of the rays lies in the plane x = 0: gain exactly 0, all their
    impulses become zero-volume impulses.  Source and microphone sit close to a side wall in that plane, so that the earliest
    arrival of the unscaled trace belongs to one of the nulled rays (asserted below on the oracle's data)."""
    from parallel_reverb_raytracer_amd import capi
    scene = cathedral[0]
    mic, src, nrefl = (0.0, 12.0, 11.0), (0.0, 12.5, 11.5), 6
    dirs = scenes.sphere_directions(NRAYS, seed=0).copy()
    half = NRAYS // 2
    dirs[half:, 0] = 0.0
    length = np.sqrt(dirs[half:, 1] * dirs[half:, 1] + dirs[half:, 2] * dirs[half:, 2], dtype=np.float32)
    dirs[half:, 1] /= length
    dirs[half:, 2] /= length
    case = oracle_case(oracle, scene, mic, src, dirs, nrefl)
    facing, shapes = (1.0, 0.0, 0.0), np.ones(8, np.float32)
    diffuse, _, g_diffuse, _ = expected_records(oracle, case, facing, shapes)
    assert not g_diffuse[half * nrefl:].any() and g_diffuse[:half * nrefl].all()
    want_range, plain_range = oracle_range(diffuse), oracle_range(case["diffuse"])
    assert want_range != plain_range, "the null does not move the range"
    assert (diffuse["volume"] != 0).any(axis=1).mean() >= 0.4, "too few records still live"

    speakers = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])
    chans = [oracle.attenuate_speaker(mic, diffuse, d, c) for d, c in zip(*speakers)]
    pd = oracle.find_predelay(chans)
    for c in chans:
        oracle.fix_predelay(c, pd)
    flat = [oracle.flatten(c, 44100.0) for c in chans]

    ctx.set_source_pattern(facing, shapes)
    try:
        ctx.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        assert same_records(ctx.get_raw_diffuse(), diffuse)
        ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
        assert ctx.ir_time_range() == want_range
        exact = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
    finally:
        ctx.set_source_pattern(None)
    assert np.float32(pd) == np.float32(want_range[0])
    for ch in range(2):
        n = flat[ch].shape[1]
        assert np.array_equal(exact[ch][:, :n], flat[ch]) and not exact[ch][:, n:].any(), ch
    ctx.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)          # ... and without the pattern the range is the unscaled one again
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    assert ctx.ir_time_range() == plain_range


def trace_scaled(ctx, main_case):
    """The main case traced with the pattern: the context holds the scaled trace afterwards (a millisecond), the pattern is off again."""
    ctx.set_source_pattern(FACING, SHAPES)
    try:
        ctx.raytrace(main_case["mic"], main_case["source"], main_case["dirs"], NREFL, AIR_COEFFICIENTS)
    finally:
        ctx.set_source_pattern(None)


@pytest.fixture(scope="module")
def scaled(ctx, oracle, main_case):
    """The oracle's scaled records of the main case in reference order, and the merged images of the GPU's scaled trace."""
    diffuse, images, _, _ = expected_records(oracle, main_case, FACING, SHAPES)
    trace_scaled(ctx, main_case)
    got_images = ctx.get_raw_images(False)
    assert same_records(got_images, images)
    return {"all_raw": np.concatenate([diffuse, images]), "images": got_images}


def oracle_chain(oracle, model, mic, impulses, trim, sr):
    if model == "hrtf":
        table, facing, up = hrtf()
        chans = [oracle.attenuate_hrtf(mic, impulses, table[ch], facing, up, ch) for ch in (0, 1)]
    else:
        chans = [oracle.attenuate_speaker(mic, impulses, d, c) for d, c in zip(*layout(model))]
    if trim:
        pd = oracle.find_predelay(chans)
        for c in chans:
            oracle.fix_predelay(c, pd)
    return [oracle.flatten(c, sr) for c in chans], chans


@functools.lru_cache(maxsize=1)
def hrtf():
    return scenes.hrtf_test_table(), (1.0, 0.0, 0.2), (0.0, 1.0, 0.0)


def layout(model):
    n = {"speakers2": 2, "speakers9": 9}[model]
    return scenes.sphere_directions(n, seed=101)[:, :3], np.linspace(0.0, 1.0, n).astype(np.float32)


@pytest.mark.parametrize("sr", [44100.0, 1000.0])
@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("model", ["speakers2", "speakers9", "hrtf"])
def test_impulse_responses_of_scaled_records_equal_the_oracle_chain(ctx, oracle, main_case, scaled, model, trim, sr):
    """Two speakers (the eight-channel kernels), nine (the wide fold) and the HRTF model all read the scaled records."""
    from parallel_reverb_raytracer_amd import capi
    mic = main_case["mic"]
    flat, chans = oracle_chain(oracle, model, mic, scaled["all_raw"], trim, sr)
    nb = max(f.shape[1] for f in flat)
    if sr == 1000.0:
        live = (scaled["all_raw"]["volume"] != 0).any(axis=1)
        per_bin = np.bincount(np.round(chans[0]["time"][live] * np.float32(sr)).astype(np.int64))
        assert (per_bin >= 8).sum() >= 300, "too few crowded bins: the summation ORDER would not be under test"
    trace_scaled(ctx, main_case)
    if model == "hrtf":
        ctx.ir_configure_hrtf(mic, *hrtf(), capi.IR_ALL, scaled["images"])
    else:
        ctx.ir_configure_speakers(mic, *layout(model), capi.IR_ALL, scaled["images"])
    exact = ctx.ir_download(trim, sr, capi.IR_EXACT)
    assert exact.shape == (len(flat), 8, nb)
    for ch in range(len(flat)):
        n = flat[ch].shape[1]                     # the reference bins every channel on its own maxtime
        assert np.array_equal(exact[ch][:, :n], flat[ch]), (model, trim, sr, ch)
        assert not exact[ch][:, n:].any()
    fast = ctx.ir_download(trim, sr, capi.IR_FAST)
    assert fast.shape == exact.shape and fast.any()
    assert (np.abs(fast.astype(np.float64) - exact) <= fast_bound(exact, chans, sr)).all(), (model, trim, sr)


def test_trace_pairs_takes_a_pattern_per_pair_or_one_for_all(ctx, cathedral):
    """3 pairs x 256 rays: every pair equals the same pair traced alone with its pattern, bit for bit; two patterns are refused."""
    from parallel_reverb_raytracer_amd import capi
    info = cathedral[1]
    mics = np.array([info["mic"], (0.0, 12.0, 11.0), (2.0, 3.0, 0.3)], np.float32)
    sources = np.array([info["source"], (0.0, 12.5, 11.5), (-4.0, 2.0, -0.4)], np.float32)
    facings = np.array([FACING, (-1.0, 0.0, 0.0), (0.1, -1.0, 0.3)], np.float32)
    shapes = np.stack([SHAPES, SHAPES[::-1], np.full(8, 0.5, np.float32)])
    nrefl, nrays = 10, 256
    ctx.set_directions(scenes.sphere_directions(nrays, seed=5))
    speakers = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])

    def per_pair_results(pair_mics):
        """(direct impulse, diffuse time range) of every pair of the context's last trace"""
        out = []
        for p, m in enumerate(pair_mics):
            ctx.select_pair(p)
            direct = ctx.get_direct()
            ctx.ir_configure_speakers(m, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
            out.append((direct, ctx.ir_time_range()))
        return out

    try:
        for per_pair in (True, False):
            alone = []
            for p in range(3):
                ctx.set_source_pattern(facings[p if per_pair else 0], shapes[p if per_pair else 0])
                ctx.trace(mics[p], sources[p], nrefl, AIR_COEFFICIENTS)
                alone.append((ctx.get_raw_diffuse(), ctx.get_image_candidates(), per_pair_results([mics[p]])[0]))
            if per_pair:
                ctx.set_source_pattern(facings, shapes)
            else:
                ctx.set_source_pattern(facings[0], shapes[0])
            ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
            diffuse, cand, res = ctx.get_raw_diffuse().reshape(3, -1), ctx.get_image_candidates(), per_pair_results(mics)
            assert len(cand) > 3
            for p in range(3):
                assert same_records(diffuse[p], alone[p][0]), (per_pair, p)
                mine = ctx.get_pair_candidates(p, cand)
                assert mine.shape == alone[p][1].shape and mine.tobytes() == alone[p][1].tobytes(), (per_pair, p)
                assert same_records(res[p][0], alone[p][2][0]) and res[p][1] == alone[p][2][1], (per_pair, p)
            assert not same_records(alone[1][0], alone[2][0])
        ctx.set_source_pattern(facings[:2], shapes[:2])
        with pytest.raises(capi.RvbError) as e:
            ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
        assert e.value.code == 1, str(e.value)          # RVB_ERR_INVALID
        with pytest.raises(capi.RvbError) as e:
            ctx.trace(mics[0], sources[0], nrefl, AIR_COEFFICIENTS)
        assert e.value.code == 1, str(e.value)
    finally:
        ctx.set_source_pattern(None)
        ctx.npairs = 1


def test_a_cleared_pattern_leaves_no_trace(ctx, cathedral):
    from parallel_reverb_raytracer_amd import capi
    scene, info = cathedral
    dirs = scenes.sphere_directions(300, seed=9)
    fresh = capi.Context(0)
    try:
        fresh.set_scene(scene)
        fresh.raytrace(info["mic"], info["source"], dirs, 12, AIR_COEFFICIENTS)
        want = (fresh.get_raw_diffuse().tobytes(), fresh.get_direct().tobytes(), fresh.get_image_candidates().tobytes())
        fresh.ir_configure_speakers(info["mic"], [(-1, 0, -1)], [0.5], capi.IR_DIFFUSE, None)
        want_range = fresh.ir_time_range()
    finally:
        fresh.close()
    ctx.set_source_pattern(FACING, SHAPES)
    ctx.raytrace(info["mic"], info["source"], dirs, 12, AIR_COEFFICIENTS)
    assert ctx.get_raw_diffuse().tobytes() != want[0]
    ctx.set_source_pattern(None)
    ctx.raytrace(info["mic"], info["source"], dirs, 12, AIR_COEFFICIENTS)
    names = [k for k, _ in ctx.last_timings()]
    assert names and "source_pattern_kernel" not in names
    assert (ctx.get_raw_diffuse().tobytes(), ctx.get_direct().tobytes(), ctx.get_image_candidates().tobytes()) == want
    ctx.ir_configure_speakers(info["mic"], [(-1, 0, -1)], [0.5], capi.IR_DIFFUSE, None)
    assert ctx.ir_time_range() == want_range


def test_ray_shards_equal_one_context(ctx, main_case, scaled):
    """MultiContext([0, 0]), and two contexts that fold consecutive ray halves into one histogram, in exact mode."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    mic, src, dirs = main_case["mic"], main_case["source"], main_case["dirs"]
    directions, coefficients = layout("speakers2")
    trace_scaled(ctx, main_case)
    ctx.ir_configure_speakers(mic, directions, coefficients, capi.IR_ALL, scaled["images"])
    want = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
    lo, hi = ctx.ir_time_range()
    nbins = ctx.ir_bins(hi, lo, 44100.0)
    assert want.shape == (2, 8, nbins) and want.any()

    multi = capi.MultiContext([0, 0])
    try:
        multi.set_scene(main_case["scene"])
        multi.set_source_pattern(FACING, SHAPES)
        multi.raytrace(mic, src, dirs, NREFL, AIR_COEFFICIENTS)
        assert same_records(multi.get_raw_diffuse(), scaled["all_raw"][:NRAYS * NREFL])
        assert same_records(multi.get_raw_images(False), scaled["images"])
        assert np.array_equal(multi.ir_speakers(mic, directions, coefficients, True, 44100.0, capi.IR_EXACT), want)
    finally:
        multi.close()

    halves = [capi.Context(0) for _ in range(2)]
    try:
        chain = torch.zeros((2, 8, nbins), device="cuda", dtype=torch.float32)
        first = 0
        for c, n in zip(halves, (NRAYS // 2 - 40, NRAYS - (NRAYS // 2 - 40))):
            c.set_scene(main_case["scene"])
            c.set_directions(dirs[first:first + n])
            c.set_source_pattern(FACING, SHAPES)
            c.trace(mic, src, NREFL, AIR_COEFFICIENTS, ray_offset=first)
            c.ir_configure_speakers(mic, directions, coefficients, capi.IR_DIFFUSE, None)
            c.ir_accumulate_tensor(lo, 44100.0, nbins, capi.IR_EXACT, chain)
            c.synchronize()
            first += n
        cand = np.concatenate([c.get_image_candidates() for c in halves])
        images = capi.merge_images(cand, halves[0].get_direct(), False)
        assert same_records(images, scaled["images"])
        halves[1].ir_configure_speakers(mic, directions, coefficients, capi.IR_IMAGES, images)
        halves[1].ir_accumulate_tensor(lo, 44100.0, nbins, capi.IR_EXACT, chain)
        halves[1].synchronize()
        assert np.array_equal(chain.cpu().numpy(), want)
    finally:
        for c in halves:
            c.close()
