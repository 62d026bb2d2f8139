"""The live list of exact mode (live_keys_kernel, live_offsets_kernel, live_compact_kernel of csrc/exact_kernels.hip; the live count of the
shadow kernels): only the impulses that carry volume are sorted, the list is sized by the trace's count.  Every histogram is held bit for
bit against the CPU oracle's chain attenuate -> findPredelay / fixPredelay -> flattenImpulses, as tests/test_gpu_attenuation_edges.py does
(a NaN must be a NaN where the oracle has one: IEEE 754 leaves its payload open); rvb_ir_exact_list_info (include/rvb_capi_live.h) says what was listed.

Constructed records enter as image sources (RVB_IR_IMAGES) of a context that holds a one-ray, one-bounce trace; the traces with blocked
shadow rays are made in the non-convex room of tests/image_edges.py."""
import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, aligned_zeros

from test_gpu_attenuation_edges import TIME_MODELS, oracle_histograms
from test_gpu_reshade import AIR_B, SPEAKERS

pytestmark = pytest.mark.gpu

FACING_UP = ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
RATES = (44100.0, 8192.0)
PATTERNS = ("all_dead", "all_live", "alternating", "tile_edges_dead", "last_only", "signed_zero_subnormal_nan")
# nrays x nreflections = 4 T - 1, 4 T, 4 T + 1 for the tile of 1024 records
TRACE_SHAPES = ((315, 13), (256, 16), (241, 17))


def tile():
    from parallel_reverb_raytracer_amd import capi
    return capi.LIVE_TILE


def sizes():
    t = tile()
    return (1, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t + 1)


@pytest.fixture(scope="module")
def table():
    return scenes.hrtf_synthetic_table()


def make_ctx(keep=False):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(E.room())
    if keep:
        c.keep_paths(True, listener=True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def records():
    """2 T + 1 records, computed once and left unchanged: seeded positions around the microphones of TIME_MODELS, times below 20 ms
    (several records per bin at either rate, so the order of a bin's sum shows), volumes in [0.1, 1)."""
    n = 2 * tile() + 1
    rng = np.random.default_rng(61)
    rec = aligned_zeros(n, IMPULSE)
    rec["volume"] = rng.uniform(0.1, 1.0, (n, 8)).astype(np.float32)
    rec["position"][:, :3] = rng.uniform(-6.0, 6.0, (n, 3)).astype(np.float32)
    rec["time"] = rng.uniform(0.002, 0.02, n).astype(np.float32)
    return rec


def with_pattern(rec, pattern):
    """A copy of `rec` with the volumes of `pattern`; the second value: which records carry volume."""
    rec = rec.copy()
    n, t = rec.shape[0], tile()
    i = np.arange(n)
    vol = rec["volume"]
    if pattern == "all_dead":
        vol[:] = 0.0
    elif pattern == "alternating":
        vol[i % 2 == 1] = 0.0
    elif pattern == "tile_edges_dead":
        vol[(i % t == 0) | (i % t == t - 1)] = 0.0
    elif pattern == "last_only":
        vol[:-1] = 0.0
    elif pattern == "signed_zero_subnormal_nan":
        vol[i % 4 == 0] = -0.0                                  # dead, as a record of +0 is
        vol[i % 4 == 1] = 0.0
        vol[i % 4 == 1, 2] = np.float32(1e-40)                  # one subnormal band: live
        vol[i % 4 == 2, 5] = np.nan                             # live
    else:
        assert pattern == "all_live"
    live = (rec["volume"] != 0).any(axis=1)
    return rec, live


def configure(ctx, oracle, model, rec, table, which=None, mic=None):
    """Configures the fused stage for the images `rec` (and the context's diffuse impulses where `which` takes them); returns the
    function that attenuates records as the oracle does, channel by channel."""
    from parallel_reverb_raytracer_amd import capi
    m = TIME_MODELS[model]
    mic = m["mic"] if mic is None else mic
    which = capi.IR_IMAGES if which is None else which
    if "hrtf" in m:
        ctx.ir_configure_hrtf(mic, table, m["hrtf"][0], m["hrtf"][1], which, rec)
        return lambda r: [oracle.attenuate_hrtf(mic, r, table[ear], m["hrtf"][0], m["hrtf"][1], ear) for ear in (0, 1)]
    ctx.ir_configure_speakers(mic, [d for d, _ in m["speakers"]], [k for _, k in m["speakers"]], which, rec)
    return lambda r: [oracle.attenuate_speaker(mic, r, d, k) for d, k in m["speakers"]]


def assert_bits_equal_the_oracle(got, flat, nb, what):
    assert got.shape == (len(flat), 8, nb), (what, got.shape, nb)
    for ch, f in enumerate(flat):
        n = f.shape[1]                        # the reference bins every channel on its own maxtime
        g = got[ch][:, :n]
        nan = np.isnan(f)
        same = np.where(nan, np.isnan(g), g.view(np.uint32) == f.view(np.uint32))
        if not same.all():
            band, bin_ = np.argwhere(~same)[0]
            raise AssertionError("%s: channel %d band %d bin %d: got %r, the oracle has %r (%d band-bins differ)"
                                 % (what, ch, band, bin_, g[band, bin_], f[band, bin_], np.count_nonzero(~same)))
        assert not got[ch][:, n:].view(np.uint32).any(), what


def check_against_oracle(ctx, oracle, attenuate, impulses, what, rates=RATES):
    from parallel_reverb_raytracer_amd import capi
    chans = attenuate(impulses)
    for sr in rates:
        for trim in (False, True):
            flat, nb, _ = oracle_histograms(oracle, chans, sr, trim)
            assert_bits_equal_the_oracle(ctx.ir_download(trim, sr, capi.IR_EXACT), flat, nb, "%s, %g Hz, trim %s" % (what, sr, trim))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("model", list(TIME_MODELS))
def test_constructed_records_equal_the_oracle(ctx, oracle, records, table, model, pattern):
    """Every size around a round of 64, a workgroup of 256 and the tile: the list holds every image, the key pass finds the live ones."""
    ctx.raytrace(E.PAIRS[0][0], E.PAIRS[0][1], scenes.sphere_directions(1, seed=23), 1, AIR_COEFFICIENTS)
    for n in sizes():
        rec, live = with_pattern(records[:n], pattern)
        attenuate = configure(ctx, oracle, model, rec, table)
        check_against_oracle(ctx, oracle, attenuate, rec, "%s, %s, %d records" % (model, pattern, n))
        listed, on_device, valid = ctx.ir_exact_list_info()
        assert (listed, on_device, valid) == (n, np.count_nonzero(live), True), (model, pattern, n)
    if pattern not in ("all_dead", "all_live"):
        assert 0 < np.count_nonzero(live) < live.shape[0]


def live_rows(impulses):
    return int(np.count_nonzero((impulses["volume"] != 0).any(axis=1)))


def check_trace(ctx, oracle, table, mic, diffuse, images, what, models=("speakers_2", "hrtf")):
    """The context's selected pair has the diffuse impulses `diffuse` (host copy) and the merged images `images`."""
    from parallel_reverb_raytracer_amd import capi
    n, live = diffuse.shape[0], live_rows(diffuse)
    assert 0 < live < n, (what, "dead and live impulses must both occur", live, n)
    for model in models:
        attenuate = configure(ctx, oracle, model, images, table, capi.IR_ALL, mic)
        check_against_oracle(ctx, oracle, attenuate, np.concatenate([diffuse, images]), "%s, %s, all" % (what, model), RATES[:1])
        assert ctx.ir_exact_list_info() == (live + images.shape[0], live + live_rows(images), True), (what, model)
        attenuate = configure(ctx, oracle, model, None, table, capi.IR_DIFFUSE, mic)
        check_against_oracle(ctx, oracle, attenuate, diffuse, "%s, %s, diffuse" % (what, model), RATES[:1])
        assert ctx.ir_exact_list_info() == (live, live, True), (what, model)


@pytest.mark.parametrize("shape", TRACE_SHAPES)
def test_a_trace_with_blocked_shadow_rays(ctx, oracle, table, shape):
    nrays, nrefl = shape
    assert abs(nrays * nrefl - 4 * tile()) <= 1
    mic, src = E.PAIRS[0]
    ctx.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
    check_trace(ctx, oracle, table, mic, ctx.get_raw_diffuse(), ctx.get_raw_images(False), "%d x %d" % shape)


@pytest.mark.parametrize("shape", TRACE_SHAPES)
def test_a_trace_group_of_two_contexts(ctx, oracle, table, shape):
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = shape
    other = make_ctx()
    try:
        for c in (ctx, other):
            c.set_directions(E.directions(nrays))
        capi.Context.trace_group([ctx, other], E.MICS[:2], E.SOURCES[:2], nrefl, AIR_COEFFICIENTS)
        for k, c in enumerate((ctx, other)):
            mic = tuple(float(x) for x in E.MICS[k])
            check_trace(c, oracle, table, mic, c.get_raw_diffuse(), c.get_raw_images(False), "group member %d, %d x %d" % ((k,) + shape),
                        models=("speakers_2",))
    finally:
        other.close()


@pytest.mark.parametrize("shape", TRACE_SHAPES)
def test_two_pairs_in_one_launch(ctx, oracle, table, shape):
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = shape
    n = nrays * nrefl
    ctx.set_directions(E.directions(nrays))
    try:
        ctx.trace_pairs(E.MICS[:2], E.SOURCES[:2], nrefl, AIR_COEFFICIENTS)
        diffuse = ctx.get_raw_diffuse()
        for pair in (1, 0):
            ctx.select_pair(pair)
            images = capi.merge_images(ctx.get_pair_candidates(pair), ctx.get_direct(), False)
            check_trace(ctx, oracle, table, tuple(float(x) for x in E.MICS[pair]), diffuse[pair * n:(pair + 1) * n], images,
                        "pair %d of 2, %d x %d" % ((pair,) + shape), models=("speakers_2",))
    finally:
        ctx.npairs = 1


def check_invalidated(ctx, oracle, table, mic, what):
    """The trace's count no longer holds: every impulse is listed, and the histogram is the oracle's all the same."""
    from parallel_reverb_raytracer_amd import capi
    diffuse, images = ctx.get_raw_diffuse(), ctx.get_raw_images(False)
    live = live_rows(diffuse)
    assert 0 < live < diffuse.shape[0], what
    for model in ("speakers_2", "hrtf"):
        attenuate = configure(ctx, oracle, model, images, table, capi.IR_ALL, mic)
        check_against_oracle(ctx, oracle, attenuate, np.concatenate([diffuse, images]), "%s, %s" % (what, model), RATES[:1])
        assert ctx.ir_exact_list_info() == (diffuse.shape[0] + images.shape[0], live + live_rows(images), False), (what, model)
    return live


def test_what_rewrites_the_records_invalidates_the_count(oracle, table):
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = TRACE_SHAPES[0]
    mic, src = E.PAIRS[0]
    # every fifth ray leaves at right angles to the pattern's axis: a figure of eight along x gives it the gain 0
    dirs = np.array(E.directions(nrays), np.float32).reshape(-1, 4).copy()
    dirs[::5, 0] = 0.0
    dirs[:, :3] /= np.linalg.norm(dirs[:, :3].astype(np.float64), axis=1)[:, None].astype(np.float32)
    assert not dirs[::5, 0].any()
    c = make_ctx(keep=True)
    try:
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        c.ir_download(True, RATES[0], capi.IR_EXACT)
        live_plain = live_rows(c.get_raw_diffuse())
        assert c.ir_exact_list_info() == (live_plain, live_plain, True)
        c.set_source_pattern((1.0, 0.0, 0.0), 1.0)
        c.trace(mic, src, nrefl, AIR_COEFFICIENTS)
        assert check_invalidated(c, oracle, table, mic, "a source pattern") < live_plain, "the pattern silences no record"
        c.set_source_pattern(None)
        c.trace(mic, src, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        c.ir_download(True, RATES[0], capi.IR_EXACT)
        assert c.ir_exact_list_info() == (live_plain, live_plain, True), "the next trace counts again"
        c.reshade(E.table_b(), AIR_B)
        check_invalidated(c, oracle, table, mic, "rvb_reshade")
        c.trace(mic, src, nrefl, AIR_COEFFICIENTS)
        mic1 = tuple(float(x) for x in E.MICS[1])
        c.relisten(mic1)
        check_invalidated(c, oracle, table, mic1, "rvb_relisten")
    finally:
        c.close()


@pytest.mark.parametrize("model", list(TIME_MODELS))
def test_prepare_and_fold_over_three_bin_ranges_equal_one_accumulate(ctx, oracle, table, model):
    import torch
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = TRACE_SHAPES[2]
    mic, src = E.PAIRS[0]
    ctx.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
    diffuse, images = ctx.get_raw_diffuse(), ctx.get_raw_images(False)
    attenuate = configure(ctx, oracle, model, images, table, capi.IR_ALL, mic)
    lo, hi = ctx.ir_time_range()
    nb = ctx.ir_bins(hi, lo, RATES[0])
    nch = len(TIME_MODELS[model].get("speakers", (0, 1)))
    # a histogram that is not empty: both ways add on top of what it holds
    start = torch.arange(nch * 8 * nb, device="cuda", dtype=torch.float32).reshape(nch, 8, nb) * 0.25
    once, folded = start.clone(), start.clone()
    ctx.ir_accumulate_tensor(lo, RATES[0], nb, capi.IR_EXACT, once)
    ctx.ir_exact_prepare(lo, RATES[0], nb)
    for b0, b1 in ((nb // 3, nb - 7), (0, nb // 3), (nb - 7, nb)):
        ctx.ir_exact_fold_tensor(nb, b0, b1, folded)
    ctx.synchronize()
    live = live_rows(diffuse)
    assert ctx.ir_exact_list_info() == (live + images.shape[0], live + live_rows(images), True)
    assert torch.equal(once.view(torch.int32), folded.view(torch.int32)), model
    # ... and from zero it is the oracle's
    flat, nb_oracle, _ = oracle_histograms(oracle, attenuate(np.concatenate([diffuse, images])), RATES[0], True)
    assert nb_oracle == nb
    hist = torch.zeros((nch, 8, nb), device="cuda", dtype=torch.float32)
    ctx.ir_exact_prepare(lo, RATES[0], nb)
    for b0, b1 in ((0, nb // 3), (nb // 3, nb - 7), (nb - 7, nb)):
        ctx.ir_exact_fold_tensor(nb, b0, b1, hist)
    ctx.synchronize()
    assert_bits_equal_the_oracle(hist.cpu().numpy(), flat, nb, model)
