"""The exact fold by coarse bin (csrc/exact_kernels.hip: bin_starts_kernel with a shift, ordered_sum_coarse_kernel; csrc/sort.hip:
sort_and_bin with a coarse_shift): for up to 8 speakers the list is ordered on bin >> 5 only and a wave folds the 32 bins of a coarse
bin in rounds of 64 entries.  Every histogram is held bit for bit against the CPU oracle's chain attenuate -> findPredelay /
fixPredelay -> flattenImpulses, as tests/test_gpu_live_list.py and tests/test_gpu_attenuation_edges.py do.

Constructed records enter as image sources (RVB_IR_IMAGES) of a context that holds a one-ray, one-bounce trace.  Their times are whole
multiples of 1 / 8192 s, so at 8192 Hz and without a predelay a record's bin is the number it was built with and the histogram's length
is the largest of them + 1; the list keeps the records' (shuffled) order, so a bin's entries are spread over its coarse bin's run."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import attenuation_edges as ae
import image_edges as E
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, aligned_zeros

from test_gpu_attenuation_edges import TIME_MODELS, oracle_histograms, padded
from test_gpu_live_list import assert_bits_equal_the_oracle

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
RATE = 8192.0
MIC = (1.0, 1.5, -2.0)
FEW_BINS = (1, 31, 32, 33, 65)
SPEAKER_COUNTS = (1, 2, 3, 4, 6)
# (bin, entries): bin 0 stays empty; 1, 63, 64, 65 and 200 entries in bins of coarse bin 0; coarse bin 1 is a run of exactly 64 entries
# and coarse bin 2 one of exactly 128; coarse bin 3 is empty between them and coarse bin 4, which ends the histogram in its ninth bin
RUN_LENGTHS = ((1, 1), (2, 63), (3, 64), (4, 65), (5, 200), (32, 40), (50, 24)) + tuple((64 + b, 4) for b in range(32)) + ((128, 3), (131, 70), (136, 2))


def make_ctx():
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(E.room())
    c.raytrace(E.PAIRS[0][0], E.PAIRS[0][1], scenes.sphere_directions(1, seed=23), 1, AIR_COEFFICIENTS)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def records_in_bins(bins, seed, dead_every=4):
    """A record per entry of `bins`, in a seeded shuffle of that order: volumes over six orders of magnitude (the order of a bin's sum
    shows in its last bits), seeded positions; every `dead_every`-th record of the shuffled list carries no volume (0: none does)."""
    rng = np.random.default_rng(seed)
    bins = rng.permutation(np.asarray(bins, np.int64))
    n = bins.shape[0]
    rec = aligned_zeros(n, IMPULSE)
    rec["volume"] = (rng.uniform(0.1, 1.0, (n, 8)) * 10.0 ** rng.uniform(-3.0, 3.0, (n, 1))).astype(np.float32)
    rec["position"][:, :3] = rng.uniform(-6.0, 6.0, (n, 3)).astype(np.float32)
    rec["time"] = (bins / RATE).astype(np.float32)
    assert np.array_equal(np.round(rec["time"].astype(np.float64) * RATE), bins)
    if dead_every:
        dead = np.arange(n) % dead_every == dead_every - 1
        dead[np.flatnonzero(bins == bins.max())[0]] = False       # (the histogram keeps its length)
        rec["volume"][dead] = 0.0
    return rec


def few_bins(nbins):
    """0 to 4 entries per bin, at least one in the last."""
    return [b for b in range(nbins) for _ in range((b * 7) % 5 if b + 1 < nbins else 3)]


def run_lengths():
    return [b for b, count in RUN_LENGTHS for _ in range(count)]


def speakers(count):
    sp = ae.EDGE_SPEAKERS[:count]
    return [d for d, _ in sp], [k for _, k in sp]


def configure(ctx, oracle, count, rec, which=None, mic=MIC):
    """The fused stage for the images `rec` and `count` speakers; returns the function that attenuates records as the oracle does."""
    from parallel_reverb_raytracer_amd import capi
    directions, coefficients = speakers(count)
    ctx.ir_configure_speakers(mic, directions, coefficients, capi.IR_IMAGES if which is None else which, rec)
    return lambda r: [oracle.attenuate_speaker(mic, r, d, k) for d, k in zip(directions, coefficients)]


def fold_ranges(ctx, nb, ranges, hist):
    ctx.ir_exact_prepare(0.0, RATE, nb)
    for b0, b1 in ranges:
        ctx.ir_exact_fold_tensor(nb, b0, b1, hist)
    ctx.synchronize()


@pytest.mark.parametrize("nbins", FEW_BINS)
def test_fewer_bins_than_a_coarse_bin_and_a_last_coarse_bin_cut_by_the_end(ctx, oracle, nbins):
    """1 and 31 bins: one run, no sort.  32: one whole coarse bin, the sentinel entries in a second one.  33 and 65: the last coarse
    bin holds one bin and shares its run with the sentinel entries of the dead records."""
    from parallel_reverb_raytracer_amd import capi
    rec = records_in_bins(few_bins(nbins), 100 + nbins)
    chans = configure(ctx, oracle, 2, rec)(rec)
    flat, nb, _ = oracle_histograms(oracle, chans, RATE, False)
    assert nb == nbins
    assert_bits_equal_the_oracle(ctx.ir_download(False, RATE, capi.IR_EXACT), flat, nb, "%d bins" % nbins)
    assert ctx.ir_exact_list_info()[:2] == (rec.shape[0], int(np.count_nonzero(rec["volume"].any(axis=1))))
    if nbins > 1:                             # (one bin: every time is 0 and there is no predelay to find)
        flat, nb, _ = oracle_histograms(oracle, chans, RATE, True)
        assert_bits_equal_the_oracle(ctx.ir_download(True, RATE, capi.IR_EXACT), flat, nb, "%d bins, predelay trimmed" % nbins)


@pytest.mark.parametrize("nbins", (31, 33, 40))
def test_live_records_behind_the_histogram_end_stand_inside_the_last_run(ctx, oracle, nbins):
    """A histogram shorter than the records' times ask for: the live records behind its end are keyed like the sentinel entries but keep
    their places in the list — in front of, between and behind the entries of the last coarse bin's bins."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    rec = records_in_bins(few_bins(65), 7)
    chans = configure(ctx, oracle, 2, rec)(rec)
    flat, nb, _ = oracle_histograms(oracle, chans, RATE, False)
    assert nb == 65
    hist = torch.zeros((2, 8, nbins), device="cuda", dtype=torch.float32)
    ctx.ir_accumulate_tensor(0.0, RATE, nbins, capi.IR_EXACT, hist)
    ctx.synchronize()
    assert_bits_equal_the_oracle(hist.cpu().numpy(), [f[:, :nbins] for f in flat], nbins, "%d of 65 bins" % nbins)


@pytest.mark.parametrize("count", SPEAKER_COUNTS)
def test_run_lengths_speaker_counts_and_fold_ranges_that_cut_coarse_bins(ctx, oracle, count):
    """Bins of 0, 1, 63, 64, 65 and 200 entries, runs of exactly 64 and 128, an empty coarse bin between two full ones (RUN_LENGTHS);
    one accumulate, then prepare + folds over ranges that start and end inside coarse bins, in any order."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    rec = records_in_bins(run_lengths(), 11, dead_every=0 if count == 3 else 4)
    chans = configure(ctx, oracle, count, rec)(rec)
    flat, nb, _ = oracle_histograms(oracle, chans, RATE, False)
    assert nb == 137
    assert_bits_equal_the_oracle(ctx.ir_download(False, RATE, capi.IR_EXACT), flat, nb, "%d speakers" % count)
    for ranges in (((0, 7), (7, 40), (40, nb)), ((97, nb), (0, 33), (33, 97))):
        hist = torch.zeros((count, 8, nb), device="cuda", dtype=torch.float32)
        fold_ranges(ctx, nb, ranges, hist)
        assert_bits_equal_the_oracle(hist.cpu().numpy(), flat, nb, "%d speakers, ranges %r" % (count, ranges))
    # a range alone leaves every other bin as it was
    hist = torch.full((count, 8, nb), 3.0, device="cuda", dtype=torch.float32)
    fold_ranges(ctx, nb, ((7, 40),), hist)
    got = hist.cpu().numpy()
    assert (got[:, :, :7] == 3.0).all() and (got[:, :, 40:] == 3.0).all() and (got[:, :, 7:40] != 3.0).any()


@pytest.mark.parametrize("count", (2, 6))
def test_a_second_fold_adds_on_top_of_the_first_ones_sums(ctx, oracle, count):
    """The chain of the multi-device fold: a second list folded on top of the first one's histogram is the serial sum over both."""
    import torch
    first, second = records_in_bins(run_lengths(), 21), records_in_bins(run_lengths(), 22)
    hist = torch.zeros((count, 8, 137), device="cuda", dtype=torch.float32)
    for rec in (first, second):
        attenuate = configure(ctx, oracle, count, rec)
        fold_ranges(ctx, 137, ((0, 40), (40, 137)), hist)
    both = np.concatenate([first, second])
    flat, nb, _ = oracle_histograms(oracle, attenuate(both), RATE, False)
    assert nb == 137
    assert_bits_equal_the_oracle(hist.cpu().numpy(), flat, nb, "%d speakers, two lists" % count)


def test_diffuse_impulses_and_images_in_one_list_with_dead_ones_between(ctx, oracle):
    """Values on both sides of ndiffuse: a trace with blocked shadow rays in the non-convex room, then constructed images."""
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = 241, 17
    mic, src = E.PAIRS[0]
    c = make_ctx()
    try:
        c.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
        diffuse = c.get_raw_diffuse()
        live = int(np.count_nonzero(diffuse["volume"].any(axis=1)))
        assert 0 < live < diffuse.shape[0]
        images = records_in_bins(run_lengths(), 31)
        everything = np.concatenate([diffuse, images])
        for count in (2, 4):
            attenuate = configure(c, oracle, count, images, capi.IR_ALL, mic)
            for rate, trim in ((RATE, False), (44100.0, True)):
                flat, nb, _ = oracle_histograms(oracle, attenuate(everything), rate, trim)
                assert_bits_equal_the_oracle(c.ir_download(trim, rate, capi.IR_EXACT), flat, nb, "%d speakers, %g Hz" % (count, rate))
            assert c.ir_exact_list_info() == (live + images.shape[0], live + int(np.count_nonzero(images["volume"].any(axis=1))), True)
    finally:
        c.close()


# ---- the forms that keep the list ordered by bin: a child process each -------------------------------------------------------------

CHILD_CASES = {"hrtf": "hrtf", "speakers_9": "speakers_9", "switch_off": "speakers_2"}


def child_records():
    return records_in_bins(run_lengths(), 41)


def child_main(case):
    """What a child process runs: the case's histogram at 8192 Hz, untrimmed, as one CRC line."""
    from parallel_reverb_raytracer_amd import capi
    from test_gpu_live_list import configure as configure_model
    c = make_ctx()
    configure_model(c, None, CHILD_CASES[case], child_records(), scenes.hrtf_synthetic_table())
    hist = c.ir_download(False, RATE, capi.IR_EXACT)
    print("CRC", case, hist.shape[2], zlib.crc32(np.ascontiguousarray(hist).tobytes()))
    c.close()


@pytest.mark.parametrize("case", list(CHILD_CASES))
def test_hrtf_more_than_8_speakers_and_the_switch_give_the_bytes_they_gave(oracle, case):
    """The HRTF fold, the wide fold and RVB_EXACT_COARSE=0 (read once per process) sort on the whole key as before: the child's
    histogram is the oracle's."""
    rec, model = child_records(), TIME_MODELS[CHILD_CASES[case]]
    if "hrtf" in model:
        table = scenes.hrtf_synthetic_table()
        chans = [oracle.attenuate_hrtf(model["mic"], rec, table[ear], model["hrtf"][0], model["hrtf"][1], ear) for ear in (0, 1)]
    else:
        chans = [oracle.attenuate_speaker(model["mic"], rec, d, k) for d, k in model["speakers"]]
    flat, nb, _ = oracle_histograms(oracle, chans, RATE, False)
    want = zlib.crc32(padded(flat, nb).tobytes())
    env = dict(os.environ)
    env.pop("RVB_EXACT_COARSE", None)
    if case == "switch_off":
        env["RVB_EXACT_COARSE"] = "0"
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import rvb_import; rvb_import.load();"
            "import test_gpu_exact_coarse as t; t.child_main(%r)") % (os.path.dirname(TESTS), TESTS, case)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l.split() for l in out.stdout.splitlines() if l.startswith("CRC ")]
    assert lines == [["CRC", case, str(nb), str(want)]], (lines, nb, want)
