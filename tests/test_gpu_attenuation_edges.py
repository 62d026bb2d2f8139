"""The stages behind the trace — attenuate_kernel, time_range_kernel, bin_keys_*, ordered_sum_*, histogram_fast_kernel, flat_keys_kernel —
on the constructed edge inputs of tests/attenuation_edges.py, against the CPU oracle's chain attenuate -> findPredelay / fixPredelay ->
flattenImpulses (tests/test_attenuation_edge_inputs.py shows, without a GPU, that these inputs hold the edges they are built for).

Bars: materialised attenuation and RVB_IR_EXACT histograms bit for bit the oracle's; RVB_IR_FAST within the re-ordered-sum bound of
tests/test_gpu_speaker_arrays.py (fast_bound).

The records enter the fused stage as image sources (RVB_IR_IMAGES) of a context that holds a one-ray, one-bounce trace, because
rvb_ir_configure_* needs a trace."""
import os

import numpy as np
import pytest

import attenuation_edges as ae
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS
from test_gpu_speaker_arrays import fast_bound

pytestmark = pytest.mark.gpu

FRAMES = {"canonical": ae.CANONICAL, "oblique": ae.OBLIQUE}
SWITCHES = ("RVB_HRTF_EXACT_ROWS", "RVB_HRTF_SPLIT_EARS")
PREFIXES = (1, 3, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def ctx():
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    scene, info = scenes.cathedral(3000)
    c.set_scene(scene)
    c.raytrace(info["mic"], info["source"], scenes.sphere_directions(1, seed=23), 1, AIR_COEFFICIENTS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def boundary(oracle):
    """Per frame, computed once and left unchanged: the boundary records and the oracle's attenuated channels under the row-code table."""
    table = ae.row_code_table()
    out = {}
    for name, fr in FRAMES.items():
        rec, b, names = ae.boundary_set(fr)
        chans = [oracle.attenuate_hrtf(fr["mic"], rec, table[ear], fr["facing"], fr["up"], ear) for ear in (0, 1)]
        out[name] = {"rec": rec, "b": b, "names": names, "chans": chans}
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def oracle_histograms(oracle, chans, sr, trim=False, predelay=None):
    """findPredelay / fixPredelay (or a caller-given predelay) and flattenImpulses on COPIES of the attenuated channels."""
    chans = [c.copy() for c in chans]
    if predelay is None and trim:
        predelay = oracle.find_predelay(chans)
    if predelay is not None:
        for c in chans:
            oracle.fix_predelay(c, predelay)
    flat = [oracle.flatten(c, sr) for c in chans]
    return flat, max(f.shape[1] for f in flat), chans


def assert_equals_oracle(got, flat, nb, what):
    assert got.shape == (len(flat), 8, nb), (what, got.shape, nb)
    for ch, f in enumerate(flat):
        n = f.shape[1]                        # the reference bins every channel on its own maxtime
        if not np.array_equal(got[ch][:, :n], f):
            band, bin_ = np.argwhere(got[ch][:, :n] != f)[0]
            raise AssertionError("%s: channel %d band %d bin %d: got %r, the oracle has %r (%d band-bins differ)"
                                 % (what, ch, band, bin_, got[ch][band, bin_], f[band, bin_], np.count_nonzero(got[ch][:, :n] != f)))
        assert not got[ch][:, n:].any(), what


def padded(flat, nb):
    out = np.zeros((len(flat), 8, nb), np.float32)
    for ch, f in enumerate(flat):
        out[ch][:, :f.shape[1]] = f
    return out


class switches:
    """RVB_HRTF_EXACT_ROWS / RVB_HRTF_SPLIT_EARS for the calls inside (the library reads them per call); the environment is restored."""

    def __init__(self, **on):
        self.on = on

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        for k in self.on:
            assert k in SWITCHES
            os.environ[k] = "1"

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- HRTF rows ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", list(FRAMES))
def test_materialised_hrtf_rows_equal_the_oracle(ctx, boundary, frame):
    """attenuate_kernel<true>: hrtf_row_quad over four-lane quads."""
    fr, s = FRAMES[frame], boundary[frame]
    table = ae.row_code_table()
    for ear in (0, 1):
        want = s["chans"][ear]
        got = ctx.attenuate_hrtf(fr["mic"], s["rec"], table[ear], fr["facing"], fr["up"], ear)
        bad = np.flatnonzero((bits(got["volume"]) != bits(want["volume"])).any(axis=1))
        if bad.size:
            az, el = ae.listener_angles(fr["facing"], fr["up"], fr["mic"], s["rec"]["position"][:, :3])
            rows_want, rows_got = ae.rows_from_codes(want["volume"]), ae.rows_from_codes(got["volume"])
            raise AssertionError("%d records of ear %d got another table row; the first: %s" % (bad.size, ear, "; ".join(
                "%s (binary64 az %.7f, el %.7f): row %d expected, got %d" % (ae.describe(s["b"], s["names"], i), az[i], el[i], rows_want[i], rows_got[i])
                for i in bad[:8])))
        assert np.array_equal(bits(got["time"]), bits(want["time"])), (frame, ear)
        assert not got["pad"].any()


@pytest.mark.parametrize("frame", list(FRAMES))
def test_fused_exact_hrtf_rows_equal_the_oracle_in_all_three_evaluations(ctx, oracle, boundary, frame):
    """ordered_sum_hrtf_kernel (hrtf_row_quad over lane pairs, inside a loop with a data-dependent exit), ordered_sum_kernel<true, 1>
    (hrtf_row, one lane: RVB_HRTF_SPLIT_EARS=1) and the always-binary64 rows (RVB_HRTF_EXACT_ROWS=1): nearly one record per bin, so a
    wrong row of one record is a wrong bin; time_range_kernel gives the oracle's earliest and latest attenuated time."""
    from parallel_reverb_raytracer_amd import capi
    fr, s = FRAMES[frame], boundary[frame]
    table = ae.row_code_table()
    both = np.concatenate([c["time"] for c in s["chans"]])
    want_range = (both[both != 0].min(), both.max())
    for trim in (False, True):
        flat, nb, _ = oracle_histograms(oracle, s["chans"], 44100.0, trim)
        for name, on in (("default", {}), ("split ears", {"RVB_HRTF_SPLIT_EARS": "1"}), ("exact rows", {"RVB_HRTF_EXACT_ROWS": "1"})):
            with switches(**on):
                ctx.ir_configure_hrtf(fr["mic"], table, fr["facing"], fr["up"], capi.IR_IMAGES, s["rec"])
                lo, hi = ctx.ir_time_range()
                got = ctx.ir_download(trim, 44100.0, capi.IR_EXACT)
            assert (np.float32(lo), np.float32(hi)) == want_range, (frame, name)
            assert_equals_oracle(got, flat, nb, "%s frame, %s, trim %s" % (frame, name, trim))


@pytest.mark.parametrize("frame", list(FRAMES))
def test_fused_fast_hrtf_rows_within_the_bound_under_a_table_that_separates_neighbours(ctx, oracle, frame):
    """histogram_fast_kernel (hrtf_row, one lane per record) with spread_table(): a neighbouring row moves a bin by more than four
    times the bound (tests/test_attenuation_edge_inputs.py)."""
    from parallel_reverb_raytracer_amd import capi
    fr = FRAMES[frame]
    rec, _, _ = ae.boundary_set(fr)
    table = ae.spread_table()
    chans = [oracle.attenuate_hrtf(fr["mic"], rec, table[ear], fr["facing"], fr["up"], ear) for ear in (0, 1)]
    flat, nb, fixed = oracle_histograms(oracle, chans, 44100.0, True)
    exact = padded(flat, nb)
    ctx.ir_configure_hrtf(fr["mic"], table, fr["facing"], fr["up"], capi.IR_IMAGES, rec)
    fast = ctx.ir_download(True, 44100.0, capi.IR_FAST)
    assert fast.shape == exact.shape and fast.any()
    excess = np.abs(fast.astype(np.float64) - exact) - fast_bound(exact, fixed, 44100.0)
    assert (excess <= 0).all(), (frame, np.count_nonzero(excess > 0), np.argwhere(excess > 0)[:5].tolist())


# ---- time edges -----------------------------------------------------------------------------------------------------------------

TIME_MODELS = {
    "speakers_2": {"mic": (1.0, 1.5, -2.0), "speakers": ae.EDGE_SPEAKERS[5:7]},
    "speakers_9": {"mic": (1.0, 1.5, -2.0), "speakers": ae.EDGE_SPEAKERS},          # more than eight channels: ordered_sum_wide_kernel
    "hrtf": {"mic": ae.OBLIQUE["mic"], "hrtf": (ae.OBLIQUE["facing"], ae.OBLIQUE["up"])},
}


def time_model(ctx, oracle, model, rec):
    """Configures the fused stage for `rec`; returns the oracle's attenuated channels."""
    from parallel_reverb_raytracer_amd import capi
    m = TIME_MODELS[model]
    if "hrtf" in m:
        table = scenes.hrtf_synthetic_table()
        ctx.ir_configure_hrtf(m["mic"], table, m["hrtf"][0], m["hrtf"][1], capi.IR_IMAGES, rec)
        return [oracle.attenuate_hrtf(m["mic"], rec, table[ear], m["hrtf"][0], m["hrtf"][1], ear) for ear in (0, 1)]
    ctx.ir_configure_speakers(m["mic"], [d for d, _ in m["speakers"]], [k for _, k in m["speakers"]], capi.IR_IMAGES, rec)
    return [oracle.attenuate_speaker(m["mic"], rec, d, k) for d, k in m["speakers"]]


@pytest.mark.parametrize("model", list(TIME_MODELS))
def test_time_edges_half_bins_predelay_and_run_lengths_equal_the_oracle(ctx, oracle, model):
    import torch
    from parallel_reverb_raytracer_amd import capi
    mic = TIME_MODELS[model]["mic"]
    for sr in (44100.0, 8192.0):              # at the power-of-two rate (k + 0.5) / sr is exact: every k is a half bin
        rec, _ = ae.time_edge_records(sr, mic)
        for n in (PREFIXES if sr == 44100.0 else ()) + (rec.shape[0],):
            chans = time_model(ctx, oracle, model, rec[:n])
            for trim in (False, True):
                flat, nb, _ = oracle_histograms(oracle, chans, sr, trim)
                assert_equals_oracle(ctx.ir_download(trim, sr, capi.IR_EXACT), flat, nb, "%s, %g Hz, %d records, trim %s" % (model, sr, n, trim))
        # (the whole set stays configured) fast mode, predelay trimmed
        flat, nb, fixed = oracle_histograms(oracle, chans, sr, True)
        exact = padded(flat, nb)
        fast = ctx.ir_download(True, sr, capi.IR_FAST)
        assert fast.shape == exact.shape
        assert (np.abs(fast.astype(np.float64) - exact) <= fast_bound(exact, fixed, sr)).all(), (model, sr)
        # a caller-given predelay above the earliest 50 records, equal to the 51st: all of them land in bin 0
        times = np.unique(np.concatenate([c["time"] for c in chans]))
        predelay = float(times[times != 0][50])
        flat, nb, fixed = oracle_histograms(oracle, chans, sr, predelay=predelay)
        assert sum(np.count_nonzero((c["time"] == 0) & c["volume"].any(axis=1)) for c in fixed) >= 50
        lo, hi = ctx.ir_time_range()
        assert lo < predelay < hi and ctx.ir_bins(hi, predelay, sr) == nb
        hist = torch.zeros((len(chans), 8, nb), device="cuda", dtype=torch.float32)
        ctx.ir_accumulate_tensor(predelay, sr, nb, capi.IR_EXACT, hist)
        ctx.synchronize()
        assert_equals_oracle(hist.cpu().numpy(), flat, nb, "%s, %g Hz, caller-given predelay" % (model, sr))
        # flattenImpulses on the oracle's attenuated channel (flat_keys_kernel, flat_ordered_sum_kernel), prefixes included
        for att in (chans[-1], fixed[0]):
            for n in PREFIXES + (att.shape[0],):
                want = oracle.flatten(att[:n], sr)
                got = ctx.flatten(att[:n], sr)
                assert got.shape == want.shape and np.array_equal(got, want), (model, sr, n)


# ---- speaker edges --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mic", [(0.0, 0.0, 0.0), (1.0, 1.5, -2.0)], ids=["mic_at_origin", "mic_off_origin"])
def test_speaker_gain_edges_equal_the_oracle(ctx, oracle, mic):
    """Degenerate normalisations (length3 underflows to 0 or overflows), gains that cancel to exactly 0, -0.0 and subnormal volumes:
    attenuate_kernel<false> per speaker, then the fused exact path with 3 channels (ordered_sum_kernel<false, 3>) and with 9
    (ordered_sum_wide_kernel), and the fast path with 3."""
    from parallel_reverb_raytracer_amd import capi
    rec, names = ae.speaker_edge_records(mic)
    silent = ~(rec["volume"] != 0).any(axis=1)                   # all-zero and all -0.0 volumes (quirk Q2)
    assert 40 < np.count_nonzero(silent) < 60
    chans = []
    for direction, k in ae.EDGE_SPEAKERS:
        want = oracle.attenuate_speaker(mic, rec, direction, k)
        got = ctx.attenuate_speaker(mic, rec, direction, k)
        assert not got["volume"][silent].any() and not got["time"][silent].any()
        assert not bits(got["volume"][silent]).any(), "a silent record attenuates to +0"
        bad = np.flatnonzero(~silent & ((bits(got["volume"]) != bits(want["volume"])).any(axis=1) | (bits(got["time"]) != bits(want["time"]))))
        assert bad.size == 0, [(direction, k, names[i], got["volume"][i].tolist(), want["volume"][i].tolist()) for i in bad[:4]]
        chans.append(want)
    for nch in (3, 9):
        sp = ae.EDGE_SPEAKERS[:nch]
        ctx.ir_configure_speakers(mic, [d for d, _ in sp], [k for _, k in sp], capi.IR_IMAGES, rec)
        for trim in (False, True):
            flat, nb, fixed = oracle_histograms(oracle, chans[:nch], 44100.0, trim)
            assert_equals_oracle(ctx.ir_download(trim, 44100.0, capi.IR_EXACT), flat, nb, "%d channels, trim %s" % (nch, trim))
        if nch == 3:
            exact = padded(flat, nb)
            fast = ctx.ir_download(True, 44100.0, capi.IR_FAST)
            assert fast.shape == exact.shape
            assert (np.abs(fast.astype(np.float64) - exact) <= fast_bound(exact, fixed, 44100.0)).all()
