"""The numpy reference of the decay calls (tests/decay_reference.py) against things it does not contain: central finite differences of
its own loss for the adjoint, and the closed form of an exponential decay for the reverberation time."""
import numpy as np
import pytest

import decay_reference as ref


def inputs(seed=3, nrows=3, nbins=200):
    """3 x 200: a full row, a row whose tail is zero from bin 120 on, an all-zero row; the target is another decay."""
    rng = np.random.default_rng(seed)
    k = np.arange(nbins)
    h = rng.standard_normal((nrows, nbins)) * np.exp(-0.03 * k)[None, :]
    h[rng.random(h.shape) < 0.35] = 0.0
    h[1, 120:] = 0.0
    h[2] = 0.0
    t = ref.curve(rng.standard_normal((nrows, nbins)) * np.exp(-0.025 * k)[None, :])
    m = ref.mask_of(t).astype(np.float64)
    m[0] *= 0.5                                   # a mask is any weight >= 0
    return h, t, m


def total(h, t, m, normalised):
    return float(ref.loss(h, ref.curve(h), t, m, normalised)["loss_rows"].sum())


@pytest.mark.parametrize("normalised", [False, True])
def test_the_adjoint_equals_central_differences_of_the_loss(normalised):
    h, t, m = inputs()
    out = ref.loss(h, ref.curve(h), t, m, normalised)
    w = out["w"]
    assert out["loss_rows"][0] > 0 and out["loss_rows"][1] > 0 and out["loss_rows"][2] == 0
    assert not w[2].any() and not w[h == 0].any() and w[0].any() and w[1].any()
    scale = np.abs(w).max()
    worst = 0.0
    for r in range(h.shape[0]):
        for j in range(h.shape[1]):
            step = 1e-5 * max(abs(h[r, j]), 1e-3 * np.abs(h[r]).max(), 1e-12)
            hp, hm = h.copy(), h.copy()
            hp[r, j] += step
            hm[r, j] -= step
            fd = (total(hp, t, m, normalised) - total(hm, t, m, normalised)) / (2 * step)
            worst = max(worst, abs(fd - w[r, j]) / scale)
    print("decay reference, normalised=%s: max |fd - w| / max |w| = %.3g" % (normalised, worst))
    assert worst < 1e-6


def test_a_row_that_does_not_count_under_the_flag():
    """T[r][0] == 0 for row 0: with the flag the row has loss 0 and no weights; without it the row counts wherever T > 0."""
    h, t, m = inputs()
    t = t.copy()
    t[0, 0] = 0.0
    e = ref.curve(h)
    flagged, plain = ref.loss(h, e, t, m, True), ref.loss(h, e, t, m, False)
    assert flagged["loss_rows"][0] == 0 and not flagged["w"][0].any() and not flagged["rows"][0]
    assert plain["loss_rows"][0] > 0 and plain["w"][0].any()


def test_the_time_of_an_exponential_decay():
    """H[k] = exp(-a k): the level falls by 20 a / ln 10 dB per bin, so T60 = 3 ln 10 / (a sample_rate) — 0.6907755 s at a = 0.01, 1 kHz."""
    a, rate = 0.01, 1000.0
    h = np.exp(-a * np.arange(6000))[None, :]
    e = ref.curve(h)
    want = 3.0 * np.log(10.0) / (a * rate)
    assert abs(want - 0.6907755) < 1e-7
    for db_begin, db_end in ((-5.0, -35.0), (0.0, -10.0), (-5.0, -25.0)):
        seconds, rel = ref.times(e, rate, db_begin, db_end)
        assert abs(seconds[0] - want) <= 1e-9, (db_begin, db_end, seconds[0])
        assert 0 < rel[0] < 1e-9


def test_times_that_are_not_available():
    k = np.arange(400)
    h = np.exp(-0.05 * k)[None, :].repeat(4, axis=0)
    h[0] = 0.0                                    # E[0] == 0
    h[1, 60:] = 0.0                               # the last positive bin lies above -35 dB, but a bin with E = 0 is below every level
    h[2, 1:] = 0.0                                # a window of one bin: E[1] = 0 is below every level
    e = ref.curve(h)
    seconds, _ = ref.times(e, 1000.0, -5.0, -35.0)
    assert np.isnan(seconds[0]) and np.isnan(seconds[2]) and np.isfinite(seconds[3])
    assert np.isfinite(seconds[1])                # zeros behind the truncation count as below: the window closes there
    cut = ref.curve(np.exp(-0.05 * k)[None, :])[:, :50]     # a curve CUT at 50 bins (-21.7 dB): never below -35 dB inside nbins
    assert np.isnan(ref.times(cut, 1000.0, -5.0, -35.0)[0][0])
    assert ref.window(e[3], -5.0, -35.0) == (int(np.flatnonzero(e[3] <= e[3, 0] * ref.ratio(-5.0))[0]), int(np.flatnonzero(e[3] < e[3, 0] * ref.ratio(-35.0))[0]))
