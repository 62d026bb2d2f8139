"""tests/speech_reference.py on its own (no GPU, no library): closed forms of the modulation transfer function, the analytic adjoint and
dSTI/dm against central differences of the reference itself, and the GROUND conditions of tests/test_gpu_speech.py — that its bars pin
the kernels to something: the bar of m stays at or below 2^-28 in every case, and in the two ground cases at least 90 % of the non-zero
weights have c_j <= 2^-26 |w_ref|, so the weights test holds them to float precision and not to a cancellation allowance."""
import numpy as np
import pytest

import speech_cases as cases
import speech_reference as ref

FS = 51200.0


@pytest.mark.parametrize("seconds", [0.3, 1.0, 2.5, 6.0])
def test_an_exponential_decay_has_the_closed_form(seconds):
    """H_j^2 = exp(-13.8155 j / (fs T)), cut at 3 T: m(F) = 1 / sqrt(1 + (2 pi F T / 13.8155)^2) within 1e-6 — the discretisation, the cut
    and the float32 row, not a kernel tolerance (measured with a prototype: 5e-8)."""
    h = cases.spike_rows(FS, seconds)[2:3]
    assert h.shape[1] == int(round(3 * seconds * FS))
    got = ref.mtf(h, FS, ref.STI_FREQS)["m"][0]
    miss = np.abs(got - cases.exponential_mtf(ref.STI_FREQS, seconds)).max()
    print("exponential row, T = %g s: largest difference %.3e" % (seconds, miss))
    assert miss <= 1e-6


def test_a_spike_has_m_one_and_two_spikes_the_cosine():
    h = cases.spike_rows(FS)[:2]
    fw = ref.mtf(h, FS, ref.STI_FREQS)
    assert (np.abs(fw["m"][0] - 1.0) <= fw["m_bar"][0]).all()
    assert (np.abs(fw["m"][1] - np.abs(np.cos(np.pi * np.asarray(ref.STI_FREQS) * 0.4))) <= fw["m_bar"][1]).all()
    assert fw["sums"][0, 0] == 9.0 and fw["sums"][1, 0] == 0.125


def test_an_empty_row_is_nan_with_zero_weights():
    h = np.zeros((2, 50), np.float32)
    h[1, 3] = 1.0
    fw = ref.mtf(h, 100.0, (0.63, 2.0))
    assert np.isnan(fw["m"][0]).all() and np.isfinite(fw["m"][1]).all()
    w, c = ref.adjoint(h, 100.0, (0.63, 2.0), np.ones((2, 2)), fw)
    assert not w[0].any() and not c[0].any()


def test_the_adjoint_is_the_derivative_of_the_reference():
    """L = sum_i c_i m_i on a float64 row of 40 bins: dL/dH_j by central differences against the analytic w, to 1e-7 of the largest."""
    rng = np.random.default_rng(4)
    fs, freqs = 100.0, (0.63, 2.0, 12.5)
    h = rng.standard_normal((2, 40)) * np.exp(-0.05 * np.arange(40))
    coeffs = rng.standard_normal((2, 3))
    w, _ = ref.adjoint(h, fs, freqs, coeffs)

    def loss(x):
        return float((coeffs * ref.mtf(x, fs, freqs)["m_ld"]).sum())

    step = 1e-6
    for r, j in ((0, 0), (0, 7), (1, 13), (1, 39)):
        up, down = h.copy(), h.copy()
        up[r, j] += step
        down[r, j] -= step
        numeric = (loss(up) - loss(down)) / (2 * step)
        assert abs(numeric - w[r, j]) <= 1e-7 * np.abs(w).max(), (r, j, numeric, w[r, j])


def test_the_index_derivative_is_the_derivative_of_the_reference():
    rng = np.random.default_rng(5)
    m = rng.uniform(0.1, 0.9, (7, 14))
    snr = np.array([20.0, 15.0, 10.0, np.inf, 5.0, 25.0, 30.0])
    for snr_db in (None, snr):
        sti, mti, derivative, _ = ref.speech_index(m, ref.ALPHA_MALE, ref.BETA_MALE, snr_db)
        assert 0.0 < sti < 1.0 and mti.shape == (7,)
        step = 1e-6
        for k, i in ((0, 0), (3, 5), (6, 13), (2, 9)):
            up, down = m.copy(), m.copy()
            up[k, i] += step
            down[k, i] -= step
            numeric = (ref.speech_index(up, ref.ALPHA_MALE, ref.BETA_MALE, snr_db)[0] - ref.speech_index(down, ref.ALPHA_MALE, ref.BETA_MALE, snr_db)[0]) / (2 * step)
            assert abs(numeric - derivative[k, i]) <= 1e-8, (k, i, numeric, derivative[k, i])


def test_the_index_of_its_edges():
    """All ones: every TI is 1 and STI = sum alpha - sum beta = 1; all zeros: 0; a clipped entry has no derivative; a NaN gives NaN."""
    assert abs(sum(ref.ALPHA_MALE) - sum(ref.BETA_MALE) - 1.0) < 1e-12
    assert abs(ref.speech_index(np.ones((7, 14)), ref.ALPHA_MALE, ref.BETA_MALE)[0] - 1.0) < 1e-12
    sti, mti, derivative, _ = ref.speech_index(np.zeros((7, 14)), ref.ALPHA_MALE, ref.BETA_MALE)
    assert sti == 0.0 and not mti.any() and not derivative.any()
    m = np.full((7, 14), 0.5)
    m[2, 3], m[4, 4] = 0.99, 0.01                                # beyond +-15 dB
    _, _, derivative, _ = ref.speech_index(m, ref.ALPHA_MALE, ref.BETA_MALE)
    assert derivative[2, 3] == 0.0 and derivative[4, 4] == 0.0 and (np.delete(derivative.reshape(-1), [2 * 14 + 3, 4 * 14 + 4]) > 0).all()
    m[1, 1] = np.nan
    assert np.isnan(ref.speech_index(m, ref.ALPHA_MALE, ref.BETA_MALE)[0])


def test_ground_the_bar_of_m_is_at_most_2_to_the_minus_28_in_every_case():
    for (nrows, nbins, fs), freqs in [(c, cases.FREQS) for c in cases.CASES] + cases.EXTRA_FREQS + [((3, cases.spike_rows().shape[1], FS), cases.FREQS)]:
        eps0 = (nbins + 16) * 2.0 ** -52
        bar = 1.5 * (eps0 + ref.tau(freqs, nbins, fs)) + eps0 + 2.0 ** -49          # (m <= 1)
        assert bar.max() <= 2.0 ** -28, (nrows, nbins, fs)


@pytest.mark.parametrize("nrows,nbins,fs", cases.GROUND_CASES)
def test_ground_the_weights_are_pinned_to_float_precision(nrows, nbins, fs):
    r = cases.reference(nrows, nbins, fs)
    assert (r["fw"]["m_bar"] <= 2.0 ** -28).all()
    nonzero = r["w"] != 0
    share = float((r["c"][nonzero] <= 2.0 ** -26 * np.abs(r["w"][nonzero])).mean())
    print("ground %d x %d at %g Hz: %d non-zero weights, share with c_j <= 2^-26 |w| = %.4f" % (nrows, nbins, fs, nonzero.sum(), share))
    assert nonzero.sum() > 0.4 * nrows * nbins and share >= 0.9
