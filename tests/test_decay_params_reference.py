"""The reference of the room acoustic parameters (tests/decay_params_reference.py) against itself and against closed forms, on the CPU:
its adjoint against central differences of its own loss, and the seven parameters of an exponential decay."""
import numpy as np
import pytest

import decay_params_reference as pref
import decay_reference as dref
from test_gpu_decay import histogram

NROWS, NBINS, FS = 3, 400, 2000.0          # k50 = 100, k80 = 160; the rows fall by 60 dB over their length
STEP = 1e-6                                # central, relative to the row's largest |H|: a step relative to a tiny H_j itself (1e-12 and less)
                                           # leaves nothing of the difference of two losses in binary64


def _inputs():
    h = histogram(NROWS, NBINS, 77).astype(np.float64)
    q, _ = pref.params(dref.curve(h), FS)
    assert np.isfinite(q).all()
    targets = q * (1.0 + 0.2 * np.random.default_rng(3).standard_normal(q.shape))
    return h, q, targets


@pytest.mark.parametrize("which", list(range(pref.NPARAMS)) + [None], ids=["EDT", "T20", "T30", "C50", "C80", "D50", "Ts", "all"])
def test_the_adjoint_against_central_differences(which):
    """w = dL/dH of the reference against (L(H + d e_j) - L(H - d e_j)) / 2d, d = 1e-6 max |H_row|, for every non-zero H_j of 3 x 400; one
    parameter at a time and all seven weighted with 1 / q^2.  Bar: 1e-5 of max |w|."""
    h, q, targets = _inputs()
    weights = 1.0 / (q * q)
    if which is not None:
        keep = np.zeros(pref.NPARAMS)
        keep[which] = 1.0
        weights = weights * keep[None, :]
    w = pref.loss(h, dref.curve(h), FS, targets, weights)["w"]
    assert np.abs(w).max() > 0 and (w[h == 0] == 0).all()
    worst = 0.0
    for r in range(NROWS):
        def value(row):
            return pref.row_loss(dref.curve(row[None, :])[0], FS, targets[r], weights[r], adjoint=False)["loss"]
        for j in np.flatnonzero(h[r]):
            d = STEP * np.abs(h[r]).max()
            up, down = h[r].copy(), h[r].copy()
            up[j] += d
            down[j] -= d
            worst = max(worst, abs((value(up) - value(down)) / (2.0 * d) - w[r, j]))
    print("decay params adjoint (%s): max |fd - w| / max |w| = %.3g" % (which, worst / np.abs(w).max()))
    assert worst <= 1e-5 * np.abs(w).max()


def test_closed_forms_of_an_exponential_decay():
    """H[k] = exp(-a k) on a long row: T = 3 ln 10 / (a fs), C_te = 10 log10(exp(2 a ke) - 1), D50 = 1 - exp(-2 a k50),
    Ts -> 1 / (fs (exp(2a) - 1))."""
    a, fs, nbins = 0.004, 8000.0, 20000                  # exp(-2 a nbins) = exp(-160): the row's end leaves no trace
    e = dref.curve(np.exp(-a * np.arange(nbins))[None, :])
    q, dq = pref.params(e, fs)
    q, dq = q[0], dq[0]
    k50, k80 = pref.bin_of(0.05, fs, nbins), pref.bin_of(0.08, fs, nbins)
    assert (k50, k80) == (400, 640)
    want = np.array([3.0 * np.log(10.0) / (a * fs)] * 3 + [10.0 * np.log10(np.exp(2 * a * k50) - 1.0), 10.0 * np.log10(np.exp(2 * a * k80) - 1.0),
                     1.0 - np.exp(-2 * a * k50), 1.0 / (fs * (np.exp(2 * a) - 1.0))])
    print("decay params of exp(-a k):", q, "closed forms:", want)
    assert (np.abs(q - want) <= 1e-9 * np.abs(want)).all()
    assert (dq <= 1e-9 * np.abs(q)).all()                # the bars of a well-conditioned row are far below float precision


def test_what_is_not_available():
    """E[0] == 0: all NaN.  A row shorter than 50 ms: C and D50 NaN, Ts finite; one bin: Ts == 0.  late == 0: C NaN, D50 == 1."""
    q, _ = pref.params(np.zeros((1, 50)), 1000.0)
    assert np.isnan(q).all()
    q, _ = pref.params(dref.curve(np.exp(-0.2 * np.arange(40))[None, :]), 1000.0)
    assert np.isnan(q[0, [pref.C50, pref.C80, pref.D50]]).all() and np.isfinite(q[0, [pref.EDT, pref.T20, pref.T30, pref.TS]]).all()
    q, _ = pref.params(np.ones((1, 1)), 1000.0)
    assert q[0, pref.TS] == 0 and np.isnan(q[0, :pref.TS]).all()
    h = np.zeros((1, 100))
    h[0, :30] = 1.0
    q, _ = pref.params(dref.curve(h), 1000.0)
    assert np.isnan(q[0, pref.C50]) and q[0, pref.D50] == 1.0
