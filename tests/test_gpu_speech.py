"""rvb_mtf and rvb_mtf_adjoint on the GPU (include/rvb_capi_speech.h; csrc/speech_kernels.hip) against the extended-precision numpy
reference of tests/speech_reference.py, on the histograms of tests/test_gpu_decay.py (tests/speech_cases.py holds the shapes, the
seeded coefficients and the reference of each case, computed once).

THE BARS are derived in speech_reference.py from the formulas and the formats, never from what the kernels return:
  sums     |gpu - ref| <= ((nbins + 16) 2^-52 + tau_i) S for A_i and B_i, (nbins + 16) 2^-52 S for S
  m        |gpu - ref| <= 1.5 eps_i + m eps0 + 2^-49; NaN exactly where the reference has it (the all-zero rows)
  weights  |gpu - ref| <= 2^-23 |w_ref| + c_j
GROUND (tests/test_speech_reference.py, on the reference alone): the bar of m is at most 2^-28 in every case here, and at 16 x (2T + 65)
and 8 x (T - 1) at least 90 % of the non-zero weights have c_j <= 2^-26 |w_ref|.  At 2 x (130 T + 5) that share is lower (about 0.75 with
a crude bar): the case runs — the fold's wave takes three rounds there — but is not a ground case."""
import ctypes

import numpy as np
import pytest

import speech_cases as cases
import speech_reference as ref
from test_gpu_decay import T, dev

pytestmark = pytest.mark.gpu

SUMS_NAMES = ["mtf_sums_kernel", "mtf_fold_kernel"]
ADJOINT_NAMES = SUMS_NAMES + ["mtf_adjoint_kernel"]


@pytest.fixture(scope="module")
def ctx():
    from parallel_reverb_raytracer_amd import capi
    assert capi.DECAY_TILE == T
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    yield c
    c.close()


def names_of(ctx):
    return [k for k, _ in ctx.last_timings()]


def run_adjoint(ctx, h_dev, nrows, nbins, fs, freqs, coeffs):
    import torch
    out = torch.full((nrows, nbins), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.mtf_adjoint(h_dev.data_ptr(), nrows, nbins, fs, freqs, coeffs, out.data_ptr())
    return out.cpu().numpy()


def check(ctx, h, fs, freqs, fw, coeffs, w_ref, c_bar, label):
    """Every assertion of a case; returns the device's m."""
    nrows, nbins = h.shape
    h_dev = dev(h)
    m, sums = ctx.mtf(h_dev.data_ptr(), nrows, nbins, fs, freqs, want_sums=True)
    assert names_of(ctx) == SUMS_NAMES
    m_again, sums_again = ctx.mtf(h_dev.data_ptr(), nrows, nbins, fs, freqs, want_sums=True)
    assert m.tobytes() == m_again.tobytes() and sums.tobytes() == sums_again.tobytes()                 # bit for bit
    assert ctx.mtf(h_dev.data_ptr(), nrows, nbins, fs, freqs).tobytes() == m.tobytes()                 # (sums == NULL)
    empty = ~h.any(axis=1)
    assert (np.isnan(m) == np.isnan(fw["m"])).all() and (np.isnan(m).all(axis=1) == empty).all()
    full = ~empty
    miss_sums = np.abs(sums - fw["sums"])
    miss_m = np.abs(m[full] - fw["m"][full])
    print("%s: sums at most %.3f of their bar, m at most %.3f of its bar (largest difference %.3e)"
          % (label, float(np.max(miss_sums[full] / fw["sums_bar"][full], initial=0.0)), float(np.max(miss_m / fw["m_bar"][full], initial=0.0)),
             float(np.max(miss_m, initial=0.0))))
    assert (miss_sums <= fw["sums_bar"]).all() and not sums[empty].any()
    assert (miss_m <= fw["m_bar"][full]).all()

    w = run_adjoint(ctx, h_dev, nrows, nbins, fs, freqs, coeffs)
    assert names_of(ctx) == ADJOINT_NAMES
    assert run_adjoint(ctx, h_dev, nrows, nbins, fs, freqs, coeffs).tobytes() == w.tobytes()           # bit for bit
    assert not (w == 7.0).any() and np.isfinite(w).all()                                               # no entry left unwritten
    assert not w[h == 0].any() and not w[empty].any()                                                  # exactly 0 where H is 0
    miss_w = np.abs(w.astype(np.float64) - w_ref)
    allowed = 2.0 ** -23 * np.abs(w_ref) + c_bar
    nonzero = w_ref != 0
    print("%s: weights at most %.3f of their bar; largest relative difference where c_j <= 2^-26 |w_ref|: %.3e"
          % (label, float(np.max(miss_w[nonzero] / allowed[nonzero], initial=0.0)),
             float(np.max((miss_w / np.where(nonzero, np.abs(w_ref), 1.0))[nonzero & (c_bar <= 2.0 ** -26 * np.abs(w_ref))], initial=0.0))))
    assert (miss_w <= allowed).all()
    assert h_dev.cpu().numpy().tobytes() == h.tobytes()                                                # H unchanged
    return m


@pytest.mark.parametrize("nrows,nbins,fs", cases.CASES)
def test_mtf_and_adjoint(ctx, nrows, nbins, fs):
    r = cases.reference(nrows, nbins, fs)
    check(ctx, r["h"], fs, cases.FREQS, r["fw"], r["coeffs"], r["w"], r["c"], "%d x %d at %g Hz" % (nrows, nbins, fs))
    if nrows >= 4:
        assert not r["h"][2].any() and np.isnan(r["fw"]["m"][2]).all()                                 # the all-zero row took part


@pytest.mark.parametrize("shape,freqs", cases.EXTRA_FREQS, ids=["1 frequency", "16 frequencies"])
def test_other_frequency_counts(ctx, shape, freqs):
    """nfreqs 1 and RVB_MTF_MAX_FREQS; the bytes of a frequency's m do not depend on how many others the call computes."""
    nrows, nbins, fs = shape
    r = cases.reference(nrows, nbins, fs, freqs)
    m = check(ctx, r["h"], fs, freqs, r["fw"], r["coeffs"], r["w"], r["c"], "%d x %d, %d frequencies" % (nrows, nbins, len(freqs)))
    h_dev = dev(r["h"])
    standard = ctx.mtf(h_dev.data_ptr(), nrows, nbins, fs, cases.FREQS)
    shared = [i for i, f in enumerate(cases.FREQS) if f in freqs]
    assert shared and standard[:, shared].tobytes() == m[:, [freqs.index(cases.FREQS[i]) for i in shared]].tobytes()


def test_spikes_and_an_exponential_decay(ctx):
    """A single spike: m = 1; two equal spikes 0.4 s apart: |cos(pi F 0.4)|; H^2 = exp(-13.8155 t / T), T = 0.3 s, cut at 3 T: the closed
    form within 1e-6 (tests/test_speech_reference.py: the discretisation and the float32 row, not a kernel tolerance)."""
    fs = 51200.0
    h = cases.spike_rows(fs, 0.3)
    fw = ref.mtf(h, fs, cases.FREQS)
    coeffs = cases.coefficients(3, len(cases.FREQS))
    w_ref, c_bar = ref.adjoint(h, fs, cases.FREQS, coeffs, fw)
    m = check(ctx, h, fs, cases.FREQS, fw, coeffs, w_ref, c_bar, "spike rows")
    assert (np.abs(m[0] - 1.0) <= fw["m_bar"][0]).all()
    assert (np.abs(m[1] - np.abs(np.cos(np.pi * np.asarray(cases.FREQS) * 0.4))) <= 2 * fw["m_bar"][1]).all()      # (the reference's own bar too)
    assert np.abs(m[2] - cases.exponential_mtf(cases.FREQS, 0.3)).max() <= 1e-6


def test_refusals_write_nothing(ctx):
    """Every refusal of the header with its code and a text that names the condition; the host outputs and the weights keep their fill."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    nrows, nbins, fs = 4, 100, 51200.0
    h = torch.ones((nrows, nbins), dtype=torch.float32, device="cuda")
    w = torch.full((nrows, nbins), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    lib, handle = ctx.lib, ctx.handle
    out, sums = np.full((nrows, 16), 7.0), np.full((nrows, 33), 7.0)
    good_freqs, good_coeffs = np.array(cases.FREQS), np.ones((nrows, 14))

    def both(code, word, h_ptr=h.data_ptr(), rows=nrows, bins=nbins, rate=fs, freqs=good_freqs, nfreqs=14, only=None):
        f = freqs.ctypes.data if freqs is not None else None
        calls = {"rvb_mtf": lambda: lib.rvb_mtf(handle, h_ptr, rows, bins, rate, f, nfreqs, out.ctypes.data, sums.ctypes.data),
                 "rvb_mtf_adjoint": lambda: lib.rvb_mtf_adjoint(handle, h_ptr, rows, bins, rate, f, nfreqs, good_coeffs.ctypes.data, w.data_ptr())}
        for name, call in calls.items():
            if only in (None, name):
                assert call() == code, (name, word)
                text = lib.rvb_last_error(handle).decode()
                assert name + ":" in text and word in text, text

    both(capi.ERR_INVALID, "null histogram", h_ptr=None)
    both(capi.ERR_INVALID, "null modulation frequencies", freqs=None)
    both(capi.ERR_INVALID, "no rows", rows=0)
    both(capi.ERR_INVALID, "no bins", bins=0)
    both(capi.ERR_INVALID, "no modulation frequencies", nfreqs=0)
    both(capi.ERR_INVALID, "more than 16", freqs=np.linspace(1.0, 17.0, 17), nfreqs=17)
    for rate in (0.0, -1.0, float("inf"), float("nan")):
        both(capi.ERR_INVALID, "sample rate", rate=rate)
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        freqs = good_freqs.copy()
        freqs[5] = bad
        both(capi.ERR_INVALID, "modulation frequency 5 is not", freqs=freqs)
    for bad in (25600.0, 30000.0):
        freqs = good_freqs.copy()
        freqs[13] = bad
        both(capi.ERR_INVALID, "modulation frequency 13 is at or above half", freqs=freqs)
    both(capi.ERR_CAPACITY, "4096 rows", rows=4097)
    both(capi.ERR_CAPACITY, "32-bit", bins=0xFFFFFFFF)
    assert lib.rvb_mtf(handle, h.data_ptr(), nrows, nbins, fs, good_freqs.ctypes.data, 14, None, sums.ctypes.data) == capi.ERR_INVALID
    assert "rvb_mtf: null output" in lib.rvb_last_error(handle).decode()
    for coeffs_ptr, w_ptr, word in ((None, w.data_ptr(), "null coefficients"), (good_coeffs.ctypes.data, None, "null weights")):
        assert lib.rvb_mtf_adjoint(handle, h.data_ptr(), nrows, nbins, fs, good_freqs.ctypes.data, 14, coeffs_ptr, w_ptr) == capi.ERR_INVALID
        assert word in lib.rvb_last_error(handle).decode()
    for bad in (float("inf"), float("nan")):
        coeffs = good_coeffs.copy()
        coeffs[3, 13] = bad
        assert lib.rvb_mtf_adjoint(handle, h.data_ptr(), nrows, nbins, fs, good_freqs.ctypes.data, 14, coeffs.ctypes.data, w.data_ptr()) == capi.ERR_INVALID
        assert "a coefficient is not finite" in lib.rvb_last_error(handle).decode()
    for shift in (0, 4 * (nrows * nbins - 1), -4 * (nrows * nbins - 1)):
        assert lib.rvb_mtf_adjoint(handle, h.data_ptr(), nrows, nbins, fs, good_freqs.ctypes.data, 14, good_coeffs.ctypes.data,
                                   h.data_ptr() + shift) == capi.ERR_INVALID
        assert "overlap" in lib.rvb_last_error(handle).decode()
    ctx.synchronize()
    assert (out == 7.0).all() and (sums == 7.0).all()
    assert (w.cpu().numpy() == 7.0).all() and (h.cpu().numpy() == 1.0).all()
    # ... and the context still works: four rows of ones have m = |sum_j exp(-2 pi i F j / fs)| / nbins, close to 1 at 100 bins
    m = ctx.mtf(h.data_ptr(), nrows, nbins, fs, cases.FREQS)
    assert (m > 0.99).all() and (m <= 1.0 + 2.0 ** -40).all()
