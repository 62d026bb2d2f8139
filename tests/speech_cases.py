"""The inputs that tests/test_speech_reference.py (GROUND, on the reference alone) and tests/test_gpu_speech.py share: the histograms of
tests/test_gpu_decay.py (`case`, T = 4096), the shapes and sample rates, seeded coefficients dL/dm, and the reference of a case computed
once and left unchanged."""
import numpy as np

import speech_reference as ref
from test_gpu_decay import T, case

FREQS = ref.STI_FREQS
FREQS_16 = FREQS + (16.0, 20.0)
FREQS_1 = (2.0,)
CASES = [(16, 1, 51200.0), (16, 2, 51200.0), (16, 63, 51200.0), (16, T - 1, 51200.0), (16, T, 51200.0), (16, T + 1, 51200.0),
         (16, 2 * T + 65, 51200.0), (1, 2 * T + 65, 51200.0), (72, 2 * T + 65, 51200.0), (2, 130 * T + 5, 51200.0), (8, T - 1, 25600.0)]
DECAY_60 = 13.8155              # ln 10^6: H^2 = exp(-DECAY_60 t / T) falls by 60 dB in T
GROUND_CASES = [(16, 2 * T + 65, 51200.0), (8, T - 1, 25600.0)]
EXTRA_FREQS = [((16, 2 * T + 65, 51200.0), FREQS_1), ((16, 2 * T + 65, 51200.0), FREQS_16)]


def coefficients(nrows, nfreqs):
    """dL/dm [nrows][nfreqs]: seeded standard normal values, any loss's."""
    return np.random.default_rng(300 + 17 * nrows + nfreqs).standard_normal((nrows, nfreqs))


_references = {}


def reference(nrows, nbins, fs, freqs=FREQS):
    """{"h", "coeffs", "fw" (speech_reference.mtf), "w", "c" (speech_reference.adjoint)} of a case, read-only."""
    key = (nrows, nbins, fs, tuple(freqs))
    if key not in _references:
        h = case(nrows, nbins)["h"]
        coeffs = coefficients(nrows, len(freqs))
        fw = ref.mtf(h, fs, freqs)
        w, c = ref.adjoint(h, fs, freqs, coeffs, fw)
        for a in (coeffs, w, c, fw["m"], fw["m_bar"], fw["sums"], fw["sums_bar"]):
            a.setflags(write=False)
        _references[key] = {"h": h, "coeffs": coeffs, "fw": fw, "w": w, "c": c}
    return _references[key]


def spike_rows(fs=51200.0, seconds=0.3):
    """Three rows of 3 * seconds * fs bins: a single spike; two equal spikes 0.4 s apart; H^2 = exp(-13.8155 t / seconds) (a decay of 60 dB
    in `seconds`).  float32."""
    nbins = int(round(3 * seconds * fs))
    h = np.zeros((3, nbins), np.float32)
    h[0, 17] = 3.0
    h[1, 5] = h[1, 5 + int(round(0.4 * fs))] = 0.25
    h[2] = np.exp(-0.5 * DECAY_60 * np.arange(nbins) / (fs * seconds)).astype(np.float32)
    return h


def exponential_mtf(freqs, seconds):
    return 1.0 / np.sqrt(1.0 + (2 * np.pi * np.asarray(freqs) * seconds / DECAY_60) ** 2)
