"""CPU-side checks of include/rvb_capi_speech.h, the extension header of the speech calls: capi.py's fifth signature table says of every
entry point what the header's prototype says, the library exports the names with those signatures beside the other tables',
include/rvb_capi.h does not name them, the device calls refuse a NULL context without a GPU and write nothing, and rvb_speech_index
— host arithmetic, no context — equals tests/speech_reference.py in value and derivative on random matrices with clipped entries, m = 0,
m = 1, a NaN, and signal-to-noise ratios absent, finite and +inf."""
import ctypes
import os
import re

import numpy as np
import pytest

import speech_reference as ref
from capi_header import CLASSES, HEADER, prototypes
from conftest import ROOT
from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

SPEECH_HEADER = os.path.join(ROOT, "include", "rvb_capi_speech.h")
NAMES = ["rvb_mtf", "rvb_mtf_adjoint", "rvb_speech_index"]


def test_fifth_table_equals_the_extension_header_and_the_library():
    lib = built_library()
    declared = prototypes(SPEECH_HEADER)
    with open(SPEECH_HEADER) as f:
        text = f.read()
    assert set(re.findall(r"\b(rvb_[a-z_0-9]+)\s*\(", text)) == {name for name, _, _ in declared}     # no prototype escaped the parser
    assert [name for name, _, _ in declared] == capi.SPEECH_SYMBOLS == NAMES
    assert '#include "rvb_capi.h"' in text
    for name, returns, parameters in declared:
        restype, *argtypes = capi._SPEECH_SIGNATURES[name]
        assert restype is CLASSES[returns], name
        assert argtypes == [CLASSES[p] for p in parameters], name
        function = getattr(lib, name)
        assert function.restype is restype and list(function.argtypes) == argtypes, name


def test_the_fifth_table_is_disjoint_from_the_other_four_and_the_constants_are_the_headers():
    others = set(capi.SYMBOLS) | set(capi.IMAGE_SYMBOLS) | set(capi.LIVE_SYMBOLS) | set(capi.WINDOW_SYMBOLS)
    assert not set(capi.SPEECH_SYMBOLS) & others
    with open(HEADER) as f:
        first_header = f.read()
    assert "rvb_mtf" not in first_header and "rvb_speech" not in first_header and "RVB_MTF" not in first_header and "RVB_STI" not in first_header
    with open(SPEECH_HEADER) as f:
        defines = dict(re.findall(r"^#define (RVB_[A-Z_]+) +(\d+)", f.read(), flags=re.M))
    assert defines == {"RVB_MTF_MAX_FREQS": str(capi.MTF_MAX_FREQS), "RVB_STI_BANDS": str(capi.STI_BANDS), "RVB_STI_FREQS": str(capi.STI_FREQS)}
    from parallel_reverb_raytracer_amd import speech
    assert speech.STI_FREQS == ref.STI_FREQS and speech.ALPHA_MALE == ref.ALPHA_MALE and speech.BETA_MALE == ref.BETA_MALE


def test_a_null_context_is_refused_without_a_gpu_and_nothing_is_written():
    lib = built_library()
    freqs = np.array(ref.STI_FREQS)
    block = np.full(4 * 64, 0xFF, dtype=np.uint8)             # (stands in for the device arrays: a NULL context touches none of them)
    out, sums, coeffs = np.full((4, 14), 7.0), np.full((4, 29), 7.0), np.ones((4, 14))
    assert lib.rvb_mtf(None, block.ctypes.data, 4, 16, 51200.0, freqs.ctypes.data, 14, out.ctypes.data, sums.ctypes.data) == capi.ERR_INVALID
    assert lib.rvb_mtf_adjoint(None, block.ctypes.data, 4, 16, 51200.0, freqs.ctypes.data, 14, coeffs.ctypes.data, block.ctypes.data) == capi.ERR_INVALID
    assert (out == 7.0).all() and (sums == 7.0).all() and (block == 0xFF).all()


def test_the_index_refuses_missing_arrays_and_frequency_counts_out_of_range():
    lib = built_library()
    m, alpha, beta = np.full((7, 14), 0.5), np.array(ref.ALPHA_MALE), np.array(ref.BETA_MALE)
    sti = ctypes.c_double(7.0)
    ok = (m.ctypes.data, 14, None, alpha.ctypes.data, beta.ctypes.data, ctypes.byref(sti), None, None)
    for position, value in ((0, None), (3, None), (4, None), (5, None), (1, 0), (1, capi.MTF_MAX_FREQS + 1)):
        args = list(ok)
        args[position] = value
        assert lib.rvb_speech_index(*args) == capi.ERR_INVALID, position
        assert sti.value == 7.0
    assert lib.rvb_speech_index(*ok) == capi.OK and abs(sti.value - 0.5) < 1e-12         # every TI is 0.5: 0.5 (sum alpha - sum beta)
    with pytest.raises(capi.RvbError):
        capi.speech_index(np.zeros((7, 17)), alpha, beta)


def matrices():
    """(label, mtf [7][nfreqs], snr_db): random values with the edges the header names."""
    rng = np.random.default_rng(77)
    out = []
    for nfreqs in (14, 1, 16):
        plain = rng.uniform(0.02, 0.98, (7, nfreqs))                  # some entries beyond +-15 dB (m < 0.0307, m > 0.9693): clipped
        edges = plain.copy()
        edges[0, 0], edges[1, -1], edges[2, 0], edges[3, 0], edges[6, -1] = 0.0, 1.0, 0.999, 0.001, 1.5
        dead = edges.copy()
        dead[4] = 0.0                                                # MTI_4 = 0: the square-root terms next to it have product 0
        for label, m in (("plain", plain), ("edges", edges), ("a band of zeros", dead)):
            out.append(("%s, %d frequencies, no noise" % (label, nfreqs), m, None))
            out.append(("%s, %d frequencies, finite snr" % (label, nfreqs), m, rng.uniform(-5.0, 30.0, 7)))
            mixed = rng.uniform(0.0, 20.0, 7)
            mixed[[1, 5]] = np.inf
            out.append(("%s, %d frequencies, snr with +inf" % (label, nfreqs), m, mixed))
    return out


@pytest.mark.parametrize("label,m,snr_db", matrices(), ids=[label for label, _, _ in matrices()])
def test_the_index_is_the_references(label, m, snr_db):
    """Value within speech_reference.speech_index_bars, the derivative entry by entry within its bar, zeros of the derivative (clipped
    entries, dead square roots) exactly zero in both; snr_db all +inf is snr_db NULL bit for bit."""
    built_library()
    alpha, beta = ref.ALPHA_MALE, ref.BETA_MALE
    want_sti, want_mti, want_d, scale = ref.speech_index(m, alpha, beta, snr_db)
    sti, mti, d = capi.speech_index(m, alpha, beta, snr_db, want_derivative=True)
    sti_bar, d_bar = ref.speech_index_bars(alpha, beta, scale)
    print("%s: STI %.15g against %.15g, largest derivative difference %.3e" % (label, sti, want_sti, np.abs(d - want_d).max()))
    assert abs(sti - want_sti) <= sti_bar and (np.abs(mti - want_mti) <= sti_bar).all()
    assert (np.abs(d - want_d) <= d_bar).all()
    assert ((d == 0) == (want_d == 0)).all() and (want_d != 0).any() and ((want_d == 0).any() or label.startswith("plain"))
    assert capi.speech_index(m, alpha, beta, snr_db)[0] == sti
    if snr_db is None:
        again = capi.speech_index(m, alpha, beta, np.full(7, np.inf), want_derivative=True)
        assert again[0] == sti and again[1].tobytes() == mti.tobytes() and again[2].tobytes() == d.tobytes()


def test_a_nan_gives_nan():
    built_library()
    m = np.full((7, 14), 0.5)
    m[3, 2] = np.nan
    sti, mti = capi.speech_index(m, ref.ALPHA_MALE, ref.BETA_MALE)
    assert np.isnan(sti) and np.isnan(mti[3]) and np.isfinite(np.delete(mti, 3)).all()
    assert np.isnan(ref.speech_index(m, ref.ALPHA_MALE, ref.BETA_MALE)[0])
