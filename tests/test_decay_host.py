"""CPU-side checks of the decay interface (include/rvb_capi.h: rvb_decay_curve, rvb_decay_times, rvb_decay_loss): the header declares
the three entry points and the phrases of their contract, the built library exports them, each refuses a NULL handle with
RVB_ERR_INVALID before it touches a device and leaves the host outputs alone, and the Python binding offers them."""
import ctypes
import os
import re

import numpy as np

from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points_and_the_contract():
    header = open(os.path.join(ROOT, "include", "rvb_capi.h")).read()
    assert re.search(r"int rvb_decay_curve\(rvb_ctx \* ctx, const void \* d_histogram, uint64_t nrows, uint64_t nbins, void \* d_curve\);", header)
    assert re.search(r"int rvb_decay_times\(rvb_ctx \* ctx, const void \* d_curve, uint64_t nrows, uint64_t nbins, float sample_rate,\s*"
                     r"float db_begin, float db_end, float \* seconds[^,)]*\);", header)
    assert re.search(r"int rvb_decay_loss\(rvb_ctx \* ctx, const void \* d_histogram, const void \* d_curve, const void \* d_target, const void \* d_mask,\s*"
                     r"uint64_t nrows, uint64_t nbins, unsigned flags, double \* loss_rows[^,)]*, void \* d_weights\);", header)
    assert re.search(r"#define RVB_DECAY_TILE %d\b" % capi.DECAY_TILE, header)
    assert re.search(r"enum \{ RVB_DECAY_NORMALISED = %d \};" % capi.DECAY_NORMALISED, header)
    # the section stands behind rvb_reshade_grad, and its contract is part of the text
    assert header.index("int rvb_reshade_grad(") < header.index("---- decay curves") < header.index("int rvb_decay_curve(")
    block = header[header.index("---- decay curves"):header.index("int rvb_decay_curve(")]
    for phrase in ("fixed order", "quiet NaN", "RVB_DECAY_NORMALISED", "not available", "binary64", "identical bytes", "No atomics",
                   "RVB_ERR_CAPACITY", "A failed call writes nothing", "decay_curve_scan_kernel", "decay_times_fit_kernel", "decay_loss_scan_kernel"):
        assert phrase in block, phrase


def test_library_exports_the_entry_points():
    lib = built_library()
    for name, nargs in (("rvb_decay_curve", 5), ("rvb_decay_times", 8), ("rvb_decay_loss", 10)):
        assert name in capi.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs


def test_a_null_handle_is_refused_and_the_host_outputs_stay():
    lib = built_library()
    fake = [ctypes.c_void_p(4096 * (i + 1)) for i in range(5)]          # never dereferenced: the handle is looked at first
    seconds = np.full(4, 7.0, dtype=np.float32)
    losses = np.full(4, 7.0, dtype=np.float64)
    assert lib.rvb_decay_curve(None, fake[0], 4, 100, fake[1]) == capi.ERR_INVALID
    assert lib.rvb_decay_times(None, fake[0], 4, 100, 44100.0, -5.0, -35.0, seconds.ctypes.data_as(ctypes.c_void_p)) == capi.ERR_INVALID
    for weights in (fake[4], None):
        assert lib.rvb_decay_loss(None, fake[0], fake[1], fake[2], fake[3], 4, 100, capi.DECAY_NORMALISED,
                                  losses.ctypes.data_as(ctypes.c_void_p), weights) == capi.ERR_INVALID
    assert (seconds == 7.0).all() and (losses == 7.0).all()


def test_python_binding_offers_the_decay_calls():
    for name in ("decay_curve", "decay_times", "decay_loss", "decay_curve_tensor", "decay_times_tensor", "decay_loss_tensor"):
        assert hasattr(capi.Context, name), name
    assert capi.DECAY_TILE == 4096 and capi.DECAY_NORMALISED == 1
    from parallel_reverb_raytracer_amd import fitting
    assert callable(fitting.decay_loss_and_grad) and callable(fitting.fit_decay)
