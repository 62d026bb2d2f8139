"""CPU-side checks of the room acoustic parameter interface (include/rvb_capi.h: rvb_decay_params, rvb_decay_params_loss): the header
declares the two entry points, the enum and the phrases of their contract, the built library exports them, each refuses a NULL handle
with RVB_ERR_INVALID before it touches a device and leaves the host outputs alone, and the Python layers offer the new names."""
import ctypes
import os
import re

import numpy as np

from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("EDT", "T20", "T30", "C50", "C80", "D50", "TS")


def test_header_declares_the_entry_points_the_enum_and_the_contract():
    header = open(os.path.join(ROOT, "include", "rvb_capi.h")).read()
    assert re.search(r"int rvb_decay_params\(rvb_ctx \* ctx, const void \* d_curve, uint64_t nrows, uint64_t nbins, float sample_rate,\s*"
                     r"float \* params[^,)]*\);", header)
    assert re.search(r"int rvb_decay_params_loss\(rvb_ctx \* ctx, const void \* d_histogram, const void \* d_curve, uint64_t nrows, uint64_t nbins, "
                     r"float sample_rate,\s*const float \* targets[^,)]*, const float \* param_weights[^,)]*,\s*double \* loss_rows[^,)]*, "
                     r"float \* params[^)]*,\s*void \* d_weights[^)]*\);", header)
    assert re.search(r"enum \{ " + ", ".join("RVB_DECAY_%s = %d" % (n, i) for i, n in enumerate(NAMES)) + r" \};", header)
    assert re.search(r"#define RVB_DECAY_NPARAMS %d\b" % capi.DECAY_NPARAMS, header)
    # the section stands behind the decay calls, and its contract is part of the text
    assert header.index("int rvb_decay_loss(") < header.index("---- room acoustic parameters") < header.index("int rvb_decay_params(")
    block = header[header.index("---- room acoustic parameters"):header.index("int rvb_decay_params(")]
    for phrase in ("byte-equal", "quiet NaN", "not available", "binary64", "identical bytes", "no atomics", "synchronous", "C10 = 10 / ln 10",
                   "RVB_ERR_INVALID", "RVB_ERR_CAPACITY", "a failed call writes nothing", "exactly 0 where H is 0", "no entry left unwritten",
                   "decay_params_find_kernel", "decay_params_window_kernel", "decay_params_sums_kernel", "decay_params_fit_kernel",
                   "decay_params_adjoint_sums_kernel", "decay_params_adjoint_carry_kernel", "decay_params_adjoint_scan_kernel", "MEASURED"):
        assert phrase in block, phrase


def test_library_exports_the_entry_points():
    lib = built_library()
    for name, nargs in (("rvb_decay_params", 6), ("rvb_decay_params_loss", 11)):
        assert name in capi.SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == nargs


def test_a_null_handle_is_refused_and_the_host_outputs_stay():
    lib = built_library()
    fake = [ctypes.c_void_p(4096 * (i + 1)) for i in range(3)]          # never dereferenced: the handle is looked at first
    params = np.full((4, 7), 7.0, dtype=np.float32)
    losses = np.full(4, 7.0, dtype=np.float64)
    targets, weights = np.ones((4, 7), dtype=np.float32), np.ones((4, 7), dtype=np.float32)
    pp, lp = params.ctypes.data_as(ctypes.c_void_p), losses.ctypes.data_as(ctypes.c_void_p)
    tp, wp = targets.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p)
    assert lib.rvb_decay_params(None, fake[0], 4, 100, 44100.0, pp) == capi.ERR_INVALID
    for d_weights in (fake[2], None):
        assert lib.rvb_decay_params_loss(None, fake[0], fake[1], 4, 100, 44100.0, tp, wp, lp, pp, d_weights) == capi.ERR_INVALID
    assert (params == 7.0).all() and (losses == 7.0).all()


def test_the_python_layers_offer_the_new_names():
    for name in ("decay_params", "decay_params_loss", "decay_params_tensor", "decay_params_loss_tensor"):
        assert hasattr(capi.Context, name), name
    assert [getattr(capi, "DECAY_" + n) for n in NAMES] == list(range(7)) and capi.DECAY_NPARAMS == 7
    from parallel_reverb_raytracer_amd import fitting, listeners
    assert callable(fitting.params_loss_and_grad) and callable(fitting.params_loss) and callable(fitting.fit_params)
    assert callable(fitting.fit_decay) and callable(listeners.parameter_map) and callable(listeners.decay_map)
