"""CPU-side checks of the material-gradient interface (include/rvb_capi.h: rvb_reshade_grad): the header declares the entry point, the
built library exports it, it refuses a NULL handle with RVB_ERR_INVALID before it touches a device, and the Python binding offers it."""
import ctypes
import os
import re

import numpy as np

from host_lib import built_library
from parallel_reverb_raytracer_amd import capi
from parallel_reverb_raytracer_amd.dtypes import SURFACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point():
    header = open(os.path.join(ROOT, "include", "rvb_capi.h")).read()
    assert re.search(r"int rvb_reshade_grad\(rvb_ctx \* ctx, float predelay, float sample_rate, uint64_t nbins, const void \* d_weights,\s*"
                     r"rvb_surface \* grad_surfaces,\s*float grad_air\[8\]\);", header)
    # the scope of this version is part of the contract's text
    block = header[header.index("material gradients of a weighted impulse response"):header.index("int rvb_reshade_grad(")]
    for phrase in ("RVB_IR_DIFFUSE", "Image-source gradients are a follow-up", "HRTF", "more than 8 channels", "rvb_multi_*", "never divides"):
        assert phrase in block, phrase


def test_library_exports_the_entry_point():
    lib = built_library()
    assert "rvb_reshade_grad" in capi.SYMBOLS and hasattr(lib, "rvb_reshade_grad")
    assert lib.rvb_reshade_grad.argtypes is not None and len(lib.rvb_reshade_grad.argtypes) == 7


def test_a_null_handle_is_refused():
    lib = built_library()
    grads = np.zeros(3, dtype=SURFACE)
    air = np.zeros(8, dtype=np.float32)
    fake_weights = ctypes.c_void_p(64)          # never dereferenced: the handle is looked at first
    args = (ctypes.c_float(0.0), ctypes.c_float(44100.0), ctypes.c_uint64(16), fake_weights, grads.ctypes.data_as(ctypes.c_void_p))
    assert lib.rvb_reshade_grad(None, *args, air.ctypes.data_as(ctypes.c_void_p)) == capi.ERR_INVALID
    assert lib.rvb_reshade_grad(None, *args, None) == capi.ERR_INVALID
    assert not grads.view(np.uint8).any() and not air.any()


def test_python_binding_offers_reshade_grad():
    assert hasattr(capi.Context, "reshade_grad")
