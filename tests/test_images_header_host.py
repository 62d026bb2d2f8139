"""CPU-side checks of include/rvb_capi_images.h, the extension header of the C-ABI (the merged image list on the device, the
image-source part of the material gradient): capi.py's second signature table says of every entry point what the header's prototype
says, the library exports the names with those signatures beside the first table's, include/rvb_capi.h does not name them, every new
call refuses a NULL context without a GPU, and fitting.py refuses what the per-triangle map does not offer."""
import ctypes
import os
import re

import pytest

from capi_header import CLASSES, HEADER, prototypes
from conftest import ROOT
from host_lib import built_library
from parallel_reverb_raytracer_amd import capi, fitting

IMAGES_HEADER = os.path.join(ROOT, "include", "rvb_capi_images.h")
NAMES = ["rvb_ir_configure_speakers_merged", "rvb_ir_configure_hrtf_merged", "rvb_reshade_grad_images"]


def test_second_table_equals_the_extension_header_and_the_library():
    lib = built_library()
    declared = prototypes(IMAGES_HEADER)
    with open(IMAGES_HEADER) as f:
        text = f.read()
    assert set(re.findall(r"\b(rvb_[a-z_0-9]+)\s*\(", text)) == {name for name, _, _ in declared}     # no prototype escaped the parser
    assert [name for name, _, _ in declared] == capi.IMAGE_SYMBOLS == NAMES
    assert '#include "rvb_capi.h"' in text
    for name, returns, parameters in declared:
        restype, *argtypes = capi._IMAGE_SIGNATURES[name]
        assert restype is CLASSES[returns], name
        assert argtypes == [CLASSES[p] for p in parameters], name
        function = getattr(lib, name)
        assert function.restype is restype and list(function.argtypes) == argtypes, name
    # the first table is applied as before, and the two do not overlap
    assert not set(capi.IMAGE_SYMBOLS) & set(capi.SYMBOLS)
    with open(HEADER) as f:
        first_header = f.read()
    assert not any(name in first_header for name in NAMES), "include/rvb_capi.h names an entry point of the extension header"
    first = getattr(lib, "rvb_reshade_grad")
    assert list(first.argtypes) == list(capi._SIGNATURES["rvb_reshade_grad"][1:])


def test_a_null_context_is_refused_without_a_gpu():
    lib = built_library()
    mic = (ctypes.c_float * 3)(0, 0, 0)
    n = ctypes.c_uint64(7)
    assert lib.rvb_ir_configure_speakers_merged(None, mic, None, 1, capi.IR_ALL, 0, ctypes.byref(n)) == capi.ERR_INVALID
    assert lib.rvb_ir_configure_hrtf_merged(None, mic, None, mic, mic, capi.IR_ALL, 0, ctypes.byref(n)) == capi.ERR_INVALID
    assert lib.rvb_reshade_grad_images(None, 0.0, 44100.0, 16, None, None, None) == capi.ERR_INVALID
    assert n.value == 7


def test_the_sensitivity_map_refuses_image_sources():
    """Before anything of the context is touched: None stands in for it."""
    for which in (capi.IR_ALL, capi.IR_IMAGES):
        with pytest.raises(ValueError, match="IR_DIFFUSE"):
            fitting.decay_sensitivity_map(None, None, None, None, None, None, None, 44100.0, 0.0, 16, which=which)
