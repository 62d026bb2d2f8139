"""CPU-side checks of include/rvb_capi_source_grad.h, the extension header of the source-end gradients: capi.py's sixth signature table
says of every entry point what the header's prototype says, the library exports the names with those signatures beside the other
tables', include/rvb_capi.h does not name them, both calls refuse a NULL context without a GPU and write nothing, and
directivity.balloon_gradient — host arithmetic — adds rows up as its text says."""
import ctypes
import os
import re

import numpy as np

from capi_header import CLASSES, HEADER, prototypes
from conftest import ROOT
from host_lib import built_library
from parallel_reverb_raytracer_amd import capi, directivity

SOURCE_GRAD_HEADER = os.path.join(ROOT, "include", "rvb_capi_source_grad.h")
NAMES = ["rvb_source_grad", "rvb_source_grad_images"]


def test_sixth_table_equals_the_extension_header_and_the_library():
    lib = built_library()
    declared = prototypes(SOURCE_GRAD_HEADER)
    with open(SOURCE_GRAD_HEADER) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)               # (the comments speak of the calls these two mirror)
    assert set(re.findall(r"\b(rvb_[a-z_0-9]+)\s*\(", code)) == {name for name, _, _ in declared}     # no prototype escaped the parser
    assert [name for name, _, _ in declared] == capi.SOURCE_GRAD_SYMBOLS == NAMES
    assert '#include "rvb_capi.h"' in text
    for name, returns, parameters in declared:
        restype, *argtypes = capi._SOURCE_GRAD_SIGNATURES[name]
        assert restype is CLASSES[returns], name
        assert argtypes == [CLASSES[p] for p in parameters], name
        function = getattr(lib, name)
        assert function.restype is restype and list(function.argtypes) == argtypes, name


def test_the_sixth_table_is_disjoint_from_the_other_five_and_the_structure_is_the_headers():
    others = set(capi.SYMBOLS) | set(capi.IMAGE_SYMBOLS) | set(capi.LIVE_SYMBOLS) | set(capi.WINDOW_SYMBOLS) | set(capi.SPEECH_SYMBOLS)
    assert not set(capi.SOURCE_GRAD_SYMBOLS) & others
    with open(HEADER) as f:
        first_header = f.read()
    assert "rvb_source_grad" not in first_header and "rvb_source_pattern_grad" not in first_header
    with open(SOURCE_GRAD_HEADER) as f:
        text = f.read()
    assert "typedef struct { float shape[8]; float direction[4]; } rvb_source_pattern_grad;" in text
    assert [(name, kind._length_) for name, kind in capi.SourcePatternGrad._fields_] == [("shape", 8), ("direction", 4)]
    assert ctypes.sizeof(capi.SourcePatternGrad) == 48


def test_a_null_context_is_refused_without_a_gpu_and_nothing_is_written():
    lib = built_library()
    block = np.full(4 * 64, 0xFF, dtype=np.uint8)             # (stands in for the device arrays: a NULL context touches none of them)
    pattern = capi.SourcePatternGrad()
    pattern.shape[:] = [7.0] * 8
    pattern.direction[:] = [7.0] * 4
    at = block.ctypes.data
    assert lib.rvb_source_grad(None, 0.0, 44100.0, 16, at, at, at, ctypes.byref(pattern)) == capi.ERR_INVALID
    assert lib.rvb_source_grad_images(None, 0.0, 44100.0, 16, at, at, at, at, ctypes.byref(pattern)) == capi.ERR_INVALID
    assert (block == 0xFF).all() and list(pattern.shape) == [7.0] * 8 and list(pattern.direction) == [7.0] * 4


def test_balloon_gradient_adds_by_row_and_leaves_the_zero_row_out():
    rng = np.random.default_rng(3)
    grad = rng.standard_normal((50, 8)).astype(np.float32)
    rows = rng.integers(0, 360 * 180, 50)
    rows[[4, 9, 30]] = rows[0]                                 # several rays leave through one cell
    rows[[7, 8]] = 360 * 180                                   # the zero row behind the table: no cell
    balloon = directivity.balloon_gradient(grad, rows.astype(np.uint32))
    assert balloon.shape == (360, 180, 8) and balloon.dtype == np.float64
    want = np.zeros((360 * 180, 8))
    for g, row in zip(grad.astype(np.float64), rows):
        if row < 360 * 180:
            want[row] += g
    assert np.array_equal(balloon.reshape(-1, 8), want)
    assert np.array_equal(directivity.balloon_gradient(grad, rows.astype(np.int32)), balloon)
