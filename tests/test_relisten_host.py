"""CPU-side checks of the relisten interface (include/rvb_capi.h: RVB_KEEP_LISTENER, rvb_relisten): the header declares the entry point
and the keep bits and states memory and scope, the built library exports the symbol, it refuses a NULL handle with RVB_ERR_INVALID before
it touches a device, and the Python binding and the listener loop are there."""
import ctypes
import os
import re

import numpy as np

from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_point_and_the_keep_bits():
    header = open(os.path.join(ROOT, "include", "rvb_capi.h")).read()
    assert re.search(r"int rvb_relisten\(rvb_ctx \* ctx, const float \* mics, uint64_t npairs\);", header)
    assert re.search(r"enum \{ RVB_KEEP_MATERIALS = 1, RVB_KEEP_LISTENER = 2 \};", header)
    assert re.search(r"int rvb_keep_paths\(rvb_ctx \* ctx, int keep\);", header)
    assert (capi.KEEP_MATERIALS, capi.KEEP_LISTENER) == (1, 2)


def test_header_states_memory_and_scope():
    header = open(os.path.join(ROOT, "include", "rvb_capi.h")).read()
    block = header[header.index("a new microphone on a kept trace"):header.index("int rvb_relisten(")]
    assert "8 bytes per (ray, bounce) beside the 16 kept for re-shading" in block and "102 MB" in block
    assert 100_000 * 128 * 8 == 102_400_000                           # the figure is the product it names
    assert "Not offered by rvb_multi_* and rvb_pipeline_*".lower() in block.lower()
    assert "RVB_ERR_STATE" in block and "RVB_ERR_INVALID" in block and "bit for bit" in block


def test_library_exports_the_entry_point():
    lib = built_library()
    assert "rvb_relisten" in capi.SYMBOLS and hasattr(lib, "rvb_relisten")


def test_a_null_handle_is_refused():
    lib = built_library()
    mic = np.array([1.0, 2.0, 3.0], np.float32)
    assert lib.rvb_relisten(None, mic.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(1)) == capi.ERR_INVALID
    assert lib.rvb_relisten(None, None, ctypes.c_uint64(0)) == capi.ERR_INVALID
    assert lib.rvb_keep_paths(None, ctypes.c_int(capi.KEEP_MATERIALS | capi.KEEP_LISTENER)) == capi.ERR_INVALID


def test_python_binding_and_listener_loop_exist():
    import inspect
    from parallel_reverb_raytracer_amd import listeners
    assert hasattr(capi.Context, "relisten")
    assert list(inspect.signature(capi.Context.keep_paths).parameters) == ["self", "on", "listener"]
    assert inspect.signature(capi.Context.keep_paths).parameters["listener"].default is False
    names = list(inspect.signature(listeners.decay_map).parameters)
    assert names == ["ctx", "mics", "speakers", "sample_rate", "nbins", "db_begin", "db_end", "mode"]
    assert inspect.signature(listeners.decay_map).parameters["mode"].default == capi.IR_EXACT
