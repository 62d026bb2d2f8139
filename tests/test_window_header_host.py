"""CPU-side checks of include/rvb_capi_window.h, the extension header of the echo finder: capi.py's fourth signature table says of every
entry point what the header's prototype says, the library exports the names with those signatures beside the other tables',
include/rvb_capi.h does not name them, the three structures and the two constants of capi.py are what a C compiler makes of the header
(tests/cpp/window_layout.c), and both calls refuse a NULL context without a GPU, writing nothing."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from capi_header import CLASSES, HEADER, prototypes
from conftest import ROOT
from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

WINDOW_HEADER = os.path.join(ROOT, "include", "rvb_capi_window.h")
NAMES = ["rvb_window_select", "rvb_window_paths"]
MIRRORS = {"rvb_window_entry": capi.WINDOW_ENTRY, "rvb_window_path": capi.WINDOW_PATH, "rvb_window_hit": capi.WINDOW_HIT}


def test_fourth_table_equals_the_extension_header_and_the_library():
    lib = built_library()
    declared = prototypes(WINDOW_HEADER)
    with open(WINDOW_HEADER) as f:
        text = f.read()
    assert set(re.findall(r"\b(rvb_[a-z_0-9]+)\s*\(", text)) == {name for name, _, _ in declared}     # no prototype escaped the parser
    assert [name for name, _, _ in declared] == capi.WINDOW_SYMBOLS == NAMES
    assert '#include "rvb_capi.h"' in text
    for name, returns, parameters in declared:
        restype, *argtypes = capi._WINDOW_SIGNATURES[name]
        assert restype is CLASSES[returns], name
        assert argtypes == [CLASSES[p] for p in parameters], name
        function = getattr(lib, name)
        assert function.restype is restype and list(function.argtypes) == argtypes, name


def test_the_fourth_table_is_disjoint_from_the_other_three():
    others = set(capi.SYMBOLS) | set(capi.IMAGE_SYMBOLS) | set(capi.LIVE_SYMBOLS)
    assert not set(capi.WINDOW_SYMBOLS) & others
    with open(HEADER) as f:
        first_header = f.read()
    assert not any(name in first_header for name in NAMES), "include/rvb_capi.h names an entry point of the extension header"
    assert "rvb_window" not in first_header and "RVB_WINDOW" not in first_header


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """tests/cpp/window_layout.c compiled with the system's C compiler against the header, run: its lines, split."""
    compiler = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/llvm/bin/clang"
    tool = str(tmp_path_factory.mktemp("window_layout") / "window_layout")
    subprocess.check_call([compiler, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "window_layout.c"), "-o", tool])
    facts = {"sizeof": {}, "field": {}, "value": {}}
    for line in subprocess.check_output([tool], universal_newlines=True).splitlines():
        kind, name, *rest = line.split()
        if kind == "field":
            facts[kind].setdefault(name, []).append((rest[0], int(rest[1]), int(rest[2]), rest[3]))
        else:
            assert name not in facts[kind]
            facts[kind][name] = int(rest[0])
    return facts


def test_the_structures_are_the_headers(layout):
    assert layout["sizeof"] == {"rvb_window_entry": 16, "rvb_window_path": 64, "rvb_window_hit": 16}
    for name, mirror in MIRRORS.items():
        assert mirror.itemsize == layout["sizeof"][name], name
        fields = sorted(((member, offset, sub.itemsize, sub.base.kind) for member, (sub, offset) in mirror.fields.items()), key=lambda f: f[1])
        assert fields == layout["field"][name], name
        assert list(mirror.names) == [member for member, _, _, _ in layout["field"][name]], name
        assert all(mirror.fields[member][0].base.itemsize in (4, 8) for member in mirror.names)
    assert capi.WINDOW_PATH.fields["volume"][0].shape == (8,) and capi.WINDOW_HIT.fields["position"][0].shape == (3,)
    assert capi.WINDOW_ENTRY.fields["record"][0] == np.dtype("<u8") and capi.WINDOW_PATH.fields["ray"][0] == np.dtype("<u8")


def test_the_constants_are_the_headers(layout):
    assert layout["value"] == {"RVB_WINDOW_TILE": capi.WINDOW_TILE, "RVB_WINDOW_MAX_PATHS": capi.WINDOW_MAX_PATHS}
    assert capi.WINDOW_TILE % 64 == 0


def test_a_null_context_is_refused_without_a_gpu():
    lib = built_library()
    count, inside = ctypes.c_uint64(7), ctypes.c_uint64(7)
    weights = (ctypes.c_float * 8)(*[1.0] * 8)
    block = np.full(4 * 64, 0xFF, dtype=np.uint8)             # (stands in for the device arrays: a NULL context touches none of them)
    assert lib.rvb_window_select(None, block.ctypes.data, 4, 0.0, 1.0, weights, 4, block.ctypes.data, ctypes.byref(count), ctypes.byref(inside)) == capi.ERR_INVALID
    assert lib.rvb_window_paths(None, 0.0, 1.0, weights, 4, 2, block.ctypes.data, None, ctypes.byref(count), ctypes.byref(inside)) == capi.ERR_INVALID
    assert (count.value, inside.value) == (7, 7)
    assert (block == 0xFF).all()
