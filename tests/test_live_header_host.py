"""CPU-side checks of include/rvb_capi_live.h, the extension header with the diagnostic of exact mode's live list: capi.py's third
signature table says of its entry point what the header's prototype says, the library exports the name with that signature beside the
other tables', include/rvb_capi.h does not name it, the tile size of capi.py is the header's, and the call refuses a NULL context
without a GPU."""
import ctypes
import os
import re

from capi_header import CLASSES, HEADER, prototypes
from conftest import ROOT
from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

LIVE_HEADER = os.path.join(ROOT, "include", "rvb_capi_live.h")
NAMES = ["rvb_ir_exact_list_info"]


def test_third_table_equals_the_extension_header_and_the_library():
    lib = built_library()
    declared = prototypes(LIVE_HEADER)
    with open(LIVE_HEADER) as f:
        text = f.read()
    assert set(re.findall(r"\b(rvb_[a-z_0-9]+)\s*\(", text)) == {name for name, _, _ in declared}     # no prototype escaped the parser
    assert [name for name, _, _ in declared] == capi.LIVE_SYMBOLS == NAMES
    assert '#include "rvb_capi.h"' in text
    for name, returns, parameters in declared:
        restype, *argtypes = capi._LIVE_SIGNATURES[name]
        assert restype is CLASSES[returns], name
        assert argtypes == [CLASSES[p] for p in parameters], name
        function = getattr(lib, name)
        assert function.restype is restype and list(function.argtypes) == argtypes, name
    assert not set(capi.LIVE_SYMBOLS) & (set(capi.SYMBOLS) | set(capi.IMAGE_SYMBOLS))
    with open(HEADER) as f:
        assert not any(name in f.read() for name in NAMES), "include/rvb_capi.h names an entry point of the extension header"
    tile = re.search(r"#define RVB_LIVE_TILE (\d+)", text)
    assert tile and int(tile.group(1)) == capi.LIVE_TILE and capi.LIVE_TILE % 64 == 0


def test_a_null_context_is_refused_without_a_gpu():
    lib = built_library()
    listed, live, valid = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_int(7)
    assert lib.rvb_ir_exact_list_info(None, ctypes.byref(listed), ctypes.byref(live), ctypes.byref(valid)) == capi.ERR_INVALID
    assert (listed.value, live.value, valid.value) == (7, 7, 7)
