"""CPU-side checks of the directional-source interface (include/rvb_capi.h: rvb_source_pattern): the built library exports the four
entry points, each refuses a NULL handle with RVB_ERR_INVALID before it touches a device, and the Python mirror of the pattern is the
header's 48 bytes."""
import ctypes

from host_lib import built_library
from parallel_reverb_raytracer_amd import capi

NEW_SYMBOLS = ["rvb_set_source_pattern", "rvb_multi_set_source_pattern", "rvb_pipeline_set_source_pattern", "rvb_pipeline_submit_directed"]


def test_library_exports_the_source_pattern_entry_points():
    lib = built_library()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS and hasattr(lib, name), name


def test_null_handles_are_refused():
    lib = built_library()
    pattern = capi.make_source_patterns([(1.0, 0.0, 0.0)], 0.5)
    f3, f8 = (ctypes.c_float * 3)(1.0, 0.0, 0.0), (ctypes.c_float * 8)(*([0.5] * 8))
    assert lib.rvb_set_source_pattern(None, pattern, ctypes.c_uint64(1)) == capi.ERR_INVALID
    assert lib.rvb_set_source_pattern(None, None, ctypes.c_uint64(0)) == capi.ERR_INVALID
    assert lib.rvb_multi_set_source_pattern(None, pattern) == capi.ERR_INVALID
    assert lib.rvb_pipeline_set_source_pattern(None, f8, f3) == capi.ERR_INVALID
    assert lib.rvb_pipeline_submit_directed(None, f3, f3, None, None, f3) == capi.ERR_INVALID


def test_python_mirror_of_the_pattern_is_48_bytes():
    assert ctypes.sizeof(capi.SourcePattern) == 48
    assert capi.SourcePattern.direction.offset == 0 and capi.SourcePattern.shape.offset == 16
    pats = capi.make_source_patterns([(0.0, 2.0, 0.0), (1.0, 0.0, 0.0)], [[0.0] * 8, [1.0] * 8])
    assert len(pats) == 2 and ctypes.sizeof(pats) == 96
    assert list(pats[0].direction) == [0.0, 2.0, 0.0, 0.0] and list(pats[1].shape) == [1.0] * 8 and list(pats[0].shape) == [0.0] * 8
    one = capi.make_source_patterns((0.0, 0.0, 1.0), 0.25)
    assert len(one) == 1 and list(one[0].shape) == [0.25] * 8
