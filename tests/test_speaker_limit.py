"""The speaker-count limit of the fused impulse-response path: one number in the C header and in the ctypes binding."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_speakers_is_64_in_the_header_and_in_the_binding():
    from parallel_reverb_raytracer_amd import capi
    with open(os.path.join(ROOT, "include", "rvb_capi.h")) as f:
        found = re.findall(r"^#define\s+RVB_MAX_SPEAKERS\s+(\d+)\s*$", f.read(), re.M)
    assert len(found) == 1
    assert int(found[0]) == capi.MAX_SPEAKERS == 64
