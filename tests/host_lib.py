"""The product library for the host tests: built if it is missing, then loaded through capi.py."""
import os

from parallel_reverb_raytracer_amd import capi


def built_library():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load_library()
