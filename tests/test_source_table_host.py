"""CPU-side checks of the tabulated source directivity (include/rvb_capi.h: rvb_set_source_table): the header states the contract, the
built library exports the entry point and refuses a NULL handle before it touches a device (the refusals that need a context are held
in tests/test_gpu_source_table.py: no context exists without a GPU), and the cells of directivity.py are the cells that the oracle's row
selection addresses."""
import ctypes
import os
import re

import numpy as np

from attenuation_edges import CANONICAL, OBLIQUE, listener_angles
from conftest import ROOT
from host_lib import built_library
from parallel_reverb_raytracer_amd import capi, directivity


def test_header_declares_the_entry_point_and_its_contract():
    header = open(os.path.join(ROOT, "include", "rvb_capi.h")).read()
    assert re.search(r"typedef struct \{ float facing\[4\]; float up\[4\]; \} rvb_source_orientation;", header)
    assert re.search(r"int rvb_set_source_table\(rvb_ctx \* ctx, const float \* table[^;]*const rvb_source_orientation \* orientations, uint64_t norientations\);", header)
    section = header[header.index("tabulated source directivity"):header.index("int rvb_set_source_table(")]
    assert header.index("int rvb_set_source_pattern(") < header.index("tabulated source directivity") < header.index("int rvb_keep_paths(")
    for phrase in ("row a * 180 + e", "one zero row, row 64800", "row_of(to_listener(basis(facing, up), normalize3(v)))", "kernel.cpp:538-584",
                   "pos - mic replaced", "e == 180 runs into the next azimuth row", "margin scheme of angle_deg", "the ray's own direction",
                   "mic - position", "volume_b = volume_b * table[row][b]", "zero-volume", "time range", "reads the zero", "norientations == 1",
                   "norientations == n", "turns any pattern off", "turns the table off", "no extra launch and no extra allocation",
                   "before any device is touched", "not finite", "normalize3(cross3(up, facing))", "in stream order", "rvb_relisten uses",
                   "source_table_rays_kernel", "source_table_kernel", "rvb_multi_*", "rvb_pipeline_*", "MEASURED", "profiles/source_table_n1.txt"):
        assert phrase in section, phrase


def test_library_exports_the_entry_point_and_the_binding_knows_it():
    lib = built_library()
    assert "rvb_set_source_table" in capi.SYMBOLS and hasattr(lib, "rvb_set_source_table")
    assert ctypes.sizeof(capi.SourceOrientation) == 32 and capi.SourceOrientation.up.offset == 16
    o = capi.make_source_orientations([(0.0, 0.0, 1.0), (0.6, 0.0, 0.8)], (0.0, 1.0, 0.0))
    assert len(o) == 2 and list(o[1].facing) == [np.float32(0.6), 0.0, np.float32(0.8), 0.0] and list(o[1].up) == [0.0, 1.0, 0.0, 0.0]
    assert hasattr(capi.Context, "set_source_table")


def test_a_null_handle_is_refused_whatever_else_is_passed():
    lib = built_library()
    table = np.ones(360 * 180 * 8, np.float32)
    o = capi.make_source_orientations((0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
    bad = capi.make_source_orientations((0.0, 1.0, 0.0), (0.0, 1.0, 0.0))         # up parallel to facing
    p = table.ctypes.data_as(ctypes.c_void_p)
    for args in ((p, o, 1), (None, None, 0), (p, None, 0), (p, o, 0), (p, bad, 1)):
        assert lib.rvb_set_source_table(None, args[0], args[1], ctypes.c_uint64(args[2])) == capi.ERR_INVALID, args[2:]


def unit_directions(n, seed):
    d = np.random.default_rng(seed).normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def test_cell_centres_are_the_cells_the_oracle_selects(oracle):
    """3000 seeded unit directions in two frames: the centre of the cell that oracle.hrtf_index selects lies within 1 degree of the
    direction's true angles (binary64), 2 degrees in elevation for the equator cell, which spans (-1, 1)."""
    az_c, el_c = directivity.cell_centres()
    assert az_c.shape == (360, 180) and el_c.shape == (360, 180)
    assert el_c[0, 90] == 0.0 and el_c[0, 89] == 1.5 and el_c[0, 91] == -1.5 and el_c[0, 179] == -89.5 and az_c[0, 0] == -179.5 and az_c[359, 0] == 179.5
    dirs = unit_directions(3000, 31)
    equator = 0
    for frame in (CANONICAL, OBLIQUE):
        az, el = listener_angles(frame["facing"], frame["up"], (0.0, 0.0, 0.0), dirs)
        rows = np.array([oracle.hrtf_index(frame["facing"], frame["up"], d) for d in dirs])
        assert (rows >= 0).all() and (rows < 360 * 180).all()
        a, e = rows // 180, rows % 180
        daz = np.abs((az_c[a, e] - az + 180.0) % 360.0 - 180.0)
        dele = np.abs(el_c[a, e] - el)
        assert (daz <= 1.0).all(), float(daz.max())
        assert (dele <= np.where(e == 90, 2.0, 1.0)).all(), float(dele.max())
        equator += int((e == 90).sum())
        assert len(set(a)) > 300 and len(set(e)) > 150
    assert equator > 20, "the equator cell is not under test"


def test_table_from_function_equals_the_expression_at_the_centres():
    shape = np.linspace(0.0, 1.0, 8)
    fn = directivity.polar_pattern(shape)
    table = directivity.table_from_function(fn)
    az, el = directivity.cell_centres()
    want = ((1.0 - shape) + shape * (np.cos(np.radians(az)) * np.cos(np.radians(el)))[..., None]).astype(np.float32)
    assert table.shape == (360, 180, 8) and table.dtype == np.float32 and np.array_equal(table, want)
    assert (table[:, :, 0] == 1.0).all() and table[:, :, 7].min() < -0.99 and table[:, :, 7].max() > 0.99
    # a function that takes one cell at a time gives the same table
    import math
    scalar = directivity.table_from_function(lambda a, e: (1.0 - shape) + shape * (math.cos(math.radians(a)) * math.cos(math.radians(e))))
    assert np.allclose(scalar, table, rtol=0, atol=1e-6)


def test_table_from_balloon_resamples_bilinearly():
    az = np.arange(-180.0, 181.0, 10.0)
    el = np.arange(-90.0, 91.0, 10.0)
    # bilinear resampling returns a function that is linear between the grid's nodes exactly: |azimuth| and elevation, per band a factor
    band = np.arange(1.0, 9.0)
    gains = (np.abs(az)[:, None, None] + 2.0 * el[None, :, None]) * band[None, None, :]
    table = directivity.table_from_balloon(az, el, gains)
    caz, cel = directivity.cell_centres()
    want = (np.abs(caz) + 2.0 * cel)[..., None] * band
    assert table.shape == (360, 180, 8) and np.allclose(table, want, rtol=1e-6, atol=1e-4)
    # the azimuth wraps: a grid without the duplicate column gives the same table; one band for all
    assert np.array_equal(directivity.table_from_balloon(az[:-1], el, gains[:-1]), table)
    flat = directivity.table_from_balloon(az, el, gains[:, :, 0])
    assert np.array_equal(flat, np.repeat(table[:, :, :1], 8, axis=2))
    # a grid that stops short of the poles is held beyond its last ring
    short = directivity.table_from_balloon(az, el[3:-3], gains[:, 3:-3])
    assert np.array_equal(short[:, 0], short[:, 29]) and np.allclose(short[:, 40:140], table[:, 40:140], rtol=1e-6, atol=1e-4)


def test_normalised_takes_binary64_and_gives_binary32():
    v = directivity.normalised((3.0, 0.0, 4.0))
    assert v.dtype == np.float32 and np.array_equal(v, np.array([0.6, 0.0, 0.8], np.float32))
    many = directivity.normalised(np.array([(0.0, 2.0, 0.0), (1e-30, 0.0, 0.0)]))
    assert many.shape == (2, 3) and np.array_equal(many, np.array([(0, 1, 0), (1, 0, 0)], np.float32))
