"""CPU-side checks of the product: the C-ABI library loads and exports every symbol of include/rvb_capi.h, capi.py's signature table
says of every entry point what the header's prototype says, the Python mirrors of the header's structures and constants equal what a C
compiler makes of the header (tests/cpp/capi_layout.c), the library refuses to run without a GPU (no CPU fallback), and its host-only
image-source merge reproduces the reference's de-dup map (reference rayverb.cpp:654-676, :692-706)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from capi_header import CLASSES, HEADER, prototypes
from conftest import ROOT, load_golden
from host_lib import built_library as _build_lib
from parallel_reverb_raytracer_amd import capi, dtypes
from parallel_reverb_raytracer_amd.dtypes import IMPULSE, NUM_IMAGE_SOURCE

# the header's structures and their Python mirrors (numpy dtypes and ctypes.Structure classes); rvb_float3 is a row of four floats
MIRRORS = {"rvb_triangle": dtypes.TRIANGLE, "rvb_surface": dtypes.SURFACE, "rvb_impulse": dtypes.IMPULSE, "rvb_attenuated_impulse": dtypes.ATTENUATED,
           "rvb_speaker": dtypes.SPEAKER, "rvb_image_candidate": capi.IMAGE_CANDIDATE, "rvb_source_pattern": capi.SourcePattern,
           "rvb_source_orientation": capi.SourceOrientation, "rvb_pipeline_result": capi.PipelineResult, "rvb_pipeline_options": capi.PipelineOptions}


def test_library_exports_every_declared_symbol():
    """For every prototype the header declares: the table has the name, at the header's place, with the same number of parameters and
    the same class for each parameter and for the return type; the library exports the name and carries that signature."""
    lib = _build_lib()
    declared = prototypes()
    with open(HEADER) as f:
        assert set(re.findall(r"\b(rvb_[a-z_0-9]+)\s*\(", f.read())) == {name for name, _, _ in declared}     # no prototype escaped the parser
    assert [name for name, _, _ in declared] == capi.SYMBOLS and len(declared) == 92
    for name, returns, parameters in declared:
        restype, *argtypes = capi._SIGNATURES[name]
        assert restype is CLASSES[returns], name
        assert len(argtypes) == len(parameters), name
        assert argtypes == [CLASSES[p] for p in parameters], name
        function = getattr(lib, name)
        assert function.restype is restype and list(function.argtypes) == argtypes, name


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """tests/cpp/capi_layout.c compiled with the system's C compiler against the header, run: its lines, split."""
    compiler = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc") or "/opt/rocm/llvm/bin/clang"
    tool = str(tmp_path_factory.mktemp("capi_layout") / "capi_layout")
    subprocess.check_call([compiler, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "capi_layout.c"), "-o", tool])
    facts = {"sizeof": {}, "field": {}, "value": {}}
    for line in subprocess.check_output([tool], universal_newlines=True).splitlines():
        kind, name, *rest = line.split()
        if kind == "field":
            facts[kind].setdefault(name, []).append((rest[0].rstrip("_"), int(rest[1]), int(rest[2]), rest[3]))
        else:
            assert name not in facts[kind]
            facts[kind][name] = int(rest[0])
    return facts


def _ctypes_kind(kind):
    if issubclass(kind, ctypes.Array):
        return _ctypes_kind(kind._type_)
    return {ctypes.c_float: "f", ctypes.c_uint64: "u", ctypes.c_uint32: "u", ctypes.POINTER(ctypes.c_float): "p"}[kind]


def _fields(mirror):
    """[(member, offset, bytes, kind of the element: f float, u unsigned integer, p pointer to float, s the impulse structure)]"""
    if isinstance(mirror, np.dtype):
        kinds = {"f": "f", "u": "u", "V": "s"}
        return sorted(((name, offset, sub.itemsize, kinds[sub.base.kind]) for name, (sub, offset) in mirror.fields.items()), key=lambda f: f[1])
    return [(name, getattr(mirror, name).offset, getattr(mirror, name).size, _ctypes_kind(kind)) for name, kind in mirror._fields_]


def test_pod_sizes_match_reference_contract(layout):
    for name, size in (("rvb_triangle", 32), ("rvb_float3", 16), ("rvb_surface", 64), ("rvb_impulse", 64),
                       ("rvb_attenuated_impulse", 64), ("rvb_speaker", 32), ("rvb_image_candidate", 80)):
        assert layout["sizeof"][name] == size, name
    assert capi.IMAGE_CANDIDATE.itemsize == 80
    assert dtypes.float3_array([(1.0, 2.0, 3.0)]).nbytes == layout["sizeof"]["rvb_float3"]


def test_python_mirrors_have_the_compiled_layout(layout):
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    structs = set(re.findall(r"typedef\s+struct\s*\{[^}]*\}\s*(\w+)\s*;", text))
    assert structs == set(layout["sizeof"]) == set(MIRRORS) | {"rvb_float3"}         # every struct typedef of the header is measured
    for name, mirror in MIRRORS.items():
        size = mirror.itemsize if isinstance(mirror, np.dtype) else ctypes.sizeof(mirror)
        assert size == layout["sizeof"][name], name
        assert _fields(mirror) == sorted(layout["field"][name], key=lambda f: f[1]), name


def test_python_constants_have_the_header_values(layout):
    values = dict(layout["value"])
    for name in ("NUM_IMAGE_SOURCE", "NUM_BANDS"):
        assert getattr(dtypes, name) == values.pop("RVB_" + name), name
    assert len(values) == 27
    for name, value in values.items():
        assert getattr(capi, name[len("RVB_"):]) == value, name
    assert capi.TABLE_FLOATS == 360 * 180 * layout["value"]["RVB_NUM_BANDS"]


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    _build_lib()
    with pytest.raises(capi.RvbError) as e:
        capi.Context(0)
    assert e.value.code == capi.ERR_NO_DEVICE == 2 and "no CPU path" in str(e.value)


def _candidates_from(image, index):
    nrays = index.shape[0] // NUM_IMAGE_SOURCE
    idx = index.reshape(nrays, NUM_IMAGE_SOURCE)
    rays, slots = np.nonzero(idx[:, 1:])
    cand = np.zeros(rays.shape[0], dtype=capi.IMAGE_CANDIDATE)
    cand["ray"], cand["slot"] = rays, slots + 1
    cand["index"] = idx[rays, slots + 1]
    cand["impulse"] = image.reshape(nrays, NUM_IMAGE_SOURCE)[rays, slots + 1]
    return cand, image[:1].copy()


@pytest.mark.parametrize("name", ["trace_large_square", "trace_echo_tunnel", "trace_random_pillars", "trace_vault"])
@pytest.mark.parametrize("remove_direct", [False, True])
def test_merge_images_equals_reference_dedup(oracle, name, remove_direct):
    _build_lib()
    g = load_golden(name)
    nrays = g["directions"].shape[0]
    image = np.zeros(nrays * NUM_IMAGE_SOURCE, dtype=IMPULSE)
    image["volume"], image["time"] = g["image_volume"], g["image_time"]
    image["position"][:, :3] = g["image_position"]
    want = oracle.collect_images(image, g["image_index"], remove_direct)
    cand, direct = _candidates_from(image, g["image_index"])
    rng = np.random.default_rng(0)
    got = capi.merge_images(cand[rng.permutation(cand.shape[0])], direct, remove_direct)   # order must not matter
    assert got.shape == want.shape
    for f in ("volume", "position", "time"):
        assert np.array_equal(got[f], want[f])


def test_merge_images_key_collision_first_ray_wins():
    """Quirk Q4: keys with interior zeros collide across different paths; the lowest ray index wins."""
    _build_lib()
    cand = np.zeros(3, dtype=capi.IMAGE_CANDIDATE)
    cand["ray"] = [5, 2, 2]
    cand["slot"] = [3, 3, 1]
    cand["index"] = [7, 7, 9]
    cand["impulse"]["time"] = [0.5, 0.25, 0.125]
    direct = np.zeros(1, dtype=IMPULSE)
    direct["time"] = 0.01
    out = capi.merge_images(cand, direct, False)
    # keys: {0} direct, ray5 {0,0,0,7}, ray2 {0,9}, ray2 {0,9,0,7}; std::map order is lexicographic
    assert list(out["time"]) == [np.float32(0.01), np.float32(0.5), np.float32(0.125), np.float32(0.25)]
    assert list(capi.merge_images(cand, direct, True)["time"]) == [np.float32(0.5), np.float32(0.125), np.float32(0.25)]
