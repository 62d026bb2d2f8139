"""The trace stage on the constructed scenes of tests/bvh_edges.py, bit for bit against the CPU oracle's brute-force scan: raw diffuse
records (positions, times, volumes), image candidates, the direct slot and the merged images with and without the direct path — through
all three path kernels (four, two and one lane per ray), and through the four-lane and one-lane shadow kernels in child processes.
tests/test_bvh_edge_inputs.py shows what the scenes hold (exact ties across leaves and subtrees, root-only trees, a tree without any
triangle, a traversal stack of 45 and 47 entries, coordinates up to 5e8 and a blocked axis-parallel line of sight there),
tests/test_bvh_host.py checks the builder alone."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import bvh_edges as E
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, NUM_IMAGE_SOURCE

pytestmark = pytest.mark.gpu

CASES = list(E.all_cases())
MAX_RAYS_PER_LAUNCH = 700
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module", params=["four_lanes_per_ray", "two_lanes_per_ray", "one_lane_per_ray"])
def ctx(request):
    """All three path kernels, as in tests/test_gpu_parity.py."""
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    if request.param == "two_lanes_per_ray":
        c.set_concurrent_traces(1 << 20)
    if request.param == "one_lane_per_ray":
        c.set_path_lanes(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built_cases():
    """name -> the built case, shared by every test of the module (and left unchanged)."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = E.all_cases()[name]()
        return made[name]
    return get


@pytest.fixture(scope="module")
def reference(oracle, built_cases):
    """name -> the oracle's (impulses, image, index) per source, computed once."""
    done = {}

    def get(name):
        if name not in done:
            scene, mic, _, dirs, nrefl = case = built_cases(name)
            done[name] = [oracle.raytrace(scene, mic, s, dirs, nrefl, AIR_COEFFICIENTS) for s in E.sources_of(case)]
        return done[name]
    return get


@pytest.fixture(scope="module")
def kept_by_the_host_builder(tmp_path_factory, built_cases):
    """name -> the number of triangles the builder keeps, from tests/cpp/bvh_dump.cpp (built as in tests/test_bvh_host.py)."""
    import test_bvh_host as host
    tool = host.build_dump_tool(tmp_path_factory.mktemp("bvh_dump_gpu"))
    base = tmp_path_factory.mktemp("bvh_kept")
    done = {}

    def get(name):
        if name not in done:
            dump = host.run_dump(tool, built_cases(name)[0], base / name)
            assert dump["error"] == ""
            done[name] = dump["tris"].shape[0]
        return done[name]
    return get


def trace_case(ctx, case):
    """The case through the context: per source a dict of diffuse records, image candidates (ray numbers of the source's own trace) and
    the direct slot.  One source is one rvb_trace; a set of sources goes into several-pairs launches of at most 700 rays.  Every launch
    runs twice: the second must give the bytes of the first."""
    scene, mic, _, dirs, nrefl = case
    sources = E.sources_of(case)
    ctx.set_scene(scene)
    ctx.set_directions(dirs)
    nrays = dirs.shape[0]
    out = []
    if sources.shape[0] == 1:
        ctx.trace(mic, sources[0], nrefl, AIR_COEFFICIENTS)
        result = {"diffuse": ctx.get_raw_diffuse(), "candidates": ctx.get_image_candidates(), "direct": ctx.get_direct()}
        ctx.trace(mic, sources[0], nrefl, AIR_COEFFICIENTS)
        assert ctx.get_raw_diffuse().tobytes() == result["diffuse"].tobytes(), "second trace"
        return [result]
    per_launch = max(1, MAX_RAYS_PER_LAUNCH // nrays)
    for first in range(0, sources.shape[0], per_launch):
        batch = sources[first:first + per_launch]
        mics = np.repeat(np.asarray(mic, np.float64)[None], batch.shape[0], 0)
        ctx.trace_pairs(mics, batch, nrefl, AIR_COEFFICIENTS)
        diffuse = ctx.get_raw_diffuse()
        candidates = ctx.get_image_candidates()
        for p in range(batch.shape[0]):
            ctx.select_pair(p)
            out.append({"diffuse": diffuse.reshape(batch.shape[0], -1)[p], "candidates": ctx.get_pair_candidates(p, candidates), "direct": ctx.get_direct()})
        ctx.trace_pairs(mics, batch, nrefl, AIR_COEFFICIENTS)
        assert ctx.get_raw_diffuse().tobytes() == diffuse.tobytes(), "second trace"
    return out


def diffuse_crc(results):
    return zlib.crc32(b"".join(r["diffuse"].tobytes() for r in results))


def assert_impulses_equal(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got["position"][:, :3], want["position"][:, :3]), what + " positions"
    assert np.array_equal(got["time"], want["time"]), what + " times"
    assert got["volume"].tobytes() == want["volume"].tobytes(), what + " volumes"


@pytest.mark.parametrize("name", CASES)
def test_constructed_scene_matches_brute_force(ctx, oracle, built_cases, reference, kept_by_the_host_builder, name):
    from parallel_reverb_raytracer_amd import capi
    case = built_cases(name)
    nrays = case[3].shape[0]
    results = trace_case(ctx, case)
    assert ctx.scene_info()["kept_triangles"] == kept_by_the_host_builder(name)
    wants = reference(name)
    assert len(results) == len(wants)
    for k, (got, (impulses, image, index)) in enumerate(zip(results, wants)):
        what = "%s source %d" % (name, k)
        assert_impulses_equal(got["diffuse"], impulses, what)
        assert not got["diffuse"]["pad"].any() and not got["diffuse"]["position"][:, 3].any()
        idx = index.reshape(nrays, NUM_IMAGE_SOURCE)
        rays, slots = np.nonzero(idx[:, 1:])
        cand = got["candidates"]
        assert cand.shape[0] == rays.shape[0], what
        assert np.array_equal(cand["ray"], rays) and np.array_equal(cand["slot"], slots + 1), what
        assert np.array_equal(cand["index"], idx[rays, slots + 1]), what
        assert_impulses_equal(cand["impulse"], image.reshape(nrays, NUM_IMAGE_SOURCE)[rays, slots + 1], what + " candidates")
        assert_impulses_equal(got["direct"], image[:1], what + " direct")
        for remove_direct in (False, True):
            assert_impulses_equal(capi.merge_images(cand, got["direct"], remove_direct), oracle.collect_images(image, index, remove_direct),
                                  what + " images")


def child_main():
    """What the child processes of the shadow-kernel test run: every case through a default context, one line per case."""
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)
    for name, make in E.all_cases().items():
        results = trace_case(c, make())
        print("CRC", name, diffuse_crc(results), sorted(dict(c.last_timings())))
    c.close()


def test_other_shadow_kernels_give_the_same_bytes(reference):
    """RVB_SHADOW_LANES=4 (the four-lane shadow kernel) and =1 (one lane per record), read once per process: a child process each traces
    every case; per case the CRC of its diffuse records is that of the oracle's, which this process's kernels are held to above."""
    want = {name: zlib.crc32(b"".join(impulses.tobytes() for impulses, _, _ in reference(name))) for name in CASES}
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import rvb_import; rvb_import.load();"
            "import test_gpu_bvh_edges as t; t.child_main()") % (os.path.dirname(TESTS), TESTS)
    for lanes, kernel in (("4", "shadow_kernel"), ("1", "shadow_lane_kernel")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RVB_SHADOW_LANES=lanes), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = {l.split()[1]: l for l in out.stdout.splitlines() if l.startswith("CRC ")}
        assert sorted(lines) == sorted(CASES)
        for name in CASES:
            assert int(lines[name].split()[2]) == want[name], (lanes, name)
            if name != "none_hittable":                                # (no record: the shadow stage may have nothing to launch)
                assert "'%s'" % kernel in lines[name] and "shadow_pair_kernel" not in lines[name], lines[name]
