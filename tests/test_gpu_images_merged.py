"""The merged image list made on the device (rvb_ir_configure_speakers_merged / rvb_ir_configure_hrtf_merged of
include/rvb_capi_images.h; csrc/images.hip, image_gather_kernel) on the constructed room of tests/image_edges.py.

The contract is "the context is left exactly as the existing configure call would leave it with images = the host merge", so every
expectation is the SAME context configured through the host path — get_image_candidates, get_direct, merge_images, ir_configure_* —,
whose pieces the oracle tests pin (tests/test_gpu_image_edges.py): the time range and the RVB_IR_EXACT histogram byte for byte, the
number of images, for three models, remove_direct 0 and 1, after the trace, after a re-shade (where the list comes from the cache and
the call is one gather), after a relisten (where the winners change), for a pair of a launch of three, with a ray offset, in the room
with a hole and at the small shapes."""
import ctypes

import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_reshade import AIR_B, SPEAKERS

pytestmark = pytest.mark.gpu

SR = 44100.0
FACING_UP = ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
MODELS = ("speakers all", "speakers images", "hrtf all")


@pytest.fixture(scope="module")
def hrtf_table():
    return scenes.hrtf_synthetic_table()


def make_ctx(hole=False, keep=True):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(E.room(hole=hole))
    if keep:
        c.keep_paths(True, listener=True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def configure(ctx, model, mic, table, images=None, remove_direct=None):
    """images given: the existing call with the host's list; else the merged call.  Returns the number of images."""
    from parallel_reverb_raytracer_amd import capi
    which = capi.IR_IMAGES if model == "speakers images" else capi.IR_ALL
    if model.startswith("speakers"):
        if images is not None:
            ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], which, images)
            return images.shape[0]
        return ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], which, remove_direct)
    if images is not None:
        ctx.ir_configure_hrtf(mic, table, FACING_UP[0], FACING_UP[1], which, images)
        return images.shape[0]
    return ctx.ir_configure_hrtf_merged(mic, table, FACING_UP[0], FACING_UP[1], which, remove_direct)


def results(ctx):
    from parallel_reverb_raytracer_amd import capi
    return ctx.ir_time_range(), ctx.ir_download(True, SR, capi.IR_EXACT).tobytes()


def host_images(ctx, remove_direct, pair=None):
    from parallel_reverb_raytracer_amd import capi
    if pair is None:
        return ctx.get_raw_images(remove_direct)
    return capi.merge_images(ctx.get_pair_candidates(pair), ctx.get_direct(), remove_direct)


def assert_same_as_the_host_path(ctx, mic, table, what, pair=None, models=MODELS, expect_images=None):
    """merged, host, merged again (the list now comes from the cache, or is made anew after the other remove_direct): all equal."""
    for model in models:
        for remove_direct in (False, True):
            label = "%s, %s, remove_direct %d" % (what, model, remove_direct)
            n0 = configure(ctx, model, mic, table, remove_direct=remove_direct)
            assert "image_gather_kernel" in [k for k, _ in ctx.last_timings()] or n0 == 0, label
            first = results(ctx)
            images = host_images(ctx, remove_direct, pair)
            n1 = configure(ctx, model, mic, table, images=images)
            want = results(ctx)
            n2 = configure(ctx, model, mic, table, remove_direct=remove_direct)
            again = results(ctx)
            assert n0 == n1 == n2, label + ": %d images, the host list has %d" % (n0, n1)
            assert first[0] == want[0] and again[0] == want[0], label + ": time range %r, the host path gives %r" % (first[0], want[0])
            assert first[1] == want[1] and again[1] == want[1], label + ": the exact histogram differs from the host path's"
            if expect_images is not None:
                assert n1 == expect_images[remove_direct], label
            assert np.frombuffer(want[1], np.float32).any(), label + ": an empty histogram shows nothing"


def test_main_shape_after_the_trace_a_reshade_and_a_relisten(ctx, hrtf_table):
    """509 x 12, pair 0: 801 candidates merge into 161 images (the de-dup is exercised).  After reshade(table B, AIR_B) the volumes on the
    device have changed and the winners have not; after relisten to MICS[1] the winners change."""
    nrays, nrefl = E.MAIN
    mic, src = E.PAIRS[0]
    ctx.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
    assert ctx.get_image_candidates().shape[0] == 801
    assert_same_as_the_host_path(ctx, mic, hrtf_table, "after the trace", expect_images={False: 161, True: 160})
    before = ctx.get_raw_images(False)
    table_b, air_b = E.tables()["B"]
    ctx.reshade(table_b, air_b)
    after = ctx.get_raw_images(False)
    assert before.shape == after.shape and (before["volume"] != after["volume"]).any() and before["position"].tobytes() == after["position"].tobytes()
    assert_same_as_the_host_path(ctx, mic, hrtf_table, "after reshade(B, AIR_B)", expect_images={False: 161, True: 160})
    mic1 = tuple(float(x) for x in E.MICS[1])
    ctx.relisten(mic1)
    moved = ctx.get_raw_images(False)
    assert moved.shape != after.shape or moved["position"].tobytes() != after["position"].tobytes(), "the relisten leaves the winners alone"
    assert_same_as_the_host_path(ctx, mic1, hrtf_table, "after relisten to MICS[1]")
    ctx.reshade(E.surfaces(), AIR_B)
    assert_same_as_the_host_path(ctx, mic1, hrtf_table, "after the relisten and a reshade", models=MODELS[:1])


def test_a_pair_of_a_launch_of_three(ctx, hrtf_table):
    nrays, nrefl = E.MAIN
    ctx.set_directions(E.directions(nrays))
    try:
        ctx.trace_pairs(E.MICS, E.SOURCES, nrefl, AIR_COEFFICIENTS)
        ctx.select_pair(1)
        mic = tuple(float(x) for x in E.MICS[1])
        assert not E.DIRECT_VISIBLE[1] and not ctx.get_direct()["volume"].any()      # a hidden direct path: one dead impulse in the list
        assert_same_as_the_host_path(ctx, mic, hrtf_table, "pair 1 of 3", pair=1)
        ctx.select_pair(2)                      # another pair: the cached list is pair 1's and must not be used
        assert_same_as_the_host_path(ctx, tuple(float(x) for x in E.MICS[2]), hrtf_table, "pair 2 of 3", pair=2, models=MODELS[:1])
        ctx.reshade(E.tables()["B"][0], AIR_B)
        ctx.select_pair(1)
        assert_same_as_the_host_path(ctx, mic, hrtf_table, "pair 1 of 3 after a reshade", pair=1, models=MODELS[:2])
    finally:
        ctx.npairs = 1


@pytest.mark.parametrize("shape", [(64, 1), (64, 2), (5, 12)])
def test_small_shapes(ctx, hrtf_table, shape):
    """64 x 1: orders 0 and 1 only; 64 x 2; 5 x 12: fewer rays than a wave"""
    nrays, nrefl = shape
    mic, src = E.PAIRS[0]
    ctx.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
    assert_same_as_the_host_path(ctx, mic, hrtf_table, "%d x %d" % shape, models=MODELS[:1] + MODELS[2:])


def test_the_room_with_a_hole_and_a_ray_offset_without_a_kept_trace(hrtf_table):
    """hole: rays escape.  RAY_OFFSET: the candidates' ray numbers lie above 2^32.  No keep_paths: the list needs no kept trace."""
    nrays, nrefl = E.MAIN
    mic, src = E.PAIRS[0]
    c = make_ctx(hole=True, keep=False)
    try:
        c.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
        assert_same_as_the_host_path(c, mic, hrtf_table, "hole", models=MODELS[:1] + MODELS[2:])
        c.trace(mic, src, nrefl, AIR_COEFFICIENTS, ray_offset=E.RAY_OFFSET)
        assert (c.get_image_candidates()["ray"] >= np.uint64(E.RAY_OFFSET)).all()
        assert_same_as_the_host_path(c, mic, hrtf_table, "hole, ray offset", models=MODELS[:1])
    finally:
        c.close()


def test_ray_offset_in_a_launch_of_pairs(ctx, hrtf_table):
    """a candidate's pair is (ray - ray_offset) / nrays: the offset must not move a candidate into another pair"""
    nrays, nrefl = 64, 9
    ctx.set_directions(E.directions(nrays))
    try:
        ctx.trace_pairs(E.MICS, E.SOURCES, nrefl, AIR_COEFFICIENTS, ray_offset=E.RAY_OFFSET)
        ctx.select_pair(2)
        assert_same_as_the_host_path(ctx, tuple(float(x) for x in E.MICS[2]), hrtf_table, "pair 2 of 3, ray offset", pair=2, models=MODELS[:1])
    finally:
        ctx.npairs = 1
        ctx.ray_offset = 0


def test_refusals_equal_the_existing_calls(hrtf_table):
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = 64, 2
    mic, src = E.PAIRS[0]
    c = make_ctx()

    def code(call):
        try:
            call()
        except capi.RvbError as e:
            return e.code
        return capi.OK

    def both(existing, merged):
        a, b = code(existing), code(merged)
        assert a == b != capi.OK, (a, b)
        return a

    try:
        # nothing traced
        assert both(lambda: c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, None),
                    lambda: c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1])) == capi.ERR_STATE
        assert both(lambda: c.ir_configure_hrtf(mic, hrtf_table, *FACING_UP, capi.IR_ALL, None),
                    lambda: c.ir_configure_hrtf_merged(mic, hrtf_table, *FACING_UP)) == capi.ERR_STATE
        c.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
        # which outside 1..3
        for which in (0, 4):
            assert both(lambda: c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], which, None),
                        lambda: c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], which)) == capi.ERR_INVALID
        # more speakers than RVB_MAX_SPEAKERS
        many = ([(1.0, 0.0, 0.0)] * (capi.MAX_SPEAKERS + 1), [0.5] * (capi.MAX_SPEAKERS + 1))
        assert both(lambda: c.ir_configure_speakers(mic, many[0], many[1], capi.IR_ALL, None),
                    lambda: c.ir_configure_speakers_merged(mic, many[0], many[1])) == capi.ERR_INVALID
        # table == NULL without an earlier table on this context
        fresh = make_ctx()
        try:
            fresh.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
            assert both(lambda: fresh.ir_configure_hrtf(mic, None, *FACING_UP, capi.IR_ALL, None),
                        lambda: fresh.ir_configure_hrtf_merged(mic, None, *FACING_UP)) == capi.ERR_STATE
            fresh.ir_configure_hrtf_merged(mic, hrtf_table, *FACING_UP)
            with_table = results(fresh)
            fresh.ir_configure_hrtf_merged(mic, None, *FACING_UP)           # the table of the call before stays
            assert results(fresh) == with_table
        finally:
            fresh.close()
        # a capacity too small for the download, under either configuration
        count = ctypes.c_uint64(0)
        out = np.zeros(2 * 8 * 4, np.float32)
        for merged in (False, True):
            if merged:
                c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1])
            else:
                c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, c.get_raw_images(False))
            rc = c.lib.rvb_ir_download(c.handle, 1, SR, capi.IR_EXACT, out.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(count))
            assert rc == capi.ERR_CAPACITY and count.value > 4
        # what voids the existing configuration voids this one: a re-shade, a relisten, the selection of a pair, new directions
        for void in (lambda: c.reshade(None, AIR_B), lambda: c.relisten(E.MICS[1]), lambda: c.select_pair(0)):
            c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1])
            void()
            assert code(c.ir_time_range) == capi.ERR_STATE
        c.set_directions(E.directions(nrays))
        assert both(lambda: c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, None),
                    lambda: c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1])) == capi.ERR_STATE
    finally:
        c.close()
