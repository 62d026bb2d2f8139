"""A new microphone on a kept trace (rvb_keep_paths with RVB_KEEP_LISTENER / rvb_relisten, csrc/relisten_kernels.hip): the work records
of the path stage restored, then the shadow and image stages of a trace.  The contract is "the bytes a full trace with the new microphone
would have produced", so every expectation is the CPU oracle's trace with that microphone (oracle.raytrace, oracle.collect_images);
nothing is compared with a second GPU trace but the two fixed-order sums named below (rvb_reshade_grad, listeners.decay_map).

Bars: records, direct slots, merged images, time ranges bit for bit.  Every test asserts its ground on the oracle's data first."""
import itertools

import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, aligned_copy

from test_gpu_reshade import AIR_B, SPEAKERS, assert_state, oracle_case, set_b, spread_over_70, time_range
from test_gpu_source_pattern import FACING, SHAPES, bits, expected_records, oracle_range, same_records

pytestmark = pytest.mark.gpu

# A is the scene's own microphone (asserted in the fixture); the direct path is visible from A and C and hidden from B
MICS = {"A": (14.0, 1.6, -0.9), "B": (9.12, 0.4, -8.33), "C": (-10.28, 3.85, -2.24)}
SOURCE_2 = (-12.0, 2.5, 3.0)
SEED = 23
# shapes that miss assert_ground under seed 23: 8 x 33 has 23 records that see one microphone and not the other where 27 are asked
# for (seed 1: 39); 8 x 1 leaves every record of microphone C without volume (seed 4 meets every precondition)
SEEDS = {(8, 33): 1, (8, 1): 4}


@pytest.fixture(scope="module")
def cathedral():
    scene, info = scenes.cathedral(3000)
    assert tuple(np.float32(info["mic"])) == tuple(np.float32(MICS["A"]))
    return {"scene": scene, "mic": info["mic"], "source": info["source"], "B": set_b(scene[2], 2, 4, 5)}


@pytest.fixture(scope="module")
def ctx(cathedral):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(cathedral["scene"])
    c.keep_paths(True, listener=True)
    yield c
    c.close()


def mic_cases(oracle, cathedral, nrays, nrefl, surfaces=None, air=AIR_COEFFICIENTS, tag="own", source=None):
    """{name: oracle case} for the three microphones"""
    seed = SEEDS.get((nrays, nrefl), SEED)
    dirs = scenes.sphere_directions(nrays, seed=seed)
    table = cathedral["scene"][2] if surfaces is None else surfaces
    src = cathedral["source"] if source is None else source
    return {m: oracle_case(oracle, cathedral["scene"], table, MICS[m], src, dirs, nrefl, air, key=("relisten", m, nrays, nrefl, tag)) for m in MICS}


def visible(case):
    return case["diffuse"]["time"] != 0


def live(case):
    return (case["diffuse"]["volume"] != 0).any(axis=1)


def assert_ground(cases, one_sided=1):
    """The microphones must matter: under each some records are live and some dead, every two of them differ in their records, in which
    records see the microphone (in both directions) and in the time range."""
    for name, case in cases.items():
        assert live(case).any() and not live(case).all(), name
    for x, y in itertools.permutations(cases, 2):
        assert not same_records(cases[x]["diffuse"], cases[y]["diffuse"]), (x, y)
        assert (visible(cases[x]) & ~visible(cases[y])).sum() >= one_sided, (x, y)
        assert oracle_range(cases[x]["diffuse"]) != oracle_range(cases[y]["diffuse"]), (x, y)


def assert_direct_ground(cases):
    assert (cases["A"]["images"]["volume"][0] != 0).any() and (cases["C"]["images"]["volume"][0] != 0).any()
    assert not cases["B"]["images"][:1].view(np.uint32).any(), "the direct path is not hidden from B"


def relisten_names(ctx, pattern=False):
    names = [k for k, _ in ctx.last_timings()]
    assert "relisten_records_kernel" in names and "image_kernel" in names and sum("shadow" in k for k in names) == 1, names
    assert ("source_pattern_kernel" in names) == pattern, names
    assert not any("path" in k for k in names) and "record_sort_kernels" not in names, names
    assert len(names) == (4 if pattern else 3), names


# records that see one microphone and not the other, at least (a precondition on the oracle's data): 1000 at 509 x 24 and 27 at every
# other shape but one — 8 x 1 has eight records in all, and there assert_ground's own floor of 1 is all the ground there can be
ONE_SIDED = {(509, 24): 1000, (8, 1): 1}


@pytest.mark.parametrize("nrays,nrefl", [(509, 24), (5, 70), (130, 64), (8, 33), (17, 32), (8, 1)])
def test_relistened_records_equal_the_oracle_trace_with_the_other_microphone(ctx, oracle, cathedral, nrays, nrefl):
    """509 x 24: a partial last wave and a ray shorter than a tile; 5 x 70: a ray longer than a tile and fewer rays than a wave takes;
    130 x 64: nrefl % 32 == 0 selects the 16-bit key runs of the trace.  The edges of a wave and of a tile: 8 x 33: exactly one wave's
    rays, a second tile that holds one bounce; 17 x 32: a last wave of one ray, exactly one tile; 8 x 1: a single bounce."""
    cases = mic_cases(oracle, cathedral, nrays, nrefl)
    assert_ground(cases, one_sided=ONE_SIDED.get((nrays, nrefl), 27))
    assert_direct_ground(cases)
    if nrays == 509:
        assert all(c["images"].shape[0] >= 3 for c in cases.values())
    a = cases["A"]
    ctx.raytrace(a["mic"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
    assert "path_keep_kernel" in [k for k, _ in ctx.last_timings()]
    executed = ctx.executed_bounces()
    assert executed > 0
    assert_state(ctx, a)                                             # keeping changes nothing
    for m in "BCA":                                                  # B: the hidden direct path; A: back to the original trace
        ctx.relisten(MICS[m])
        relisten_names(ctx)
        assert_state(ctx, cases[m])
        assert ctx.executed_bounces() == executed


def test_the_surface_table_read_through_l2(oracle, cathedral):
    """130 x 24 with the seven surfaces spread over a table of 70 (test_gpu_reshade.spread_over_70): relisten_records_kernel reads the
    table from memory.  The records carry no surface number, so the seven-surface oracle cases are the expectation, byte for byte."""
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = 130, 24
    cases = mic_cases(oracle, cathedral, nrays, nrefl)
    assert_ground(cases)
    assert_direct_ground(cases)
    a = cases["A"]
    wide_scene, = spread_over_70(cathedral["scene"])
    c = capi.Context(0)
    try:
        c.set_scene(wide_scene)
        c.keep_paths(True, listener=True)
        c.raytrace(a["mic"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
        assert_state(c, a)
        for m in "CB":
            c.relisten(MICS[m])
            relisten_names(c)
            assert_state(c, cases[m])
    finally:
        c.close()


def test_the_kept_order_survives_a_full_exact_impulse_response(ctx, oracle, cathedral):
    """The exact binning sorts in the context's buffers; the grouping order of the records must not be one of them."""
    from parallel_reverb_raytracer_amd import capi
    cases = mic_cases(oracle, cathedral, 130, 64)
    assert_ground(cases)
    a = cases["A"]
    ctx.raytrace(a["mic"], a["source"], a["dirs"], 64, AIR_COEFFICIENTS)
    ctx.ir_configure_speakers(a["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, ctx.get_raw_images(False))
    ir = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
    assert ir.any()
    ctx.relisten(MICS["C"])
    assert_state(ctx, cases["C"])


def test_relisten_with_reshading_and_gradients(ctx, oracle, cathedral):
    from parallel_reverb_raytracer_amd import capi
    from test_gpu_reshade_grad import on_device, weights
    nrays, nrefl = 509, 24
    own = mic_cases(oracle, cathedral, nrays, nrefl)
    other = mic_cases(oracle, cathedral, nrays, nrefl, cathedral["B"], AIR_B, "B")
    assert_ground(own, one_sided=1000)
    assert_ground(other)
    assert not same_records(own["C"]["diffuse"], other["C"]["diffuse"]) and not same_records(own["C"]["images"], other["C"]["images"])
    a = own["A"]
    ctx.raytrace(a["mic"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
    ctx.reshade(cathedral["B"], AIR_B)
    assert_state(ctx, other["A"])
    ctx.relisten(MICS["C"])                                          # the table and the air of the re-shade, microphone C
    assert_state(ctx, other["C"])
    ctx.reshade(None, AIR_COEFFICIENTS)                              # the re-shade works from the new microphone
    assert_state(ctx, own["C"])

    # rvb_reshade_grad after the relisten against a fresh kept trace at C on a second context: the one comparison of two GPU results
    # here, both fixed-order sums over identical records
    sr = 44100.0
    def gradient(c):
        c.ir_configure_speakers(MICS["C"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        nbins = c.ir_bins(c.ir_time_range()[1], 0.0, sr)
        w = on_device(weights(2, nbins, 5))
        return nbins, c.reshade_grad(0.0, sr, nbins, w.data_ptr())
    nbins, (grads, grad_air) = gradient(ctx)
    assert grads["specular"].any() and grads["diffuse"].any() and grad_air.any()
    fresh = capi.Context(0)
    try:
        fresh.set_scene(cathedral["scene"])
        fresh.keep_paths(True)
        fresh.raytrace(MICS["C"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
        nbins_fresh, (want, want_air) = gradient(fresh)
    finally:
        fresh.close()
    assert nbins_fresh == nbins and grads.tobytes() == want.tobytes() and grad_air.tobytes() == want_air.tobytes()


def test_every_pair_of_trace_pairs_is_relistened(ctx, oracle, cathedral):
    """2 pairs x 67 rays x 24: 67 is no multiple of 8, so one wave of the restore kernel holds rays of both pairs."""
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = 67, 24
    sources = np.array([cathedral["source"], SOURCE_2], np.float32)
    dirs = scenes.sphere_directions(nrays, seed=SEED)
    first = mic_cases(oracle, cathedral, nrays, nrefl)
    second = mic_cases(oracle, cathedral, nrays, nrefl, tag="source 2", source=SOURCE_2)
    assert_ground(first)
    assert_ground(second)                                            # the second source is inside the room and its rays live and die
    assert not same_records(first["A"]["diffuse"], second["A"]["diffuse"])

    def assert_pairs(want):
        diffuse, cand = ctx.get_raw_diffuse().reshape(2, -1), ctx.get_image_candidates()
        for p in range(2):
            assert same_records(diffuse[p], want[p]["diffuse"]), p
            assert not diffuse[p]["pad"].any() and not diffuse[p]["position"][:, 3].any()
            ctx.select_pair(p)
            direct = ctx.get_direct()
            assert same_records(direct, want[p]["images"][:1]), p
            images = capi.merge_images(ctx.get_pair_candidates(p, cand), direct, False)
            assert images.shape == want[p]["images"].shape and same_records(images, want[p]["images"]), p
            assert time_range(ctx, want[p]["mic"]) == oracle_range(want[p]["diffuse"]), p

    ctx.set_directions(dirs)
    try:
        ctx.trace_pairs(np.array([MICS["A"], MICS["C"]], np.float32), sources, nrefl, AIR_COEFFICIENTS)
        executed = ctx.executed_bounces()
        assert_pairs([first["A"], second["C"]])
        with pytest.raises(capi.RvbError) as e:
            ctx.relisten(MICS["B"])                                  # one microphone for two pairs
        assert e.value.code == capi.ERR_INVALID
        ctx.relisten([MICS["B"], MICS["A"]])
        relisten_names(ctx)
        assert_pairs([first["B"], second["A"]])
        assert ctx.executed_bounces() == executed
    finally:
        ctx.npairs = 1


def test_a_source_pattern_is_applied_with_the_new_microphone(ctx, oracle, cathedral):
    """The direct and image impulses take their gain from mic - position: the new microphone's."""
    nrays, nrefl = 130, 24
    cases = mic_cases(oracle, cathedral, nrays, nrefl)
    assert_ground(cases)
    diffuse, images, g_diffuse, g_images = expected_records(oracle, cases["C"], FACING, SHAPES)
    assert (g_diffuse < 0).any() and (g_diffuse > 0).any()
    assert (images["volume"][0] != 0).any() and (images["volume"][:1, 1:] != cases["C"]["images"]["volume"][:1, 1:]).any()
    a = cases["A"]
    ctx.set_source_pattern(FACING, SHAPES)
    try:
        ctx.raytrace(a["mic"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
        ctx.relisten(MICS["C"])
        relisten_names(ctx, pattern=True)
        got_diffuse, got_direct, got_images, got_range = ctx.get_raw_diffuse(), ctx.get_direct(), ctx.get_raw_images(False), time_range(ctx, MICS["C"])
    finally:
        ctx.set_source_pattern(None)
    assert same_records(got_diffuse, diffuse) and same_records(got_direct, images[:1])
    assert got_images.shape == images.shape and same_records(got_images, images)
    assert got_range == oracle_range(diffuse)


@pytest.mark.parametrize("pattern", [False, True])
def test_slots_behind_an_escape_are_zero_again(oracle, pattern):
    """scenes.shoebox() without its last two triangles: rays leave the room.  The restore pass must zero their remaining slots: under a
    source pattern the last pass left -0 in them, and a second scaling of -0 would give +0 where a trace gives -0."""
    from parallel_reverb_raytracer_amd import capi
    triangles, vertices, surfaces = scenes.shoebox()
    scene = (aligned_copy(triangles[:-2]), vertices, surfaces)
    mic_1, mic_2, src, nrays, nrefl = (0.5, 1.0, 2.0), (-1.1, 2.0, 30.0), (-0.7, -1.2, -5.0), 130, 24
    dirs = scenes.sphere_directions(nrays, seed=3)
    one = oracle_case(oracle, scene, surfaces, mic_1, src, dirs, nrefl, AIR_COEFFICIENTS)
    two = oracle_case(oracle, scene, surfaces, mic_2, src, dirs, nrefl, AIR_COEFFICIENTS)
    empty = ~one["diffuse"].view(np.uint32).reshape(-1, 16).any(axis=1)
    assert np.array_equal(empty, ~two["diffuse"].view(np.uint32).reshape(-1, 16).any(axis=1))
    per_ray = empty.reshape(nrays, nrefl)
    assert empty.sum() >= 1000 and not per_ray[:, 0].all() and not per_ray[:, -1].all(), "too few escaping rays, or too many"
    assert live(one).sum() >= 100 and live(two).sum() >= 100 and not same_records(one["diffuse"], two["diffuse"])
    want = two["diffuse"], two["images"]
    if pattern:
        want = expected_records(oracle, two, FACING, SHAPES)[:2]
        assert (bits(want[0]["volume"][empty]) == 0x80000000).any(), "no empty slot under a negative gain"
    c = capi.Context(0)
    try:
        c.set_scene(scene)
        c.keep_paths(True, listener=True)
        if pattern:
            c.set_source_pattern(FACING, SHAPES)
        c.raytrace(mic_1, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.relisten(mic_2)
        got = c.get_raw_diffuse()
        assert same_records(got, want[0]) and not got["pad"].any() and not got["position"][:, 3].any()
        assert same_records(c.get_direct(), want[1][:1])
        images = c.get_raw_images(False)
        assert images.shape == want[1].shape and same_records(images, want[1])
        assert time_range(c, mic_2) == oracle_range(want[0])
        raw = got.view(np.uint32).reshape(-1, 16)
        if pattern:
            assert not raw[empty][:, 8:].any()                       # (the volumes are 0 times the ray's gain, as a trace leaves them)
        else:
            assert not raw[empty].any()
    finally:
        c.close()


def test_state_and_arguments(oracle, cathedral):
    from parallel_reverb_raytracer_amd import capi
    cases = mic_cases(oracle, cathedral, 509, 24)
    a = cases["A"]

    def refused(c, code, mics=MICS["C"]):
        with pytest.raises(capi.RvbError) as e:
            c.relisten(mics)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    c = capi.Context(0)
    try:
        c.set_scene(cathedral["scene"])
        refused(c, capi.ERR_STATE)                                    # before any trace
        c.keep_paths(True)
        c.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
        assert "RVB_KEEP_LISTENER" in refused(c, capi.ERR_STATE)      # kept for re-shading only
        assert_state(c, a)
        c.keep_paths(True, listener=True)
        refused(c, capi.ERR_STATE)                                    # switching it on afterwards does not change that
        c.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
        refused(c, capi.ERR_INVALID, [MICS["B"], MICS["C"]])          # two microphones for one pair
        refused(c, capi.ERR_INVALID, (1.0, float("nan"), 0.0))
        refused(c, capi.ERR_INVALID, (float("inf"), 0.0, 0.0))
        assert_state(c, a)                                           # a failed relisten leaves the trace's results
        c.relisten(MICS["C"])
        assert_state(c, cases["C"])
        c.set_directions(a["dirs"])
        refused(c, capi.ERR_STATE)
        c.trace(a["mic"], a["source"], 24, AIR_COEFFICIENTS)
        c.keep_paths(False)
        refused(c, capi.ERR_STATE)                                    # the side buffers are gone
        assert_state(c, a)
    finally:
        c.close()


def test_keeping_for_materials_alone_is_unchanged(oracle, cathedral):
    from parallel_reverb_raytracer_amd import capi
    a = mic_cases(oracle, cathedral, 509, 24)["A"]
    b = oracle_case(oracle, cathedral["scene"], cathedral["B"], a["mic"], a["source"], a["dirs"], 24, AIR_B, key=("relisten", "A", 509, 24, "B"))
    c = capi.Context(0)
    try:
        c.set_scene(cathedral["scene"])
        c.keep_paths(True)
        c.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
        names = [k for k, _ in c.last_timings()]
        assert names.count("path_keep_kernel") == 1 and not any("relisten" in k for k in names)
        assert_state(c, a)
        c.reshade(cathedral["B"], AIR_B)
        names = [k for k, _ in c.last_timings()]
        assert names == ["reshade_kernel", "reshade_images_kernel"]
        assert_state(c, b)
    finally:
        c.close()


def test_decay_map_equals_a_fresh_trace_per_listener(ctx, oracle, cathedral):
    """listeners.decay_map over [A, C], mono omni, RVB_IR_EXACT: bit for bit the values of a fresh kept trace per listener through the
    same calls (fixed-order sums over identical records)."""
    import torch
    from parallel_reverb_raytracer_amd import capi, listeners
    nrays, nrefl, sr = 130, 64, 44100.0
    cases = mic_cases(oracle, cathedral, nrays, nrefl)
    assert_ground(cases)
    speakers = ([(0.0, 0.0, 1.0)], [0.0])
    nbins = ctx.ir_bins(max(oracle_range(cases[m]["diffuse"])[1] for m in "AC"), 0.0, sr)
    a = cases["A"]
    ctx.raytrace(MICS["B"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)       # the kept trace is at neither listener
    got = listeners.decay_map(ctx, [MICS["A"], MICS["C"]], speakers, sr, nbins)
    assert got.shape == (2, 1, 8) and got.dtype == np.float32
    print("decay_map T30 [A, C]:", got.tolist())
    want = np.zeros_like(got)
    fresh = capi.Context(0)
    try:
        fresh.set_scene(cathedral["scene"])
        for i, m in enumerate("AC"):
            fresh.raytrace(MICS[m], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
            fresh.ir_configure_speakers(MICS[m], speakers[0], speakers[1], capi.IR_DIFFUSE, None)
            hist = torch.zeros((1, 8, nbins), dtype=torch.float32, device="cuda")
            curve = torch.empty_like(hist)
            fresh.ir_accumulate_tensor(0.0, sr, nbins, capi.IR_EXACT, hist)
            fresh.decay_curve(hist.data_ptr(), 8, nbins, curve.data_ptr())
            want[i] = fresh.decay_times(curve.data_ptr(), 8, nbins, sr).reshape(1, 8)
    finally:
        fresh.close()
    assert np.isfinite(want).any() and not np.array_equal(bits(want[0]), bits(want[1])), "no decay time, or the same at both listeners"
    assert np.array_equal(bits(got), bits(want))
