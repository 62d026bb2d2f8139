"""Tabulated source directivity (rvb_set_source_table, csrc/source_kernels.hip): a [360][180][8] gain table at the source end, its row
selected by the departure vector with the reference's own HRTF row rule.  Expected values come from the CPU oracle only: a gain is the
oracle's attenuate_hrtf (channel 0, the test's table and orientation) on a fake unit-volume impulse — diffuse records: fake microphone
0, fake position = the ray's direction; image-source and direct impulses: fake microphone = the impulse's position, fake position = the
real microphone, so that the subtraction is the contract's mic - position —, and expected records are the oracle's records times those
gains in numpy float32.

Bars: records, direct slot, merged images, time ranges and RVB_IR_EXACT histograms bit for bit; RVB_IR_FAST within fast_bound of
tests/test_gpu_speaker_arrays.py."""
import ctypes

import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, aligned_zeros

from attenuation_edges import CANONICAL, OBLIQUE, hrtf_boundary_records, row_code_table, spread_table
from test_gpu_reshade import AIR_B, SPEAKERS, set_b
from test_gpu_reshade_grad import binning_of, compare, on_device, traced, weights
from test_gpu_source_pattern import FACING, SHAPES, bits, layout, oracle_case, oracle_chain, oracle_range, same_records
from test_gpu_speaker_arrays import fast_bound

pytestmark = pytest.mark.gpu

SPREAD = spread_table()[0]
ORIENT = (OBLIQUE["facing"], OBLIQUE["up"])
OTHER_ORIENT = ((0.0, -0.8, 0.6), (1.0, 0.0, 0.0))
OTHER_MIC = (2.0, 3.0, 0.3)
SOURCE_KERNELS = ("source_pattern_kernel", "source_table_rays_kernel", "source_table_kernel")


def table_gains(oracle, fake_mics, fake_positions, table, orient):
    """[n][8] gains: oracle.attenuate_hrtf on unit-volume impulses (one call for one fake microphone, else one call per impulse)."""
    fake_mics = np.asarray(fake_mics, np.float32).reshape(-1, 3)
    fake_positions = np.asarray(fake_positions, np.float32).reshape(-1, 3)
    n = fake_positions.shape[0]
    fake = aligned_zeros(n, IMPULSE)
    fake["volume"] = 1.0
    fake["position"][:, :3] = fake_positions
    if fake_mics.shape[0] == 1:
        return oracle.attenuate_hrtf(fake_mics[0], fake, table, orient[0], orient[1], 0)["volume"].copy()
    assert fake_mics.shape[0] == n
    return np.array([oracle.attenuate_hrtf(fake_mics[i], fake[i:i + 1], table, orient[0], orient[1], 0)["volume"][0] for i in range(n)], np.float32).reshape(n, 8)


def expected_records(oracle, case, table, orient):
    """The oracle's trace of `case`, scaled: (diffuse, merged images with the direct one first, diffuse gains, image gains)."""
    g_rays = table_gains(oracle, [(0.0, 0.0, 0.0)], case["dirs"][:, :3], table, orient)
    g_diffuse = np.repeat(g_rays, case["nrefl"], axis=0)
    diffuse = case["diffuse"].copy()
    diffuse["volume"] = diffuse["volume"] * g_diffuse
    images = case["images"].copy()
    g_images = table_gains(oracle, images["position"][:, :3], np.tile(np.asarray(case["mic"], np.float32), (images.shape[0], 1)), table, orient)
    images["volume"] = images["volume"] * g_images
    return diffuse, images, g_diffuse, g_images


@pytest.fixture(scope="module")
def cathedral():
    return scenes.cathedral(3000)


@pytest.fixture(scope="module")
def ctx(cathedral):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(cathedral[0])
    yield c
    c.close()


def time_range(ctx, mic):
    from parallel_reverb_raytracer_amd import capi
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    return ctx.ir_time_range()


def state_of(ctx, mic):
    """Every byte a trace leaves for the host, and the diffuse time range."""
    return (ctx.get_raw_diffuse().tobytes(), ctx.get_direct().tobytes(), ctx.get_image_candidates().tobytes(), time_range(ctx, mic))


def names_of(ctx):
    return [k for k, _ in ctx.last_timings()]


def test_refusals_come_before_any_device_is_touched(ctx):
    """Every RVB_ERR_INVALID case of the header on a live context (a NULL handle: tests/test_source_table_host.py); the directivity that
    was set stays as it was."""
    from parallel_reverb_raytracer_amd import capi
    lib, table = ctx.lib, np.ascontiguousarray(SPREAD, np.float32).reshape(-1)
    p = table.ctypes.data_as(ctypes.c_void_p)
    good = capi.make_source_orientations(*ORIENT)
    assert lib.rvb_set_source_table(ctx.handle, p, None, ctypes.c_uint64(1)) == capi.ERR_INVALID
    assert lib.rvb_set_source_table(ctx.handle, p, good, ctypes.c_uint64(0)) == capi.ERR_INVALID
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = table.copy()
        bad[360 * 180 * 8 - 1] = bad_value
        assert lib.rvb_set_source_table(ctx.handle, bad.ctypes.data_as(ctypes.c_void_p), good, ctypes.c_uint64(1)) == capi.ERR_INVALID
        for facing, up in (((bad_value, 0.0, 1.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, 1.0), (0.0, bad_value, 0.0))):
            o = capi.make_source_orientations(facing, up)
            assert lib.rvb_set_source_table(ctx.handle, p, o, ctypes.c_uint64(1)) == capi.ERR_INVALID
    for facing, up in (((0.0, 1.0, 0.0), (0.0, 2.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 1.0, 0.0)), ((0.0, 0.0, 1.0), (0.0, 0.0, 0.0)),
                       ((1e-30, 0.0, 0.0), (0.0, 1e-30, 0.0)), ((3e38, 0.0, 0.0), (0.0, 3e38, 0.0))):
        two = capi.make_source_orientations([ORIENT[0], facing], [ORIENT[1], up])           # the second orientation is the bad one
        assert lib.rvb_set_source_table(ctx.handle, p, two, ctypes.c_uint64(2)) == capi.ERR_INVALID, (facing, up)
        assert "orientation 1" in lib.rvb_last_error(ctx.handle).decode()


@pytest.mark.parametrize("nrays,nrefl", [(509, 24), (5, 70)])
def test_raw_records_equal_the_oracle_records_times_the_oracle_gain(ctx, oracle, cathedral, nrays, nrefl):
    """509 x 24 = 12 216 records: a partial last workgroup and wave, several rays per wave; 5 x 70: a ray longer than a wave.  The table
    is the spread table: a neighbouring row lands far away.  (An image besides the direct one is asserted where 509 rays find one.)"""
    from parallel_reverb_raytracer_amd import capi
    scene, info = cathedral
    case = oracle_case(oracle, scene, info["mic"], info["source"], scenes.sphere_directions(nrays, seed=23), nrefl)
    diffuse, images, g_diffuse, g_images = expected_records(oracle, case, SPREAD, ORIENT)
    # the oracle's data must put the feature under test
    assert (np.diff(g_diffuse, axis=1) != 0).all() and len(set(g_diffuse[:, 0].tolist())) >= min(nrays, 400), "gains do not differ per band and ray"
    if nrays == 509:
        assert case["images"].shape[0] >= 2, "no image-source impulse besides the direct one"
    assert case["images"].shape[0] >= 1 and (case["images"]["volume"][0] != 0).any(), "the direct path is hidden"
    live = (case["diffuse"]["volume"] != 0).any(axis=1)
    assert live.any() and not live.all()
    assert (g_images != 0).all() and (np.diff(g_images, axis=1) != 0).all()

    ctx.set_source_table(None)
    ctx.raytrace(case["mic"], case["source"], case["dirs"], nrefl, AIR_COEFFICIENTS)
    assert same_records(ctx.get_raw_diffuse(), case["diffuse"]) and same_records(ctx.get_raw_images(False), case["images"])
    names = names_of(ctx)
    assert names and not set(names) & set(SOURCE_KERNELS)
    plain = state_of(ctx, case["mic"])
    ctx.set_source_table(SPREAD, *ORIENT)
    try:
        ctx.raytrace(case["mic"], case["source"], case["dirs"], nrefl, AIR_COEFFICIENTS)
        names = names_of(ctx)
        got_diffuse, got_direct, got_images = ctx.get_raw_diffuse(), ctx.get_direct(), ctx.get_raw_images(False)
        got_range = time_range(ctx, case["mic"])
        if nrays == 509:
            flat, chans = oracle_chain(oracle, "speakers2", case["mic"], np.concatenate([diffuse, images]), True, 44100.0)
            ctx.ir_configure_speakers(case["mic"], *layout("speakers2"), capi.IR_ALL, got_images)
            exact = ctx.ir_download(True, 44100.0, capi.IR_EXACT)
            fast = ctx.ir_download(True, 44100.0, capi.IR_FAST)
    finally:
        ctx.set_source_table(None)
    assert "source_table_rays_kernel" in names and "source_table_kernel" in names and "source_pattern_kernel" not in names
    assert names.index("source_table_rays_kernel") < names.index("source_table_kernel")
    assert same_records(got_diffuse, diffuse)
    assert not got_diffuse["pad"].any() and not got_diffuse["position"][:, 3].any()
    assert same_records(got_direct, images[:1])            # std::map order: the direct path's key {0} comes first
    assert got_images.shape == images.shape and same_records(got_images, images)
    assert got_range == oracle_range(diffuse)
    if nrays == 509:
        for ch in range(2):
            n = flat[ch].shape[1]
            assert np.array_equal(exact[ch][:, :n], flat[ch]) and not exact[ch][:, n:].any(), ch
        assert fast.shape == exact.shape and fast.any()
        assert (np.abs(fast.astype(np.float64) - exact) <= fast_bound(exact, chans, 44100.0)).all()
    # ... and with the table off again the plain trace is back
    ctx.raytrace(case["mic"], case["source"], case["dirs"], nrefl, AIR_COEFFICIENTS)
    names = names_of(ctx)
    assert names and not set(names) & set(SOURCE_KERNELS)
    assert state_of(ctx, case["mic"]) == plain


@pytest.fixture(scope="module")
def box():
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)
    c.set_scene(scenes.shoebox())
    yield c
    c.close()


_plain_box = {}


def edge_directions(frame_name):
    frame = {"canonical": CANONICAL, "oblique": OBLIQUE}[frame_name]
    pos = hrtf_boundary_records(frame["facing"], frame["up"], (0.0, 0.0, 0.0), 1.0)["position"]
    dirs = np.zeros((pos.shape[0], 4), np.float32)
    dirs[:, :3] = pos
    return dirs


@pytest.mark.parametrize("boundaries_of,orientation", [("canonical", "canonical"), ("canonical", "oblique"), ("oblique", "oblique")])
def test_row_edges(box, oracle, boundaries_of, orientation):
    """The ~80 k constructed directions round every integer boundary of azimuth and elevation (radius 1 about a microphone at 0: unit
    vectors) as rays of a one-reflection trace in the shoebox, with the row-code table: every live record names the row of its ray.
    With CANONICAL's directions under both orientations, and with the boundaries constructed in OBLIQUE's own frame."""
    frame = {"canonical": CANONICAL, "oblique": OBLIQUE}[orientation]
    dirs = edge_directions(boundaries_of)
    assert dirs.shape[0] > 75000
    mic, src = (-0.7, -1.0, -3.0), (0.5, 0.3, 2.0)
    codes = table_gains(oracle, [(0.0, 0.0, 0.0)], dirs[:, :3], row_code_table()[0], (frame["facing"], frame["up"]))
    rows = (np.abs(codes[:, 0].astype(np.int64)) - 1) // 8
    assert len(set(rows.tolist())) > 1000 and (codes[:, 0] != 0).all()
    if boundaries_of not in _plain_box:
        box.set_source_table(None)
        box.raytrace(mic, src, dirs, 1, AIR_COEFFICIENTS)
        _plain_box[boundaries_of] = box.get_raw_diffuse()
    plain = _plain_box[boundaries_of]
    live = (plain["volume"] != 0).any(axis=1)
    assert live.mean() > 0.9
    box.set_source_table(row_code_table()[0], frame["facing"], frame["up"])
    try:
        box.raytrace(mic, src, dirs, 1, AIR_COEFFICIENTS)
        got = box.get_raw_diffuse()
    finally:
        box.set_source_table(None)
    want = plain["volume"] * codes
    wrong = np.flatnonzero((bits(got["volume"]) != bits(want)).any(axis=1) & live)
    assert wrong.size == 0, (wrong[:5], got["volume"][wrong[:5], 0], want[wrong[:5], 0])
    assert not got["volume"][~live].any()
    assert np.array_equal(bits(got["position"]), bits(plain["position"])) and np.array_equal(bits(got["time"]), bits(plain["time"]))


def test_trace_pairs_takes_an_orientation_per_pair_or_one_for_all(ctx, cathedral):
    """2 pairs x 130 rays x 3 reflections = 390 records per pair: the pair boundary falls inside a wave.  Every pair equals the same
    pair traced alone with its orientation, bit for bit; three orientations for two pairs are refused at the trace."""
    from parallel_reverb_raytracer_amd import capi
    info = cathedral[1]
    mics = np.array([info["mic"], (0.0, 12.0, 11.0)], np.float32)
    sources = np.array([info["source"], (0.0, 12.5, 11.5)], np.float32)
    facings = np.array([ORIENT[0], OTHER_ORIENT[0]], np.float32)
    ups = np.array([ORIENT[1], OTHER_ORIENT[1]], np.float32)
    nrefl, nrays = 3, 130
    ctx.set_directions(scenes.sphere_directions(nrays, seed=5))

    def per_pair_results(pair_mics):
        out = []
        for p, m in enumerate(pair_mics):
            ctx.select_pair(p)
            direct = ctx.get_direct()
            out.append((direct.tobytes(), time_range(ctx, m)))
        return out

    try:
        for per_pair in (True, False):
            alone = []
            for p in range(2):
                ctx.set_source_table(SPREAD, facings[p if per_pair else 0], ups[p if per_pair else 0])
                ctx.trace(mics[p], sources[p], nrefl, AIR_COEFFICIENTS)
                alone.append((ctx.get_raw_diffuse(), ctx.get_image_candidates(), per_pair_results([mics[p]])[0]))
            if per_pair:
                ctx.set_source_table(SPREAD, facings, ups)
            else:
                ctx.set_source_table(SPREAD, facings[0], ups[0])
            ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
            diffuse, cand, res = ctx.get_raw_diffuse().reshape(2, -1), ctx.get_image_candidates(), per_pair_results(mics)
            for p in range(2):
                assert same_records(diffuse[p], alone[p][0]), (per_pair, p)
                assert (diffuse[p]["volume"] != 0).any()
                mine = ctx.get_pair_candidates(p, cand)
                assert mine.shape == alone[p][1].shape and mine.tobytes() == alone[p][1].tobytes(), (per_pair, p)
                assert res[p] == alone[p][2], (per_pair, p)
            if per_pair:
                both_first = diffuse.copy()
        # the second pair under its own orientation is not the second pair under the first
        assert not same_records(both_first[1], diffuse[1])
        ctx.set_source_table(SPREAD, np.concatenate([facings, facings[:1]]), np.concatenate([ups, ups[:1]]))
        with pytest.raises(capi.RvbError) as e:
            ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
        assert e.value.code == capi.ERR_INVALID, str(e.value)
        with pytest.raises(capi.RvbError) as e:
            ctx.trace(mics[0], sources[0], nrefl, AIR_COEFFICIENTS)
        assert e.value.code == capi.ERR_INVALID, str(e.value)
    finally:
        ctx.set_source_table(None)
        ctx.npairs = 1


def test_a_source_has_one_directivity_at_a_time(ctx, cathedral):
    info = cathedral[1]
    mic, src = info["mic"], info["source"]
    dirs = scenes.sphere_directions(300, seed=9)

    def trace():
        ctx.raytrace(mic, src, dirs, 12, AIR_COEFFICIENTS)
        names = names_of(ctx)          # (before state_of: the time-range query starts the timings again)
        return state_of(ctx, mic), names

    try:
        ctx.set_source_pattern(None)
        plain, names = trace()
        assert not set(names) & set(SOURCE_KERNELS)
        ctx.set_source_table(SPREAD, *ORIENT)
        table_only, names = trace()
        assert "source_table_kernel" in names and "source_pattern_kernel" not in names
        ctx.set_source_table(None)
        ctx.set_source_pattern(FACING, SHAPES)
        pattern_only, names = trace()
        assert "source_pattern_kernel" in names and "source_table_kernel" not in names
        assert len({plain[0], table_only[0], pattern_only[0]}) == 3
        # pattern, then table: the table alone
        ctx.set_source_table(SPREAD, *ORIENT)
        got, names = trace()
        assert got == table_only and "source_pattern_kernel" not in names
        # table, then pattern: the pattern alone
        ctx.set_source_pattern(FACING, SHAPES)
        got, names = trace()
        assert got == pattern_only and "source_table_kernel" not in names and "source_table_rays_kernel" not in names
        # table, then "no pattern": nothing at the source end
        ctx.set_source_table(SPREAD, *ORIENT)
        ctx.set_source_pattern(None)
        got, names = trace()
        assert got == plain and names and not set(names) & set(SOURCE_KERNELS)
    finally:
        ctx.set_source_pattern(None)


def test_identical_table_traces_give_identical_bytes(ctx, cathedral):
    info = cathedral[1]
    dirs = scenes.sphere_directions(509, seed=3)
    ctx.set_source_table(SPREAD, *ORIENT)
    try:
        states = []
        for _ in range(2):
            ctx.raytrace(info["mic"], info["source"], dirs, 24, AIR_COEFFICIENTS)
            states.append(state_of(ctx, info["mic"]))
    finally:
        ctx.set_source_table(None)
    assert states[0] == states[1]


@pytest.fixture(scope="module")
def kept_world():
    """scenes.cathedral(3000) as tests/test_gpu_reshade_grad.py takes it, with another surface table B"""
    scene, info = scenes.cathedral(3000)
    return {"scene": scene, "mic": info["mic"], "source": info["source"], "B": set_b(scene[2], 2, 4, 5)}


@pytest.fixture(scope="module")
def kept(kept_world):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)
    c.set_scene(kept_world["scene"])
    c.keep_paths(True, listener=True)
    yield c
    c.close()


def fresh_state(world, surfaces, air, mic, dirs, nrefl, table, orient, pattern=None, source=None):
    """A trace on a context of its own in the scene with the surface table `surfaces`; pattern: (direction, shape) instead of a table;
    source: another than the world's."""
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)
    try:
        c.set_scene((world["scene"][0], world["scene"][1], surfaces))
        if table is not None:
            c.set_source_table(table, *orient)
        if pattern is not None:
            c.set_source_pattern(*pattern)
        c.raytrace(mic, world["source"] if source is None else source, dirs, nrefl, air)
        return state_of(c, mic)
    finally:
        c.close()


def test_kept_traces_reshade_and_relisten_with_the_table(kept, kept_world):
    """256 x 16 kept for materials and listeners: reshade and relisten equal fresh traces, bit for bit; a table set after the kept trace
    is ignored by relisten (which re-applies what the records reflect) and taken up by the next reshade."""
    w = kept_world
    nrays, nrefl = 256, 16
    dirs = scenes.sphere_directions(nrays, seed=23)
    own = w["scene"][2]
    other_table = np.ascontiguousarray(SPREAD[::-1, ::-1])
    want = {
        "A": fresh_state(w, own, AIR_COEFFICIENTS, w["mic"], dirs, nrefl, SPREAD, ORIENT),
        "B": fresh_state(w, w["B"], AIR_B, w["mic"], dirs, nrefl, SPREAD, ORIENT),
        "B other mic": fresh_state(w, w["B"], AIR_B, OTHER_MIC, dirs, nrefl, SPREAD, ORIENT),
        "A other mic": fresh_state(w, own, AIR_COEFFICIENTS, OTHER_MIC, dirs, nrefl, SPREAD, ORIENT),
        "A other table": fresh_state(w, own, AIR_COEFFICIENTS, w["mic"], dirs, nrefl, other_table, OTHER_ORIENT),
        "A plain": fresh_state(w, own, AIR_COEFFICIENTS, w["mic"], dirs, nrefl, None, None),
    }
    assert len({v[0] for v in want.values()}) == len(want)
    assert want["A"][1] != want["A other mic"][1] and want["A"][1] != want["A plain"][1], "the direct slot does not see the microphone or the table"
    kept.set_source_table(SPREAD, *ORIENT)
    try:
        kept.raytrace(w["mic"], w["source"], dirs, nrefl, AIR_COEFFICIENTS)
        assert state_of(kept, w["mic"]) == want["A"]
        kept.reshade(w["B"], AIR_B)
        assert "source_table_rays_kernel" in names_of(kept) and "source_table_kernel" in names_of(kept)
        assert state_of(kept, w["mic"]) == want["B"]
        kept.relisten(OTHER_MIC)
        names = names_of(kept)
        assert "source_table_kernel" in names and "source_table_rays_kernel" not in names          # the gains are reused
        assert state_of(kept, OTHER_MIC) == want["B other mic"]
        kept.reshade(None, AIR_COEFFICIENTS)
        assert state_of(kept, OTHER_MIC) == want["A other mic"]
        # another table, set now: relisten still shades with what the records reflect ...
        kept.set_source_table(other_table, *OTHER_ORIENT)
        kept.relisten(w["mic"])
        assert state_of(kept, w["mic"]) == want["A"]
        # ... a switched-off table too ...
        kept.set_source_table(None)
        kept.relisten(OTHER_MIC)
        assert state_of(kept, OTHER_MIC) == want["A other mic"]
        kept.relisten(w["mic"])
        # ... and the next reshade takes up what is set
        kept.set_source_table(other_table, *OTHER_ORIENT)
        kept.reshade(None, AIR_COEFFICIENTS)
        assert state_of(kept, w["mic"]) == want["A other table"]
        kept.set_source_table(None)
        for again in (lambda: kept.reshade(None, AIR_COEFFICIENTS), lambda: kept.relisten(w["mic"])):
            again()
            names = names_of(kept)
            assert names and not set(names) & set(SOURCE_KERNELS)
            assert state_of(kept, w["mic"]) == want["A plain"]
    finally:
        kept.set_source_table(None)


def test_kept_traces_across_pattern_and_table_and_changing_pair_counts(kept, kept_world):
    """256 x 16, kept for materials and listeners, against fresh traces on contexts of their own, bit for bit.  (a) from a pattern to a
    table and back on one kept trace: relisten shades with what the records reflect, whichever of the two has been set since, and the
    next reshade takes up what is set.  (b) 3 pairs, 2 pairs and new microphones for them, 1 pair, 3 pairs again on one context, an
    orientation per pair: every pair's diffuse slice, direct path and time range are those of that pair traced alone."""
    w = kept_world
    nrays, nrefl = 256, 16
    dirs = scenes.sphere_directions(nrays, seed=23)
    own, air = w["scene"][2], AIR_COEFFICIENTS
    pattern = (FACING, SHAPES)
    mics = np.array([w["mic"], (0.0, 12.0, 11.0), (-10.28, 3.85, -2.24)], np.float32)
    sources = np.array([w["source"], (0.0, 12.5, 11.5), (-12.0, 2.5, 3.0)], np.float32)
    new_mics = np.array([OTHER_MIC, w["mic"]], np.float32)
    facings = np.array([ORIENT[0], OTHER_ORIENT[0], (0.6, 0.0, 0.8)], np.float32)
    ups = np.array([ORIENT[1], OTHER_ORIENT[1], (0.0, 1.0, 0.0)], np.float32)

    def pair_alone(p, mic):
        return fresh_state(w, own, air, tuple(mic), dirs, nrefl, SPREAD, (facings[p], ups[p]), source=tuple(sources[p]))

    want = {
        "pattern": fresh_state(w, own, air, w["mic"], dirs, nrefl, None, None, pattern=pattern),
        "pattern other mic": fresh_state(w, own, air, OTHER_MIC, dirs, nrefl, None, None, pattern=pattern),
        "table": fresh_state(w, own, air, w["mic"], dirs, nrefl, SPREAD, ORIENT),
        "table other mic": fresh_state(w, own, air, OTHER_MIC, dirs, nrefl, SPREAD, ORIENT),
        "pair 1": pair_alone(1, mics[1]),
        "pair 2": pair_alone(2, mics[2]),
        "pair 1 new mic": pair_alone(1, new_mics[1]),
    }
    want["pair 0"], want["pair 0 new mic"] = want["table"], want["table other mic"]          # (pair 0 is the world's own, under ORIENT)
    assert len({v[0] for v in want.values()}) == len(want) - 2
    assert len({want[n][1] for n in ("pattern", "pattern other mic", "table", "table other mic")}) == 4, "the direct slot does not see the microphone or the directivity"
    assert len({v[3] for v in want.values()}) > 1

    def pairs_of(ctx, pair_mics):
        """Per pair what state_of gives for a single pair, without the candidates: (diffuse slice, direct path, time range)."""
        diffuse = ctx.get_raw_diffuse().reshape(len(pair_mics), -1)
        out = []
        for p, m in enumerate(pair_mics):
            ctx.select_pair(p)
            out.append((diffuse[p].tobytes(), ctx.get_direct().tobytes(), time_range(ctx, tuple(m))))
        return out

    def alone(*names):
        return [(want[n][0], want[n][1], want[n][3]) for n in names]

    try:
        # (a)
        kept.set_source_pattern(*pattern)
        kept.raytrace(w["mic"], w["source"], dirs, nrefl, air)
        assert state_of(kept, w["mic"]) == want["pattern"]
        kept.set_source_table(SPREAD, *ORIENT)
        kept.relisten(OTHER_MIC)
        names = names_of(kept)          # (before state_of: the time-range query starts the timings again)
        assert "source_pattern_kernel" in names and "source_table_kernel" not in names and "source_table_rays_kernel" not in names
        assert state_of(kept, OTHER_MIC) == want["pattern other mic"]
        kept.reshade(None, air)
        assert state_of(kept, OTHER_MIC) == want["table other mic"]
        kept.set_source_pattern(*pattern)
        kept.relisten(w["mic"])
        names = names_of(kept)
        assert "source_table_kernel" in names and "source_table_rays_kernel" not in names and "source_pattern_kernel" not in names
        assert state_of(kept, w["mic"]) == want["table"]
        kept.reshade(None, air)
        assert state_of(kept, w["mic"]) == want["pattern"]
        # (b)
        kept.set_source_table(SPREAD, facings, ups)
        kept.trace_pairs(mics, sources, nrefl, air)
        assert pairs_of(kept, mics) == alone("pair 0", "pair 1", "pair 2")
        kept.set_source_table(SPREAD, facings[:2], ups[:2])
        kept.trace_pairs(mics[:2], sources[:2], nrefl, air)
        assert pairs_of(kept, mics[:2]) == alone("pair 0", "pair 1")
        kept.relisten(new_mics)
        assert pairs_of(kept, new_mics) == alone("pair 0 new mic", "pair 1 new mic")
        kept.set_source_table(SPREAD, facings[2], ups[2])
        kept.trace(mics[2], sources[2], nrefl, air)
        assert state_of(kept, tuple(mics[2])) == want["pair 2"]
        kept.set_source_table(SPREAD, facings, ups)
        kept.trace_pairs(mics, sources, nrefl, air)
        assert pairs_of(kept, mics) == alone("pair 0", "pair 1", "pair 2")
    finally:
        kept.set_source_table(None)
        kept.set_source_pattern(None)
        kept.npairs = 1


BAND_FACTORS = np.array([0.5, 1.0, 2.0, 4.0, 0.25, 1.0, 2.0, 0.5], np.float32)


def test_gradient_a_constant_table_scales_every_band_by_its_power_of_two(kept, oracle, kept_world):
    """Every row of the table holds the same eight powers of two: the records, and with them every term of the gradient, are the
    table-off ones scaled exactly, so the gradient of band b is the table-off gradient times that power, bit for bit."""
    from parallel_reverb_raytracer_amd import capi
    w = kept_world
    nrays, nrefl, mic = 130, 24, kept_world["mic"]
    kept.set_source_table(None)
    traced(kept, oracle, w, nrays, nrefl)
    predelay, nbins = binning_of(kept, mic, SPEAKERS, 44100.0)
    w_dev = on_device(weights(len(SPEAKERS[1]), nbins, 5))
    off = kept.reshade_grad(predelay, 44100.0, nbins, w_dev.data_ptr())
    assert off[0]["specular"].any() and off[0]["diffuse"].any() and off[1].all()
    kept.set_source_table(np.broadcast_to(BAND_FACTORS, (360, 180, 8)), *ORIENT)
    try:
        kept.reshade(None, AIR_COEFFICIENTS)
        assert binning_of(kept, mic, SPEAKERS, 44100.0) == (predelay, nbins)
        on = kept.reshade_grad(predelay, 44100.0, nbins, w_dev.data_ptr())
    finally:
        kept.set_source_table(None)
    assert np.array_equal(bits(on[0]["specular"]), bits(off[0]["specular"] * BAND_FACTORS))
    assert np.array_equal(bits(on[0]["diffuse"]), bits(off[0]["diffuse"] * BAND_FACTORS))
    assert np.array_equal(bits(on[1]), bits(off[1] * BAND_FACTORS))


def test_gradient_a_table_gain_is_a_factor_of_every_term_of_its_ray(kept, oracle, kept_world):
    """The spread table: every ray and band has another gain.  The reference of tests/test_gpu_reshade_grad.py is built from the records
    in the context, so its own bars hold the gradient, after the trace and after a reshade."""
    w = kept_world
    nrays, nrefl, mic = 130, 24, kept_world["mic"]
    from test_gpu_reshade_grad import table_t
    T = table_t(w["scene"][2])
    kept.set_source_table(SPREAD, *ORIENT)
    try:
        chain, _ = traced(kept, oracle, w, nrays, nrefl)
        compare(kept, chain, w["scene"][2], mic, nrefl, "source table after the trace")
        kept.reshade(T, AIR_B)
        scaled = compare(kept, chain, T, mic, nrefl, "source table after reshade")
    finally:
        kept.set_source_table(None)
    # the records still carry the table although it has been switched off for the traces that follow
    again = kept.reshade_grad(scaled["predelay"], 44100.0, scaled["nbins"], scaled["w_dev"].data_ptr())
    assert again[0].tobytes() == scaled["got"][0].tobytes() and again[1].tobytes() == scaled["got"][1].tobytes()
    kept.reshade(T, AIR_B)
    from parallel_reverb_raytracer_amd import capi
    kept.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    plain = kept.reshade_grad(scaled["predelay"], 44100.0, scaled["nbins"], scaled["w_dev"].data_ptr())
    assert (plain[0]["diffuse"] != scaled["got"][0]["diffuse"]).any()
