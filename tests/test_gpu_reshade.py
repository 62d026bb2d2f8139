"""Re-shading a finished trace (rvb_keep_paths / rvb_reshade, csrc/reshade_kernels.hip): new surfaces and a new air coefficient without
retracing.  The contract is "the bytes a full trace with the new surfaces and air would have produced", so every expectation is the CPU
oracle's trace of the scene with the other surface table (oracle.raytrace, oracle.collect_images, the usual oracle chain for impulse
responses); nothing is compared with a second GPU trace.

Bars: records, direct slots, merged images, time ranges and RVB_IR_EXACT histograms bit for bit; RVB_IR_FAST within fast_bound of
tests/test_gpu_speaker_arrays.py."""
import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, aligned_copy

from test_gpu_source_pattern import FACING, SHAPES, bits, expected_records, layout, oracle_chain, oracle_range, same_records
from test_gpu_speaker_arrays import fast_bound

pytestmark = pytest.mark.gpu

NEW_KERNELS = ("path_keep_kernel", "reshade_kernel", "reshade_images_kernel")
# all eight differ from AIR_COEFFICIENTS
AIR_B = (AIR_COEFFICIENTS * np.float32(1.7) - np.float32(1e-4)).astype(np.float32)
SPEAKERS = ([(-1, 0, -1), (1, 0, -1)], [0.5, 0.5])


def set_b(surfaces, dead_specular, dead_diffuse, mute):
    """Another table for the same scene: every coefficient of every surface changed; band 3 of surface `dead_specular` reflects nothing
    specularly (the chains of that band die there), band 5 of `dead_diffuse` nothing diffusely, and surface `mute` nothing diffusely in
    any band, so that its records lose all volume (that moves the time range: asserted where it is used)."""
    rng = np.random.default_rng(7)
    b = aligned_copy(surfaces)
    b["specular"] = rng.uniform(0.55, 0.9, b["specular"].shape).astype(np.float32)
    b["diffuse"] = rng.uniform(0.3, 0.85, b["diffuse"].shape).astype(np.float32)
    b["specular"][dead_specular][3] = 0.0
    b["diffuse"][dead_diffuse][5] = 0.0
    b["diffuse"][mute][:] = 0.0
    assert (b["specular"] != surfaces["specular"]).all() and (b["diffuse"] != surfaces["diffuse"]).all()
    return b


@pytest.fixture(scope="module")
def cathedral():
    """scenes.cathedral(3000) with its own source and microphone; surfaces: default, glass, lime_wall, marble, plaster, stone_floor, wood"""
    scene, info = scenes.cathedral(3000)
    assert scene[2].shape[0] == 7
    return {"scene": scene, "mic": info["mic"], "source": info["source"], "B": set_b(scene[2], 2, 4, 5)}


_cases = {}


def oracle_case(oracle, scene, surfaces, mic, src, dirs, nrefl, air, key=None):
    """The oracle's trace of `scene` with the surface table `surfaces`, in the form test_gpu_source_pattern.expected_records takes.
    Computed once per key and never changed."""
    if key is not None and key in _cases:
        return _cases[key]
    diffuse, image, index = oracle.raytrace((scene[0], scene[1], surfaces), mic, src, dirs, nrefl, air)
    case = {"mic": mic, "source": src, "dirs": dirs, "nrefl": nrefl, "diffuse": diffuse, "images": oracle.collect_images(image, index, False)}
    if key is not None:
        _cases[key] = case
    return case


def cathedral_cases(oracle, cathedral, nrays, nrefl, seed=23):
    """(A, B): the scene's own surfaces with AIR_COEFFICIENTS, set B with AIR_B"""
    dirs = scenes.sphere_directions(nrays, seed=seed)
    args = (cathedral["mic"], cathedral["source"], dirs, nrefl)
    return (oracle_case(oracle, cathedral["scene"], cathedral["scene"][2], *args, AIR_COEFFICIENTS, key=("A", nrays, nrefl, seed)),
            oracle_case(oracle, cathedral["scene"], cathedral["B"], *args, AIR_B, key=("B", nrays, nrefl, seed)))


def assert_ground(a, b, want_images=1):
    """Preconditions on the oracle's data: a test must not pass on empty ground."""
    assert a["images"].shape[0] >= want_images and (a["images"]["volume"][0] != 0).any(), "the direct path is hidden, or too few images"
    live_a, live_b = (a["diffuse"]["volume"] != 0).any(axis=1), (b["diffuse"]["volume"] != 0).any(axis=1)
    assert live_a.any() and not live_a.all() and live_b.any() and not live_b.all()
    assert (live_a & ~live_b).any(), "no record loses all its volume under set B"
    for band in range(8):
        assert (a["diffuse"]["volume"][live_a, band] != b["diffuse"]["volume"][live_a, band]).any(), band
        assert (a["images"]["volume"][:, band] != b["images"]["volume"][:, band]).all(), band
    assert oracle_range(a["diffuse"]) != oracle_range(b["diffuse"]), "set B does not move the time range"


@pytest.fixture(scope="module")
def ctx(cathedral):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(cathedral["scene"])
    c.keep_paths(True)
    yield c
    c.close()


def time_range(ctx, mic):
    from parallel_reverb_raytracer_amd import capi
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    return ctx.ir_time_range()


def assert_state(ctx, case):
    """diffuse records (padding too), direct slot, merged images and the speaker model's time range equal the oracle case"""
    got = ctx.get_raw_diffuse()
    assert same_records(got, case["diffuse"])
    assert not got["pad"].any() and not got["position"][:, 3].any()
    assert same_records(ctx.get_direct(), case["images"][:1])          # std::map order: the direct path's key {0} comes first
    images = ctx.get_raw_images(False)
    assert images.shape == case["images"].shape and same_records(images, case["images"])
    assert time_range(ctx, case["mic"]) == oracle_range(case["diffuse"])


@pytest.mark.parametrize("nrays,nrefl", [(509, 24), (5, 70), (130, 64), (8, 33), (17, 32), (8, 1)])
def test_reshaded_records_equal_the_oracle_trace_of_the_other_surfaces(ctx, oracle, cathedral, nrays, nrefl):
    """509 x 24: a partial last workgroup and wave, several rays per wave, a ray shorter than a tile; 5 x 70: a ray longer than a wave
    and longer than an LDS tile, fewer rays than a wave takes; 130 x 64: nrefl % 32 == 0 selects the 16-bit key runs of the trace.
    The edges of a wave and of a tile: 8 x 33: exactly one wave's rays, a second tile that holds one bounce; 17 x 32: a last wave of one
    ray, exactly one tile (and the 16-bit key runs); 8 x 1: a single bounce."""
    a, b = cathedral_cases(oracle, cathedral, nrays, nrefl)
    assert_ground(a, b, want_images=2 if nrays == 509 else 1)
    ctx.raytrace(a["mic"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
    assert "path_keep_kernel" in [k for k, _ in ctx.last_timings()]
    executed = ctx.executed_bounces()
    assert_state(ctx, a)                                             # keeping changes nothing
    ctx.reshade(cathedral["B"], AIR_B)
    names = [k for k, _ in ctx.last_timings()]
    assert "reshade_kernel" in names and "reshade_images_kernel" in names and not any("path" in k or "shadow" in k for k in names)
    assert_state(ctx, b)
    assert ctx.executed_bounces() == executed


PLACE = np.array([0, 63, 64, 65, 3, 69, 6])


def spread_over_70(scene, *tables):
    """The scene with its seven surfaces at PLACE in a table of 70 (triangles renumbered), and every table of `tables` spread the same
    way: more surfaces than a table in LDS holds, so the kept-trace kernels read the table through L2."""
    assert scene[2].shape[0] == PLACE.shape[0]
    triangles = aligned_copy(scene[0])
    triangles["surface"] = PLACE[scene[0]["surface"]]
    wide = []
    for table in (scene[2],) + tables:
        w = aligned_copy(np.resize(table, 70))
        w[PLACE] = table
        wide.append(w)
    return ((triangles, scene[1], wide[0]),) + tuple(wide[1:])


def test_the_surface_table_read_through_l2(oracle, cathedral):
    """130 x 24 with the seven surfaces spread over a table of 70: reshade_kernel reads the table from memory.  The records carry no
    surface number, so the seven-surface oracle cases are the expectation, byte for byte."""
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = 130, 24
    a, b = cathedral_cases(oracle, cathedral, nrays, nrefl)
    assert_ground(a, b)
    wide_scene, wide_b = spread_over_70(cathedral["scene"], cathedral["B"])
    c = capi.Context(0)
    try:
        c.set_scene(wide_scene)
        c.keep_paths(True)
        c.raytrace(a["mic"], a["source"], a["dirs"], nrefl, AIR_COEFFICIENTS)
        assert_state(c, a)
        c.reshade(wide_b, AIR_B)
        assert [k for k, _ in c.last_timings()] == ["reshade_kernel", "reshade_images_kernel"]
        assert_state(c, b)
    finally:
        c.close()


def test_slots_behind_an_escape_stay_zero(oracle):
    """scenes.shoebox() without its last two triangles (one long wall): rays leave the room, and their remaining slots are all-zero."""
    from parallel_reverb_raytracer_amd import capi
    triangles, vertices, surfaces = scenes.shoebox()
    scene = (aligned_copy(triangles[:-2]), vertices, surfaces)
    table_b = set_b(surfaces, 1, 1, 0)                               # (surface 0, the default, is on no triangle: nothing is muted here)
    mic, src, nrays, nrefl = (0.5, 1.0, 2.0), (-0.7, -1.2, -5.0), 130, 24
    dirs = scenes.sphere_directions(nrays, seed=3)
    a = oracle_case(oracle, scene, surfaces, mic, src, dirs, nrefl, AIR_COEFFICIENTS)
    b = oracle_case(oracle, scene, table_b, mic, src, dirs, nrefl, AIR_B)
    empty = ~a["diffuse"].view(np.uint32).reshape(-1, 16).any(axis=1)
    per_ray = empty.reshape(nrays, nrefl)
    assert per_ray[:, -1].sum() >= 10 and not per_ray[:, 0].all() and not per_ray[:, -1].all(), "too few escaping rays, or too many"
    live = (a["diffuse"]["volume"] != 0).any(axis=1)
    assert live.any() and (a["diffuse"]["volume"][live] != b["diffuse"]["volume"][live]).any()
    c = capi.Context(0)
    try:
        c.set_scene(scene)
        c.keep_paths(True)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        assert_state(c, a)
        c.reshade(table_b, AIR_B)
        assert_state(c, b)
        assert not c.get_raw_diffuse().view(np.uint32).reshape(-1, 16)[empty].any()
    finally:
        c.close()


def snapshot(ctx, mic):
    return (ctx.get_raw_diffuse().tobytes(), ctx.get_direct().tobytes(), ctx.get_image_candidates().tobytes(), time_range(ctx, mic))


def test_a_sweep_returns_to_the_original_trace_bit_for_bit(ctx, oracle, cathedral):
    a, b = cathedral_cases(oracle, cathedral, 509, 24)
    ctx.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
    original = snapshot(ctx, a["mic"])
    assert len(ctx.get_image_candidates()) >= 1
    ctx.reshade(cathedral["B"], AIR_B)
    other = snapshot(ctx, a["mic"])
    assert all(x != y for x, y in zip(original, other))
    assert_state(ctx, b)
    ctx.reshade(None, AIR_COEFFICIENTS)
    assert snapshot(ctx, a["mic"]) == original


def test_air_alone(ctx, oracle, cathedral):
    dirs = scenes.sphere_directions(509, seed=23)
    want = oracle_case(oracle, cathedral["scene"], cathedral["scene"][2], cathedral["mic"], cathedral["source"], dirs, 24, AIR_B)
    a, _ = cathedral_cases(oracle, cathedral, 509, 24)
    assert not same_records(want["diffuse"], a["diffuse"]) and not same_records(want["images"], a["images"])
    ctx.raytrace(a["mic"], a["source"], dirs, 24, AIR_COEFFICIENTS)
    ctx.reshade(None, AIR_B)
    assert_state(ctx, want)


def test_every_pair_of_trace_pairs_is_reshaded(ctx, oracle, cathedral):
    """3 pairs x 100 rays x 24: 300 rays in 38 waves, two of which hold rays of two pairs."""
    from parallel_reverb_raytracer_amd import capi
    mics = np.array([cathedral["mic"], (0.0, 12.0, 11.0), (2.0, 3.0, 0.3)], np.float32)
    sources = np.array([cathedral["source"], (0.0, 12.5, 11.5), (-4.0, 2.0, -0.4)], np.float32)
    nrays, nrefl = 100, 24
    dirs = scenes.sphere_directions(nrays, seed=5)
    want = [oracle_case(oracle, cathedral["scene"], cathedral["B"], tuple(mics[p]), tuple(sources[p]), dirs, nrefl, AIR_B) for p in range(3)]
    assert sum(w["images"].shape[0] for w in want) > 3 and len({oracle_range(w["diffuse"]) for w in want}) == 3
    ctx.set_directions(dirs)
    try:
        ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
        ctx.reshade(cathedral["B"], AIR_B)
        diffuse, cand = ctx.get_raw_diffuse().reshape(3, -1), ctx.get_image_candidates()
        for p in range(3):
            assert same_records(diffuse[p], want[p]["diffuse"]), p
            ctx.select_pair(p)
            direct = ctx.get_direct()
            assert same_records(direct, want[p]["images"][:1]), p
            images = capi.merge_images(ctx.get_pair_candidates(p, cand), direct, False)
            assert images.shape == want[p]["images"].shape and same_records(images, want[p]["images"]), p
            assert time_range(ctx, mics[p]) == oracle_range(want[p]["diffuse"]), p
    finally:
        ctx.npairs = 1


def staged_upload_cases(oracle, cathedral):
    """The oracle's side of test_staged_uploads_in_sequence: 2 pairs x 130 rays x 24, per step the (diffuse, images) each pair must
    show, the source pattern's gain applied.  Asserts the ground on the oracle's data: no step may pass on an unchanged state."""
    scene, nrays, nrefl = cathedral["scene"], 130, 24
    dirs = scenes.sphere_directions(nrays, seed=23)
    mics = np.array([cathedral["mic"], (-10.28, 3.85, -2.24)], np.float32)
    sources = np.array([cathedral["source"], (-12.0, 2.5, 3.0)], np.float32)
    other_mics = mics[::-1].copy()
    facings = np.array([FACING, (-1.0, 0.0, 0.0)], np.float32)
    b2 = set_b(scene[2], 1, 3, 6)
    assert (b2["specular"] != cathedral["B"]["specular"]).any() and (b2["diffuse"] != cathedral["B"]["diffuse"]).any()

    def want(table, air, pair_mics, pair_facings, tag):
        out = []
        for p in range(2):
            case = oracle_case(oracle, scene, table, tuple(pair_mics[p]), tuple(sources[p]), dirs, nrefl, air, key=("staged", tag, p))
            diffuse, images, g_diffuse, _ = expected_records(oracle, case, pair_facings[p], SHAPES)
            assert (g_diffuse < 0).any() and (g_diffuse > 0).any()
            out.append({"mic": tuple(pair_mics[p]), "diffuse": diffuse, "images": images})
        return out

    for p in range(2):            # assert_ground's preconditions on the unscaled cases, per pair
        args = (tuple(mics[p]), tuple(sources[p]), dirs, nrefl)
        assert_ground(oracle_case(oracle, scene, scene[2], *args, AIR_COEFFICIENTS, key=("staged", "A", p)),
                      oracle_case(oracle, scene, cathedral["B"], *args, AIR_B, key=("staged", "B", p)))
    steps = {"traced": want(scene[2], AIR_COEFFICIENTS, mics, [FACING, FACING], "A"),
             "B": want(cathedral["B"], AIR_B, mics, facings, "B"),
             "B2": want(b2, AIR_COEFFICIENTS, mics, facings, "B2"),
             "relistened": want(cathedral["B"], AIR_B, other_mics, facings, "B at the other microphones")}
    for p in range(2):            # every state differs from the one the context is in before it, and B2 from both its neighbours
        for x, y in (("traced", "B"), ("B", "B2"), ("B2", "traced"), ("B", "relistened")):
            one, two = steps[x][p], steps[y][p]
            assert not same_records(one["diffuse"], two["diffuse"]) and not same_records(one["images"], two["images"]), (x, y, p)
        assert oracle_range(steps["traced"][p]["diffuse"]) != oracle_range(steps["B"][p]["diffuse"]), p
        assert oracle_range(steps["B"][p]["diffuse"]) != oracle_range(steps["relistened"][p]["diffuse"]), p
        assert (steps["relistened"][p]["images"]["volume"][0] != 0).any(), "the direct path is hidden from the other microphone"
    return {"dirs": dirs, "nrefl": nrefl, "mics": mics, "sources": sources, "other_mics": other_mics, "facings": facings, "B2": b2, "steps": steps}


def test_staged_uploads_in_sequence(oracle, cathedral):
    """The uploads that go through a pinned staging block (source patterns, the re-shade surface table, the per-pair geometry), back
    to back on one context: blocks that grow while in use, a second upload that has to wait for the block, the pair staging written
    again by rvb_relisten, and the kept buffers released and made again.  Every state is the oracle's, bit for bit, pair by pair."""
    from parallel_reverb_raytracer_amd import capi
    w = staged_upload_cases(oracle, cathedral)
    steps, nrefl = w["steps"], w["nrefl"]

    def assert_pairs(c, want):
        diffuse, cand = c.get_raw_diffuse().reshape(2, -1), c.get_image_candidates()
        for p in range(2):
            assert same_records(diffuse[p], want[p]["diffuse"]), p
            assert not diffuse[p]["pad"].any() and not diffuse[p]["position"][:, 3].any()
            c.select_pair(p)
            direct = c.get_direct()
            assert same_records(direct, want[p]["images"][:1]), p
            images = capi.merge_images(c.get_pair_candidates(p, cand), direct, False)
            assert images.shape == want[p]["images"].shape and same_records(images, want[p]["images"]), p
            assert time_range(c, want[p]["mic"]) == oracle_range(want[p]["diffuse"]), p
        return diffuse.tobytes(), cand.tobytes()

    c = capi.Context(0)
    try:
        c.set_scene(cathedral["scene"])
        c.keep_paths(True, listener=True)
        c.set_directions(w["dirs"])
        c.set_source_pattern(FACING, SHAPES)                             # 1. one pattern for both pairs
        c.trace_pairs(w["mics"], w["sources"], nrefl, AIR_COEFFICIENTS)
        assert_pairs(c, steps["traced"])
        c.set_source_pattern(w["facings"], SHAPES)                       # 2. one per pair: the pattern blocks grow while in use;
        c.reshade(cathedral["B"], AIR_B)                                 #    the first surface upload
        first = assert_pairs(c, steps["B"])
        c.reshade(w["B2"], AIR_COEFFICIENTS)                             # 3. no host read in between: the second upload waits for the block
        c.reshade(cathedral["B"], AIR_B)
        assert assert_pairs(c, steps["B"]) == first
        c.relisten(w["other_mics"])                                      # 4. the pair staging again
        assert_pairs(c, steps["relistened"])
        c.keep_paths(False)                                              # 5. released and made again: the bytes of step 2
        c.keep_paths(True, listener=True)
        c.trace_pairs(w["mics"], w["sources"], nrefl, AIR_COEFFICIENTS)
        c.reshade(cathedral["B"], AIR_B)
        assert assert_pairs(c, steps["B"]) == first
        c.reshade(w["B2"], AIR_COEFFICIENTS)                             # the intermediate state of step 3, on its own
        assert assert_pairs(c, steps["B2"]) != first
    finally:
        c.close()


def test_a_source_pattern_is_applied_to_the_reshaded_records(ctx, oracle, cathedral):
    a, b = cathedral_cases(oracle, cathedral, 509, 24)
    diffuse, images, g_diffuse, _ = expected_records(oracle, b, FACING, SHAPES)
    assert (g_diffuse < 0).any() and (g_diffuse > 0).any()
    ctx.set_source_pattern(FACING, SHAPES)
    try:
        ctx.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
        ctx.reshade(cathedral["B"], AIR_B)
        assert "source_pattern_kernel" in [k for k, _ in ctx.last_timings()]
        got_diffuse, got_direct, got_images, got_range = ctx.get_raw_diffuse(), ctx.get_direct(), ctx.get_raw_images(False), time_range(ctx, a["mic"])
    finally:
        ctx.set_source_pattern(None)
    assert same_records(got_diffuse, diffuse) and same_records(got_direct, images[:1])
    assert got_images.shape == images.shape and same_records(got_images, images)
    assert got_range == oracle_range(diffuse)


def test_impulse_responses_of_reshaded_records_equal_the_oracle_chain(ctx, oracle, cathedral):
    from parallel_reverb_raytracer_amd import capi
    a, b = cathedral_cases(oracle, cathedral, 509, 24)
    mic, sr = a["mic"], 44100.0
    flat, chans = oracle_chain(oracle, "speakers2", mic, np.concatenate([b["diffuse"], b["images"]]), True, sr)
    nb = max(f.shape[1] for f in flat)
    ctx.raytrace(mic, a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
    ctx.reshade(cathedral["B"], AIR_B)
    ctx.ir_configure_speakers(mic, *layout("speakers2"), capi.IR_ALL, ctx.get_raw_images(False))
    exact = ctx.ir_download(True, sr, capi.IR_EXACT)
    assert exact.shape == (2, 8, nb) and exact.any()
    for ch in range(2):
        n = flat[ch].shape[1]                     # the reference bins every channel on its own maxtime
        assert np.array_equal(bits(exact[ch][:, :n]), bits(flat[ch])) and not exact[ch][:, n:].any(), ch
    fast = ctx.ir_download(True, sr, capi.IR_FAST)
    assert fast.shape == exact.shape and fast.any()
    assert (np.abs(fast.astype(np.float64) - exact) <= fast_bound(exact, chans, sr)).all()


def test_state_and_arguments(oracle, cathedral):
    from parallel_reverb_raytracer_amd import capi
    a, _ = cathedral_cases(oracle, cathedral, 509, 24)

    def refused(c, code, surfaces=None):
        with pytest.raises(capi.RvbError) as e:
            c.reshade(surfaces, AIR_B)
        assert e.value.code == code, str(e.value)

    c = capi.Context(0)
    try:
        c.set_scene(cathedral["scene"])
        refused(c, capi.ERR_STATE)                                    # before any trace
        c.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
        names = [k for k, _ in c.last_timings()]
        assert names and not any(k in names for k in NEW_KERNELS)   # keeping off: no new kernel
        refused(c, capi.ERR_STATE)                                    # the trace was made without keeping
        c.keep_paths(True)
        refused(c, capi.ERR_STATE)                                    # ... and switching it on afterwards does not change that
        c.raytrace(a["mic"], a["source"], a["dirs"], 24, AIR_COEFFICIENTS)
        refused(c, capi.ERR_INVALID, cathedral["B"][:-1])             # wrong nsurfaces
        assert_state(c, a)                                           # a failed re-shade leaves the trace's results
        c.set_directions(a["dirs"])
        refused(c, capi.ERR_STATE)
        c.trace(a["mic"], a["source"], 24, AIR_COEFFICIENTS)
        c.set_scene(cathedral["scene"])
        refused(c, capi.ERR_STATE)
        c.trace(a["mic"], a["source"], 24, AIR_COEFFICIENTS)
        c.keep_paths(False)
        refused(c, capi.ERR_STATE)                                    # the side buffers are gone
        assert_state(c, a)
    finally:
        c.close()
