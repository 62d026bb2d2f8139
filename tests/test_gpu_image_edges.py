"""The image-source stage and every pass that rewrites its results on the constructed room of tests/image_edges.py, bit for bit against
the CPU oracle: image_plan_kernel / image_check_kernel (csrc/image_kernels.hip) in a plain trace, in a launch of three pairs with a
microphone and a source each, under a ray offset above 2^32 and in rvb_trace_group; reshade_images_kernel; the image stage that
rvb_relisten runs again; source_pattern_images_kernel and source_table_images_kernel.  The room has image sources of every order 1 .. 9
in every pair, (ray, order) items that a closest-hit or visibility query rejects, hidden direct paths, escaping rays and, under table B,
chains that die in one band: tests/test_image_edge_inputs.py asserts all of that on the oracle's data.

Every candidate is compared by (ray, slot), not only the merged images, and every volume by its bits (the sign of a zero included).
Nothing is compared with a second GPU result but "the same call again gives the same bytes"."""
import functools

import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, NUM_IMAGE_SOURCE

from test_gpu_reshade import AIR_B
from test_gpu_source_pattern import expected_records as pattern_records
from test_gpu_source_pattern import bits, oracle_range, same_records
from test_gpu_source_table import ORIENT, OTHER_ORIENT, SPREAD
from test_gpu_source_table import expected_records as table_records

pytestmark = pytest.mark.gpu

VARIANTS = [(True, False), (False, False), (True, True), (False, True)]            # (panel, hole)
KEPT_SHAPES = [E.MAIN, (64, 2), (64, 9), (130, 32)]
# cardioid in some bands, figure-of-eight in the others; a facing per pair
PATTERN_SHAPES = np.array([0.5, 1.0, 0.5, 1.0, 1.0, 0.5, 0.5, 1.0], np.float32)
FACINGS = np.array([(0.8, 0.35, -0.5), (-1.0, 0.2, 0.1), (0.1, -0.6, 0.9)], np.float32)
TABLE_FACINGS = np.array([ORIENT[0], OTHER_ORIENT[0], (0.6, 0.0, 0.8)], np.float32)
TABLE_UPS = np.array([ORIENT[1], OTHER_ORIENT[1], (0.0, 1.0, 0.0)], np.float32)
# what the three-pair relisten moves to: every pair's source heard from the next pair's microphone
NEXT_MIC = (1, 2, 0)


@functools.lru_cache(maxsize=None)
def room(panel=True, hole=False):
    return E.room(panel, hole)


_cases = {}


def case_of(oracle, mic, source, shape=E.MAIN, table="A", panel=True, hole=False):
    """The oracle's trace as a dict: diffuse records, the direct slot, the candidates by (ray, slot) in ray-major order, the raw image
    and index arrays, and the keys tests/test_gpu_source_pattern.expected_records reads.  Computed once per key and never changed."""
    mic, source = tuple(float(x) for x in mic), tuple(float(x) for x in source)
    key = (mic, source, shape, table, panel, hole)
    if key not in _cases:
        nrays, nrefl = shape
        surfaces, air = E.tables()[table]
        dirs = E.directions(nrays)
        diffuse, image, index = oracle.raytrace(E.with_table(room(panel, hole), surfaces), mic, source, dirs, nrefl, air)
        idx = index.reshape(nrays, NUM_IMAGE_SOURCE)
        rays, slots = np.nonzero(idx[:, 1:])
        cand = {"ray": rays.astype(np.uint64), "slot": (slots + 1).astype(np.uint64), "index": idx[rays, slots + 1].astype(np.uint64),
                "impulse": image.reshape(nrays, NUM_IMAGE_SOURCE)[rays, slots + 1].copy()}
        _cases[key] = {"mic": mic, "source": source, "dirs": dirs, "nrefl": nrefl, "nrays": nrays, "diffuse": diffuse, "direct": image[:1].copy(),
                       "cand": cand, "image": image, "index": index, "images": oracle.collect_images(image, index, False)}
    return _cases[key]


def pair_cases(oracle, shape=E.MAIN, table="A", mics=None, **variant):
    """The three pairs' cases; mics: other microphones than the pairs' own"""
    return [case_of(oracle, E.PAIRS[p][0] if mics is None else mics[p], E.PAIRS[p][1], shape, table, **variant) for p in range(3)]


def scaled(oracle, case, kind, pair=0):
    """`case` under the source directivity of pair `pair` — kind "pattern": PATTERN_SHAPES facing FACINGS[pair]; "table": the spread table
    in the orientation TABLE_FACINGS / TABLE_UPS[pair] —: the oracle's records times the oracle's gains, as the existing directivity
    tests compute them (expected_records of tests/test_gpu_source_pattern.py and tests/test_gpu_source_table.py), here for the direct
    slot and EVERY candidate: one gain row per distinct position, since a gain depends on microphone - position alone."""
    records = np.concatenate([case["direct"], case["cand"]["impulse"]])
    _, first, inverse = np.unique(bits(records["position"]), axis=0, return_index=True, return_inverse=True)
    fake = dict(case, images=records[first])
    if kind == "pattern":
        diffuse, _, g_diffuse, gains = pattern_records(oracle, fake, FACINGS[pair], PATTERN_SHAPES)
    else:
        diffuse, _, g_diffuse, gains = table_records(oracle, fake, SPREAD, (TABLE_FACINGS[pair], TABLE_UPS[pair]))
    assert (g_diffuse != 1).any() and len({g.tobytes() for g in gains}) > len(gains) // 2, "the gains hardly differ"
    records["volume"] = records["volume"] * gains[inverse.reshape(-1)]
    out = {k: case[k] for k in ("mic", "source", "nrays", "nrefl")}
    out.update({"diffuse": diffuse, "direct": records[:1], "cand": dict(case["cand"], impulse=records[1:])})
    return out


def states_of(ctx, npairs=1, offset=0, pairs=False):
    """Per pair what the context holds: the diffuse slice, the pair's candidates with ray numbers relative to the pair, the direct slot.
    pairs: through select_pair / get_pair_candidates; else a single trace, whose reported rays carry the offset."""
    diffuse = ctx.get_raw_diffuse().reshape(npairs, -1)
    cand = ctx.get_image_candidates()
    assert (cand["ray"] >= np.uint64(offset)).all() and (cand["ray"] < np.uint64(offset + npairs * ctx.nrays)).all(), "a reported ray is not offset + ray"
    out = []
    for p in range(npairs):
        if pairs:
            ctx.select_pair(p)
            mine = ctx.get_pair_candidates(p, cand)
        else:
            mine = cand.copy()
            mine["ray"] -= np.uint64(offset)
        out.append({"diffuse": diffuse[p], "cand": mine, "direct": ctx.get_direct()})
    assert sum(s["cand"].shape[0] for s in out) == cand.shape[0], "a candidate belongs to no pair"
    return out


def snapshot(states):
    return [(s["diffuse"].tobytes(), s["cand"].tobytes(), s["direct"].tobytes()) for s in states]


def assert_equal(oracle, state, want, what):
    """diffuse records (padding too), every candidate by (ray, slot, index) with its impulse, the direct slot; for an unscaled case also
    the merged images with and without the direct path"""
    from parallel_reverb_raytracer_amd import capi
    got = state["diffuse"]
    assert got.shape == want["diffuse"].shape and same_records(got, want["diffuse"]), what + ": diffuse records"
    assert not got["pad"].any() and not got["position"][:, 3].any(), what
    cand, w = state["cand"], want["cand"]
    assert cand.shape[0] == w["ray"].shape[0], what + ": %d candidates, the oracle has %d" % (cand.shape[0], w["ray"].shape[0])
    for field in ("ray", "slot", "index"):
        assert np.array_equal(cand[field].astype(np.uint64), w[field]), what + ": candidate " + field
    wrong = np.flatnonzero((bits(cand["impulse"]["volume"]) != bits(w["impulse"]["volume"])).any(axis=1))
    assert wrong.size == 0, what + ": candidate volumes, first at (ray %d, slot %d): %r, the oracle has %r" % (
        cand["ray"][wrong[0]], cand["slot"][wrong[0]], cand["impulse"]["volume"][wrong[0]].tolist(), w["impulse"]["volume"][wrong[0]].tolist())
    assert same_records(cand["impulse"], w["impulse"]), what + ": candidate positions and times"
    assert not cand["impulse"]["pad"].any() and not cand["impulse"]["position"][:, 3].any(), what
    assert state["direct"].view(np.uint32).tobytes() == np.ascontiguousarray(want["direct"]).view(np.uint32).tobytes(), what + ": direct slot"
    if "image" in want:
        for remove_direct in (False, True):
            images = capi.merge_images(cand, state["direct"], remove_direct)
            merged = oracle.collect_images(want["image"], want["index"], remove_direct)
            assert images.shape == merged.shape and same_records(images, merged), what + ": merged images"


def assert_states(oracle, states, wants, what):
    assert len(states) == len(wants)
    for p, (state, want) in enumerate(zip(states, wants)):
        assert_equal(oracle, state, want, "%s, pair %d" % (what, p))


def assert_ground(wants):
    """Not on empty ground (tests/test_image_edge_inputs.py holds the inputs to much more): candidates of every order the shape has, at
    least three each at 509 rays, one each at 64 and 130; five rays reach order 2."""
    for want in wants:
        last = min(want["nrefl"], NUM_IMAGE_SOURCE - 1) if want["nrays"] >= 64 else 2
        per_order = np.bincount(want["cand"]["slot"].astype(np.int64), minlength=NUM_IMAGE_SOURCE)[1:]
        assert (per_order[:last] >= (3 if want["nrays"] == E.MAIN[0] else 1)).all(), per_order


def new_context(scene, keep=None):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(scene)
    if keep is not None:
        c.keep_paths(True, listener=keep == "listener")
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_context(room())
    yield c
    c.close()


@pytest.fixture(scope="module", params=["four_lanes_per_ray", "two_lanes_per_ray", "one_lane_per_ray"])
def lanes_ctx(request):
    """All three path kernels, as in tests/test_gpu_parity.py."""
    c = new_context(room())
    if request.param == "two_lanes_per_ray":
        c.set_concurrent_traces(1 << 20)
    if request.param == "one_lane_per_ray":
        c.set_path_lanes(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kept():
    """keep_paths(True): what a re-shade needs"""
    c = new_context(room(), "materials")
    yield c
    c.close()


@pytest.fixture(scope="module")
def kept_listener():
    """keep_paths(True, listener=True): and what a relisten needs"""
    c = new_context(room(), "listener")
    yield c
    c.close()


def trace_twice(oracle, c, want, what, offset=0):
    """One pair through rvb_trace, held to the oracle; the second trace must give the bytes of the first."""
    c.set_directions(want["dirs"])
    c.trace(want["mic"], want["source"], want["nrefl"], AIR_COEFFICIENTS, ray_offset=offset)
    states = states_of(c, offset=offset)
    assert_equal(oracle, states[0], want, what)
    c.trace(want["mic"], want["source"], want["nrefl"], AIR_COEFFICIENTS, ray_offset=offset)
    assert snapshot(states_of(c, offset=offset)) == snapshot(states), what + ": second trace"


# ---- 1. the plain trace -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [E.MAIN] + list(E.EDGE_SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("panel,hole", VARIANTS)
def test_plain_trace_of_every_variant_and_shape(ctx, oracle, panel, hole, shape):
    """509 x 12 and the edge shapes of tests/image_edges.py, each of the three pairs, with and without the panel and the hole."""
    wants = pair_cases(oracle, shape, panel=panel, hole=hole)
    assert_ground(wants if shape == E.MAIN else wants[:1])
    ctx.set_scene(room(panel, hole))
    try:
        for p, want in enumerate(wants):
            trace_twice(oracle, ctx, want, "panel %s, hole %s, %d x %d, pair %d" % (panel, hole, shape[0], shape[1], p))
    finally:
        ctx.set_scene(room())


@pytest.mark.parametrize("hole", [False, True])
def test_main_shape_through_every_path_kernel(lanes_ctx, oracle, hole):
    wants = pair_cases(oracle, hole=hole)
    assert_ground(wants)
    lanes_ctx.set_scene(room(True, hole))
    for p, want in enumerate(wants):
        trace_twice(oracle, lanes_ctx, want, "hole %s, pair %d" % (hole, p))


# ---- 2. three pairs in one launch, a ray offset ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("hole", [False, True])
@pytest.mark.parametrize("offset", [0, E.RAY_OFFSET])
def test_three_pairs_in_one_launch_each_with_its_own_microphone_and_source(ctx, oracle, offset, hole):
    """3 x 509 rays: the pair boundaries fall inside waves of the plan kernel.  The reported rays are offset + pair * 509 + ray, and
    get_pair_candidates sorts them into their pairs."""
    wants = pair_cases(oracle, hole=hole)
    assert_ground(wants)
    nrays, nrefl = E.MAIN
    ctx.set_scene(room(True, hole))
    try:
        ctx.set_directions(E.directions(nrays))
        ctx.trace_pairs(E.MICS, E.SOURCES, nrefl, AIR_COEFFICIENTS, ray_offset=offset)
        reported = ctx.get_image_candidates()["ray"]
        assert np.array_equal(reported, np.concatenate([w["cand"]["ray"] + np.uint64(offset + p * nrays) for p, w in enumerate(wants)]))
        states = states_of(ctx, 3, offset, pairs=True)
        assert_states(oracle, states, wants, "three pairs, offset %d" % offset)
        ctx.trace_pairs(E.MICS, E.SOURCES, nrefl, AIR_COEFFICIENTS, ray_offset=offset)
        assert snapshot(states_of(ctx, 3, offset, pairs=True)) == snapshot(states), "second trace"
    finally:
        ctx.set_scene(room())


@pytest.mark.parametrize("pair", [0, 1, 2])
def test_a_single_trace_with_a_ray_offset_above_32_bits(ctx, oracle, pair):
    trace_twice(oracle, ctx, pair_cases(oracle)[pair], "pair %d, offset 2^32 + 5" % pair, offset=E.RAY_OFFSET)


# ---- 3. re-shading ----------------------------------------------------------------------------------------------------------------------

def reshade_there_and_back(oracle, c, trace, a_wants, b_wants, what, **how):
    """Traced with table A; reshade(B, air B) gives the oracle's trace with B, reshade(None, air A) the original bytes."""
    trace(c)
    states = states_of(c, len(a_wants), **how)
    assert_states(oracle, states, a_wants, what + ": kept trace")
    c.reshade(E.table_b(), AIR_B)
    names = [k for k, _ in c.last_timings()]
    assert "reshade_images_kernel" in names and not any("path" in k or "shadow" in k or "image_kernel" in k for k in names), names
    other = states_of(c, len(a_wants), **how)
    assert_states(oracle, other, b_wants, what + ": re-shaded to B")
    assert all(x[i] != y[i] for x, y in zip(snapshot(states), snapshot(other)) for i in (0, 1))
    c.reshade(None, AIR_COEFFICIENTS)
    assert snapshot(states_of(c, len(a_wants), **how)) == snapshot(states), what + ": back to A"


@pytest.mark.parametrize("hole", [False, True])
@pytest.mark.parametrize("shape", KEPT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_reshaded_candidates_equal_the_oracle_trace_with_the_other_table(kept, oracle, shape, hole):
    """Every pair on its own: the chain over the first slot - 1 bounces of the candidate's ray at every order, the dead band's zeros with
    their signs, the hidden direct slots of pairs two and three staying all-zero."""
    a_wants, b_wants = pair_cases(oracle, shape, "A", hole=hole), pair_cases(oracle, shape, "B", hole=hole)
    assert_ground(a_wants[:1])
    if shape == E.MAIN:
        for b in b_wants:
            dead = b["cand"]["impulse"]["volume"][:, E.DEAD_BAND]
            assert ((dead == 0) & np.signbit(dead)).any() and ((dead == 0) & ~np.signbit(dead)).any() and (dead != 0).any()
        assert not b_wants[1]["direct"].view(np.uint32).any() and not b_wants[2]["direct"].view(np.uint32).any()
    kept.set_scene(room(True, hole))
    try:
        for p in range(3):
            def trace(c, want=a_wants[p]):
                c.set_directions(want["dirs"])
                c.trace(want["mic"], want["source"], want["nrefl"], AIR_COEFFICIENTS)
            reshade_there_and_back(oracle, kept, trace, a_wants[p:p + 1], b_wants[p:p + 1], "%d x %d, hole %s, pair %d" % (shape[0], shape[1], hole, p))
    finally:
        kept.set_scene(room())


@pytest.mark.parametrize("offset", [0, E.RAY_OFFSET])
def test_reshaded_candidates_of_a_three_pair_launch(kept, oracle, offset):
    """candidates[i] and image_dist[i] in the order the image kernel appended them, over three pairs; the early ids of ray - ray_offset"""
    a_wants, b_wants = pair_cases(oracle, table="A"), pair_cases(oracle, table="B")

    def trace(c):
        c.set_directions(E.directions(E.MAIN[0]))
        c.trace_pairs(E.MICS, E.SOURCES, E.MAIN[1], AIR_COEFFICIENTS, ray_offset=offset)
    reshade_there_and_back(oracle, kept, trace, a_wants, b_wants, "three pairs, offset %d" % offset, offset=offset, pairs=True)


def test_a_reshaded_single_trace_with_a_ray_offset(kept, oracle):
    a, b = pair_cases(oracle, table="A")[2], pair_cases(oracle, table="B")[2]

    def trace(c):
        c.set_directions(a["dirs"])
        c.trace(a["mic"], a["source"], a["nrefl"], AIR_COEFFICIENTS, ray_offset=E.RAY_OFFSET)
    reshade_there_and_back(oracle, kept, trace, [a], [b], "pair 2, offset 2^32 + 5", offset=E.RAY_OFFSET)


# ---- 4. a new microphone ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [E.MAIN, (64, 2), (64, 9)], ids=lambda s: "%dx%d" % s)
def test_relistened_candidates_equal_the_oracle_trace_with_the_other_microphone(kept_listener, oracle, shape):
    """Pair one traced, then heard from the microphones of pairs two and three (both behind the panel: the direct slot becomes all-zero)
    and from its own again; then re-shaded to B and heard from each once more.  Orders 2 and above read the ray's volume from the
    records that the relisten rebuilt."""
    c = kept_listener
    source = E.PAIRS[0][1]
    own = {t: [case_of(oracle, E.PAIRS[m][0], source, shape, t) for m in range(3)] for t in "AB"}
    if shape == E.MAIN:
        assert_ground(own["A"] + own["B"])
        assert (own["A"][0]["direct"]["volume"] != 0).all() and not own["A"][1]["direct"].view(np.uint32).any()
    a = own["A"][0]
    c.set_directions(a["dirs"])
    c.trace(a["mic"], source, a["nrefl"], AIR_COEFFICIENTS)
    assert_equal(oracle, states_of(c)[0], a, "kept trace")
    for m in (1, 2, 0):
        c.relisten(E.PAIRS[m][0])
        names = [k for k, _ in c.last_timings()]
        assert "image_kernel" in names and not any("path" in k for k in names), names
        assert_equal(oracle, states_of(c)[0], own["A"][m], "relistened from microphone %d" % m)
    c.reshade(E.table_b(), AIR_B)
    assert_equal(oracle, states_of(c)[0], own["B"][0], "re-shaded to B")
    for m in (2, 1):
        c.relisten(E.PAIRS[m][0])
        assert_equal(oracle, states_of(c)[0], own["B"][m], "B, relistened from microphone %d" % m)
    c.reshade(None, AIR_COEFFICIENTS)
    assert_equal(oracle, states_of(c)[0], own["A"][1], "back to A at microphone 1")


@pytest.mark.parametrize("offset", [0, E.RAY_OFFSET])
def test_every_pair_of_a_three_pair_launch_is_relistened(kept_listener, oracle, offset):
    c = kept_listener
    other_mics = np.array([E.PAIRS[m][0] for m in NEXT_MIC], np.float32)
    wants = {(t, moved): pair_cases(oracle, table=t, mics=other_mics if moved else None) for t in "AB" for moved in (False, True)}
    assert_ground(wants["A", True] + wants["B", True])
    c.set_directions(E.directions(E.MAIN[0]))
    c.trace_pairs(E.MICS, E.SOURCES, E.MAIN[1], AIR_COEFFICIENTS, ray_offset=offset)
    assert_states(oracle, states_of(c, 3, offset, pairs=True), wants["A", False], "kept trace")
    c.relisten(other_mics)
    assert_states(oracle, states_of(c, 3, offset, pairs=True), wants["A", True], "relistened")
    c.reshade(E.table_b(), AIR_B)
    assert_states(oracle, states_of(c, 3, offset, pairs=True), wants["B", True], "relistened, then re-shaded")
    c.relisten(E.MICS)
    assert_states(oracle, states_of(c, 3, offset, pairs=True), wants["B", False], "... and heard from the pairs' own microphones")


# ---- 5. source directivity on the candidates ------------------------------------------------------------------------------------------

def set_directivity(c, kind, pairs):
    """The directivity of scaled(): of pair 0 for a single trace, one per pair for the three-pair launch"""
    n = 3 if pairs else 1
    if kind == "pattern":
        c.set_source_pattern(FACINGS[:n] if pairs else FACINGS[0], PATTERN_SHAPES)
    else:
        c.set_source_table(SPREAD, TABLE_FACINGS[:n] if pairs else TABLE_FACINGS[0], TABLE_UPS[:n] if pairs else TABLE_UPS[0])


def clear_directivity(c):
    c.set_source_table(None)
    c.set_source_pattern(None)


@pytest.mark.parametrize("pairs", [False, True], ids=["one_pair", "three_pairs_with_offset"])
@pytest.mark.parametrize("kind", ["pattern", "table"])
def test_source_directivity_on_every_candidate(ctx, kept, oracle, kind, pairs):
    """The candidates and the direct slot(s) equal the oracle's records times the oracle's gain for microphone - position, with the
    microphone and the directivity of the candidate's own pair — after a trace, and after a re-shade of a kept trace (which scales the
    re-shaded records again)."""
    offset = E.RAY_OFFSET if pairs else 0
    plain = {t: pair_cases(oracle, table=t)[:3 if pairs else 1] for t in "AB"}
    assert_ground(plain["A"])
    wants = {t: [scaled(oracle, case, kind, p) for p, case in enumerate(plain[t])] for t in "AB"}
    for p, (want, case) in enumerate(zip(wants["A"], plain["A"])):
        for b in range(8):
            assert (want["cand"]["impulse"]["volume"][:, b] != case["cand"]["impulse"]["volume"][:, b]).any(), (p, b)
    kernel = "source_pattern_kernel" if kind == "pattern" else "source_table_kernel"

    def trace(c):
        c.set_directions(E.directions(E.MAIN[0]))
        if pairs:
            c.trace_pairs(E.MICS, E.SOURCES, E.MAIN[1], AIR_COEFFICIENTS, ray_offset=offset)
        else:
            c.trace(*E.PAIRS[0], E.MAIN[1], AIR_COEFFICIENTS)
        return states_of(c, len(wants["A"]), offset, pairs=pairs)

    for c in (ctx, kept):
        try:
            set_directivity(c, kind, pairs)
            states = trace(c)
            assert kernel in [k for k, _ in c.last_timings()]
            assert_states(oracle, states, wants["A"], kind + " after the trace")
            if c is kept:
                c.reshade(E.table_b(), AIR_B)
                assert kernel in [k for k, _ in c.last_timings()]
                assert_states(oracle, states_of(c, len(wants["A"]), offset, pairs=pairs), wants["B"], kind + " after the re-shade")
                c.reshade(None, AIR_COEFFICIENTS)
                assert snapshot(states_of(c, len(wants["A"]), offset, pairs=pairs)) == snapshot(states), kind + " back to A"
        finally:
            clear_directivity(c)
    assert_states(oracle, trace(ctx), plain["A"], "the directivity switched off again")


# ---- 6. rvb_trace_group ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [0, 2], ids=["a_launch_per_context", "one_group_launch"])
def test_trace_group_each_context_equals_the_oracle(oracle, lanes):
    """Three contexts, one pair and one ray offset each.  509 rays per context are too few for the group kernel to be chosen, so the
    second case asks for two lanes per ray: the three path stages are one path_pair_group_kernel launch."""
    from parallel_reverb_raytracer_amd import capi
    wants = pair_cases(oracle)
    offsets = [0, E.MAIN[0], E.RAY_OFFSET]
    contexts = [new_context(room()) for _ in range(3)]
    try:
        for c in contexts:
            c.set_directions(E.directions(E.MAIN[0]))
            c.set_path_lanes(lanes)
        for again in range(2):
            capi.Context.trace_group(contexts, E.MICS, E.SOURCES, E.MAIN[1], AIR_COEFFICIENTS, offsets)
            for p, c in enumerate(contexts):
                assert ("path_pair_kernel" if lanes == 2 else "path_kernel") in dict(c.last_timings())
                assert_equal(oracle, states_of(c, offset=offsets[p])[0], wants[p], "context %d, launch %d" % (p, again))
    finally:
        for c in contexts:
            c.close()


def test_time_ranges_follow_the_kept_passes(kept_listener, oracle):
    """The diffuse time range of the selected pair after a relisten and a re-shade of the three-pair launch (the mute wall of table B and
    the other microphone move it)."""
    from parallel_reverb_raytracer_amd import capi
    c = kept_listener
    other_mics = np.array([E.PAIRS[m][0] for m in NEXT_MIC], np.float32)
    wants = pair_cases(oracle, table="B", mics=other_mics)
    plain = pair_cases(oracle)
    assert any(oracle_range(w["diffuse"]) != oracle_range(p["diffuse"]) for w, p in zip(wants, plain))
    c.set_directions(E.directions(E.MAIN[0]))
    c.trace_pairs(E.MICS, E.SOURCES, E.MAIN[1], AIR_COEFFICIENTS)
    c.relisten(other_mics)
    c.reshade(E.table_b(), AIR_B)
    for p, want in enumerate(wants):
        c.select_pair(p)
        c.ir_configure_speakers(want["mic"], [(-1, 0, -1), (1, 0, -1)], [0.5, 0.5], capi.IR_DIFFUSE, None)
        assert c.ir_time_range() == oracle_range(want["diffuse"]), p
