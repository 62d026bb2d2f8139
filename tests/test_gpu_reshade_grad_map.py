"""The sensitivity map: material gradients per triangle from a kept trace (rvb_reshade_grad_map, csrc/reshade_grad_map_kernels.hip).

The reference is the binary64 numpy gradient of tests/test_gpu_reshade_grad.py, applied to the same scene RELABELLED with one surface per
triangle: triangles["surface"] = arange(ntriangles), table[t] = T[surface(t)].  Its per-surface gradient is then the per-triangle one, and
its bar holds entry by entry as derived there:  |gpu - ref| <= 4 (nreflections + 16) 2^-24 A + 1e-30;  an entry with A = 0 is exactly 0.
The context under test holds the scene as it is (seven surfaces); only the CPU oracle traces the relabelled one, once per shape and
module (chains: one probe trace per seven triangles).
Largest observed |gpu - ref| / bound per case: profiles/reshade_grad_map_n1.txt (printed by every comparison)."""
import ctypes

import numpy as np
import pytest

import decay_reference
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, SURFACE, aligned_copy

from test_gpu_reshade import AIR_B, SPEAKERS
from test_gpu_reshade_grad import (assert_ground, binning_of, bound_of, chains, compare, on_device, reference, snapshot, state_terms, table_t,
                                   weights)
from test_gpu_source_pattern import FACING, SHAPES
from test_gpu_source_table import ORIENT, SPREAD

pytestmark = pytest.mark.gpu

SR = 44100.0
OTHER_MIC, OTHER_SOURCE = (0.0, 12.0, 11.0), (0.0, 12.5, 11.5)          # the second pair of tests/test_gpu_reshade_grad.py
PLACE = np.array([0, 63, 64, 65, 3, 69, 6])                             # its seven surfaces in a table of 70


def per_triangle(scene, table):
    """The scene with one surface per triangle and the table that gives triangle t the coefficients of its surface in `table`."""
    triangles = aligned_copy(scene[0])
    triangles["surface"] = np.arange(triangles.shape[0])
    return triangles, scene[1], aligned_copy(np.ascontiguousarray(table[scene[0]["surface"].astype(np.int64)]))


def nan_map(ctx):
    import torch
    return torch.full((ctx.ntriangles, 16), float("nan"), dtype=torch.float32, device="cuda")


def map_of(ctx, predelay, nbins, w_dev, sr=SR):
    """The map into a tensor filled with NaN: every entry must have been written."""
    out = nan_map(ctx)
    assert ctx.reshade_grad_map(predelay, sr, nbins, w_dev.data_ptr(), out=out) is out
    m = out.cpu().numpy()
    assert not np.isnan(m).any(), "an entry of the map was not written"
    return m


def as_surfaces(m):
    return np.ascontiguousarray(m).view(SURFACE).reshape(-1)


def assert_map(m, r, label):
    worst = 0.0
    for what, cols in (("spec", m[:, :8]), ("diff", m[:, 8:])):
        worst = max(worst, float((np.abs(cols.astype(np.float64) - r["ref"][what]) / bound_of(r, what)).max()))
    print("reshade_grad_map %-48s max |gpu - ref| / bound = %.4f" % (label, worst))
    for what, cols in (("spec", m[:, :8]), ("diff", m[:, 8:])):
        assert (np.abs(cols.astype(np.float64) - r["ref"][what]) <= bound_of(r, what)).all(), (label, what)
        assert not cols[r["a"][what] == 0].any(), (label, what, "an entry with A = 0 is not exactly 0")
    assert not m[~r["touched"]].any(), label


def check(ctx, chain, table, mic, nrefl, label, speakers=SPEAKERS, seed=5, records=None):
    """The map of seeded normal weights against the relabelled reference of the current records.  chain, table: of the relabelled scene."""
    from parallel_reverb_raytracer_amd import capi
    predelay, nbins = binning_of(ctx, mic, speakers, SR)
    w = weights(len(speakers[1]), nbins, seed)
    term, absterm, dist, _, _ = state_terms(ctx, mic, speakers, predelay, SR, nbins, w, records)
    r = reference(term, absterm, dist, chain, table, nrefl)
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    w_dev = on_device(w)
    m = map_of(ctx, predelay, nbins, w_dev)
    assert_map(m, r, label)
    return {"map": m, "r": r, "w_dev": w_dev, "predelay": predelay, "nbins": nbins}


def ground_of(r):
    """(triangles with A > 0 somewhere, share of the entries with A > 0 that stand 100 bounds clear of zero): on the reference alone."""
    positive = np.concatenate([r["a"][k] > 0 for k in ("spec", "diff")], axis=1)
    clear = np.concatenate([np.abs(r["ref"][k]) >= 100.0 * bound_of(r, k) for k in ("spec", "diff")], axis=1)
    return int(positive.any(axis=1).sum()), float(clear[positive].mean()) if positive.any() else 0.0


def kept_context(scene):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(scene)
    c.keep_paths(True, listener=True)
    return c


@pytest.fixture(scope="module")
def small():
    """scenes.cathedral(100): its smallest mesh, 816 triangles — 117 probe traces of the oracle per shape."""
    scene, info = scenes.cathedral(100)
    assert scene[0].shape[0] == 816 and scene[2].shape[0] == 7
    return {"scene": scene, "mic": info["mic"], "source": info["source"], "T": table_t(scene[2]), "name": "cathedral(100)"}


@pytest.fixture(scope="module")
def small_ctx(small):
    c = kept_context(small["scene"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def cathedral():
    scene, info = scenes.cathedral(3000)
    assert scene[2].shape[0] == 7
    return {"scene": scene, "mic": info["mic"], "source": info["source"], "T": table_t(scene[2]), "name": "cathedral(3000)"}


@pytest.fixture(scope="module")
def ctx(cathedral):
    c = kept_context(cathedral["scene"])
    yield c
    c.close()


def traced(ctx, oracle, world, nrays, nrefl, relabelled, seed=23):
    """Traces on the GPU; the chains of the oracle in the relabelled scene (relabelled: per triangle) or in the scene as it is."""
    dirs = scenes.sphere_directions(nrays, seed=seed)
    if relabelled:
        scene = per_triangle(world["scene"], world["scene"][2])
        key = (world["name"] + " per triangle", nrays, nrefl, seed)
    else:
        scene, key = world["scene"], ("cathedral", nrays, nrefl, seed)            # (the key of tests/test_gpu_reshade_grad.py: the same chains)
    chain = chains(oracle, key, scene, world["mic"], world["source"], dirs, nrefl)
    ctx.raytrace(world["mic"], world["source"], dirs, nrefl, AIR_COEFFICIENTS)
    return chain, dirs


@pytest.mark.parametrize("nrays,nrefl", [(509, 24), (5, 70), (8, 33), (8, 1)])
def test_map_equals_the_relabelled_reference_after_a_trace_and_after_a_reshade(small_ctx, oracle, small, nrays, nrefl):
    """509 x 24: a partial last wave, a partial second tile of bounces; 5 x 70: a ray longer than a wave, fewer rays than a wave takes;
    8 x 33: exactly one wave, a third tile of one bounce; 8 x 1: a single bounce.  The ground is checked on the reference alone."""
    chain, _ = traced(small_ctx, oracle, small, nrays, nrefl, True)
    own = chain[1]
    mic = small["mic"]
    for label, table in (("after the trace", small["scene"][2]), ("after reshade(T, AIR_B)", small["T"])):
        if table is small["T"]:
            small_ctx.reshade(table, AIR_B)
        out = check(small_ctx, chain, per_triangle(small["scene"], table)[2], mic, nrefl, "cathedral(100) %dx%d %s" % (nrays, nrefl, label))
        with_a, clear = ground_of(out["r"])
        print("reshade_grad_map ground %dx%d: %d triangles with A > 0, %.3f of their entries 100 bounds clear of zero" % (nrays, nrefl, with_a, clear))
        if nrays != 8:
            assert with_a >= 100 and clear >= 0.9, (with_a, clear)
        else:
            assert with_a >= 1
        assert out["map"].any()
    if (nrays, nrefl) == (509, 24):
        assert np.setdiff1d(np.arange(816), own[own >= 0]).shape[0] >= 400, "(404 of the 816 triangles have no record of their own)"


def test_runs_longer_than_a_tile(oracle):
    """The open shoebox of test_escapes_and_a_surface_on_no_triangle: ten triangles, so a few runs hold everything.  By the chains the
    longest run spans at least three tiles of the fold and ends inside one: a partial in a tile's slot 1, whole tiles, a last partial."""
    from parallel_reverb_raytracer_amd import capi
    tile = capi.GRAD_MAP_TILE
    triangles, vertices, surfaces = scenes.shoebox()
    scene = (aligned_copy(triangles[:-2]), vertices, surfaces)
    mic, src, nrays, nrefl = (0.5, 1.0, 2.0), (-0.7, -1.2, -5.0), 8000, 24
    dirs = scenes.sphere_directions(nrays, seed=3)
    chain = chains(oracle, ("open shoebox per triangle", nrays, nrefl), per_triangle(scene, surfaces), mic, src, dirs, nrefl)
    own = chain[1]
    counts = np.bincount(own[own >= 0], minlength=10)
    ends = np.cumsum(counts)
    longest = int(np.argmax(counts))
    first, last = (ends[longest] - counts[longest]) // tile, (ends[longest] - 1) // tile
    assert last - first >= 2 and ends[longest] % tile != 0, (counts, ends)
    assert (own < 0).reshape(nrays, nrefl)[:, -1].sum() >= 10, "no ray escapes"
    table = table_t(surfaces, seed=12)
    c = kept_context(scene)
    try:
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        for label, tab in (("open shoebox after the trace", surfaces), ("open shoebox after reshade", table)):
            if tab is table:
                c.reshade(table, AIR_B)
            out = check(c, chain, per_triangle(scene, tab)[2], mic, nrefl, label)
            assert_ground(out["r"])
            assert out["map"][longest].all()
    finally:
        c.close()


def test_the_sum_over_a_surface_is_the_surface_gradient(ctx, oracle, cathedral):
    """|surface_sums(map)[s] - ref[s]| <= bound[s] + 2^-24 sum_{t in s} |map[t]|: the reference's own bar for the surface and the one float
    rounding per triangle.  Surface 0 lies on no triangle: its sums are over nothing."""
    from parallel_reverb_raytracer_amd import fitting
    nrays, nrefl = 130, 24
    chain, _ = traced(ctx, oracle, cathedral, nrays, nrefl, False)
    ctx.reshade(cathedral["T"], AIR_B)
    out = compare(ctx, chain, cathedral["T"], cathedral["mic"], nrefl, "seven surfaces (for the sums of the map)")
    r = out["r"]
    m = map_of(ctx, out["predelay"], out["nbins"], out["w_dev"])
    triangles = cathedral["scene"][0]
    sums = fitting.surface_sums(as_surfaces(m), triangles, 7)
    slack = 2.0 ** -24 * fitting.surface_sums(as_surfaces(np.abs(m)), triangles, 7)
    worst = 0.0
    for what, cols in (("spec", slice(0, 8)), ("diff", slice(8, 16))):
        miss = np.abs(sums[:, cols] - r["ref"][what])
        allowed = bound_of(r, what) + slack[:, cols]
        worst = max(worst, float((miss / allowed).max()))
        assert (miss <= allowed).all(), what
    print("reshade_grad_map sums over the surfaces: max |sum - ref| / allowed = %.4f" % worst)
    assert not (triangles["surface"] == 0).any() and not sums[0].any()
    assert np.abs(sums[1:]).min() > 0


def test_bit_for_bit(ctx, oracle, cathedral):
    """Two calls; the surfaces renumbered; a relistened trace against a fresh one; a pair of two against the pair alone."""
    from parallel_reverb_raytracer_amd import capi
    nrays, nrefl = 130, 24
    scene, mic, src = cathedral["scene"], cathedral["mic"], cathedral["source"]
    dirs = scenes.sphere_directions(nrays, seed=23)

    def fresh(scene_, table, at_mic, at_source):
        c = kept_context(scene_)
        try:
            c.raytrace(at_mic, at_source, dirs, nrefl, AIR_COEFFICIENTS)
            c.reshade(table, AIR_B)
            c.ir_configure_speakers(at_mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
            return map_of(c, predelay, nbins, w_dev)
        finally:
            c.close()

    ctx.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
    ctx.reshade(cathedral["T"], AIR_B)
    predelay, nbins = binning_of(ctx, mic, SPEAKERS, SR)
    w_dev = on_device(weights(2, nbins, 5))
    first = map_of(ctx, predelay, nbins, w_dev)
    assert first[:, :8].any() and first[:, 8:].any()
    assert map_of(ctx, predelay, nbins, w_dev).tobytes() == first.tobytes()
    # the seven surfaces spread over a table of 70: the map does not depend on surface numbers
    triangles = aligned_copy(scene[0])
    triangles["surface"] = PLACE[scene[0]["surface"]]
    wide, wide_t = aligned_copy(np.resize(scene[2], 70)), aligned_copy(np.resize(cathedral["T"], 70))
    wide[PLACE], wide_t[PLACE] = scene[2], cathedral["T"]
    assert fresh((triangles, scene[1], wide), wide_t, mic, src).tobytes() == first.tobytes()
    # another microphone on the kept trace against a fresh kept trace there
    ctx.relisten(OTHER_MIC)
    ctx.ir_configure_speakers(OTHER_MIC, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    relistened = map_of(ctx, predelay, nbins, w_dev)
    assert relistened.tobytes() != first.tobytes()
    assert relistened.tobytes() == fresh(scene, cathedral["T"], OTHER_MIC, src).tobytes()
    # pair 1 of two pairs against the pair traced alone
    mics, sources = np.array([mic, OTHER_MIC], np.float32), np.array([src, OTHER_SOURCE], np.float32)
    ctx.set_directions(dirs)
    try:
        ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
        ctx.reshade(cathedral["T"], AIR_B)
        ctx.select_pair(1)
        ctx.ir_configure_speakers(OTHER_MIC, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        second_pair = map_of(ctx, predelay, nbins, w_dev)
        ctx.select_pair(0)
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        assert map_of(ctx, predelay, nbins, w_dev).tobytes() == first.tobytes()
    finally:
        ctx.npairs = 1
    assert second_pair.any() and second_pair.tobytes() != relistened.tobytes()
    assert second_pair.tobytes() == fresh(scene, cathedral["T"], OTHER_MIC, OTHER_SOURCE).tobytes()


@pytest.mark.parametrize("directivity", ["pattern", "table"])
def test_a_source_pattern_and_a_source_table(small_ctx, oracle, small, directivity):
    """Either is a factor of every term of its ray; state_terms starts from the scaled records in the context."""
    nrays, nrefl = 130, 24
    if directivity == "pattern":
        small_ctx.set_source_pattern(FACING, SHAPES)
    else:
        small_ctx.set_source_table(SPREAD, *ORIENT)
    try:
        chain, _ = traced(small_ctx, oracle, small, nrays, nrefl, True)
        check(small_ctx, chain, per_triangle(small["scene"], small["scene"][2])[2], small["mic"], nrefl, "source %s after the trace" % directivity)
        small_ctx.reshade(small["T"], AIR_B)
        scaled = check(small_ctx, chain, per_triangle(small["scene"], small["T"])[2], small["mic"], nrefl, "source %s after reshade" % directivity)
    finally:
        small_ctx.set_source_pattern(None)
        small_ctx.set_source_table(None)
    from parallel_reverb_raytracer_amd import capi
    traced(small_ctx, oracle, small, nrays, nrefl, True)
    small_ctx.reshade(small["T"], AIR_B)
    small_ctx.ir_configure_speakers(small["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    plain = map_of(small_ctx, scaled["predelay"], scaled["nbins"], scaled["w_dev"])
    assert (plain[:, 9:] != scaled["map"][:, 9:]).any()


def raw_call(c, predelay, rate, nbins, weights_pointer, map_pointer, ntriangles):
    rc = c.lib.rvb_reshade_grad_map(c.handle, ctypes.c_float(predelay), ctypes.c_float(rate), ctypes.c_uint64(nbins), ctypes.c_void_p(weights_pointer),
                                    ctypes.c_void_p(map_pointer), ctypes.c_uint64(ntriangles))
    return rc, c.lib.rvb_last_error(c.handle).decode()


def test_side_effects_states_and_arguments(small):
    import torch
    from parallel_reverb_raytracer_amd import capi
    mic, src, nrays, nrefl = small["mic"], small["source"], 509, 24
    dirs = scenes.sphere_directions(nrays, seed=23)
    w_dev = on_device(weights(2, 4096, 9))
    c = capi.Context(0)
    out = None

    def refused(code, predelay=0.0, rate=SR, nbins=4096, w=None, m=0, ntriangles=None):
        """The call's code and text; the map keeps its NaN fill."""
        rc, text = raw_call(c, predelay, rate, nbins, w_dev.data_ptr() if w is None else w, out.data_ptr() if m == 0 else m,
                            c.ntriangles if ntriangles is None else ntriangles)
        c.synchronize()
        assert rc == code, (rc, text)
        assert torch.isnan(out).all(), "a refused call wrote to the map"
        return text

    try:
        c.set_scene(small["scene"])
        out = nan_map(c)
        torch.cuda.synchronize()
        refused(capi.ERR_STATE)                                       # before any trace
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        assert "RVB_KEEP_LISTENER" in refused(capi.ERR_STATE)         # the trace was made without keeping
        c.keep_paths(True)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        assert "RVB_KEEP_LISTENER" in refused(capi.ERR_STATE)         # kept for the materials alone
        c.keep_paths(True, listener=True)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        assert "configuration" in refused(capi.ERR_STATE)             # no IR configuration since the trace
        before = snapshot(c, mic)
        predelay, nbins = binning_of(c, mic, SPEAKERS, SR)
        w = on_device(weights(2, nbins, 5))
        grad_before = c.reshade_grad(predelay, SR, nbins, w.data_ptr())
        hist_before = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
        c.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist_before)
        c.synchronize()
        first = map_of(c, predelay, nbins, w)
        names = [k for k, _ in c.last_timings()]
        assert len(names) == len(set(names)) == 5 and "reshade_grad_map_terms_kernel" in names and "reshade_grad_map_fold_kernel" in names, names
        assert first[:, :8].any() and first[:, 8:].any()
        assert snapshot(c, mic) == before                            # the records, the direct slot, the images, the time range
        grad_after = c.reshade_grad(predelay, SR, nbins, w.data_ptr())
        assert grad_after[0].tobytes() == grad_before[0].tobytes() and grad_after[1].tobytes() == grad_before[1].tobytes()
        map_of(c, predelay, nbins, w)
        hist_after = torch.zeros_like(hist_before)
        c.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist_after)
        c.synchronize()
        assert torch.equal(hist_before, hist_after) and bool(hist_after.any())
        # a prepared exact list is voided: the call sorts in the same buffers
        c.ir_exact_prepare(predelay, SR, nbins)
        folded = torch.zeros_like(hist_before)
        c.ir_exact_fold_tensor(nbins, 0, nbins, folded)
        map_of(c, predelay, nbins, w)
        with pytest.raises(capi.RvbError) as e:
            c.ir_exact_fold_tensor(nbins, 0, nbins, folded)
        assert e.value.code == capi.ERR_STATE
        # arguments
        refused(capi.ERR_INVALID, nbins=0)
        refused(capi.ERR_INVALID, rate=float("nan"))
        refused(capi.ERR_INVALID, predelay=float("inf"))
        refused(capi.ERR_INVALID, w=0)
        refused(capi.ERR_INVALID, m=None)
        assert "816" in refused(capi.ERR_INVALID, ntriangles=815)
        refused(capi.ERR_INVALID, ntriangles=817)
        wide = torch.full((2 * 8 * 4096 + 816 * 16,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for offset in (0, 2 * 8 * 4096 - 1):                         # the map on the weights; its first float on their last
            assert "overlaps" in refused(capi.ERR_INVALID, w=wide.data_ptr(), m=wide.data_ptr() + 4 * offset)
        assert torch.isnan(wide).all()
        # states
        c.ir_configure_hrtf(mic, scenes.hrtf_synthetic_table(), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), capi.IR_DIFFUSE, None)
        assert "HRTF" in refused(capi.ERR_STATE)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, c.get_raw_images(False))
        assert "RVB_IR_DIFFUSE" in refused(capi.ERR_STATE)
        nine = ([(np.cos(i), 0.0, np.sin(i)) for i in range(9)], [0.5] * 9)
        c.ir_configure_speakers(mic, nine[0], nine[1], capi.IR_DIFFUSE, None)
        assert "9 speaker" in refused(capi.ERR_STATE)
        assert snapshot(c, mic) == before                            # failed calls leave the results as they were
        # more reflections than a ray's chain checkpoints in LDS hold (the other RVB_ERR_CAPACITY, 2^32 records of a pair, would take
        # 256 GB of term rows: not run)
        c.raytrace(mic, src, dirs[:8], 2049, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        assert "2048" in refused(capi.ERR_CAPACITY)
        c.set_directions(dirs)
        assert "nothing traced" in refused(capi.ERR_STATE)            # the directions changed since
        # the scratch goes with the kept buffers
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        assert map_of(c, predelay, nbins, w).tobytes() == first.tobytes()
        c.keep_paths(False)
        assert "RVB_KEEP_LISTENER" in refused(capi.ERR_STATE)
        c.set_scene(small["scene"])
        assert "nothing traced" in refused(capi.ERR_STATE)            # the scene changed since
    finally:
        c.close()


def test_decay_sensitivity_map(small_ctx, small):
    """fitting.decay_sensitivity_map: the loss of decay_loss_and_grad bit for bit, the map of the direct call's bytes."""
    import torch
    from parallel_reverb_raytracer_amd import capi, fitting
    mic = small["mic"]
    start, goal = table_t(small["scene"][2], seed=11), table_t(small["scene"][2], seed=12)
    small_ctx.raytrace(mic, small["source"], scenes.sphere_directions(509, seed=23), 24, AIR_COEFFICIENTS)
    predelay, nbins = binning_of(small_ctx, mic, SPEAKERS, SR)
    small_ctx.reshade(goal, AIR_COEFFICIENTS)
    small_ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    small_ctx.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist)
    target = small_ctx.decay_curve_tensor(hist)
    small_ctx.synchronize()
    mask_host = decay_reference.mask_of(target.cpu().numpy().reshape(16, nbins))
    assert mask_host.any(axis=1).all(), "a row of the target never falls by 35 dB"
    mask = torch.from_numpy(mask_host.reshape(2, 8, nbins)).cuda()
    args = (AIR_COEFFICIENTS, mic, SPEAKERS, target, mask, SR, predelay, nbins)
    loss = fitting.decay_loss_and_grad(small_ctx, start, *args)[0]
    map_loss, per_triangle_map = fitting.decay_sensitivity_map(small_ctx, start, *args)
    assert map_loss == loss and loss > 0
    assert per_triangle_map.dtype == SURFACE and per_triangle_map.shape == (816,)
    assert per_triangle_map["specular"].any() and per_triangle_map["diffuse"].any()
    # the direct call with the weights of the same evaluation
    small_ctx.reshade(start, AIR_COEFFICIENTS)
    small_ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    hist.zero_()
    small_ctx.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist)
    curve = small_ctx.decay_curve_tensor(hist)
    w = torch.empty_like(hist)
    small_ctx.decay_loss_tensor(hist, curve, target, mask, capi.DECAY_NORMALISED, w)
    assert as_surfaces(map_of(small_ctx, predelay, nbins, w)).tobytes() == per_triangle_map.tobytes()
