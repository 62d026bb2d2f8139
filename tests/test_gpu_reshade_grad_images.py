"""The image-source part of the material gradient (rvb_reshade_grad_images of include/rvb_capi_images.h, csrc/image_grad_kernels.hip)
on the constructed room of tests/image_edges.py.

The reference gradient is binary64 numpy, in the manner of tests/test_gpu_reshade_grad.py, built from things other tests pin bit for
bit: the merge is redone here in Python from get_image_candidates (and must give get_raw_images byte for byte), which names the
(ray, slot) of every image; n[i][s], how often surface s stands in image i's chain, is read off CPU-oracle traces with air 0, the
all-ones table and probe tables of powers of two; term[i][b] = sum_c w[c][b][bin_i] * attenuate_speaker(images).volume[i][b].  An
image's term is homogeneous in the coefficients, so
    ref_spec[s][b] = sum_i term n / specular[s][b],   ref_air[b] = sum_i term * (time / SECONDS_PER_METER) * ln((float) M_E),
and A is the same sums over |term|.  The bar, derived and not measured:  |gpu - ref| <= 4 (9 + 16) 2^-24 A + 1e-30  entry by entry — the
bar of tests/test_gpu_reshade_grad.py with the chain length bounded by 9.
Largest observed |gpu - ref| / bound per case: profiles/early_fit_n1.txt (printed by every comparison)."""
import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, IMPULSE, NUM_IMAGE_SOURCE, aligned_copy

from test_gpu_reshade import AIR_B, SPEAKERS
from test_gpu_reshade_grad import LN_E, SECONDS_PER_METER, bins_of, exponent_of, on_device, table_t, weights
from test_gpu_source_pattern import FACING, SHAPES
from test_gpu_source_table import ORIENT, SPREAD

pytestmark = pytest.mark.gpu

SR = 44100.0
SCALE = 4.0 * (9 + 16) * 2.0 ** -24
PROBE = 8          # surfaces per probe trace: band j counts the steps on surface 8 p + j


def python_merge(cand, have_direct, remove_direct):
    """The merge rule of rvb_merge_images (reference rayverb.cpp:654-676) on candidates sorted by (ray, slot): per output impulse the
    position in `cand`, -1 for the direct slot."""
    tally = {}
    if have_direct:
        tally[(0,)] = -1
    i = 0
    while i < cand.shape[0]:
        j = i
        row = [0] * NUM_IMAGE_SOURCE
        while j < cand.shape[0] and cand["ray"][j] == cand["ray"][i]:
            row[int(cand["slot"][j])] = int(cand["index"][j])
            j += 1
        for c in range(i, j):
            tally.setdefault(tuple(row[:int(cand["slot"][c]) + 1]), c)
        i = j
    if remove_direct:
        tally.pop((0,), None)
    return np.array([tally[k] for k in sorted(tally)], np.int64)


_counts = {}


def chain_counts(oracle, scene, mic, src, shape):
    """n [nrays][NUM_IMAGE_SOURCE][nsurfaces]: for the oracle's image (ray, slot) the number of chain steps on every surface (zeros where
    the oracle has no image).  Computed once per key and never changed."""
    mic, src = tuple(float(x) for x in mic), tuple(float(x) for x in src)
    key = (mic, src, shape, scene[0].shape[0])
    if key in _counts:
        return _counts[key]
    nrays, nrefl = shape
    dirs = E.directions(nrays)
    nsurf = scene[2].shape[0]
    zero_air = np.zeros(8, np.float32)
    ones = aligned_copy(scene[2])
    ones["specular"], ones["diffuse"] = 1.0, 1.0
    _, image, index = oracle.raytrace((scene[0], scene[1], ones), mic, src, dirs, nrefl, zero_air)
    base = image["volume"].astype(np.float64).reshape(nrays, NUM_IMAGE_SOURCE, 8)
    have = index.reshape(nrays, NUM_IMAGE_SOURCE) != 0
    have[:, 0] = False
    assert (base[have] != 0).all() and (np.abs(base[have]) == np.abs(base[have][:, :1])).all()
    n = np.zeros((nrays, NUM_IMAGE_SOURCE, nsurf), np.float64)
    for p in range((nsurf + PROBE - 1) // PROBE):
        probe = aligned_copy(ones)
        for j in range(min(PROBE, nsurf - PROBE * p)):
            probe["specular"][PROBE * p + j][j] = 2.0
        vol = oracle.raytrace((scene[0], scene[1], probe), mic, src, dirs, nrefl, zero_air)[1]["volume"].astype(np.float64).reshape(nrays, NUM_IMAGE_SOURCE, 8)
        e = exponent_of(vol[have] / base[have])          # asserts that every ratio is an exact power of two
        for j in range(min(PROBE, nsurf - PROBE * p)):
            n[have, PROBE * p + j] = e[:, j]
    assert (n >= 0).all()
    _counts[key] = n
    return n


def image_list(ctx, remove_direct, pair=None):
    """(images, ray, slot) of the selected pair's merged list from the candidates alone; the impulses equal the host merge byte for
    byte.  ray is relative to the pair; slot 0 marks the direct impulse."""
    from parallel_reverb_raytracer_amd import capi
    cand = ctx.get_image_candidates()
    cand = ctx.get_pair_candidates(0 if pair is None else pair, cand)
    direct = ctx.get_direct()
    order = python_merge(cand, True, remove_direct)
    images = np.zeros(order.shape[0], IMPULSE)
    images[order >= 0] = cand["impulse"][order[order >= 0]]
    images[order < 0] = direct[0]
    assert images.tobytes() == capi.merge_images(cand, direct, remove_direct).tobytes(), "the Python merge is not the library's"
    ray = np.where(order >= 0, cand["ray"][np.maximum(order, 0)].astype(np.int64), 0)
    slot = np.where(order >= 0, cand["slot"][np.maximum(order, 0)].astype(np.int64), 0)
    return images, ray, slot


def terms_of(ctx, mic, speakers, images, predelay, nbins, w):
    """term[i][b], |term|[i][b] in binary64, the images' bins, and the attenuated channels"""
    term, absterm, atts = np.zeros((images.shape[0], 8)), np.zeros((images.shape[0], 8)), []
    for c, (direction, coefficient) in enumerate(zip(*speakers)):
        att = ctx.attenuate_speaker(mic, images, direction, coefficient)
        bins = bins_of(att["time"], predelay, SR)
        inside = bins < nbins
        t = w[c][:, np.minimum(bins, nbins - 1)].T.astype(np.float64) * att["volume"].astype(np.float64) * inside[:, None]
        term += t
        absterm += np.abs(t)
        atts.append(att)
    return term, absterm, bins_of(images["time"], predelay, SR), atts


def reference(term, absterm, images, n, table):
    spec = table["specular"].astype(np.float64)
    dist = images["time"].astype(np.float64) / float(SECONDS_PER_METER)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = {"spec": (n.T @ term) / spec, "air": (term * dist[:, None]).sum(axis=0) * LN_E}
        a = {"spec": (n.T @ absterm) / np.abs(spec), "air": (absterm * dist[:, None]).sum(axis=0) * LN_E}
    live = absterm.any(axis=1)
    return {"ref": ref, "a": a, "touched": (n[live] > 0).any(axis=0), "live": live}


def bound_of(r, what):
    return SCALE * r["a"][what] + 1e-30


def assert_ground(r, specular=True, dead_band=None):
    """On the reference alone: at least three quarters of the touched entries, and three quarters of the air's, stand 100 bars clear of
    zero — each fraction on its own."""
    t = r["touched"]
    assert (r["a"]["air"] > 0).all()
    air_clear = np.abs(r["ref"]["air"]) >= 100.0 * bound_of(r, "air")
    assert air_clear.mean() >= 0.75, air_clear.mean()
    if specular:
        bands = np.arange(8) != (-1 if dead_band is None else dead_band)
        assert t.any() and (r["a"]["spec"][t][:, bands] > 0).all()
        clear = (np.abs(r["ref"]["spec"][t]) >= 100.0 * bound_of(r, "spec")[t]).ravel()
        assert clear.mean() >= 0.75, clear.mean()


def assert_gradient(got, r, label):
    grads, grad_air = got
    worst = 0.0
    for what, g in (("spec", grads["specular"]), ("air", grad_air)):
        err, bound = np.abs(g.astype(np.float64) - r["ref"][what]), bound_of(r, what)
        worst = max(worst, float((err / bound).max()))
    print("reshade_grad_images %-52s max |gpu - ref| / bound = %.4f" % (label, worst))
    for what, g in (("spec", grads["specular"]), ("air", grad_air)):
        assert (np.abs(g.astype(np.float64) - r["ref"][what]) <= bound_of(r, what)).all(), (label, what)
    assert grads["diffuse"].tobytes() == bytes(grads["diffuse"].nbytes), label + ": a diffuse entry is not +0.0"
    # a surface on no live image's chain gets exactly 0
    assert not grads["specular"][~r["touched"]].any(), label


def binning_of(ctx, mic, speakers, remove_direct=False):
    """The image list's own predelay and bin count"""
    from parallel_reverb_raytracer_amd import capi
    ctx.ir_configure_speakers_merged(mic, speakers[0], speakers[1], capi.IR_IMAGES, remove_direct)
    lo, hi = ctx.ir_time_range()
    return lo, ctx.ir_bins(hi, lo, SR)


def compare(ctx, oracle, scene, pair_geometry, shape, table, label, remove_direct=False, speakers=SPEAKERS, predelay=None, nbins=None, seed=5,
            pair=None, specular=True, ground=True):
    """Configures the merged list, takes the gradient of seeded normal weights under IR_IMAGES and IR_ALL (the same bytes, twice) and
    holds it against the reference of the current candidates."""
    from parallel_reverb_raytracer_amd import capi
    mic, src = pair_geometry
    mic = tuple(float(x) for x in mic)
    lo, nb = binning_of(ctx, mic, speakers, remove_direct)
    predelay = lo if predelay is None else predelay
    nbins = nb if nbins is None else nbins
    images, ray, slot = image_list(ctx, remove_direct, pair)
    counts = chain_counts(oracle, scene, mic, src, shape)
    n = counts[ray, slot]
    n[slot == 0] = 0.0
    w = weights(len(speakers[1]), nbins, seed)
    term, absterm, bins, atts = terms_of(ctx, mic, speakers, images, predelay, nbins, w)
    r = reference(term, absterm, images, n, table)
    livecand = (slot > 0) & images["volume"].any(axis=1)
    assert (n[livecand].sum(axis=1) == slot[livecand] - 1).all(), label + ": a chain's length is not slot - 1"
    if ground:
        assert_ground(r, specular)
    w_dev = on_device(w)
    got = {}
    for which in (capi.IR_IMAGES, capi.IR_ALL):
        count = ctx.ir_configure_speakers_merged(mic, speakers[0], speakers[1], which, remove_direct)
        assert count == images.shape[0]
        got[which] = ctx.reshade_grad_images(predelay, SR, nbins, w_dev.data_ptr())
        again = ctx.reshade_grad_images(predelay, SR, nbins, w_dev.data_ptr())
        assert got[which][0].tobytes() == again[0].tobytes() and got[which][1].tobytes() == again[1].tobytes(), label + ": two calls differ"
    assert got[capi.IR_IMAGES][0].tobytes() == got[capi.IR_ALL][0].tobytes() and got[capi.IR_IMAGES][1].tobytes() == got[capi.IR_ALL][1].tobytes(), label
    assert_gradient(got[capi.IR_ALL], r, label)
    return {"got": got[capi.IR_ALL], "r": r, "w": w, "w_dev": w_dev, "predelay": predelay, "nbins": nbins, "bins": bins, "n": n, "slot": slot,
            "images": images, "term": term, "absterm": absterm, "atts": atts}


@pytest.fixture(scope="module")
def scene():
    return E.room()


@pytest.fixture(scope="module")
def ctx(scene):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(scene)
    c.keep_paths(True, listener=True)
    yield c
    c.close()


def traced(ctx, shape, pair=0):
    nrays, nrefl = shape
    ctx.raytrace(E.PAIRS[pair][0], E.PAIRS[pair][1], E.directions(nrays), nrefl, AIR_COEFFICIENTS)


@pytest.mark.parametrize("shape", [E.MAIN] + list(E.EDGE_SHAPES))
def test_gradient_equals_the_reference_after_a_trace_and_after_a_reshade(ctx, oracle, scene, shape):
    """509 x 12: 801 candidates, 161 images, every order 0 .. 9, chain multiplicities up to 4, all 14 surfaces touched.  64 x 1: orders 0
    and 1 only — every chain is empty, every specular entry exactly 0, the air is checked alone."""
    traced(ctx, shape)
    T = table_t(scene[2], seed=11)
    specular = shape[1] > 1
    for remove_direct in (False, True):
        a = compare(ctx, oracle, scene, E.PAIRS[0], shape, scene[2], "%dx%d after the trace, remove_direct %d" % (shape + (remove_direct,)),
                    remove_direct=remove_direct, specular=specular)
        if shape == E.MAIN:
            assert a["images"].shape[0] == 161 - remove_direct and set(a["slot"]) == set(range(remove_direct, 10))
            assert a["n"].max() == 4 and a["r"]["touched"].all()
        if not specular:
            assert not a["got"][0]["specular"].any() and a["slot"].max() == 1
    ctx.reshade(T, AIR_B)
    out = {}
    for remove_direct in (False, True):
        out[remove_direct] = compare(ctx, oracle, scene, E.PAIRS[0], shape, T, "%dx%d after reshade(T, AIR_B), remove_direct %d" % (shape + (remove_direct,)),
                                     remove_direct=remove_direct, specular=specular, predelay=out[False]["predelay"] if out else None,
                                     nbins=out[False]["nbins"] if out else None)
    # the air entry differs by exactly the direct term's reference (the specular entries not at all: the direct chain is empty)
    with_direct, without = out[False], out[True]
    assert with_direct["slot"][0] == 0 and with_direct["images"][0]["volume"].any()
    direct_air = with_direct["term"][0] * (float(with_direct["images"][0]["time"]) / float(SECONDS_PER_METER)) * LN_E
    assert np.abs(direct_air).min() > 0
    difference = with_direct["got"][1].astype(np.float64) - without["got"][1].astype(np.float64)
    assert (np.abs(difference - direct_air) <= bound_of(with_direct["r"], "air") + bound_of(without["r"], "air")).all()
    assert with_direct["got"][0].tobytes() == without["got"][0].tobytes()


@pytest.mark.parametrize("nchannels", [1, 3, 8])
def test_channel_counts(ctx, oracle, scene, nchannels):
    rng = np.random.default_rng(100 + nchannels)
    speakers = ([tuple(v) for v in rng.standard_normal((nchannels, 3))], [float(c) for c in rng.uniform(0.2, 0.8, nchannels)])
    traced(ctx, E.MAIN)
    T = table_t(scene[2], seed=11)
    ctx.reshade(T, AIR_B)
    compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "%d channel(s)" % nchannels, speakers=speakers)


def test_binning_edges(ctx, oracle, scene):
    """A predelay behind the first arrivals, so that several images clamp to bin 0, and half the bins, so that late images are skipped"""
    traced(ctx, E.MAIN)
    T = table_t(scene[2], seed=11)
    ctx.reshade(T, AIR_B)
    mic = E.PAIRS[0][0]
    lo, nb = binning_of(ctx, mic, SPEAKERS)
    images = ctx.get_raw_images(False)
    live = images["volume"].any(axis=1)
    predelay = float(max(np.float32(lo) + np.float32(5.0 / SR), np.sort(images["time"][live])[5]))
    nbins = nb // 2
    out = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "binning edges", predelay=predelay, nbins=nbins)
    clamped = live & (images["time"] <= np.float32(predelay))
    assert clamped.sum() >= 3 and (out["bins"][clamped] == 0).all(), "no image clamps to bin 0"
    assert (live & (out["bins"] >= nbins)).sum() >= 3 and (live & (out["bins"] < nbins)).sum() >= 3, "no late image is skipped"
    assert not out["absterm"][out["bins"] >= nbins].any()


def test_pair_1_of_three_has_a_hidden_direct_path(ctx, oracle, scene):
    nrays, nrefl = E.MAIN
    ctx.set_directions(E.directions(nrays))
    try:
        ctx.trace_pairs(E.MICS, E.SOURCES, nrefl, AIR_COEFFICIENTS)
        T = table_t(scene[2], seed=11)
        ctx.reshade(T, AIR_B)
        ctx.select_pair(1)
        out = compare(ctx, oracle, scene, E.PAIRS[1], E.MAIN, T, "pair 1 of 3", pair=1)
        assert out["slot"][0] == 0 and not out["images"][0]["volume"].any() and not out["absterm"][0].any(), "the direct path of pair 1 is not hidden"
        ctx.select_pair(0)
        other = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "pair 0 of 3", pair=0)
        assert other["got"][0].tobytes() != out["got"][0].tobytes()
    finally:
        ctx.npairs = 1


def test_after_a_relisten(ctx, oracle, scene):
    traced(ctx, E.MAIN)
    T = table_t(scene[2], seed=12)
    ctx.reshade(T, AIR_B)
    before = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "before the relisten")
    mic1 = tuple(float(x) for x in E.MICS[1])
    ctx.relisten(mic1)
    after = compare(ctx, oracle, scene, (mic1, E.PAIRS[0][1]), E.MAIN, T, "after relisten to MICS[1]")
    assert after["got"][0].tobytes() != before["got"][0].tobytes()


def test_a_source_pattern(ctx, oracle, scene):
    ctx.set_source_pattern(FACING, SHAPES)
    try:
        traced(ctx, E.MAIN)
        compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, scene[2], "source pattern after the trace")
        T = table_t(scene[2], seed=11)
        ctx.reshade(T, AIR_B)
        scaled = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "source pattern after reshade")
    finally:
        ctx.set_source_pattern(None)
    traced(ctx, E.MAIN)
    ctx.reshade(T, AIR_B)
    plain = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "no source pattern", predelay=scaled["predelay"], nbins=scaled["nbins"])
    assert (plain["got"][0]["specular"][:, 1:] != scaled["got"][0]["specular"][:, 1:]).any()          # (band 0 has shape 0: gain exactly 1)


def test_a_source_table(ctx, oracle, scene):
    ctx.set_source_table(SPREAD, ORIENT[0], ORIENT[1])
    try:
        traced(ctx, E.MAIN)
        compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, scene[2], "source table after the trace")
        T = table_t(scene[2], seed=11)
        ctx.reshade(T, AIR_B)
        scaled = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "source table after reshade")
    finally:
        ctx.set_source_table(None)
    traced(ctx, E.MAIN)
    ctx.reshade(T, AIR_B)
    plain = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "no source table", predelay=scaled["predelay"], nbins=scaled["nbins"])
    assert (plain["got"][0]["specular"] != scaled["got"][0]["specular"]).any()


def lone_surface(n):
    """A surface that any image meets at most once, and at least three images meet"""
    ok = [s for s in range(n.shape[1]) if n[:, s].max() == 1 and (n[:, s] == 1).sum() >= 3]
    assert ok, "no surface is met at most once by any image and by three images"
    return ok[0]


def test_a_zero_coefficient_gets_its_derivative_without_a_division(ctx, oracle, scene):
    """specular[s][3] = 0 for a surface s that any image meets at most once: L is linear in that coefficient, so its derivative at 0 is
    the sum of the terms of the images that meet s, taken with the entry at 1.0; every other band-3 entry sees only images without s,
    which the zero volumes of the state under test say by themselves."""
    from parallel_reverb_raytracer_amd import capi
    traced(ctx, E.MAIN)
    mic = E.PAIRS[0][0]
    T = table_t(scene[2], seed=11)
    ctx.reshade(T, AIR_B)
    first = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, T, "before the zero")
    n, predelay, nbins, w = first["n"], first["predelay"], first["nbins"], first["w"]
    s = lone_surface(n)
    zeros, unit = aligned_copy(T), aligned_copy(T)
    zeros["specular"][s][3], unit["specular"][s][3] = 0.0, 1.0
    ctx.reshade(unit, AIR_B)
    ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_IMAGES, False)
    images1, _, _ = image_list(ctx, False)
    term1, abs1, _, _ = terms_of(ctx, mic, SPEAKERS, images1, predelay, nbins, w)
    once = n[:, s] == 1
    ctx.reshade(zeros, AIR_B)
    ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_IMAGES, False)
    images0, _, _ = image_list(ctx, False)
    term0, abs0, _, _ = terms_of(ctx, mic, SPEAKERS, images0, predelay, nbins, w)
    assert not term0[once, 3].any() and abs1[once, 3].all()
    r = reference(term0, abs0, images0, n, zeros)
    r["ref"]["spec"][s][3], r["a"]["spec"][s][3] = term1[once, 3].sum(), abs1[once, 3].sum()
    assert all(np.isfinite(r["ref"][k]).all() and np.isfinite(r["a"][k]).all() for k in ("spec", "air"))
    assert_ground(r, dead_band=3)
    assert abs(r["ref"]["spec"][s][3]) >= 100 * bound_of(r, "spec")[s][3]
    assert_gradient(ctx.reshade_grad_images(predelay, SR, nbins, first["w_dev"].data_ptr()), r, "zero coefficient, specular[%d][3] = 0" % s)


def test_linearity_in_a_specular_coefficient_through_the_real_binning(ctx, oracle, scene):
    """L is linear in specular[s][b] for a surface that any image meets at most once: L(0.9) - L(0.3) = 0.6 dL/dspecular[s][b], with L from
    rvb_ir_accumulate(RVB_IR_EXACT) after ir_configure_speakers_merged(IR_IMAGES) in binary64.  Allowed: 0.6 x the gradient's bar, and per
    histogram the re-ordering term of tests/test_gpu_reshade_grad.py, sum |w| n_bin 2^-23 absum_bin."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    traced(ctx, E.MAIN)
    mic, b = E.PAIRS[0][0], 2
    T = table_t(scene[2], seed=11)
    results = []
    predelay = nbins = s = None
    for value in (0.3, 0.9):
        table = aligned_copy(T)
        if s is not None:
            table["specular"][s][b] = value
        ctx.reshade(table, AIR_B)
        out = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, table, "linearity, specular = %g" % value, predelay=predelay, nbins=nbins)
        if s is None:
            s = lone_surface(out["n"])
            table["specular"][s][b] = value
            ctx.reshade(table, AIR_B)
            out = compare(ctx, oracle, scene, E.PAIRS[0], E.MAIN, table, "linearity, specular[%d][%d] = %g" % (s, b, value))
        predelay, nbins = out["predelay"], out["nbins"]
        ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_IMAGES, False)
        hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
        ctx.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist)
        ctx.synchronize()
        h = hist.cpu().numpy().astype(np.float64)
        w = out["w"].astype(np.float64)
        reorder = 0.0
        for c, att in enumerate(out["atts"]):
            bins = bins_of(att["time"], predelay, SR)
            inside = bins < nbins
            count = np.bincount(bins[inside], minlength=nbins).astype(np.float64)
            for band in range(8):
                absum = np.bincount(bins[inside], weights=np.abs(att["volume"][inside, band].astype(np.float64)), minlength=nbins)
                reorder += float((np.abs(w[c][band]) * count * 2.0 ** -23 * absum).sum())
        results.append({"L": float((w * h).sum()), "grad": float(out["got"][0]["specular"][s][b]), "bound": float(bound_of(out["r"], "spec")[s][b]),
                        "reorder": reorder, "ref": float(out["r"]["ref"]["spec"][s][b])})
    lo, hi = results
    assert abs(lo["ref"]) >= 100 * lo["bound"]
    assert abs(lo["grad"] - hi["grad"]) <= lo["bound"] + hi["bound"]
    allowed = 0.6 * lo["bound"] + lo["reorder"] + hi["reorder"]
    miss = abs(hi["L"] - lo["L"] - 0.6 * lo["grad"])
    print("reshade_grad_images linearity: |L(0.9) - L(0.3) - 0.6 grad| / allowed = %.4f (0.6 grad = %.6g)" % (miss / allowed, 0.6 * lo["grad"]))
    assert miss <= allowed
    assert abs(0.6 * lo["grad"]) >= 10 * allowed, "the difference under test drowns in its bound"


def snapshot(ctx):
    return (ctx.get_raw_diffuse().tobytes(), ctx.get_direct().tobytes(), ctx.get_image_candidates().tobytes(), ctx.ir_time_range())


def test_side_effects_states_and_arguments(scene):
    import ctypes
    import torch
    from parallel_reverb_raytracer_amd import capi, scenes
    nrays, nrefl = E.MAIN
    mic, src = E.PAIRS[0]
    dirs = E.directions(nrays)
    w_dev = on_device(weights(2, 4096, 9))

    def refused(c, code, nbins=4096, rate=SR, predelay=0.0, pointer=w_dev.data_ptr()):
        with pytest.raises(capi.RvbError) as e:
            c.reshade_grad_images(predelay, rate, nbins, pointer)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    c = capi.Context(0)
    try:
        c.set_scene(scene)
        assert "nothing traced" in refused(c, capi.ERR_STATE)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        assert "rvb_keep_paths" in refused(c, capi.ERR_STATE)         # the trace was made without keeping
        c.keep_paths(True, listener=True)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        assert "no IR configuration" in refused(c, capi.ERR_STATE)
        c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        lo, hi = c.ir_time_range()
        nbins = c.ir_bins(hi, lo, SR)
        before = snapshot(c)
        w = on_device(weights(2, nbins, 5))
        # a prepared exact list: what it folds before the calls ...
        want = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
        c.ir_exact_prepare(lo, SR, nbins)
        c.ir_exact_fold_tensor(nbins, 0, nbins, want)
        c.synchronize()
        first = c.reshade_grad_images(lo, SR, nbins, w.data_ptr())
        names = [k for k, _ in c.last_timings()]
        assert names == ["reshade_grad_images_kernel", "reshade_grad_images_reduce_kernel"]
        assert first[0]["specular"].any() and first[1].any()
        # every refusal that leaves the configuration in place, then: the state is as it was and the prepared list still folds
        refused(c, capi.ERR_INVALID, nbins=0)
        refused(c, capi.ERR_INVALID, nbins=2 ** 32)
        refused(c, capi.ERR_INVALID, rate=float("nan"))
        refused(c, capi.ERR_INVALID, predelay=float("inf"))
        refused(c, capi.ERR_INVALID, pointer=None)
        air = np.full(8, 7.0, np.float32)
        assert c.lib.rvb_reshade_grad_images(c.handle, 0.0, SR, 4096, w_dev.data_ptr(), None, air.ctypes.data_as(ctypes.c_void_p)) == capi.ERR_INVALID
        assert (air == 7.0).all()
        assert snapshot(c) == before
        folded = torch.zeros_like(want)
        c.ir_exact_fold_tensor(nbins, 0, nbins, folded)
        c.synchronize()
        assert torch.equal(folded, want) and bool(want.any())
        second = c.reshade_grad_images(lo, SR, nbins, w.data_ptr())
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        # configurations that the call does not take
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, c.get_raw_images(False))
        assert "lost its chains" in refused(c, capi.ERR_STATE)
        c.ir_configure_hrtf_merged(mic, scenes.hrtf_synthetic_table(), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), capi.IR_ALL, False)
        assert "HRTF" in refused(c, capi.ERR_STATE)
        c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, False)
        assert "RVB_IR_DIFFUSE" in refused(c, capi.ERR_STATE)
        nine = ([(np.cos(i), 0.0, np.sin(i)) for i in range(9)], [0.5] * 9)
        c.ir_configure_speakers_merged(mic, nine[0], nine[1], capi.IR_ALL, False)
        assert "9 speaker" in refused(c, capi.ERR_STATE)
        c.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        assert snapshot(c) == before                                 # refused calls leave the results as they were
        c.reshade(None, AIR_COEFFICIENTS)
        assert "no IR configuration" in refused(c, capi.ERR_STATE)   # a re-shade voids the configuration: configure again
        c.set_directions(dirs)
        assert "nothing traced" in refused(c, capi.ERR_STATE)
    finally:
        c.close()
