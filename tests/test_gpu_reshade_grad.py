"""Material gradients of a weighted impulse response from a kept trace (rvb_reshade_grad, csrc/reshade_grad_kernels.hip).

The reference gradient is binary64 numpy, built from things other tests pin bit for bit: the records in the context (get_raw_diffuse), the
materialised speaker attenuation (attenuate_speaker), the binary32 time_bin formula, and per record the surface of its bounce and the
number of earlier bounces on every surface, read off CPU-oracle traces with power-of-two probe tables (chains).  A record's term
w * gain * volume is homogeneous in the coefficients, so
    ref_spec[s,b] = sum term * n_s / specular[s,b],  ref_diff[s,b] = sum_{s_i = s} term / diffuse[s,b],  ref_air[b] = sum term * dist * ln((float) M_E)
and A is the same three sums over |term|.  The bar, derived and not measured:  |gpu - ref| <= 4 (nreflections + 16) 2^-24 A + 1e-30  entry
by entry — a term passes at most nreflections chain roundings and at most 16 others (air, diffuse, DIFF, gain, weight, pattern, the
stored volume the reference starts from) on each side, and the in-ray binary32 recurrence adds as much again.
Largest observed |gpu - ref| / bound per case: profiles/reshade_grad_n1.txt (printed by every comparison)."""
import numpy as np
import pytest

from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS, aligned_copy

from test_gpu_reshade import AIR_B, SPEAKERS
from test_gpu_source_pattern import FACING, SHAPES

pytestmark = pytest.mark.gpu

SECONDS_PER_METER = np.float32(1.0 / 340.0)
LN_E = float(np.log(np.float64(np.float32(np.e))))
PROBE = 7          # surfaces per probe trace: bands 0..6 count their bounces, band 7 names the record's own surface


def table_t(surfaces, seed=11):
    """Another table for the same scene: every coefficient uniform in [0.3, 0.9], no zeros."""
    rng = np.random.default_rng(seed)
    t = aligned_copy(surfaces)
    t["specular"] = rng.uniform(0.3, 0.9, t["specular"].shape).astype(np.float32)
    t["diffuse"] = rng.uniform(0.3, 0.9, t["diffuse"].shape).astype(np.float32)
    return t


def weights(nchannels, nbins, seed):
    return np.random.default_rng(seed).standard_normal((nchannels, 8, nbins)).astype(np.float32)


def on_device(w):
    import torch
    t = torch.from_numpy(w).cuda().contiguous()
    torch.cuda.synchronize()
    return t


def bins_of(time, predelay, sr):
    """time_bin of csrc/attenuation.h in binary32: the predelay clamp, the product, roundf (half away from zero)."""
    time = np.asarray(time, np.float32)
    t = np.where(time > np.float32(predelay), time - np.float32(predelay), np.float32(0.0)).astype(np.float32)
    x = (t * np.float32(sr)).astype(np.float32)
    return np.floor(x.astype(np.float64) + 0.5).astype(np.int64)


def exponent_of(ratio):
    m, e = np.frexp(ratio)
    assert (m == 0.5).all(), "a probe ratio is not a power of two"
    return e - 1


_chains = {}


def chains(oracle, key, scene, mic, src, dirs, nrefl):
    """(n [records][nsurfaces], s [records]): per record of the oracle's trace the number of bounces <= its own on every surface and the
    surface of its own bounce (-1 and zeros for a record without volume: escaped or invisible).  From traces with air 0 and tables of
    powers of two — specular 2 in band j for surface 7 p + j, diffuse 2^(j + 1) — against the all-ones table: the ratios are exact."""
    if key in _chains:
        return _chains[key]
    assert nrefl <= 70
    nsurf = scene[2].shape[0]
    zero_air = np.zeros(8, np.float32)
    ones = aligned_copy(scene[2])
    ones["specular"], ones["diffuse"] = 1.0, 1.0
    base = oracle.raytrace((scene[0], scene[1], ones), mic, src, dirs, nrefl, zero_air)[0]["volume"].astype(np.float64)
    live = base[:, 0] != 0
    assert (np.abs(base) == np.abs(base[:, :1])).all()
    n = np.zeros((base.shape[0], nsurf), np.float64)
    own = np.full(base.shape[0], -1, np.int64)
    for p in range((nsurf + PROBE - 1) // PROBE):
        probe = aligned_copy(ones)
        for j in range(min(PROBE, nsurf - PROBE * p)):
            probe["specular"][PROBE * p + j][j] = 2.0
            probe["diffuse"][PROBE * p + j][:] = 2.0 ** (j + 1)
        vol = oracle.raytrace((scene[0], scene[1], probe), mic, src, dirs, nrefl, zero_air)[0]["volume"].astype(np.float64)
        e = exponent_of(vol[live] / base[live])
        mine = e[:, 7] > 0
        own[np.flatnonzero(live)[mine]] = PROBE * p + e[mine, 7] - 1
        for j in range(min(PROBE, nsurf - PROBE * p)):
            n[live, PROBE * p + j] = e[:, j] - e[:, 7]
    assert (own[live] >= 0).all() and (n >= 0).all() and (n[live, own[live]] >= 1).all()
    _chains[key] = (n, own)
    return _chains[key]


def state_terms(ctx, mic, speakers, predelay, sr, nbins, w, records=None):
    """term[i][b] = sum_c w[c][b][bin_i] * att_c.volume[i][b] in binary64 (0 where bin_i >= nbins), the same over absolute values, the
    records' distances and bins, and the attenuated channels."""
    r = ctx.get_raw_diffuse() if records is None else records
    term, absterm, atts = np.zeros((r.shape[0], 8)), np.zeros((r.shape[0], 8)), []
    for c, (direction, coefficient) in enumerate(zip(*speakers)):
        att = ctx.attenuate_speaker(mic, r, direction, coefficient)
        bins = bins_of(att["time"], predelay, sr)
        inside = bins < nbins
        t = w[c][:, np.minimum(bins, nbins - 1)].T.astype(np.float64) * att["volume"].astype(np.float64) * inside[:, None]
        term += t
        absterm += np.abs(t)
        atts.append(att)
    bins = bins_of(r["time"], predelay, sr)
    dist = r["time"].astype(np.float64) / float(SECONDS_PER_METER)
    return term, absterm, dist, bins, atts


def reference(term, absterm, dist, chain, table, nrefl):
    n, own = chain
    onehot = (own[:, None] == np.arange(table.shape[0])[None, :]).astype(np.float64)
    spec, diff = table["specular"].astype(np.float64), table["diffuse"].astype(np.float64)
    scale = 4.0 * (nrefl + 16) * 2.0 ** -24
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = {"spec": (n.T @ term) / spec, "diff": (onehot.T @ term) / diff, "air": (term * dist[:, None]).sum(axis=0) * LN_E}
        a = {"spec": (n.T @ absterm) / np.abs(spec), "diff": (onehot.T @ absterm) / np.abs(diff), "air": (absterm * dist[:, None]).sum(axis=0) * LN_E}
    live = absterm.any(axis=1)
    touched = (n[live] > 0).any(axis=0)
    return {"ref": ref, "a": a, "scale": scale, "touched": touched}


def bound_of(r, what):
    return r["scale"] * r["a"][what] + 1e-30


def assert_ground(r, dead_band=None):
    """On the reference alone: every touched surface has A > 0, and at least three quarters of their entries (and of the air's) stand
    100 bounds clear of zero — a gradient of rounding noise would pass nothing.  dead_band: the band whose chains a zero coefficient
    ends; a surface met only behind it has A = 0 there, and the gradient must then be exactly 0 (bound 1e-30)."""
    t = r["touched"]
    assert t.any()
    bands = np.arange(8) != (-1 if dead_band is None else dead_band)
    assert (r["a"]["spec"][t][:, bands] > 0).all() and (r["a"]["diff"][t][:, bands] > 0).all() and (r["a"]["air"] > 0).all()
    clear = np.concatenate([(np.abs(r["ref"][k][t]) >= 100.0 * bound_of(r, k)[t]).ravel() for k in ("spec", "diff")]
                           + [np.abs(r["ref"]["air"]) >= 100.0 * bound_of(r, "air")])
    assert clear.mean() >= 0.75, clear.mean()


def assert_gradient(got, r, label):
    grads, grad_air = got
    worst = 0.0
    for what, g in (("spec", grads["specular"]), ("diff", grads["diffuse"]), ("air", grad_air)):
        err, bound = np.abs(g.astype(np.float64) - r["ref"][what]), bound_of(r, what)
        worst = max(worst, float((err / bound).max()))
    print("reshade_grad %-44s max |gpu - ref| / bound = %.4f" % (label, worst))
    for what, g in (("spec", grads["specular"]), ("diff", grads["diffuse"]), ("air", grad_air)):
        assert (np.abs(g.astype(np.float64) - r["ref"][what]) <= bound_of(r, what)).all(), (label, what)
    # a surface that no live record touches gets exactly 0
    assert not grads["specular"][~r["touched"]].any() and not grads["diffuse"][~r["touched"]].any(), label


def binning_of(ctx, mic, speakers, sr):
    """The workload's own predelay and bin count for the current records."""
    from parallel_reverb_raytracer_amd import capi
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    lo, hi = ctx.ir_time_range()
    return lo, ctx.ir_bins(hi, lo, sr)


def compare(ctx, chain, table, mic, nrefl, label, speakers=SPEAKERS, sr=44100.0, predelay=None, nbins=None, seed=5, records=None, ground=True):
    """Configures the speakers, takes the gradient of seeded normal weights and holds it against the reference of the current records."""
    from parallel_reverb_raytracer_amd import capi
    lo, nb = binning_of(ctx, mic, speakers, sr)
    predelay = lo if predelay is None else predelay
    nbins = nb if nbins is None else nbins
    w = weights(len(speakers[1]), nbins, seed)
    term, absterm, dist, bins, atts = state_terms(ctx, mic, speakers, predelay, sr, nbins, w, records)
    r = reference(term, absterm, dist, chain, table, nrefl)
    if ground:
        assert_ground(r)
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    w_dev = on_device(w)
    got = ctx.reshade_grad(predelay, sr, nbins, w_dev.data_ptr())
    assert_gradient(got, r, label)
    return {"got": got, "r": r, "w": w, "w_dev": w_dev, "predelay": predelay, "nbins": nbins, "bins": bins, "absterm": absterm, "atts": atts, "term": term}


@pytest.fixture(scope="module")
def cathedral():
    scene, info = scenes.cathedral(3000)
    assert scene[2].shape[0] == 7
    return {"scene": scene, "mic": info["mic"], "source": info["source"], "T": table_t(scene[2])}


@pytest.fixture(scope="module")
def ctx(cathedral):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(cathedral["scene"])
    c.keep_paths(True)
    yield c
    c.close()


def traced(ctx, oracle, cathedral, nrays, nrefl, seed=23):
    dirs = scenes.sphere_directions(nrays, seed=seed)
    chain = chains(oracle, ("cathedral", nrays, nrefl, seed), cathedral["scene"], cathedral["mic"], cathedral["source"], dirs, nrefl)
    ctx.raytrace(cathedral["mic"], cathedral["source"], dirs, nrefl, AIR_COEFFICIENTS)
    return chain, dirs


@pytest.mark.parametrize("nrays,nrefl", [(509, 24), (5, 70), (130, 64), (8, 33), (17, 32), (8, 1)])
def test_gradient_equals_the_reference_after_a_trace_and_after_a_reshade(ctx, oracle, cathedral, nrays, nrefl):
    """509 x 24: a partial last wave, several rays per wave, a ray of two tiles with a partial one; 5 x 70: a ray longer than a wave,
    fewer rays than a wave takes; 130 x 64: whole tiles, the 16-bit key runs of the trace.  The edges of a wave and of a tile: 8 x 33:
    exactly one wave's rays, a third tile that holds one bounce; 17 x 32: a last wave of one ray, exactly two tiles; 8 x 1: a single
    bounce."""
    chain, _ = traced(ctx, oracle, cathedral, nrays, nrefl)
    mic = cathedral["mic"]
    compare(ctx, chain, cathedral["scene"][2], mic, nrefl, "cathedral %dx%d after the trace" % (nrays, nrefl))
    ctx.reshade(cathedral["T"], AIR_B)
    compare(ctx, chain, cathedral["T"], mic, nrefl, "cathedral %dx%d after reshade(T, AIR_B)" % (nrays, nrefl))


@pytest.mark.parametrize("sr", [44100.0, 1000.0])
def test_binning_edges(ctx, oracle, cathedral, sr):
    """A predelay behind the first arrival — at the sixth live record's time and at least five samples late, so that several records
    clamp to bin 0 — and half the bins — late records are skipped."""
    chain, _ = traced(ctx, oracle, cathedral, 509, 24)
    ctx.reshade(cathedral["T"], AIR_B)
    lo, nb = binning_of(ctx, cathedral["mic"], SPEAKERS, sr)
    records = ctx.get_raw_diffuse()
    live = (records["volume"] != 0).any(axis=1)
    predelay = float(max(np.float32(lo) + np.float32(5.0 / sr), np.sort(records["time"][live])[5]))
    nbins = nb // 2
    out = compare(ctx, chain, cathedral["T"], cathedral["mic"], 24, "binning edges, %g Hz" % sr, sr=sr, predelay=predelay, nbins=nbins)
    clamped = live & (records["time"] <= np.float32(predelay))
    assert clamped.sum() >= 3 and (out["bins"][clamped] == 0).all(), "no record clamps to bin 0"
    assert (live & (out["bins"] >= nbins)).sum() >= 3 and (live & (out["bins"] < nbins)).sum() >= 3, "no late record is skipped"


@pytest.mark.parametrize("nchannels", [1, 3, 8])
def test_channel_counts(ctx, oracle, cathedral, nchannels):
    rng = np.random.default_rng(100 + nchannels)
    speakers = ([tuple(v) for v in rng.standard_normal((nchannels, 3))], [float(c) for c in rng.uniform(0.2, 0.8, nchannels)])
    chain, _ = traced(ctx, oracle, cathedral, 130, 24)
    ctx.reshade(cathedral["T"], AIR_B)
    compare(ctx, chain, cathedral["T"], cathedral["mic"], 24, "%d channel(s)" % nchannels, speakers=speakers)


def test_zero_coefficients_get_their_derivative_without_a_division(ctx, oracle, cathedral):
    """specular[s0][3] = 0 and diffuse[s1][5] = 0.  L is linear in the records that meet s0 once (in diffuse[s1][5]: whose own surface is
    s1), so the derivative at 0 is their sum of terms with the entry at 1.0; every other band-3 derivative sees only records with no
    bounce on s0, which the zero volumes of the state under test say by themselves."""
    s0, s1 = 2, 4
    chain, _ = traced(ctx, oracle, cathedral, 509, 24)
    n, own = chain
    mic, sr = cathedral["mic"], 44100.0
    zeros = aligned_copy(cathedral["T"])
    zeros["specular"][s0][3] = 0.0
    zeros["diffuse"][s1][5] = 0.0
    unit = aligned_copy(zeros)
    unit["specular"][s0][3] = 1.0
    unit["diffuse"][s1][5] = 1.0
    ctx.reshade(unit, AIR_B)
    predelay, nbins = binning_of(ctx, mic, SPEAKERS, sr)
    w = weights(2, nbins, 5)
    term1, abs1, _, _, _ = state_terms(ctx, mic, SPEAKERS, predelay, sr, nbins, w)
    once, mine = n[:, s0] == 1, own == s1
    assert once.sum() >= 10 and mine.sum() >= 10

    ctx.reshade(zeros, AIR_B)
    term0, abs0, dist, _, _ = state_terms(ctx, mic, SPEAKERS, predelay, sr, nbins, w)
    assert not term0[n[:, s0] > 0, 3].any() and not term0[mine, 5].any()
    r = reference(term0, abs0, dist, chain, zeros, 24)
    r["ref"]["spec"][s0][3], r["a"]["spec"][s0][3] = term1[once, 3].sum(), abs1[once, 3].sum()
    r["ref"]["diff"][s1][5], r["a"]["diff"][s1][5] = term1[mine, 5].sum(), abs1[mine, 5].sum()
    assert all(np.isfinite(r["ref"][k]).all() and np.isfinite(r["a"][k]).all() for k in ("spec", "diff", "air"))
    assert_ground(r, dead_band=3)
    assert abs(r["ref"]["spec"][s0][3]) >= 100 * bound_of(r, "spec")[s0][3] and abs(r["ref"]["diff"][s1][5]) >= 100 * bound_of(r, "diff")[s1][5]
    from parallel_reverb_raytracer_amd import capi
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    w_dev = on_device(w)
    assert_gradient(ctx.reshade_grad(predelay, sr, nbins, w_dev.data_ptr()), r, "zero coefficients")


def test_escapes_and_a_surface_on_no_triangle(oracle):
    """scenes.shoebox() without its last two triangles, as tests/test_gpu_reshade.py opens it: rays leave the room, the slots behind an
    escape add nothing, and surface 0 (the default, on no triangle) gets exactly 0.0 in all 16 entries."""
    from parallel_reverb_raytracer_amd import capi
    triangles, vertices, surfaces = scenes.shoebox()
    scene = (aligned_copy(triangles[:-2]), vertices, surfaces)
    mic, src, nrays, nrefl = (0.5, 1.0, 2.0), (-0.7, -1.2, -5.0), 130, 24
    dirs = scenes.sphere_directions(nrays, seed=3)
    chain = chains(oracle, ("open shoebox", nrays, nrefl), scene, mic, src, dirs, nrefl)
    escaped = (chain[1] < 0).reshape(nrays, nrefl)
    assert escaped[:, -1].sum() >= 10 and not escaped[:, -1].all() and not escaped[:, 0].all()
    table = table_t(surfaces, seed=12)
    c = capi.Context(0)
    try:
        c.set_scene(scene)
        c.keep_paths(True)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        for label, tab in (("open shoebox after the trace", surfaces), ("open shoebox after reshade", table)):
            if tab is table:
                c.reshade(table, AIR_B)
            out = compare(c, chain, tab, mic, nrefl, label)
            grads = out["got"][0]
            assert not out["r"]["touched"][0] and out["r"]["touched"][1]
            assert (grads["specular"][0] == 0.0).all() and (grads["diffuse"][0] == 0.0).all()
    finally:
        c.close()


def test_the_selected_pair(ctx, oracle, cathedral):
    mics = np.array([cathedral["mic"], (0.0, 12.0, 11.0)], np.float32)
    sources = np.array([cathedral["source"], (0.0, 12.5, 11.5)], np.float32)
    nrays, nrefl = 130, 24
    dirs = scenes.sphere_directions(nrays, seed=5)
    chain = chains(oracle, ("cathedral pair 1", nrays, nrefl), cathedral["scene"], tuple(mics[1]), tuple(sources[1]), dirs, nrefl)
    ctx.set_directions(dirs)
    try:
        ctx.trace_pairs(mics, sources, nrefl, AIR_COEFFICIENTS)
        ctx.reshade(cathedral["T"], AIR_B)
        ctx.select_pair(1)
        records = ctx.get_raw_diffuse().reshape(2, -1)[1]
        out = compare(ctx, chain, cathedral["T"], tuple(mics[1]), nrefl, "pair 1 of 2", records=records)
        ctx.select_pair(0)
        from parallel_reverb_raytracer_amd import capi
        ctx.ir_configure_speakers(tuple(mics[0]), SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        other = ctx.reshade_grad(out["predelay"], 44100.0, out["nbins"], out["w_dev"].data_ptr())
        assert (other[0]["specular"] != out["got"][0]["specular"]).any() and (other[1] != out["got"][1]).all()
    finally:
        ctx.npairs = 1


def test_a_source_pattern_is_a_factor_of_every_term_of_its_ray(ctx, oracle, cathedral):
    nrays, nrefl = 130, 24
    mic = cathedral["mic"]
    ctx.set_source_pattern(FACING, SHAPES)
    try:
        chain, _ = traced(ctx, oracle, cathedral, nrays, nrefl)
        compare(ctx, chain, cathedral["scene"][2], mic, nrefl, "source pattern after the trace")
        ctx.reshade(cathedral["T"], AIR_B)
        scaled = compare(ctx, chain, cathedral["T"], mic, nrefl, "source pattern after reshade")
    finally:
        ctx.set_source_pattern(None)
    # the records of the context still carry the pattern although it has been switched off for the traces that follow
    from parallel_reverb_raytracer_amd import capi
    again = ctx.reshade_grad(scaled["predelay"], 44100.0, scaled["nbins"], scaled["w_dev"].data_ptr())
    assert again[0].tobytes() == scaled["got"][0].tobytes() and again[1].tobytes() == scaled["got"][1].tobytes()
    traced(ctx, oracle, cathedral, nrays, nrefl)
    ctx.reshade(cathedral["T"], AIR_B)
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    plain = ctx.reshade_grad(scaled["predelay"], 44100.0, scaled["nbins"], scaled["w_dev"].data_ptr())
    assert (plain[0]["diffuse"][1:, 1:] != scaled["got"][0]["diffuse"][1:, 1:]).any()          # (band 0 has shape 0: gain exactly 1)


def test_linearity_in_a_diffuse_coefficient_through_the_real_binning(ctx, oracle, cathedral):
    """L is linear in diffuse[s][b]: L(0.8) - L(0.2) = 0.6 dL/ddiffuse[s][b], with L from rvb_ir_accumulate(RVB_IR_EXACT) in binary64.
    Allowed: 0.6 x the gradient's bound, and per histogram fast_bound's re-ordering term sum |w| n_bin 2^-23 absum_bin."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    s, b, sr, nrefl = 3, 2, 44100.0, 24
    chain, _ = traced(ctx, oracle, cathedral, 509, nrefl)
    mic = cathedral["mic"]
    results = []
    predelay = nbins = None
    for value in (0.2, 0.8):
        table = aligned_copy(cathedral["T"])
        table["diffuse"][s][b] = value
        ctx.reshade(table, AIR_B)
        out = compare(ctx, chain, table, mic, nrefl, "linearity, diffuse[%d][%d] = %g" % (s, b, value), predelay=predelay, nbins=nbins)
        predelay, nbins = out["predelay"], out["nbins"]
        hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
        ctx.ir_accumulate_tensor(predelay, sr, nbins, capi.IR_EXACT, hist)
        ctx.synchronize()
        h = hist.cpu().numpy().astype(np.float64)
        w = out["w"].astype(np.float64)
        reorder = 0.0
        for c, att in enumerate(out["atts"]):
            bins = bins_of(att["time"], predelay, sr)
            inside = bins < nbins
            count = np.bincount(bins[inside], minlength=nbins).astype(np.float64)
            for band in range(8):
                absum = np.bincount(bins[inside], weights=np.abs(att["volume"][inside, band].astype(np.float64)), minlength=nbins)
                reorder += float((np.abs(w[c][band]) * count * 2.0 ** -23 * absum).sum())
        results.append({"L": float((w * h).sum()), "grad": float(out["got"][0]["diffuse"][s][b]), "bound": float(bound_of(out["r"], "diff")[s][b]),
                        "reorder": reorder, "ref": float(out["r"]["ref"]["diff"][s][b])})
    lo, hi = results
    assert abs(lo["ref"]) >= 100 * lo["bound"]
    assert abs(lo["grad"] - hi["grad"]) <= lo["bound"] + hi["bound"]
    allowed = 0.6 * lo["bound"] + lo["reorder"] + hi["reorder"]
    miss = abs(hi["L"] - lo["L"] - 0.6 * lo["grad"])
    print("reshade_grad linearity: |L(0.8) - L(0.2) - 0.6 grad| / allowed = %.4f (0.6 grad = %.6g)" % (miss / allowed, 0.6 * lo["grad"]))
    assert miss <= allowed
    assert abs(0.6 * lo["grad"]) >= 10 * allowed, "the difference under test drowns in its bound"


def test_more_surfaces_than_a_table_in_lds_holds(ctx, oracle, cathedral):
    """The same room with its seven surfaces spread over a table of 70 (three sweeps of 64, 6 and the table read through L2): the same
    sums in the same order, so the same bytes in the rows that moved and exact zeros everywhere else."""
    from parallel_reverb_raytracer_amd import capi
    place = np.array([0, 63, 64, 65, 3, 69, 6])
    nrays, nrefl, sr = 130, 24, 44100.0
    chain, dirs = traced(ctx, oracle, cathedral, nrays, nrefl)
    ctx.reshade(cathedral["T"], AIR_B)
    out = compare(ctx, chain, cathedral["T"], cathedral["mic"], nrefl, "seven surfaces (for the table of 70)")
    triangles = aligned_copy(cathedral["scene"][0])
    triangles["surface"] = place[cathedral["scene"][0]["surface"]]
    wide = aligned_copy(np.resize(cathedral["scene"][2], 70))
    wide[place] = cathedral["scene"][2]
    wide_t = aligned_copy(np.resize(cathedral["T"], 70))
    wide_t[place] = cathedral["T"]
    c = capi.Context(0)
    try:
        c.set_scene((triangles, cathedral["scene"][1], wide))
        c.keep_paths(True)
        c.raytrace(cathedral["mic"], cathedral["source"], dirs, nrefl, AIR_COEFFICIENTS)
        c.reshade(wide_t, AIR_B)
        c.ir_configure_speakers(cathedral["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        grads, grad_air = c.reshade_grad(out["predelay"], sr, out["nbins"], out["w_dev"].data_ptr())
    finally:
        c.close()
    assert grads.shape == (70,)
    assert grads[place].tobytes() == out["got"][0].tobytes() and grad_air.tobytes() == out["got"][1].tobytes()
    rest = np.setdiff1d(np.arange(70), place)
    assert not grads["specular"][rest].any() and not grads["diffuse"][rest].any()


def snapshot(ctx, mic):
    from parallel_reverb_raytracer_amd import capi
    state = (ctx.get_raw_diffuse().tobytes(), ctx.get_direct().tobytes(), ctx.get_raw_images(False).tobytes())
    ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    return state + (ctx.ir_time_range(),)


def test_side_effects_states_and_arguments(oracle, cathedral):
    from parallel_reverb_raytracer_amd import capi
    mic, src, nrays, nrefl, sr = cathedral["mic"], cathedral["source"], 509, 24, 44100.0
    dirs = scenes.sphere_directions(nrays, seed=23)
    w_dev = on_device(weights(2, 4096, 9))

    def refused(c, code, nbins=4096, rate=sr):
        with pytest.raises(capi.RvbError) as e:
            c.reshade_grad(0.0, rate, nbins, w_dev.data_ptr())
        assert e.value.code == code, str(e.value)
        return str(e.value)

    c = capi.Context(0)
    try:
        c.set_scene(cathedral["scene"])
        refused(c, capi.ERR_STATE)                                    # before any trace
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        assert "rvb_keep_paths" in refused(c, capi.ERR_STATE)         # the trace was made without keeping
        c.keep_paths(True)
        c.raytrace(mic, src, dirs, nrefl, AIR_COEFFICIENTS)
        refused(c, capi.ERR_STATE)                                    # no IR configuration since the trace
        before = snapshot(c, mic)
        _, nbins = binning_of(c, mic, SPEAKERS, sr)
        w = on_device(weights(2, nbins, 5))
        first = c.reshade_grad(before[3][0], sr, nbins, w.data_ptr())
        names = [k for k, _ in c.last_timings()]
        assert "reshade_grad_kernel" in names and len(names) == len(set(names)) == 3
        second = c.reshade_grad(before[3][0], sr, nbins, w.data_ptr())
        assert first[0]["specular"].any() and first[0]["diffuse"].any() and first[1].any()
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()      # one fixed order of summation
        assert snapshot(c, mic) == before                            # the records, the direct slot, the images, the time range
        refused(c, capi.ERR_INVALID, nbins=0)
        refused(c, capi.ERR_INVALID, rate=float("nan"))
        c.ir_configure_hrtf(mic, scenes.hrtf_synthetic_table(), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), capi.IR_DIFFUSE, None)
        assert "HRTF" in refused(c, capi.ERR_STATE)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, c.get_raw_images(False))
        assert "RVB_IR_DIFFUSE" in refused(c, capi.ERR_STATE)
        nine = ([(np.cos(i), 0.0, np.sin(i)) for i in range(9)], [0.5] * 9)
        c.ir_configure_speakers(mic, nine[0], nine[1], capi.IR_DIFFUSE, None)
        assert "9 speaker" in refused(c, capi.ERR_STATE)
        assert snapshot(c, mic) == before                            # failed calls leave the results as they were
        c.set_directions(dirs)
        refused(c, capi.ERR_STATE)
    finally:
        c.close()
