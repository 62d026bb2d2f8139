"""The decay calls on the GPU (rvb_decay_curve, rvb_decay_times, rvb_decay_loss; csrc/decay_kernels.hip) against the binary64 numpy
reference of tests/decay_reference.py.  Inputs are seeded and made here; no call's output feeds the reference of another: every call
gets the reference's own float32 arrays.

THE BARS (derived in decay_reference.py from the formulas and the formats, never from what the kernels return):
  curve    |gpu - ref| <= 2^-23 |ref|: the binary64 sum of exact non-negative squares errs by at most nbins 2^-53 relative, and the
           rounding to float on top of that can move the float by one ulp; exactly 0 where the reference is 0.
  times    |gpu - ref| <= (2^-23 + rel) |ref|: 2^-23 for the rounding to float, rel = decay_reference.times' term for two binary64
           evaluations of the centred sums (levels good to 8 u (1 + |level|), n products and n additions per sum, 8 roundings behind
           the sum).  For the windows of this file rel stays below 1e-10: the bar IS float precision.
  loss     |gpu - ref| <= loss_bar = sum m (2 |d| D + D^2) + (nbins + 16) 2^-52 sum m d^2, D = 2^-49 Lambda the bar of one residual.
  weights  |gpu - ref| <= 2^-23 |ref| + c_j,
           c_j = 2 |H_j| [ (j + 16) 2^-52 (sum_{k<=j} |g_k| + |N|) + sum_{k<=j} 2 m_k D_k / E_k + |dN| ], N the normalisation term and
           dN its own bar (decay_reference.loss).  Against the issue's statement of c_j the residual's bar is 2^-49 Lambda, not 2^-50:
           two evaluations, each with two or four logarithms good to 2 ulp and up to three differences, add up to 14 u Lambda; and the
           normalisation term carries the bar of its sum over the whole row.
GROUND, on the reference alone: at 16 x (2T + 65) for both flag values and at 8 x (T - 1), at least 90 % of the non-zero weights have
c_j <= 2^-26 |w_ref| — the weights test pins them to float precision, not to a cancellation allowance."""
import ctypes

import numpy as np
import pytest

import decay_reference as ref

pytestmark = pytest.mark.gpu

T = 4096
ALL_BINS = [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 63, 2 * T + 65]
SHAPES = [(16, n) for n in ALL_BINS] + [(r, 2 * T + 65) for r in (1, 8, 72)]
GROUND_SHAPES = {(16, 2 * T + 65), (8, T - 1)}
LOSS_SHAPES = SHAPES + [(8, T - 1)]
CURVE_NAMES = ["decay_curve_sums_kernel", "decay_curve_carry_kernel", "decay_curve_scan_kernel"]
TIMES_NAMES = ["decay_times_find_kernel", "decay_times_window_kernel", "decay_times_sums_kernel", "decay_times_fit_kernel"]
LOSS_NAMES = ["decay_loss_sums_kernel", "decay_loss_carry_kernel", "decay_loss_scan_kernel"]


def histogram(nrows, nbins, seed):
    """Normal values under an exponential envelope that falls by 60 dB over the row (amplitude 1 -> 1e-3: every non-zero E stays above
    1e-9, far above 1e-30), 35 % exact zeros — the share of zero-volume impulses.  With at least 4 rows: row 1's tail is zero from the
    middle of its last full tile on (from nbins / 2 where there is none), row 2 is all zero, row 3's only non-zero is its last bin."""
    rng = np.random.default_rng(seed)
    rate = 6.9 / nbins if nbins >= 16 else 0.1
    h = (rng.standard_normal((nrows, nbins)) * np.exp(-rate * np.arange(nbins))[None, :]).astype(np.float32)
    h[rng.random(h.shape) < 0.35] = 0.0
    if nrows >= 4:
        full = nbins // T
        h[1, ((full - 1) * T + T // 2) if full else nbins // 2:] = 0.0
        h[2] = 0.0
        h[3] = 0.0
        h[3, -1] = 0.37
    return h


_cases = {}


def case(nrows, nbins):
    """H, the reference's own float32 curve E of it, a target T (the float32 curve of another histogram) and the mask of T's -5 .. -35 dB
    range; a row too short to hold that range takes every bin.  Computed once per shape and left unchanged."""
    key = (nrows, nbins)
    if key not in _cases:
        h = histogram(nrows, nbins, 1000 + 7 * nrows + nbins)
        e = ref.curve(h)
        e32 = e.astype(np.float32)
        other = histogram(nrows, nbins, 5000 + 7 * nrows + nbins)
        if nrows >= 4:
            other[1:4] = histogram(3, nbins, 9000 + nbins)[:3] if nbins >= 4 else 0.5          # the target rows are ordinary decays
        t32 = (ref.curve(other) * 1.3).astype(np.float32)
        m = ref.mask_of(t32)
        m[~m.any(axis=1)] = 1.0
        for a in (h, e, e32, t32, m):
            a.setflags(write=False)
        _cases[key] = {"h": h, "e": e, "e32": e32, "t32": t32, "m": m, "loss": {}}
    return _cases[key]


def loss_reference(c, normalised):
    if normalised not in c["loss"]:
        c["loss"][normalised] = ref.loss(c["h"], c["e32"], c["t32"], c["m"], normalised)
    return c["loss"][normalised]


def dev(a):
    import torch
    t = torch.from_numpy(np.array(a, order="C", copy=True)).cuda()          # (a copy: the shared inputs are read-only)
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def ctx():
    from parallel_reverb_raytracer_amd import capi
    assert capi.DECAY_TILE == T
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    yield c
    c.close()


def names_of(ctx):
    return [k for k, _ in ctx.last_timings()]


def run_curve(ctx, h_dev, nrows, nbins):
    import torch
    out = torch.full((nrows, nbins), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.decay_curve(h_dev.data_ptr(), nrows, nbins, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("nrows,nbins", SHAPES + [(2, 130 * T + 5)])
def test_curve(ctx, nrows, nbins):
    """(2 x (130 T + 5): the wave that carries a row's tiles takes three rounds, the last a partial one.)"""
    c = case(nrows, nbins)
    h_dev = dev(c["h"])
    got = run_curve(ctx, h_dev, nrows, nbins)
    assert names_of(ctx) == CURVE_NAMES
    again = run_curve(ctx, h_dev, nrows, nbins)
    want = c["e"]
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("decay curve %3d x %-7d max |gpu - ref| / (2^-23 |ref|) = %.4f" % (nrows, nbins, np.nanmax(np.where(want > 0, err / (2.0 ** -23 * want), 0.0))))
    assert (err <= 2.0 ** -23 * want).all()
    assert (got[want == 0] == 0).all() and (got[want > 0] > 0).all()
    assert got.tobytes() == again.tobytes()
    assert h_dev.cpu().numpy().tobytes() == c["h"].tobytes()
    if nrows >= 4:
        assert not got[2].any() and (got[3] == got[3, -1]).all() and got[3, -1] > 0


def exponential_curves(nbins):
    """Curves of H[k] = exp(-a k), computed over 2 nbins bins and CUT to nbins (so the cut leaves no trace in the levels), float32.
    With a = 5 / ((10 / ln 10) 2 (K - 0.5)) the level crosses -5 dB between bins K - 1 and K (k0 = K); with 35 in place of 5 it crosses
    -35 dB there (k1 = K).  Rows: k0 = T - 1, T, T + 1; k1 = 2T - 1, 2T, 2T + 1; two steeper slopes; an all-zero row; a curve that the cut
    ends above -35 dB (and above -10 dB); a window of one bin; a window of exactly two bins."""
    db_per = 20.0 / np.log(10.0)             # the level of exp(-a k) falls by db_per * a per bin
    rates = [5.0 / (db_per * (k - 0.5)) for k in (T - 1, T, T + 1)] + [35.0 / (db_per * (k - 0.5)) for k in (2 * T - 1, 2 * T, 2 * T + 1)]
    rates += [0.01, 0.002]
    k = np.arange(2 * nbins, dtype=np.float64)
    rows = [ref.curve(np.exp(-a * k)[None, :])[0, :nbins] for a in rates]
    rows.append(np.zeros(nbins))
    rows.append(ref.curve(np.exp(-(8.0 / (db_per * nbins)) * k)[None, :])[0, :nbins])
    one = np.zeros(nbins)
    one[:3] = [1.0, 0.2, 1e-5]
    two = np.zeros(nbins)
    two[:4] = [1.0, 0.2, 0.1, 1e-5]
    rows += [one, two]
    return np.array(rows).astype(np.float32)


def test_times(ctx):
    nbins, rate = 70001, 44100.0
    e32 = exponential_curves(nbins)
    nrows = e32.shape[0]
    assert [ref.window(e32[r], -5.0, -35.0)[0] for r in range(3)] == [T - 1, T, T + 1]
    assert [ref.window(e32[r], -5.0, -35.0)[1] for r in range(3, 6)] == [2 * T - 1, 2 * T, 2 * T + 1]
    assert ref.window(e32[11], -5.0, -35.0) == (1, 3) and ref.window(e32[10], -5.0, -35.0) is None
    e_dev = dev(e32)
    for db_begin, db_end in ((-5.0, -35.0), (0.0, -10.0), (-5.0, -25.0)):
        want, rel = ref.times(e32, rate, db_begin, db_end)
        got = ctx.decay_times(e_dev.data_ptr(), nrows, nbins, rate, db_begin, db_end)
        assert names_of(ctx) == TIMES_NAMES
        assert got.dtype == np.float32 and got.tobytes() == ctx.decay_times(e_dev.data_ptr(), nrows, nbins, rate, db_begin, db_end).tobytes()
        assert np.isnan(want[8]) and np.isnan(want[9]) and np.isfinite(want[:8]).all() and np.isfinite(want[11])
        assert np.isnan(want[10]) == (db_begin < 0)               # from 0 dB the window of row 10 is {0, 1}
        assert (np.isnan(got) == np.isnan(want)).all(), (got, want)
        ok = np.isfinite(want)
        assert rel[ok].max() < 1e-10
        miss = np.abs(got[ok].astype(np.float64) - want[ok]) / ((2.0 ** -23 + rel[ok]) * np.abs(want[ok]))
        print("decay times %5.0f .. %5.0f dB: max |gpu - ref| / bar = %.4f; seconds = %s" % (db_begin, db_end, miss.max(), got))
        assert (miss <= 1.0).all()
    # the closed form of the rows' own slopes: T60 = 3 ln 10 / (a sample_rate)
    got = ctx.decay_times(e_dev.data_ptr(), nrows, nbins, rate, -5.0, -35.0)
    assert abs(got[6] - 3.0 * np.log(10.0) / (0.01 * rate)) <= 1e-6 * got[6]
    assert e_dev.cpu().numpy().tobytes() == e32.tobytes()


def run_loss(ctx, c, d, nrows, nbins, flags, with_weights=True):
    import torch
    w = torch.full((nrows, nbins), 7.0, dtype=torch.float32, device="cuda") if with_weights else None
    torch.cuda.synchronize()
    losses = ctx.decay_loss(d["h"].data_ptr(), d["e"].data_ptr(), d["t"].data_ptr(), d["m"].data_ptr(), nrows, nbins, flags,
                            w.data_ptr() if with_weights else None)
    return losses, (w.cpu().numpy() if with_weights else None)


@pytest.mark.parametrize("normalised", [True, False])
@pytest.mark.parametrize("nrows,nbins", LOSS_SHAPES + [(2, 130 * T + 5)])
def test_loss_and_weights(ctx, nrows, nbins, normalised):
    from parallel_reverb_raytracer_amd import capi
    c = case(nrows, nbins)
    r = loss_reference(c, normalised)
    nonzero = r["w"] != 0
    if (nrows, nbins) in GROUND_SHAPES:
        share = float((r["c"][nonzero] <= 2.0 ** -26 * np.abs(r["w"][nonzero])).mean())
        assert nonzero.sum() > 0.3 * nrows * nbins * 0.5 and share >= 0.9, share
    d = {k: dev(c[v]) for k, v in (("h", "h"), ("e", "e32"), ("t", "t32"), ("m", "m"))}
    flags = capi.DECAY_NORMALISED if normalised else 0
    losses, w = run_loss(ctx, c, d, nrows, nbins, flags)
    assert names_of(ctx) == LOSS_NAMES
    losses2, w2 = run_loss(ctx, c, d, nrows, nbins, flags)
    alone, _ = run_loss(ctx, c, d, nrows, nbins, flags, with_weights=False)
    assert names_of(ctx) == LOSS_NAMES[:2]
    assert losses.dtype == np.float64 and losses.tobytes() == losses2.tobytes() == alone.tobytes() and w.tobytes() == w2.tobytes()
    loss_miss = np.abs(losses - r["loss_rows"])
    bar = 2.0 ** -23 * np.abs(r["w"]) + r["c"]
    miss = np.abs(w.astype(np.float64) - r["w"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print("decay loss %3d x %-7d normalised=%d: max loss miss / bar = %.4f, max weight miss / bar = %.4f, sum loss = %.6g, non-zero weights %d" %
              (nrows, nbins, normalised, np.nanmax(np.where(r["loss_bar"] > 0, loss_miss / r["loss_bar"], 0.0)),
               np.nanmax(np.where(bar > 0, miss / bar, 0.0)), r["loss_rows"].sum(), nonzero.sum()))
    assert np.isfinite(w).all()
    assert (loss_miss <= r["loss_bar"]).all()
    assert (miss <= bar).all()
    assert (w[c["h"] == 0] == 0).all()                                       # exactly 0 where H is 0 (and nothing left unwritten: no 7.0)
    idle = ~r["rows"] | ~((c["m"] > 0) & (c["e32"] > 0) & (c["t32"] > 0)).any(axis=1)
    assert (losses[idle] == 0).all() and not w[idle].any()                   # rows that do not count
    assert nrows < 4 or idle[2]
    if nbins >= 63:
        assert not idle[0] and r["loss_rows"][0] > 0 and losses[0] > 0
    for k, v in (("h", "h"), ("e", "e32"), ("t", "t32"), ("m", "m")):
        assert d[k].cpu().numpy().tobytes() == c[v].tobytes()


def test_a_target_that_starts_at_zero(ctx):
    """T[r][0] == 0: with the flag the row does not count (loss 0, weights 0); without it it counts wherever T > 0."""
    from parallel_reverb_raytracer_amd import capi
    nrows, nbins = 8, T + 1
    c = dict(case(nrows, nbins))
    t32 = c["t32"].copy()
    t32[0, 0] = 0.0
    c["t32"] = t32
    d = {k: dev(c[v]) for k, v in (("h", "h"), ("e", "e32"), ("t", "t32"), ("m", "m"))}
    for normalised in (True, False):
        r = ref.loss(c["h"], c["e32"], t32, c["m"], normalised)
        losses, w = run_loss(ctx, c, d, nrows, nbins, capi.DECAY_NORMALISED if normalised else 0)
        assert (np.abs(losses - r["loss_rows"]) <= r["loss_bar"]).all()
        assert (np.abs(w.astype(np.float64) - r["w"]) <= 2.0 ** -23 * np.abs(r["w"]) + r["c"]).all()
        assert (losses[0] == 0 and not w[0].any()) if normalised else (losses[0] > 0 and w[0].any())


def test_arguments(ctx):
    """Every refusal of the three calls; a failed call writes nothing, on the device or on the host."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    lib, handle = ctx.lib, ctx.handle
    nrows, nbins = 4, 100
    bufs = [torch.full((nrows * nbins + 50,), 7.0, dtype=torch.float32, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    h, e, t, m, w = (b.data_ptr() for b in bufs)
    seconds = np.full(nrows, 7.0, dtype=np.float32)
    losses = np.full(nrows, 7.0, dtype=np.float64)
    sp, lp = seconds.ctypes.data_as(ctypes.c_void_p), losses.ctypes.data_as(ctypes.c_void_p)

    def curve(*a):
        return lib.rvb_decay_curve(handle, *a)

    def times(*a):
        return lib.rvb_decay_times(handle, *a)

    def loss(*a):
        return lib.rvb_decay_loss(handle, *a)

    inv, cap = capi.ERR_INVALID, capi.ERR_CAPACITY
    assert curve(None, nrows, nbins, e) == inv and curve(h, nrows, nbins, None) == inv
    assert curve(h, 0, nbins, e) == inv and curve(h, nrows, 0, e) == inv
    assert curve(h, nrows, nbins, h) == inv and curve(h, nrows, nbins, h + 4 * (nrows * nbins - 1)) == inv and curve(h + 40, nrows, nbins, h) == inv
    assert curve(h, 4097, nbins, e) == cap
    assert "4096" in lib.rvb_last_error(handle).decode()
    assert times(None, nrows, nbins, 44100.0, -5.0, -35.0, sp) == inv and times(e, nrows, nbins, 44100.0, -5.0, -35.0, None) == inv
    assert times(e, 0, nbins, 44100.0, -5.0, -35.0, sp) == inv and times(e, nrows, 0, 44100.0, -5.0, -35.0, sp) == inv
    assert times(e, 4097, nbins, 44100.0, -5.0, -35.0, sp) == cap
    for rate, b, en in ((0.0, -5.0, -35.0), (-1.0, -5.0, -35.0), (float("nan"), -5.0, -35.0), (float("inf"), -5.0, -35.0),
                        (44100.0, -35.0, -5.0), (44100.0, -5.0, -5.0), (44100.0, 1.0, -35.0), (44100.0, float("nan"), -35.0),
                        (44100.0, -5.0, float("nan")), (44100.0, -5.0, float("-inf"))):
        assert times(e, nrows, nbins, rate, b, en, sp) == inv, (rate, b, en)
    norm = capi.DECAY_NORMALISED
    for args in ((None, e, t, m), (h, None, t, m), (h, e, None, m), (h, e, t, None)):
        assert loss(*args, nrows, nbins, norm, lp, w) == inv
    assert loss(h, e, t, m, nrows, nbins, norm, None, w) == inv
    assert loss(h, e, t, m, 0, nbins, norm, lp, w) == inv and loss(h, e, t, m, nrows, 0, norm, lp, w) == inv
    assert loss(h, e, t, m, 4097, nbins, norm, lp, w) == cap and loss(h, e, t, m, 4097, nbins, norm, lp, None) == cap
    assert loss(h, e, t, m, nrows, nbins, 2, lp, w) == inv
    for alias in (h, e, t, m, m + 4 * (nrows * nbins - 1)):
        assert loss(h, e, t, m, nrows, nbins, norm, lp, alias) == inv
    torch.cuda.synchronize()
    ctx.synchronize()
    assert all((b == 7.0).all().item() for b in bufs) and (seconds == 7.0).all() and (losses == 7.0).all()
    # ... and the same arguments, valid, are taken: E behind H in one allocation, touching but not overlapping
    both = torch.ones((2 * nrows * nbins,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    assert curve(both.data_ptr(), nrows, nbins, both.data_ptr() + 4 * nrows * nbins) == 0
    ctx.synchronize()
    assert (both[nrows * nbins:].cpu().numpy().reshape(nrows, nbins) == np.arange(nbins, 0, -1, dtype=np.float32)[None, :]).all()


def test_the_context_keeps_its_trace_its_configuration_and_its_prepared_list(ctx):
    """On a context with a kept trace and an IR configuration: the records, the direct slot, the candidates, ir_time_range and a
    following reshade_grad are byte-equal before and after the three calls, and a prepared exact list still folds."""
    import torch
    from parallel_reverb_raytracer_amd import capi, scenes
    from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS
    from test_gpu_reshade import SPEAKERS
    scene, info = scenes.cathedral(3000)
    mic, src, sr = info["mic"], info["source"], 44100.0
    c = capi.Context(0)
    try:
        c.set_scene(scene)
        c.keep_paths(True)
        c.raytrace(mic, src, scenes.sphere_directions(509, seed=23), 24, AIR_COEFFICIENTS)
        c.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        lo, hi = c.ir_time_range()
        nbins = c.ir_bins(hi, lo, sr)
        wts = dev(np.random.default_rng(5).standard_normal((2, 8, nbins)).astype(np.float32))

        def state():
            g = c.reshade_grad(lo, sr, nbins, wts.data_ptr())          # (fails with RVB_ERR_STATE without the IR configuration)
            return (c.get_raw_diffuse().tobytes(), c.get_direct().tobytes(), c.get_image_candidates().tobytes(), c.ir_time_range(),
                    g[0].tobytes(), g[1].tobytes())

        hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
        c.ir_accumulate_tensor(lo, sr, nbins, capi.IR_EXACT, hist)
        c.synchronize()
        before = state()
        c.ir_exact_prepare(lo, sr, nbins)
        curve = c.decay_curve_tensor(hist)
        c.synchronize()
        target = (curve * 2.0).contiguous()
        mask = dev(ref.mask_of(target.cpu().numpy().reshape(16, nbins)).reshape(2, 8, nbins))
        weights = torch.empty_like(hist)
        losses = c.decay_loss_tensor(hist, curve, target, mask, capi.DECAY_NORMALISED, weights)
        seconds = c.decay_times_tensor(curve, sr)
        assert losses.shape == (2, 8) and seconds.shape == (2, 8) and weights.shape == hist.shape
        assert np.isfinite(seconds).any() and (losses < 1e-20).all()    # twice the curve is the same decay once normalised
        plain = c.decay_loss_tensor(hist, curve, target, mask, 0, weights)
        assert (plain[np.isfinite(seconds)] > 0).all()
        folded = torch.zeros_like(hist)
        c.ir_exact_fold_tensor(nbins, 0, nbins, folded)                  # the prepared list is still valid
        c.synchronize()
        assert torch.equal(folded, hist)
        assert state() == before
    finally:
        c.close()
