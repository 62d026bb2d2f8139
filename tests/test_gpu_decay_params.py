"""rvb_decay_params and rvb_decay_params_loss on the GPU (csrc/decay_params_kernels.hip) against the binary64 numpy reference of
tests/decay_params_reference.py.  Inputs are those of tests/test_gpu_decay.py (`case`: the seeded histogram and the reference's own
float32 curve of it; `exponential_curves`): no call's output feeds the reference.

THE BARS (derived in decay_params_reference.py from the formulas and the formats, never from what the kernels return):
  params   |gpu - ref| <= 2^-23 |ref| + dq: 2^-23 for the rounding to float, dq for two binary64 evaluations — the times' rel |q| of
           decay_reference.times, C's absolute C10 (16 U (|ln early| + |ln late|) + 4 U) + 8 U |q|, D50's 8 U |q|, Ts' (nbins + 16) 2^-52 |q|;
           NaN exactly where the reference has it; the three times byte-equal to rvb_decay_times of the same curve.
  loss     |gpu - ref| <= loss_bar = sum_p weight (2 |d| dq + dq^2) + 32 U loss.
  weights  |gpu - ref| <= 2^-23 |ref| + c_j, c_j = 2 |H_j| [ (j + 16) 2^-52 sum_{k<=j} |terms of g_k| + sum_{k<=j} bars of the terms ].
Targets are the reference's parameters x (1 + 0.2 N(0, 1)), weights 1 / q^2, both as float32; where the reference has no value (or 0) the
target and the weight are 1: a weighted parameter that the model does not yield must add nothing.
GROUND, on the reference alone: at 16 x (2T + 65) with 51200 Hz and at 8 x (T - 1) with 25600 Hz at least 90 % of the non-zero weights
have c_j <= 2^-26 |w_ref| and more than 30 % of all entries are non-zero — the weights test pins them to float precision."""
import ctypes

import numpy as np
import pytest

import decay_params_reference as pref
import decay_reference as dref
from test_gpu_decay import T, case, dev, exponential_curves, histogram, names_of

pytestmark = pytest.mark.gpu

BIG = 2 * T + 65
# 51200 Hz: k50 = 2560, k80 = T; 51187.5 / 51212.5: k80 = T - 1 / T + 1; 500 Hz at 65 bins: k50 = 25, k80 = 40; 25600 Hz at 8 x (T - 1):
# k80 = 2048, one bin behind the start of row 1's zero tail (its C80 is NaN, its C50 is not); (2, 130 T + 5): the carry wave's rounds
CASES = [(16, 1, 51200.0), (16, 2, 51200.0), (16, 63, 51200.0), (16, 65, 500.0), (16, T - 1, 51200.0), (16, T, 51200.0), (16, T + 1, 51200.0),
         (16, BIG, 51200.0), (16, BIG, 51187.5), (16, BIG, 51212.5), (1, BIG, 51200.0), (72, BIG, 51200.0), (8, T - 1, 25600.0),
         (2, 130 * T + 5, 51200.0)]
GROUND = {(16, BIG, 51200.0), (8, T - 1, 25600.0)}
PARAMS_NAMES = ["decay_params_find_kernel", "decay_params_window_kernel", "decay_params_sums_kernel", "decay_params_fit_kernel"]
ADJOINT_NAMES = ["decay_params_adjoint_sums_kernel", "decay_params_adjoint_carry_kernel", "decay_params_adjoint_scan_kernel"]
LEVELS = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))


@pytest.fixture(scope="module")
def ctx():
    from parallel_reverb_raytracer_amd import capi
    assert capi.DECAY_TILE == T and capi.DECAY_NPARAMS == pref.NPARAMS
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    yield c
    c.close()


def table(q, seed):
    """(targets, weights) float32 for the reference's parameters q."""
    has = np.isfinite(q) & (q != 0)
    noise = np.random.default_rng(seed).standard_normal(q.shape)
    safe = np.where(has, q, 1.0)
    return np.where(has, safe * (1.0 + 0.2 * noise), 1.0).astype(np.float32), np.where(has, 1.0 / (safe * safe), 1.0).astype(np.float32)


def check(ctx, h, e32, fs, ground=False, label=""):
    """Every assertion on the two calls for one (H, E, sample rate)."""
    import torch
    nrows, nbins = e32.shape
    q, dq = pref.params(e32, fs)
    targets, weights = table(q, 4000 + nrows + nbins)
    r = pref.loss(h, e32, fs, targets, weights)
    bar = 2.0 ** -23 * np.abs(r["w"]) + r["c"]
    nonzero = r["w"] != 0
    if ground:
        share = float((r["c"][nonzero] <= 2.0 ** -26 * np.abs(r["w"][nonzero])).mean())
        full = np.isfinite(q[:, :3]).all(axis=1).sum()
        print("decay params ground %s: non-zero %.3f of all entries, c_j <= 2^-26 |w| for %.4f of them, %d of %d rows with all three times" %
              (label, nonzero.mean(), share, full, nrows))
        assert nonzero.mean() > 0.3 and share >= 0.9, (nonzero.mean(), share)
    h_dev, e_dev = dev(h), dev(e32)
    hp, ep = h_dev.data_ptr(), e_dev.data_ptr()

    got = ctx.decay_params(ep, nrows, nbins, fs)
    assert names_of(ctx) == PARAMS_NAMES
    assert got.dtype == np.float32 and got.shape == (nrows, pref.NPARAMS) and got.tobytes() == ctx.decay_params(ep, nrows, nbins, fs).tobytes()
    for p, (db_begin, db_end) in enumerate(LEVELS):
        assert got[:, p].tobytes() == ctx.decay_times(ep, nrows, nbins, fs, db_begin, db_end).tobytes(), p
    assert (np.isnan(got) == np.isnan(q)).all(), (got, q)
    ok = np.isfinite(q)
    pbar = 2.0 ** -23 * np.abs(q) + dq
    pmiss = np.abs(np.where(ok, got, 0.0).astype(np.float64) - np.where(ok, q, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        print("decay params %s: max |gpu - ref| / bar per parameter = %s" %
              (label, np.array2string(np.nanmax(np.where(ok & (pbar > 0), pmiss / pbar, 0.0), axis=0), precision=3)))
    assert (pmiss <= pbar)[ok].all()

    def run(with_weights):
        w = torch.full((nrows, nbins), 7.0, dtype=torch.float32, device="cuda") if with_weights else None
        torch.cuda.synchronize()
        losses, params = ctx.decay_params_loss(hp, ep, nrows, nbins, fs, targets, weights, w.data_ptr() if with_weights else None)
        return losses, params, (w.cpu().numpy() if with_weights else None)

    losses, params, w = run(True)
    assert names_of(ctx) == PARAMS_NAMES + ADJOINT_NAMES
    losses2, params2, w2 = run(True)
    alone, params3, _ = run(False)
    assert names_of(ctx) == PARAMS_NAMES
    assert losses.dtype == np.float64 and losses.tobytes() == losses2.tobytes() == alone.tobytes() and w.tobytes() == w2.tobytes()
    assert params.tobytes() == params2.tobytes() == params3.tobytes() == got.tobytes()
    loss_miss = np.abs(losses - r["loss_rows"])
    miss = np.abs(w.astype(np.float64) - r["w"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print("decay params loss %s: max loss miss / bar = %.4f, max weight miss / bar = %.4f, sum loss = %.6g, non-zero weights %d" %
              (label, np.nanmax(np.where(r["loss_bar"] > 0, loss_miss / r["loss_bar"], 0.0)), np.nanmax(np.where(bar > 0, miss / bar, 0.0)),
               r["loss_rows"].sum(), nonzero.sum()))
    assert np.isfinite(w).all()
    assert (loss_miss <= r["loss_bar"]).all()
    assert (miss <= bar).all()
    assert (w[h == 0] == 0).all()                                            # exactly 0 where H is 0 (and nothing left unwritten: no 7.0)
    assert (losses[~r["counts"]] == 0).all() and not w[~r["counts"]].any()   # rows in which no parameter counts
    assert h_dev.cpu().numpy().tobytes() == h.tobytes() and e_dev.cpu().numpy().tobytes() == e32.tobytes()
    return q, got, r


@pytest.mark.parametrize("nrows,nbins,fs", CASES)
def test_params_loss_and_weights(ctx, nrows, nbins, fs):
    c = case(nrows, nbins)
    q, got, r = check(ctx, c["h"], c["e32"], fs, ground=(nrows, nbins, fs) in GROUND, label="%d x %d at %g Hz" % (nrows, nbins, fs))
    ke = [pref.bin_of(t, float(np.float32(fs)), nbins) for t in pref.EARLY]
    if nbins <= 2:
        assert ke == [None, None] and np.isnan(got[:, pref.C50:pref.TS]).all()
        assert nbins > 1 or (got[np.isfinite(got[:, pref.TS]), pref.TS] == 0).all()
    if nrows >= 4:
        assert np.isnan(got[2]).all() and not r["counts"][2]                 # the all-zero row
    if (nrows, nbins, fs) == (8, T - 1, 25600.0):
        assert ke == [1280, 2048] and np.isnan(got[1, pref.C80]) and np.isfinite(got[1, pref.C50]) and got[1, pref.D50] < 1
    if nbins == BIG and nrows >= 16:
        assert ke[1] == {51200.0: T, 51187.5: T - 1, 51212.5: T + 1}[fs] and (ke[0] == 2560 or fs != 51200.0)
        assert np.isfinite(got[0]).all() and r["counts"][0] and r["loss_rows"][0] > 0
    if (nbins, fs) == (65, 500.0):
        assert ke == [25, 40]
    if nbins == T and fs == 51200.0:
        assert ke == [2560, None] and np.isnan(got[:, pref.C80]).all() and np.isfinite(got[0, pref.C50])


def test_window_edges_on_tile_edges(ctx):
    """exponential_curves(70001): k0 = T - 1, T, T + 1 and k1 = 2T - 1, 2T, 2T + 1 of the T30 window, steeper rows, an all-zero row, a
    curve that never falls by 10 dB, windows of one and two bins; the histogram is an unrelated one (the calls take any H and E)."""
    nbins, fs = 70001, 44100.0
    e32 = exponential_curves(nbins)
    assert [dref.window(e32[r], -5.0, -35.0)[0] for r in range(3)] == [T - 1, T, T + 1]
    assert [dref.window(e32[r], -5.0, -35.0)[1] for r in range(3, 6)] == [2 * T - 1, 2 * T, 2 * T + 1]
    h = histogram(e32.shape[0], nbins, 321)
    q, got, _ = check(ctx, h, e32, fs, label="exponential curves")
    assert np.isnan(q[8]).all() and np.isnan(q[9, :3]).all() and np.isfinite(q[:8]).all()
    assert abs(got[6, pref.T30] - 3.0 * np.log(10.0) / (0.01 * fs)) <= 1e-6 * got[6, pref.T30]


def test_arguments(ctx):
    """Every refusal of the two calls; a failed call writes nothing, on the device or on the host."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    lib, handle = ctx.lib, ctx.handle
    nrows, nbins, fs = 4, 100, 44100.0
    bufs = [torch.full((nrows * nbins + 50,), 7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    h, e, w = (b.data_ptr() for b in bufs)
    params = np.full((nrows, 7), 7.0, dtype=np.float32)
    losses = np.full(nrows, 7.0, dtype=np.float64)
    targets, weights = np.ones((nrows, 7), dtype=np.float32), np.ones((nrows, 7), dtype=np.float32)
    pp, lp = params.ctypes.data_as(ctypes.c_void_p), losses.ctypes.data_as(ctypes.c_void_p)
    tp, wp = targets.ctypes.data_as(ctypes.c_void_p), weights.ctypes.data_as(ctypes.c_void_p)

    def plain(*a):
        return lib.rvb_decay_params(handle, *a)

    def loss(*a):
        return lib.rvb_decay_params_loss(handle, *a)

    inv, cap = capi.ERR_INVALID, capi.ERR_CAPACITY
    assert plain(None, nrows, nbins, fs, pp) == inv and plain(e, nrows, nbins, fs, None) == inv
    assert plain(e, 0, nbins, fs, pp) == inv and plain(e, nrows, 0, fs, pp) == inv
    assert plain(e, 4097, nbins, fs, pp) == cap and "4096" in lib.rvb_last_error(handle).decode()
    assert plain(e, nrows, 2 ** 32, fs, pp) == cap
    for rate in (0.0, -1.0, float("nan"), float("inf")):
        assert plain(e, nrows, nbins, rate, pp) == inv and loss(h, e, nrows, nbins, rate, tp, wp, lp, pp, w) == inv, rate
    for args in ((None, e, nrows, nbins, fs, tp, wp, lp), (h, None, nrows, nbins, fs, tp, wp, lp), (h, e, nrows, nbins, fs, None, wp, lp),
                 (h, e, nrows, nbins, fs, tp, None, lp), (h, e, nrows, nbins, fs, tp, wp, None), (h, e, 0, nbins, fs, tp, wp, lp),
                 (h, e, nrows, 0, fs, tp, wp, lp)):
        assert loss(*args, pp, w) == inv and loss(*args, None, None) == inv, args
    assert loss(h, e, 4097, nbins, fs, tp, wp, lp, pp, w) == cap and loss(h, e, nrows, 2 ** 32, fs, tp, wp, lp, pp, None) == cap
    for bad in (-1.0, float("nan"), float("inf")):
        spoiled = weights.copy()
        spoiled[3, 6] = bad
        assert loss(h, e, nrows, nbins, fs, tp, spoiled.ctypes.data_as(ctypes.c_void_p), lp, pp, w) == inv, bad
    for bad in (float("nan"), float("inf")):
        spoiled = targets.copy()
        spoiled[2, 4] = bad
        assert loss(h, e, nrows, nbins, fs, spoiled.ctypes.data_as(ctypes.c_void_p), wp, lp, pp, w) == inv, bad
    for alias in (h, e, h + 4 * (nrows * nbins - 1), e + 40):
        assert loss(h, e, nrows, nbins, fs, tp, wp, lp, pp, alias) == inv
    torch.cuda.synchronize()
    ctx.synchronize()
    assert all((b == 7.0).all().item() for b in bufs) and (params == 7.0).all() and (losses == 7.0).all()
    # ... and a target that is not finite under a weight of 0 is taken, as are NULL params
    spoiled, none = targets.copy(), weights.copy()
    spoiled[2, 4], none[2, 4] = float("nan"), 0.0
    bufs[0].fill_(0.5)
    bufs[1].copy_(torch.arange(nrows * nbins + 50, 0, -1, dtype=torch.float32, device="cuda"))
    torch.cuda.synchronize()
    assert loss(h, e, nrows, nbins, fs, spoiled.ctypes.data_as(ctypes.c_void_p), none.ctypes.data_as(ctypes.c_void_p), lp, None, w) == 0
    assert np.isfinite(losses).all() and (bufs[2][:nrows * nbins] != 7.0).all().item() and (bufs[2][nrows * nbins:] == 7.0).all().item()


def test_the_context_keeps_its_trace_its_configuration_and_its_prepared_list(ctx):
    """On a context with a kept trace and an IR configuration: the records, the direct slot, the candidates, ir_time_range and a
    following reshade_grad are byte-equal before and after the two calls, and a prepared exact list still folds."""
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
        params = c.decay_params_tensor(curve, sr)
        assert params.shape == (2, 8, 7) and np.isfinite(params[..., :3]).any()
        weights = torch.empty_like(hist)
        has = np.isfinite(params)
        losses, again = c.decay_params_loss_tensor(hist, curve, sr, np.where(has, params * 1.25, 1.0), has.astype(np.float32), weights)
        assert losses.shape == (2, 8) and again.tobytes() == params.tobytes() and (losses[has.any(axis=2)] > 0).all()
        assert torch.isfinite(weights).all().item() and weights.any().item()
        folded = torch.zeros_like(hist)
        c.ir_exact_fold_tensor(nbins, 0, nbins, folded)                  # the prepared list is still valid
        c.synchronize()
        assert torch.equal(folded, hist)
        assert state() == before
    finally:
        c.close()
