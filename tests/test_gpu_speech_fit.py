"""Fitting toward a speech transmission index (parallel-reverb-raytracer_amd/fitting.py: sti_loss_and_grad, fit_sti,
sti_sensitivity_map) and the index map over listeners (listeners.sti_map) end to end on the GPU: reshade -> exact binning -> rvb_mtf ->
rvb_speech_index -> rvb_mtf_adjoint -> rvb_reshade_grad (+ rvb_reshade_grad_images).  The setup of tests/test_gpu_decay_params_fit.py:
scenes.cathedral(3000), 509 rays x 24 reflections, the stereo speakers of tests/test_gpu_reshade.py, a kept trace.  The target is the
index of another surface table, the channel weights 1.

A wrong adjoint, a wrong dSTI/dm, or weights in another layout than the histogram's, gives a direction along which the loss does not
fall: the descent test fails then.  |g|^2 > 0 is asserted, so an index clipped everywhere cannot pass vacuously."""
import numpy as np
import pytest

import speech_reference as ref
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_reshade import SPEAKERS
from test_gpu_reshade_grad import table_t

pytestmark = pytest.mark.gpu

SR, C = 44100.0, 1e-4


def histogram_of(ctx, mic, predelay, nbins, which):
    """the explicit sequence of calls for the histogram of the context's records under `which`"""
    import torch
    from parallel_reverb_raytracer_amd import capi
    if which == capi.IR_DIFFUSE:
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    else:
        ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], which, False)
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    ctx.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist)
    return hist


@pytest.fixture(scope="module")
def setup():
    from parallel_reverb_raytracer_amd import capi, fitting, speech
    scene, info = scenes.cathedral(3000)
    mic, src = info["mic"], info["source"]
    start, goal = table_t(scene[2], seed=11), table_t(scene[2], seed=12)
    ctx = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    ctx.set_scene(scene)
    ctx.keep_paths(True, listener=True)
    ctx.raytrace(mic, src, scenes.sphere_directions(509, seed=23), 24, AIR_COEFFICIENTS)
    ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, SR)
    ctx.reshade(goal, AIR_COEFFICIENTS)
    targets = {which: speech.sti(ctx, histogram_of(ctx, mic, predelay, nbins, which), SR) for which in (capi.IR_DIFFUSE, capi.IR_ALL)}
    for which, target in targets.items():
        assert target.shape == (2,) and np.isfinite(target).all(), "the target index of a channel is not available"
    free = np.zeros((scene[2].shape[0], 16), dtype=bool)
    free[:, :8] = True                                           # the specular coefficients
    args = {which: (AIR_COEFFICIENTS, mic, SPEAKERS, targets[which], np.ones(2), SR, predelay, nbins) for which in targets}
    map_nbins = ctx.ir_bins(latest + 0.01, 0.0, SR)              # from time 0, with room for a microphone half a metre away
    yield {"ctx": ctx, "fitting": fitting, "start": start, "free": free, "args": args, "nbins": map_nbins, "mic": mic, "scene": scene}
    ctx.close()


@pytest.mark.parametrize("which_name", ["IR_DIFFUSE", "IR_ALL"])
def test_the_gradient_is_a_descent_direction_and_its_negative_is_not(setup, which_name):
    """Chain rule end to end.  With (L0, g) at the start table and t0 moving the steepest specular coefficient by 0.25: some t in
    {2^-k t0, k = 0..20} satisfies L(theta - t g) <= L0 - c t |g|^2, c = 1e-4; along +g no t of the ladder does."""
    from parallel_reverb_raytracer_amd import capi
    which = getattr(capi, which_name)
    f, ctx, args = setup["fitting"], setup["ctx"], setup["args"][which]
    l0, grads, grad_air, sti = f.sti_loss_and_grad(ctx, setup["start"], *args, which=which)
    again = f.sti_loss_and_grad(ctx, setup["start"], *args, which=which)
    assert l0 == again[0] and grads.tobytes() == again[1].tobytes() and grad_air.tobytes() == again[2].tobytes()      # bit for bit
    assert sti.tobytes() == again[3].tobytes() and l0 == f.sti_loss(ctx, setup["start"], *args, which=which)
    assert l0 > 0 and sti.shape == (2,) and np.isfinite(sti).all() and grad_air.shape == (8,)
    g = grads["specular"].astype(np.float64)
    gg = float((g * g).sum())
    assert gg > 0
    t0 = 0.25 / np.abs(g).max()

    def loss_at(sign, t):
        table = setup["start"].copy()
        table["specular"] = (setup["start"]["specular"].astype(np.float64) + sign * t * g).astype(np.float32)
        return f.sti_loss(ctx, table, *args, which=which)

    ladder = [t0 * 2.0 ** -k for k in range(21)]
    down = [loss_at(-1.0, t) for t in ladder]
    up = [loss_at(+1.0, t) for t in ladder]
    print("sti fit, %s: STI = %s, target %s, L0 = %.9g, |g|^2 = %.6g, t0 = %.6g" % (which_name, sti, args[3], l0, gg, t0))
    for t, a, b in zip(ladder, down, up):
        print("    t = %.3e  L(-g) - L0 = %+.6e  L(+g) - L0 = %+.6e  c t |g|^2 = %.3e" % (t, a - l0, b - l0, C * t * gg))
    assert any(a <= l0 - C * t * gg for t, a in zip(ladder, down))
    assert not any(b <= l0 - C * t * gg for t, b in zip(ladder, up))


def test_two_steps_of_fit_sti_lower_the_loss(setup):
    from parallel_reverb_raytracer_amd import capi
    f, ctx, args = setup["fitting"], setup["ctx"], setup["args"][capi.IR_ALL]
    fitted, record = f.fit_sti(ctx, setup["start"], *args, setup["free"], 2)
    print("sti fit record:", record)
    assert len(record) == 2
    previous = None
    for step in record:
        assert step["descent"] > 0 and step["loss"] <= step["loss_before"] - C * step["descent"] and step["loss"] < step["loss_before"]
        assert previous is None or step["loss_before"] == previous           # a step starts where the last one ended, bit for bit
        previous = step["loss"]
    theta, theta0 = f.coefficients(fitted), f.coefficients(np.ascontiguousarray(setup["start"]))
    assert theta[~setup["free"]].tobytes() == theta0[~setup["free"]].tobytes() and (theta[setup["free"]] != theta0[setup["free"]]).any()
    assert f.sti_loss(ctx, fitted, *args) == record[-1]["loss"] < record[0]["loss_before"]


def test_sti_map_is_the_per_listener_calls_and_the_references_index(setup):
    """listeners.sti_map at two microphones: the loop written out by hand byte for byte, and the reference's index of the downloaded
    histograms within the bar of m carried through the index: |dSTI| <= sum_ki |dSTI/dm_ki| m_bar_ki (to first order; doubled for the
    curvature and the reference's own evaluation) + the bar of the index itself."""
    from parallel_reverb_raytracer_amd import capi, listeners, speech
    ctx, nbins = setup["ctx"], setup["nbins"]
    mic = np.asarray(setup["mic"], dtype=np.float32)
    mics = np.stack([mic, mic + np.float32([0.5, 0.0, -0.25])])
    ctx.reshade(setup["start"], AIR_COEFFICIENTS)
    got = listeners.sti_map(ctx, mics, SPEAKERS, SR, nbins)
    assert got.dtype == np.float64 and got.shape == (2, 2) and np.isfinite(got).all()
    assert listeners.sti_map(ctx, mics, SPEAKERS, SR, nbins).tobytes() == got.tobytes()
    noisy = listeners.sti_map(ctx, mics, SPEAKERS, SR, nbins, snr_db=[10.0] * 7)
    assert (noisy < got).all()
    for i, m in enumerate(mics):                                             # the loop written out by hand
        ctx.relisten(m)
        hist = histogram_of(ctx, m, 0.0, nbins, capi.IR_ALL)
        by_hand = speech.sti(ctx, hist, SR)
        assert got[i].tobytes() == by_hand.tobytes(), i
        ctx.synchronize()
        fw = ref.mtf(hist.cpu().numpy().reshape(16, nbins), SR, ref.STI_FREQS)
        for c in range(2):
            want, _, derivative, scale = ref.speech_index(fw["m"][c * 8:c * 8 + 7], ref.ALPHA_MALE, ref.BETA_MALE)
            bar = 2 * float((np.abs(derivative) * fw["m_bar"][c * 8:c * 8 + 7]).sum()) + ref.speech_index_bars(ref.ALPHA_MALE, ref.BETA_MALE, scale)[0]
            print("sti map: listener %d channel %d: %.15g against the reference's %.15g (bar %.3e)" % (i, c, got[i, c], want, bar))
            assert abs(got[i, c] - want) <= bar
    assert got[0].tobytes() != got[1].tobytes()


def test_the_sensitivity_maps_surface_sums_are_the_surface_gradient(setup):
    """fitting.sti_sensitivity_map: the loss of sti_loss_and_grad(which=IR_DIFFUSE) bit for bit; the binary64 sums of its entries over
    the triangles of a surface are that call's gradient up to rounding.  Both are binary64 sums of the same binary32 terms in different
    orders: the map rounds to float once per triangle (2^-24 |map_t| each), the gradient once per surface (2^-24 |g_s|), and the
    binary64 sums of at most 509 x 24 x 16 terms differ by less than 2^-39 of the sum of the terms' magnitudes — 2^-30 of the sum of
    |map_t| allows for terms that cancel 500-fold inside the triangles."""
    from parallel_reverb_raytracer_amd import capi
    f, ctx, args = setup["fitting"], setup["ctx"], setup["args"][capi.IR_DIFFUSE]
    loss, grads, _, _ = f.sti_loss_and_grad(ctx, setup["start"], *args, which=capi.IR_DIFFUSE)
    map_loss, per_triangle = f.sti_sensitivity_map(ctx, setup["start"], *args)
    assert map_loss == loss and loss > 0
    triangles, nsurfaces = setup["scene"][0], setup["scene"][2].shape[0]
    assert per_triangle.shape == (triangles.shape[0],) and per_triangle["specular"].any() and per_triangle["diffuse"].any()
    sums = f.surface_sums(per_triangle, triangles, nsurfaces)
    magnitudes = per_triangle.copy()
    f.coefficients(magnitudes)[:] = np.abs(f.coefficients(per_triangle))
    total = f.surface_sums(magnitudes, triangles, nsurfaces)
    g = f.coefficients(np.ascontiguousarray(grads)).astype(np.float64)
    miss, allowed = np.abs(sums - g), 2.0 ** -24 * (total + np.abs(g)) + 2.0 ** -30 * total
    print("sti sensitivity map: surface sums at most %.3f of their bar" % float(np.max(miss[allowed > 0] / allowed[allowed > 0], initial=0.0)))
    assert (miss <= allowed).all() and g.any()
    with pytest.raises(ValueError):
        f.sti_sensitivity_map(ctx, setup["start"], *args, which=capi.IR_ALL)
