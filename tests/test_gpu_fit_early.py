"""Fitting with the early reflections in the model (fitting.py and listeners.py with which=IR_ALL) end to end on the GPU: reshade ->
ir_configure_speakers_merged -> exact binning -> rvb_decay_curve -> rvb_decay_params_loss -> rvb_reshade_grad_images + rvb_reshade_grad.
The constructed room of tests/image_edges.py, pair 0, 509 rays x 12 reflections, the stereo speakers of tests/test_gpu_reshade.py.  The
targets are the seven parameters of table_t(seed 12) under IR_ALL, the weights 1 / target^2; all 7 x 16 are available there and at the
start table, table_t(seed 11), which the setup asserts.

A wrong image gradient, or one added to the diffuse part in the wrong place, gives a direction along which the loss does not fall: the
descent test fails then."""
import numpy as np
import pytest

import image_edges as E
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_reshade import SPEAKERS
from test_gpu_reshade_grad import table_t

pytestmark = pytest.mark.gpu

SR, C = 44100.0, 1e-4


def params_of(ctx, mic, table, predelay, nbins, which):
    """the explicit sequence of calls for the parameters of `table` under `which`"""
    import torch
    from parallel_reverb_raytracer_amd import capi
    ctx.reshade(table, AIR_COEFFICIENTS)
    if which == capi.IR_DIFFUSE:
        ctx.ir_configure_speakers(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    else:
        ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], which, False)
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    ctx.ir_accumulate_tensor(predelay, SR, nbins, capi.IR_EXACT, hist)
    return ctx.decay_params_tensor(ctx.decay_curve_tensor(hist), SR)


@pytest.fixture(scope="module")
def setup():
    from parallel_reverb_raytracer_amd import capi, fitting
    scene = E.room()
    mic, src = E.PAIRS[0]
    nrays, nrefl = E.MAIN
    start, goal = table_t(scene[2], seed=11), table_t(scene[2], seed=12)
    ctx = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    ctx.set_scene(scene)
    ctx.keep_paths(True, listener=True)
    ctx.raytrace(mic, src, E.directions(nrays), nrefl, AIR_COEFFICIENTS)
    ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    predelay, latest = ctx.ir_time_range()
    nbins = ctx.ir_bins(latest, predelay, SR)
    targets = params_of(ctx, mic, goal, predelay, nbins, capi.IR_ALL)
    assert targets.shape == (2, 8, 7) and np.isfinite(targets).all(), "a parameter of the target is not available"
    assert np.isfinite(params_of(ctx, mic, start, predelay, nbins, capi.IR_ALL)).all(), "a parameter of the start table is not available"
    weights = (1.0 / targets.astype(np.float64) ** 2).astype(np.float32)
    free = np.zeros((scene[2].shape[0], 16), dtype=bool)
    free[:, :8] = True                                           # the specular coefficients
    args = (AIR_COEFFICIENTS, mic, SPEAKERS, targets, weights, SR, predelay, nbins)
    map_nbins = ctx.ir_bins(latest + 0.02, 0.0, SR)
    yield {"ctx": ctx, "fitting": fitting, "start": start, "free": free, "args": args, "nbins": map_nbins, "mic": mic, "all": {"which": capi.IR_ALL}}
    ctx.close()


def test_the_gradient_is_the_sum_of_its_two_parts_and_a_descent_direction(setup):
    """params_loss_and_grad(which=IR_ALL) twice: bit-equal; its gradient is the rounded binary64 sum of reshade_grad (diffuse
    configuration) and reshade_grad_images for the same w, the image part non-zero.  Then the descent test of
    tests/test_gpu_decay_params_fit.py: some t of the ladder satisfies Armijo along -g, none along +g."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    f, ctx, kw = setup["fitting"], setup["ctx"], setup["all"]
    air, mic, speakers, targets, weights, sr, predelay, nbins = setup["args"]
    l0, grads, grad_air, params = f.params_loss_and_grad(ctx, setup["start"], *setup["args"], **kw)
    again = f.params_loss_and_grad(ctx, setup["start"], *setup["args"], **kw)
    assert l0 == again[0] and grads.tobytes() == again[1].tobytes() and grad_air.tobytes() == again[2].tobytes()      # bit for bit
    assert params.tobytes() == again[3].tobytes() and l0 == f.params_loss(ctx, setup["start"], *setup["args"], **kw)
    assert l0 > 0 and params.shape == (2, 8, 7) and grad_air.shape == (8,)
    # the same w by hand, and the two parts
    ctx.reshade(setup["start"], air)
    ctx.ir_configure_speakers_merged(mic, speakers[0], speakers[1], capi.IR_ALL, False)
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    ctx.ir_accumulate_tensor(predelay, sr, nbins, capi.IR_EXACT, hist)
    curve = ctx.decay_curve_tensor(hist)
    w = torch.empty_like(hist)
    loss, _ = ctx.decay_params_loss_tensor(hist, curve, sr, targets, weights, w)
    assert float(loss.reshape(-1).sum()) == l0
    image_part = ctx.reshade_grad_images(predelay, sr, nbins, w.data_ptr())
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    diffuse_part = ctx.reshade_grad(predelay, sr, nbins, w.data_ptr())
    assert image_part[0]["specular"].any() and image_part[1].any() and diffuse_part[0]["diffuse"].any()
    total = (f.coefficients(image_part[0]).astype(np.float64) + f.coefficients(diffuse_part[0]).astype(np.float64)).astype(np.float32)
    assert total.tobytes() == f.coefficients(np.ascontiguousarray(grads)).tobytes()
    assert (image_part[1].astype(np.float64) + diffuse_part[1].astype(np.float64)).astype(np.float32).tobytes() == grad_air.tobytes()

    g = grads["specular"].astype(np.float64)
    gg = float((g * g).sum())
    assert gg > 0
    t0 = 0.25 / np.abs(g).max()

    def loss_at(sign, t):
        table = setup["start"].copy()
        table["specular"] = (setup["start"]["specular"].astype(np.float64) + sign * t * g).astype(np.float32)
        return f.params_loss(ctx, table, *setup["args"], **kw)

    ladder = [t0 * 2.0 ** -k for k in range(21)]
    down = [loss_at(-1.0, t) for t in ladder]
    up = [loss_at(+1.0, t) for t in ladder]
    print("early fit: L0 = %.9g, |g|^2 = %.6g, t0 = %.6g" % (l0, gg, t0))
    for t, a, b in zip(ladder, down, up):
        print("    t = %.3e  L(-g) - L0 = %+.6e  L(+g) - L0 = %+.6e  c t |g|^2 = %.3e" % (t, a - l0, b - l0, C * t * gg))
    assert any(a <= l0 - C * t * gg for t, a in zip(ladder, down))
    assert not any(b <= l0 - C * t * gg for t, b in zip(ladder, up))


def test_three_steps_of_fit_params_lower_the_loss(setup):
    f, ctx, kw = setup["fitting"], setup["ctx"], setup["all"]
    fitted, record = f.fit_params(ctx, setup["start"], *setup["args"], setup["free"], 3, **kw)
    print("early fit record:", record)
    assert len(record) == 3
    previous = None
    for step in record:
        assert step["descent"] > 0 and step["loss"] <= step["loss_before"] - C * step["descent"] and step["loss"] < step["loss_before"]
        assert previous is None or step["loss_before"] == previous           # a step starts where the last one ended, bit for bit
        previous = step["loss"]
    assert f.params_loss(ctx, fitted, *setup["args"], **kw) == record[-1]["loss"] < record[0]["loss_before"]


def test_the_defaults_take_the_old_path(setup):
    """`which` not given: the bytes of the explicit old sequence of calls — reshade, ir_configure_speakers(IR_DIFFUSE), exact binning,
    curve, loss, reshade_grad — and another loss than IR_ALL's."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    f, ctx = setup["fitting"], setup["ctx"]
    air, mic, speakers, targets, weights, sr, predelay, nbins = setup["args"]
    l0, grads, grad_air, params = f.params_loss_and_grad(ctx, setup["start"], *setup["args"])
    ctx.reshade(setup["start"], air)
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
    ctx.ir_accumulate_tensor(predelay, sr, nbins, capi.IR_EXACT, hist)
    curve = ctx.decay_curve_tensor(hist)
    w = torch.empty_like(hist)
    loss, old_params = ctx.decay_params_loss_tensor(hist, curve, sr, targets, weights, w)
    old = ctx.reshade_grad(predelay, sr, nbins, w.data_ptr())
    assert float(loss.reshape(-1).sum()) == l0 and old_params.tobytes() == params.tobytes()
    assert old[0].tobytes() == grads.tobytes() and old[1].tobytes() == grad_air.tobytes()
    assert f.params_loss(ctx, setup["start"], *setup["args"]) == l0 != f.params_loss(ctx, setup["start"], *setup["args"], **setup["all"])


def test_parameter_map_with_images_is_the_per_listener_calls(setup):
    import torch
    from parallel_reverb_raytracer_amd import capi, listeners
    ctx, nbins = setup["ctx"], setup["nbins"]
    mics = np.stack([E.MICS[0], E.MICS[0] + np.float32([0.25, 0.0, -0.25])])
    ctx.reshade(setup["start"], AIR_COEFFICIENTS)
    got = listeners.parameter_map(ctx, mics, SPEAKERS, SR, nbins, which=capi.IR_ALL)
    assert got.dtype == np.float32 and got.shape == (2, 2, 8, 7) and np.isfinite(got).any()
    for i, m in enumerate(mics):                                             # the loop written out by hand
        ctx.relisten(m)
        ctx.ir_configure_speakers_merged(m, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        hist = torch.zeros((2, 8, nbins), dtype=torch.float32, device="cuda")
        ctx.ir_accumulate_tensor(0.0, SR, nbins, capi.IR_EXACT, hist)
        assert got[i].tobytes() == ctx.decay_params_tensor(ctx.decay_curve_tensor(hist), SR).tobytes(), i
    assert got[0].tobytes() != got[1].tobytes()
    assert got.tobytes() != listeners.parameter_map(ctx, mics, SPEAKERS, SR, nbins).tobytes()      # the diffuse response alone is another
