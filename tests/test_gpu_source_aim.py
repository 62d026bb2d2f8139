"""Aiming a loudspeaker from a kept trace (parallel-reverb-raytracer_amd/fitting.py: aim_loss_and_grad, fit_aim, sti_source_balloon) end to
end on the GPU: set_source_pattern -> reshade -> exact binning -> the loss and w = dL/dH -> rvb_source_grad (+ rvb_source_grad_images) ->
dL/d(direction, shapes).  The setup of tests/test_gpu_speech_fit.py: scenes.cathedral(3000), 509 rays x 24 reflections, the stereo
speakers of tests/test_gpu_reshade.py, a kept trace, the whole response (IR_ALL).

CHAIN RULE.  The directional derivative D = dL/dn . tau along a unit tangent tau of the direction n is held against the central
differences fd(h) = (L(n(h)) - L(n(-h))) / 2h, n(h) = normalize(n + h tau), at h and h / 2.  The tolerance is
    4 |fd(h) - fd(h/2)|  +  4 (nreflections + 20) 2^-24 sum_rb shape_b A_rb |u_r . tau|  +  2 eps_L / h,
the first term the reference's own spread (fd(h/2) misses the derivative by a third of it where the third derivative is steady), the
second the pattern gradient's derived bar (tests/source_grad_cases.py; A from the UNSCALED records of the same trace and the same w, rays
and images), the third the rounding of the two losses of fd(h/2): to first order a loss moves by sum |w| |dH|, and
|dH| <= 4 (nreflections + 16) 2^-24 times the bin's sum of magnitudes, so eps_L = 4 (nreflections + 16) 2^-24 sum_rb |g_rb| A_rb.
The params loss counts C50, C80, D50 and Ts — what the aim of a loudspeaker moves —: the windows of EDT, T20 and T30 move by whole bins,
which makes that part of the loss piecewise smooth, and a difference across a step of the window is no derivative."""
import numpy as np
import pytest

import source_grad_cases as S
from parallel_reverb_raytracer_amd import scenes
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_reshade import SPEAKERS
from test_gpu_reshade_grad import state_terms, table_t

pytestmark = pytest.mark.gpu

SR = 44100.0
NRAYS, NREFL = 509, 24
SHAPES = np.linspace(0.3, 0.9, 8).astype(np.float32)
H = 0.02                                                        # radians: the larger of the two difference steps


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


@pytest.fixture(scope="module")
def setup():
    from parallel_reverb_raytracer_amd import capi, fitting, speech
    scene, info = scenes.cathedral(3000)
    mic, src = info["mic"], info["source"]
    table = table_t(scene[2], seed=11)
    dirs = scenes.sphere_directions(NRAYS, seed=23)
    ctx = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    ctx.set_scene(scene)
    ctx.keep_paths(True, listener=True)
    ctx.raytrace(mic, src, dirs, NREFL, AIR_COEFFICIENTS)
    ctx.reshade(table, AIR_COEFFICIENTS)
    ctx.ir_configure_speakers_merged(mic, SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    predelay, latest = ctx.ir_time_range()                      # of the omnidirectional source: no pattern moves a time
    nbins = ctx.ir_bins(latest, predelay, SR)
    toward = unit(np.asarray(mic, np.float64) - np.asarray(src, np.float64))
    side = unit(np.cross(toward, (0.0, 1.0, 0.0)))
    common = (table, AIR_COEFFICIENTS, mic, SPEAKERS)
    binning = (SR, predelay, nbins)
    # the targets: what the seat hears when the loudspeaker faces it
    _, _, goal_sti = fitting._aim_forward(ctx, "sti", toward, SHAPES, *common, (np.zeros(2), np.ones(2), None), *binning, False, capi.IR_ALL, False)
    _, _, goal_params = fitting._aim_forward(ctx, "params", toward, SHAPES, *common, (np.zeros((2, 8, 7)), np.zeros((2, 8, 7)), ), *binning, False,
                                             capi.IR_ALL, False)
    assert np.isfinite(goal_sti).all()
    param_weights = np.zeros((2, 8, 7))
    param_weights[:, :, [capi.DECAY_C50, capi.DECAY_C80, capi.DECAY_D50, capi.DECAY_TS]] = 1.0
    param_weights[~np.isfinite(goal_params)] = 0.0
    assert param_weights.sum() >= 32
    # (an index a tenth above what facing the seat gives: the loss stays away from its floor, where its slope is all curvature)
    losses = {"sti": (np.minimum(goal_sti + 0.1, 1.0), np.ones(2), None), "params": (np.nan_to_num(goal_params), param_weights)}
    yield {"ctx": ctx, "fitting": fitting, "capi": capi, "common": common, "binning": binning, "losses": losses, "toward": toward, "side": side,
           "dirs": dirs, "mic": mic}
    ctx.close()


def magnitudes(setup, weights):
    """(A_rays [nrays][8], u_rays, A_images [n][8], u_images) for the weights w: the sums of |term| over the UNSCALED records of the kept
    trace, and the departure unit vectors"""
    ctx, capi = setup["ctx"], setup["capi"]
    table, air, mic, speakers = setup["common"]
    sr, predelay, nbins = setup["binning"]
    ctx.synchronize()
    w = weights.cpu().numpy()
    ctx.set_source_pattern(None)
    ctx.reshade(table, air)
    _, absterm, _, _, _ = state_terms(ctx, mic, speakers, predelay, sr, nbins, w)
    a_rays = absterm.reshape(NRAYS, NREFL, 8).sum(axis=1)
    images = ctx.get_raw_images(False)
    _, a_images, _, _, _ = state_terms(ctx, mic, speakers, predelay, sr, nbins, w, images)
    departures = (np.asarray(mic, np.float32)[None, :] - images["position"][:, :3]).astype(np.float32)
    return a_rays, S.unit_twice(setup["dirs"][:, :3]), a_images, S.unit_twice(departures)


@pytest.mark.parametrize("kind", ["params", "sti"])
def test_the_directional_derivative_is_the_central_difference(setup, kind):
    f, ctx, capi = setup["fitting"], setup["ctx"], setup["capi"]
    args = (*setup["common"], setup["losses"][kind], *setup["binning"])
    n = unit(0.3 * setup["toward"] + setup["side"] + (0.0, 0.2, 0.0))         # well off the seat's direction: the loss is not at its floor
    tau = unit(setup["toward"] - (setup["toward"] * n).sum() * n)               # turning toward the seat: the tangent along which the seat hears most change
    assert abs((n * tau).sum()) < 1e-12
    loss, gd, gs, _ = f.aim_loss_and_grad(ctx, kind, n, SHAPES, *args)
    again = f.aim_loss_and_grad(ctx, kind, n, SHAPES, *args)
    assert loss == again[0] and gd.tobytes() == again[1].tobytes() and gs.tobytes() == again[2].tobytes()              # bit for bit
    assert loss == f.aim_loss(ctx, kind, n, SHAPES, *args) and loss > 0 and gd.shape == (3,) and gs.shape == (8,)
    derivative = float((gd * tau).sum())

    def fd(h):
        return (f.aim_loss(ctx, kind, unit(n + h * tau), SHAPES, *args) - f.aim_loss(ctx, kind, unit(n - h * tau), SHAPES, *args)) / (2.0 * h)

    coarse, fine = fd(H), fd(H / 2)
    # the derived rounding terms, from the unscaled records under the same w
    _, weights, _ = f._aim_forward(ctx, kind, n, SHAPES, *args, True, capi.IR_ALL, False)
    a_rays, u_rays, a_images, u_images = magnitudes(setup, weights)
    shapes = SHAPES.astype(np.float64)
    gradient_bar, eps_l = 0.0, 0.0
    for a, u in ((a_rays, u_rays), (a_images, u_images)):
        _, d = S.pattern_geometry(u, n)
        gains = S.gains_of(SHAPES, d).astype(np.float64)
        gradient_bar += 4.0 * (NREFL + 20) * 2.0 ** -24 * float(((a * shapes[None, :]).sum(axis=1) * np.abs(u.astype(np.float64) @ tau)).sum())
        eps_l += 4.0 * (NREFL + 16) * 2.0 ** -24 * float((np.abs(gains) * a).sum())
    tolerance = 4.0 * abs(coarse - fine) + gradient_bar + 2.0 * eps_l / H
    print("aim, %s loss: L = %.9g, dL/dn . tau = %.9g, fd(%.3g) = %.9g, fd(%.3g) = %.9g; tolerance %.3e = 4 x %.3e + %.3e + %.3e"
          % (kind, loss, derivative, H, coarse, H / 2, fine, tolerance, abs(coarse - fine), gradient_bar, 2.0 * eps_l / H))
    assert abs(fine) >= 10.0 * tolerance, "the derivative does not stand clear of the tolerance: the comparison would show nothing"
    assert abs(derivative - fine) <= tolerance


def test_fit_aim_turns_the_loudspeaker_toward_the_seat(setup):
    """From a direction pointing away from the seat, the STI loss falls at
    every accepted step and ends below its start (the target: a tenth above the index with the loudspeaker facing the seat); the shapes stay where they were (free_shapes is off) and the direction a unit vector."""
    f, ctx = setup["fitting"], setup["ctx"]
    args = (*setup["common"], setup["losses"]["sti"], *setup["binning"])
    start = unit(-setup["toward"] + 0.3 * setup["side"])
    first = f.aim_loss(ctx, "sti", start, SHAPES, *args)
    n, shapes, record = f.fit_aim(ctx, "sti", start, SHAPES, *args, steps=3)
    print("aim fit: from %s (toward the seat: %s) to %s; record %s" % (start, setup["toward"], n, record))
    assert len(record) >= 1 and record[0]["loss_before"] == first
    previous = None
    for step in record:
        assert step["descent"] > 0 and step["loss"] <= step["loss_before"] - f.ARMIJO_C * step["descent"] and step["loss"] < step["loss_before"]
        assert previous is None or step["loss_before"] == previous           # a step starts where the last one ended, bit for bit
        previous = step["loss"]
    assert abs((n * n).sum() - 1.0) < 1e-12 and np.array_equal(shapes, SHAPES.astype(np.float64))
    assert (n * setup["toward"]).sum() > (start * setup["toward"]).sum(), "the loudspeaker did not turn toward the seat"
    assert f.aim_loss(ctx, "sti", n, shapes, *args) == record[-1]["loss"] < first


def test_free_shapes_stay_inside_zero_and_one(setup):
    f, ctx = setup["fitting"], setup["ctx"]
    args = (*setup["common"], setup["losses"]["sti"], *setup["binning"])
    start = unit(-setup["toward"] + 0.3 * setup["side"])
    n, shapes, record = f.fit_aim(ctx, "sti", start, SHAPES, *args, steps=2, free_direction=False, free_shapes=True)
    assert len(record) >= 1 and np.array_equal(n, start) and (shapes >= 0).all() and (shapes <= 1).all() and (shapes != SHAPES).any()
    assert all(step["loss"] < step["loss_before"] for step in record)


def test_the_source_balloon_is_the_gains_gradient_by_cell(setup):
    """sti_source_balloon under a table: the loss of sti_loss_and_grad bit for bit, cells that no ray or image leaves through exactly 0,
    and the balloon's total the total of the per-ray and per-image gradients."""
    from test_gpu_source_table import ORIENT, SPREAD
    f, ctx, capi = setup["fitting"], setup["ctx"], setup["capi"]
    table, air, mic, speakers = setup["common"]
    targets, channel_weights, snr = setup["losses"]["sti"]
    ctx.set_source_table(SPREAD, ORIENT[0], ORIENT[1])
    try:
        loss, sti, balloon = f.sti_source_balloon(ctx, table, air, mic, speakers, targets, channel_weights, *setup["binning"])
        want = f.sti_loss_and_grad(ctx, table, air, mic, speakers, targets, channel_weights, *setup["binning"])
        assert loss == want[0] and sti.tobytes() == want[3].tobytes() and loss > 0
        assert balloon.shape == (360, 180, 8) and balloon.dtype == np.float64
        cells = np.count_nonzero(balloon.any(axis=2))
        assert 400 <= cells <= NRAYS + ctx.nimages and cells < 360 * 180
        again = f.sti_source_balloon(ctx, table, air, mic, speakers, targets, channel_weights, *setup["binning"])[2]
        assert balloon.tobytes() == again.tobytes()
    finally:
        ctx.set_source_table(None)
        ctx.reshade(table, air)
