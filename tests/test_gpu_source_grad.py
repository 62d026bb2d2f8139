"""Source-end gradients of a weighted impulse response from a kept trace (rvb_source_grad, rvb_source_grad_images of
include/rvb_capi_source_grad.h; csrc/source_grad_kernels.hip) on a seeded small room.

The reference and its bars: tests/source_grad_cases.py — binary64 numpy from the CPU oracle's trace of the same case with NO directivity,
|gpu - ref| <= 4 (nreflections + 16) 2^-24 A + 1e-30 entry by entry, 4 more roundings for the pattern gradient.  The ground condition is
asserted on the reference alone before every comparison.  Every comparison prints its largest |gpu - ref| / bar
(profiles/source_grad_n1.txt)."""
import ctypes

import numpy as np
import pytest

import source_grad_cases as S
from parallel_reverb_raytracer_amd import directivity
from parallel_reverb_raytracer_amd.dtypes import AIR_COEFFICIENTS

from test_gpu_reshade import SPEAKERS
from test_gpu_reshade_grad import on_device
from test_gpu_source_table import ORIENT, SPREAD

pytestmark = pytest.mark.gpu

SR = S.SR


def new_context(scene):
    from parallel_reverb_raytracer_amd import capi
    c = capi.Context(0)          # raises when librvb_hip.so or the GPU is missing: no fallback
    c.set_scene(scene)
    c.keep_paths(True, listener=True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = new_context(S.room())
    yield c
    c.close()


def bring_up(ctx, c, r, directivity_on=True):
    """The kept trace of `ctx` as case `c` has it, scaled by the case's pattern: the trace, then what the case does to it"""
    scene_table = r["scene"][2]
    if directivity_on:
        ctx.set_source_pattern(c["direction"], c["shapes"])
    if c is S.PAIR_1:
        ctx.set_directions(r["dirs"])
        ctx.trace_pairs([S.MIC, S.OTHER_MIC], [S.SRC, S.OTHER_SRC], c["nrefl"], c["air"])
        ctx.select_pair(1)
    elif c is S.RELISTENED:
        ctx.raytrace(S.MIC, c["src"], r["dirs"], c["nrefl"], c["air"])
        ctx.relisten(c["mic"])
    elif c["table"] is not None or c["dead_band"] is not None:
        ctx.raytrace(c["mic"], c["src"], r["dirs"], c["nrefl"], AIR_COEFFICIENTS)
        assert r["table"].tobytes() != scene_table.tobytes()
        ctx.reshade(r["table"], c["air"])
    else:
        ctx.raytrace(c["mic"], c["src"], r["dirs"], c["nrefl"], c["air"])


def worst_of(got, want, bar):
    return float((np.abs(np.asarray(got, np.float64) - want) / bar).max())


def assert_pattern(got, want, label, what, bands=slice(None)):
    shape_err = worst_of(got["shape"][bands], want["shape"][bands], want["shape_bar"][bands])
    direction_err = worst_of(got["direction"], want["direction"], want["direction_bar"])
    print("source_grad %-44s %s pattern: max |gpu - ref| / bar = %.4f (shapes), %.4f (direction)" % (label, what, shape_err, direction_err))
    assert shape_err <= 1.0 and direction_err <= 1.0, (label, what)
    assert (np.abs(got["shape"].astype(np.float64) - want["shape"]) <= want["shape_bar"]).all(), (label, what)


def compare_rays(ctx, c, r, w_dev, want_pattern=True, want_rows=False):
    """rvb_source_grad under an IR_DIFFUSE configuration, twice (identical bytes), against the reference of the case"""
    from parallel_reverb_raytracer_amd import capi
    S.assert_ground(r)
    ctx.ir_configure_speakers(c["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    out = ctx.source_grad(r["predelay"], SR, r["nbins"], w_dev.data_ptr(), want_pattern=want_pattern, want_rows=want_rows)
    names = [k for k, _ in ctx.last_timings()]
    assert names == ["reshade_grad_weights_kernel", "source_grad_rays_kernel"] + (["source_grad_pattern_kernel", "source_grad_pattern_fold_kernel"] if want_pattern else [])
    again = ctx.source_grad(r["predelay"], SR, r["nbins"], w_dev.data_ptr(), want_pattern=want_pattern, want_rows=want_rows)
    grad = out["grad"].cpu().numpy()
    assert grad.tobytes() == again["grad"].cpu().numpy().tobytes(), c["name"] + ": two calls differ"
    print("source_grad %-44s rays: max |gpu - ref| / bar = %.4f" % (c["name"], worst_of(grad, r["lambda"], r["bar"])))
    assert (np.abs(grad.astype(np.float64) - r["lambda"]) <= r["bar"]).all(), c["name"]
    assert not grad[~r["a"].any(axis=1)].any(), c["name"] + ": a ray without a live record inside the histogram is not exactly 0"
    if want_pattern:
        for k in ("shape", "direction"):
            assert out["pattern"][k].tobytes() == again["pattern"][k].tobytes(), c["name"] + ": two calls differ"
        bands = np.arange(8) != (-1 if c["dead_band"] is None else c["dead_band"])
        assert_pattern(out["pattern"], r["rays_pattern"], c["name"], "rays", bands)
    return out


def merged_list(ctx, c):
    """The host merge of the selected pair's candidates with its direct impulse"""
    from parallel_reverb_raytracer_amd import capi
    if c is not S.PAIR_1:
        return ctx.get_raw_images(False)
    return capi.merge_images(ctx.get_pair_candidates(1), ctx.get_direct(), False)


def compare_images(ctx, c, r, w_dev, ground=True, want_pattern=True, want_rows=False):
    """rvb_source_grad_images under IR_IMAGES and IR_ALL merged configurations (the same bytes), against the reference of the case"""
    from parallel_reverb_raytracer_amd import capi
    if ground:
        S.assert_image_ground(r)
    got = {}
    for which in (capi.IR_IMAGES, capi.IR_ALL):
        count = ctx.ir_configure_speakers_merged(c["mic"], SPEAKERS[0], SPEAKERS[1], which, False)
        assert count == r["images"].shape[0], c["name"]
        got[which] = ctx.source_grad_images(r["predelay"], SR, r["nbins"], w_dev.data_ptr(), want_depart=True, want_pattern=want_pattern, want_rows=want_rows)
    assert [k for k, _ in ctx.last_timings()] == ["source_grad_images_kernel"] + (["source_grad_pattern_kernel", "source_grad_pattern_fold_kernel"] if want_pattern else [])
    out = got[capi.IR_ALL]
    grad, depart = out["grad"].cpu().numpy(), out["depart"].cpu().numpy()
    assert grad.tobytes() == got[capi.IR_IMAGES]["grad"].cpu().numpy().tobytes() and depart.tobytes() == got[capi.IR_IMAGES]["depart"].cpu().numpy().tobytes()
    # the merged list is the oracle's, image by image (the reference speaks of the same images)
    assert np.array_equal(merged_list(ctx, c)["position"], r["images"]["position"]), c["name"]
    print("source_grad %-44s images: max |gpu - ref| / bar = %.4f" % (c["name"], worst_of(grad, r["image_lambda"], r["image_bar"])))
    assert (np.abs(grad.astype(np.float64) - r["image_lambda"]) <= r["image_bar"]).all(), c["name"]
    assert not grad[~r["image_a"].any(axis=1)].any(), c["name"] + ": an image that adds nothing is not exactly 0"
    assert np.array_equal(depart[:, :3], r["images_pattern"]["u"]) and not depart[:, 3].any(), c["name"] + ": the departure unit vectors"
    if want_pattern:
        for k in ("shape", "direction"):
            assert out["pattern"][k].tobytes() == got[capi.IR_IMAGES]["pattern"][k].tobytes(), c["name"]
        assert_pattern(out["pattern"], r["images_pattern"], c["name"], "images")
    return out


@pytest.mark.parametrize("case", S.SHAPE_CASES, ids=[c["name"] for c in S.SHAPE_CASES])
def test_gradient_equals_the_reference_at_the_edges_of_a_wave_and_of_a_tile(ctx, oracle, case):
    """nrays 1, 7, 8, 9, 65: fewer rays than a wave takes, one short, exactly one wave's, one more, several waves with a last one of one
    ray; nreflections 1, 15, 16, 17, 33: a single bounce, a tile one short, exactly one, a second tile of one bounce, a third of one."""
    r = S.reference(oracle, case)
    bring_up(ctx, case, r)
    w_dev = on_device(r["w"])
    compare_rays(ctx, case, r, w_dev)
    compare_images(ctx, case, r, w_dev, ground=case["nrays"] >= 65, want_pattern=case["nrays"] >= 65)


@pytest.mark.parametrize("case", [S.HALF_BINS, S.PREDELAY, S.DEAD_BAND, S.RESHADED, S.RELISTENED, S.PAIR_1], ids=lambda c: c["name"])
def test_gradient_equals_the_reference_at_the_edges_of_the_state(ctx, oracle, case):
    """Half the bins: late records are skipped; a predelay: several records clamp to bin 0; a zero specular coefficient in band 3: every
    entry behind it exactly 0 (A = 0 there, the bar is 1e-30); a reading after rvb_reshade to another table and air, after rvb_relisten,
    and for pair 1 of a two-pair rvb_trace_pairs."""
    r = S.reference(oracle, case)
    try:
        bring_up(ctx, case, r)
        w_dev = on_device(r["w"])
        out = compare_rays(ctx, case, r, w_dev)
        if case is S.DEAD_BAND:
            assert not out["grad"].cpu().numpy()[:, 3].any() and out["pattern"]["shape"][3] == 0
        compare_images(ctx, case, r, w_dev)
    finally:
        ctx.npairs = 1


def test_escaping_rays_get_exactly_zero(oracle):
    """An open room: a ray that leaves before its first hit, or behind its last live record, adds nothing from there on"""
    case = S.ESCAPES
    r = S.reference(oracle, case)
    c = new_context(r["scene"])
    try:
        bring_up(c, case, r)
        w_dev = on_device(r["w"])
        grad = compare_rays(c, case, r, w_dev)["grad"].cpu().numpy()
        assert (~r["live_rays"]).sum() >= 5 and not grad[~r["live_rays"]].any() and grad[r["live_rays"]].any(axis=1).all()
        compare_images(c, case, r, w_dev)
    finally:
        c.close()


def test_a_ray_at_a_null_of_the_pattern_has_its_derivative(ctx, oracle):
    """Shape 1 in bands 2 and 4 and four axis-aligned rays at right angles to the pattern's direction: d == 0 exactly, their gain and so
    every stored volume of theirs in those bands is 0 — and their Lambda is non-zero and within the bar.  Fails for any implementation that
    divides a stored volume by its gain."""
    case = S.NULL
    r = S.reference(oracle, case)
    bring_up(ctx, case, r)
    records = ctx.get_raw_diffuse().reshape(case["nrays"], case["nrefl"])
    assert not records["volume"][:4][:, :, [2, 4]].any() and records["volume"][:4][:, :, 0].any(), "the null rays' records are not silent in bands 2 and 4"
    assert (r["rays_pattern"]["d"][:4] == 0).all()
    w_dev = on_device(r["w"])
    grad = compare_rays(ctx, case, r, w_dev)["grad"].cpu().numpy()
    at_null = grad[:4][:, [2, 4]].astype(np.float64)
    assert (np.abs(at_null) >= 100.0 * r["bar"][:4][:, [2, 4]]).all(), "the derivative at the null is lost"
    assert (np.abs(at_null - r["lambda"][:4][:, [2, 4]]) <= r["bar"][:4][:, [2, 4]]).all()
    compare_images(ctx, case, r, w_dev)


@pytest.mark.parametrize("which_name", ["IR_DIFFUSE", "IR_ALL"])
def test_the_weighted_histogram_is_the_gains_times_the_gradient(ctx, oracle, which_name):
    """H is linear in the gains: sum w * H, in binary64 from rvb_ir_accumulate (RVB_IR_EXACT) of the SCALED records, equals
    sum g * Lambda_gpu (plus the image part for IR_ALL) within the summed bars, g in binary32 per the pattern's CONTRACT."""
    import torch
    from parallel_reverb_raytracer_amd import capi
    which = getattr(capi, which_name)
    case = S.SHAPE_CASES[-2]                                   # 65 x 17
    r = S.reference(oracle, case)
    bring_up(ctx, case, r)
    w_dev = on_device(r["w"])
    rays = compare_rays(ctx, case, r, w_dev)["grad"].cpu().numpy().astype(np.float64)
    gains = r["rays_pattern"]["gains"].astype(np.float64)
    want, bar = (gains * rays).sum(), (np.abs(gains) * r["bar"]).sum()
    if which == capi.IR_ALL:
        images = compare_images(ctx, case, r, w_dev)["grad"].cpu().numpy().astype(np.float64)
        image_gains = r["images_pattern"]["gains"].astype(np.float64)
        want, bar = want + (image_gains * images).sum(), bar + (np.abs(image_gains) * r["image_bar"]).sum()
        ctx.ir_configure_speakers_merged(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    else:
        ctx.ir_configure_speakers(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    hist = torch.zeros((2, 8, r["nbins"]), dtype=torch.float32, device="cuda")
    ctx.ir_accumulate_tensor(r["predelay"], SR, r["nbins"], capi.IR_EXACT, hist)
    ctx.synchronize()
    got = float((hist.cpu().numpy().astype(np.float64) * r["w"].astype(np.float64)).sum())
    print("source_grad identity %-10s sum w H = %.9g, sum g Lambda = %.9g, |difference| / summed bars = %.4f" % (which_name, got, want, abs(got - want) / bar))
    assert abs(want) >= 100.0 * bar, "the identity's two sides are rounding noise"
    assert abs(got - want) <= bar


def normalised_once(v):
    v = np.asarray(v, np.float32).reshape(-1, 3)
    length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(np.float32)
    return (v / length[:, None]).astype(np.float32)


def test_rows_under_a_source_table_and_the_balloon_fold(ctx, oracle):
    """With a table the gains are the table's, Lambda is the same reference's; d_ray_rows / d_image_rows equal oracle.hrtf_index of the
    departure vectors under the orientation, and balloon_gradient sums back to Lambda.sum(0)."""
    from parallel_reverb_raytracer_amd import capi
    case = S.SHAPE_CASES[-2]                                   # 65 x 17
    r = S.reference(oracle, case)
    ctx.set_source_table(SPREAD, ORIENT[0], ORIENT[1])
    try:
        bring_up(ctx, case, r, directivity_on=False)
        w_dev = on_device(r["w"])
        out = compare_rays(ctx, case, r, w_dev, want_pattern=False, want_rows=True)
        rows = out["rows"].cpu().numpy().astype(np.int64)
        want_rows = np.array([oracle.hrtf_index(ORIENT[0], ORIENT[1], v) for v in normalised_once(r["dirs"][:, :3])], np.int64)
        assert np.array_equal(rows, want_rows) and len(set(rows)) >= 60 and (rows < 360 * 180).all()
        balloon = directivity.balloon_gradient(out["grad"], out["rows"])
        total = out["grad"].cpu().numpy().astype(np.float64).sum(axis=0)
        assert np.allclose(balloon.sum(axis=(0, 1)), total, rtol=1e-12, atol=0) and np.count_nonzero(balloon.any(axis=2)) == len(set(rows))
        images = compare_images(ctx, case, r, w_dev, want_pattern=False, want_rows=True)
        departures = (np.asarray(case["mic"], np.float32)[None, :] - r["images"]["position"][:, :3]).astype(np.float32)
        want_rows = np.array([oracle.hrtf_index(ORIENT[0], ORIENT[1], v) for v in normalised_once(departures)], np.int64)
        assert np.array_equal(images["rows"].cpu().numpy().astype(np.int64), want_rows)
        # a pattern gradient is refused while a table shades the records, for rays and for images
        with pytest.raises(capi.RvbError) as e:
            ctx.source_grad_images(r["predelay"], SR, r["nbins"], w_dev.data_ptr(), want_pattern=True)
        assert e.value.code == capi.ERR_STATE and "no polar pattern" in str(e.value)
        ctx.ir_configure_speakers(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        with pytest.raises(capi.RvbError) as e:
            ctx.source_grad(r["predelay"], SR, r["nbins"], w_dev.data_ptr(), want_pattern=True)
        assert e.value.code == capi.ERR_STATE and "no polar pattern" in str(e.value)
    finally:
        ctx.set_source_table(None)


def snapshot(ctx):
    return (ctx.get_raw_diffuse().tobytes(), ctx.get_direct().tobytes(), ctx.get_image_candidates().tobytes(), ctx.ir_time_range())


def test_side_effects(ctx, oracle):
    """The records, the candidates, the direct slot, the time range, the configuration, the next rvb_ir_accumulate and a prepared exact
    list are as they were"""
    import torch
    from parallel_reverb_raytracer_amd import capi
    case = S.SHAPE_CASES[-2]
    r = S.reference(oracle, case)
    bring_up(ctx, case, r)
    w_dev = on_device(r["w"])
    args = (r["predelay"], SR, r["nbins"])

    def histogram():
        hist = torch.zeros((2, 8, r["nbins"]), dtype=torch.float32, device="cuda")
        ctx.ir_accumulate_tensor(*args, capi.IR_EXACT, hist)
        ctx.synchronize()
        return hist.cpu().numpy().tobytes()

    ctx.ir_configure_speakers(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
    before, hist_before = snapshot(ctx), histogram()
    ctx.ir_exact_prepare(*args)
    ctx.source_grad(*args, w_dev.data_ptr(), want_pattern=True)
    folded = torch.zeros((2, 8, r["nbins"]), dtype=torch.float32, device="cuda")
    ctx.ir_exact_fold_tensor(r["nbins"], 0, r["nbins"], folded)           # the prepared list is still there, and still right
    ctx.synchronize()
    assert folded.cpu().numpy().tobytes() == hist_before
    assert snapshot(ctx) == before and histogram() == hist_before
    ctx.ir_configure_speakers_merged(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
    before, hist_before = snapshot(ctx), histogram()
    ctx.ir_exact_prepare(*args)
    ctx.source_grad_images(*args, w_dev.data_ptr(), want_depart=True, want_pattern=True)
    folded.zero_()
    ctx.ir_exact_fold_tensor(r["nbins"], 0, r["nbins"], folded)
    ctx.synchronize()
    assert folded.cpu().numpy().tobytes() == hist_before
    assert snapshot(ctx) == before and histogram() == hist_before


def test_every_refusal_has_its_code_and_writes_nothing(oracle):
    import torch
    from parallel_reverb_raytracer_amd import capi
    case = S.SHAPE_CASES[-2]
    r = S.reference(oracle, case)
    c = capi.Context(0)
    w_dev = on_device(r["w"])
    n = 256                                                     # (more than the rays and the images of the case)
    grad = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda")
    other = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    rows = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    pattern = capi.SourcePatternGrad()
    torch.cuda.synchronize()
    good = [r["predelay"], SR, r["nbins"], w_dev.data_ptr()]

    def refused(code, text, images=False, args=None, outputs=None):
        pattern.shape[:] = [7.0] * 8
        pattern.direction[:] = [7.0] * 4
        args = good if args is None else args
        if outputs is None:
            outputs = [grad.data_ptr(), other.data_ptr(), None, ctypes.byref(pattern)] if images else [grad.data_ptr(), None, ctypes.byref(pattern)]
        rc = (c.lib.rvb_source_grad_images if images else c.lib.rvb_source_grad)(c.handle, *args, *outputs)
        message = c.lib.rvb_last_error(c.handle).decode()
        assert rc == code and text in message and ("rvb_source_grad_images" if images else "rvb_source_grad:") in message, (rc, message)
        torch.cuda.synchronize()
        assert (grad == 7.0).all() and (other == 7.0).all() and (rows == 7).all() and list(pattern.shape) == [7.0] * 8 and list(pattern.direction) == [7.0] * 4

    try:
        for images in (False, True):
            refused(capi.ERR_INVALID, "null weights", images, good[:3] + [None])
            refused(capi.ERR_INVALID, "no bins", images, good[:2] + [0, good[3]])
            refused(capi.ERR_INVALID, "not finite", images, [float("nan")] + good[1:])
            refused(capi.ERR_INVALID, "not finite", images, [good[0], float("inf")] + good[2:])
            refused(capi.ERR_STATE, "nothing traced", images)
        c.set_scene(r["scene"])
        c.set_source_pattern(case["direction"], case["shapes"])
        c.raytrace(case["mic"], case["src"], r["dirs"], case["nrefl"], case["air"])
        for images in (False, True):
            refused(capi.ERR_STATE, "without rvb_keep_paths", images)
        c.keep_paths(True)
        c.raytrace(case["mic"], case["src"], r["dirs"], case["nrefl"], case["air"])
        for images in (False, True):
            refused(capi.ERR_STATE, "no IR configuration", images)
        c.ir_configure_speakers(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        refused(capi.ERR_STATE, "lost its chains", images=True)                     # (not a merged configuration: the first of the two refusals)
        refused(capi.ERR_INVALID, "d_ray_grad overlaps the weights", outputs=[w_dev.data_ptr(), None, None])
        refused(capi.ERR_INVALID, "d_ray_rows overlaps the weights", outputs=[None, w_dev.data_ptr() + 64, None])
        refused(capi.ERR_STATE, "no source table", outputs=[grad.data_ptr(), rows.data_ptr(), None])
        images_list = c.get_raw_images(False)
        c.ir_configure_speakers(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, images_list)
        refused(capi.ERR_STATE, "configured with image sources")
        refused(capi.ERR_STATE, "lost its chains", images=True)
        c.ir_configure_hrtf(case["mic"], np.ones((2, 360, 180, 8), np.float32), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), capi.IR_DIFFUSE, None)
        refused(capi.ERR_STATE, "HRTF", images=False)
        nine = ([(1.0, 0.0, 0.1 * k) for k in range(9)], [0.5] * 9)
        c.ir_configure_speakers(case["mic"], nine[0], nine[1], capi.IR_DIFFUSE, None)
        refused(capi.ERR_STATE, "9 speaker channels")
        c.ir_configure_speakers_merged(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, False)
        refused(capi.ERR_STATE, "RVB_IR_DIFFUSE", images=True)
        c.ir_configure_speakers_merged(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        for at, name in ((0, "d_image_grad"), (1, "d_image_depart")):
            outputs = [None, None, None, None]
            outputs[at] = w_dev.data_ptr() + 4 * (w_dev.numel() - 1)                    # the last float of the weights
            refused(capi.ERR_INVALID, name + " overlaps the weights", images=True, outputs=outputs)
        refused(capi.ERR_STATE, "no source table", images=True, outputs=[grad.data_ptr(), None, rows.data_ptr(), None])
        # without a pattern on the source: a pattern gradient is refused, the gains' gradient is not
        c.set_source_pattern(None)
        c.reshade(None, case["air"])
        c.ir_configure_speakers_merged(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_ALL, False)
        refused(capi.ERR_STATE, "no polar pattern", images=True)
        c.source_grad_images(*good, want_pattern=False)
        c.ir_configure_speakers(case["mic"], SPEAKERS[0], SPEAKERS[1], capi.IR_DIFFUSE, None)
        refused(capi.ERR_STATE, "no polar pattern")
        plain = c.source_grad(*good)["grad"].cpu().numpy()
        assert (np.abs(plain.astype(np.float64) - r["lambda"]) <= r["bar"]).all(), "without directivity the gradient is the same Lambda"
        # keeping off frees the kept trace and its scratch: the calls refuse again
        c.keep_paths(False)
        refused(capi.ERR_STATE, "without rvb_keep_paths")
    finally:
        c.close()
