"""Fitting materials to a measured decay — a decay curve (fit_decay), a table of room acoustic parameters (fit_params) or a target speech
transmission index (fit_sti): the loop a user of rvb_reshade / rvb_reshade_grad would otherwise write (include/rvb_capi.h).

One evaluation never leaves the device but for a few floats per row:

    reshade(table, air)                          the kept trace's records under the candidate materials
    ir_configure_speakers(..., IR_DIFFUSE)       (a re-shade voids the IR configuration)
    ir_accumulate(IR_EXACT) into a zeroed H      the exact mode adds in a fixed order: L is repeatable bit for bit
    decay_curve(H) -> E                          Schroeder integral
    decay_loss(H, E, target, mask) -> L, w       w = dL/dH in H's layout
      or decay_params_loss(H, E, targets, param_weights) -> L, w, params      against measured EDT, T20, T30, C50, C80, D50, Ts
      or mtf(H) -> speech_index -> L, dL/dm -> mtf_adjoint(H, dL/dm) -> w   against a target speech transmission index (fit_sti)
    reshade_grad(w) -> dL/dtable, dL/dair        chain rule through the binning
    (reshade_grad_map(w) -> dL/dtable per TRIANGLE: decay_sensitivity_map, "where on the walls"; needs keep_paths(True, listener=True))

With which=IR_ALL (or IR_IMAGES) the direct sound and the image sources take part (include/rvb_capi_images.h): the second line becomes
ir_configure_speakers_merged(which) — the merged image list made on the device, after a re-shade one gather kernel — and the gradient
is reshade_grad_images(w), for IR_ALL plus reshade_grad(w) under an IR_DIFFUSE configuration: L is a sum over impulses, the two are
added in binary64 and rounded to float once, for surfaces and air alike.

The same losses also have a gradient at the SOURCE end (include/rvb_capi_source_grad.h): source_gradient(w) is dL/d(source gain) per ray
and per image, and with a polar pattern on the source dL/d(direction, shapes) — aim_loss_and_grad, fit_aim ("where to point the
loudspeaker") —, with a source table dL/d(table cell) — sti_source_balloon.  A trial there is set_source_pattern + the same evaluation.

SCOPE: that of rvb_reshade_grad and rvb_reshade_grad_images — a context that holds a trace made with keep_paths(True), the speaker model
with at most 8 channels, no HRTF; by default the diffuse records only (which=IR_DIFFUSE, the calls of earlier versions one for one),
with which=IR_ALL the whole response; the per-triangle map takes IR_DIFFUSE only.  The target and the mask are float32 CUDA tensors [nchannels][8][nbins]
(numpy arrays are uploaded): the target a decay curve in linear energy, the mask >= 0 and zero outside the evaluation range."""
import numpy as np

from . import capi, speech
from .dtypes import SURFACE, aligned_copy


def coefficients(table):
    """The float32 view [nsurfaces][16] of a SURFACE table: a surface's eight specular, then its eight diffuse coefficients."""
    assert table.dtype == SURFACE and table.flags["C_CONTIGUOUS"]
    return table.view(np.float32).reshape(table.shape[0], 16)


def _on_device(x, shape):
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == tuple(shape), "target / mask: float32 [nchannels][8][nbins]"
    return x


def _configure(ctx, mic, speakers, which, remove_direct):
    if which == capi.IR_DIFFUSE:
        ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    else:
        ctx.ir_configure_speakers_merged(mic, speakers[0], speakers[1], which, remove_direct)


def _histogram_and_curve(ctx, table, air, mic, speakers, sample_rate, predelay, nbins, which=capi.IR_DIFFUSE, remove_direct=False):
    """The front of every evaluation: re-shade, bin exactly, integrate.  (hist, curve), tensors [nchannels][8][nbins]; the curve is
    enqueued on the context's stream, where the loss calls find it."""
    import torch
    assert which in (capi.IR_DIFFUSE, capi.IR_IMAGES, capi.IR_ALL)
    ctx.reshade(table, air)
    _configure(ctx, mic, speakers, which, remove_direct)
    hist = torch.zeros((ctx.nchannels, 8, int(nbins)), dtype=torch.float32, device="cuda")
    curve = torch.empty_like(hist)
    ctx.ir_accumulate_tensor(predelay, sample_rate, nbins, capi.IR_EXACT, hist)      # (waits for torch's stream: the zero fill, the uploads)
    ctx.decay_curve(hist.data_ptr(), ctx.nchannels * 8, nbins, curve.data_ptr())
    return hist, curve


def _gradient(ctx, mic, speakers, predelay, sample_rate, nbins, weights, which, remove_direct):
    """(grad_surfaces, grad_air) of the configuration that _histogram_and_curve left: reshade_grad for the diffuse records,
    reshade_grad_images for the images, for IR_ALL their binary64 sum rounded to float once."""
    if which == capi.IR_DIFFUSE:
        return ctx.reshade_grad(predelay, sample_rate, nbins, weights.data_ptr())
    grads, grad_air = ctx.reshade_grad_images(predelay, sample_rate, nbins, weights.data_ptr())
    if which == capi.IR_IMAGES:
        return grads, grad_air
    ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    diffuse, diffuse_air = ctx.reshade_grad(predelay, sample_rate, nbins, weights.data_ptr())
    total = np.zeros_like(grads)
    coefficients(total)[:] = (coefficients(grads).astype(np.float64) + coefficients(diffuse).astype(np.float64)).astype(np.float32)
    return total, (grad_air.astype(np.float64) + diffuse_air.astype(np.float64)).astype(np.float32)


def _forward(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, want_weights, which=capi.IR_DIFFUSE,
             remove_direct=False):
    """The evaluation up to the loss: (loss, curve, weights), the tensors [nchannels][8][nbins]; weights = dL/dH, or None."""
    import torch
    shape = (ctx.nchannels, 8, int(nbins))
    nrows = ctx.nchannels * 8
    target, mask = _on_device(target, shape), _on_device(mask, shape)
    hist, curve = _histogram_and_curve(ctx, table, air, mic, speakers, sample_rate, predelay, nbins, which, remove_direct)
    weights = torch.empty_like(hist) if want_weights else None
    loss_rows = ctx.decay_loss(hist.data_ptr(), curve.data_ptr(), target.data_ptr(), mask.data_ptr(), nrows, nbins,
                               capi.DECAY_NORMALISED if normalised else 0, weights.data_ptr() if want_weights else None)
    return float(loss_rows.sum()), curve, weights


def _evaluate(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, want_grad, which=capi.IR_DIFFUSE,
              remove_direct=False):
    loss, curve, weights = _forward(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, want_grad, which,
                                    remove_direct)
    if not want_grad:
        return loss, None, None, None
    times = ctx.decay_times(curve.data_ptr(), ctx.nchannels * 8, nbins, sample_rate).reshape(ctx.nchannels, 8)
    grads, grad_air = _gradient(ctx, mic, speakers, predelay, sample_rate, nbins, weights, which, remove_direct)
    return loss, grads, grad_air, times


def decay_loss_and_grad(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised=True, which=capi.IR_DIFFUSE,
                        remove_direct=False):
    """(loss, grad_surfaces, grad_air, times) of the kept trace in `ctx` under the surface table `table` and the air coefficients `air`:
    loss = sum over the rows of sum_k mask (ln E - ln target - the difference at bin 0 if normalised)^2 (rvb_decay_loss), its gradient as a
    SURFACE array and a float32[8] (rvb_reshade_grad), and the T30 of every row of the current curve, float32 [nchannels][8], NaN where
    the curve does not reach -35 dB.  speakers = (directions, coefficients).  which: IR_DIFFUSE, IR_IMAGES or IR_ALL (with the direct
    sound unless remove_direct), see the module text.  Leaves the context re-shaded with `table`."""
    return _evaluate(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, True, which, remove_direct)


def decay_loss(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised=True, which=capi.IR_DIFFUSE,
               remove_direct=False):
    """The loss of decay_loss_and_grad alone (no weights, no gradient): what a line search evaluates."""
    return _evaluate(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, False, which, remove_direct)[0]


def decay_sensitivity_map(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised=True, which=capi.IR_DIFFUSE):
    """(loss, map): the loss of decay_loss_and_grad, bit for bit, and its gradient per TRIANGLE (rvb_reshade_grad_map) as a SURFACE array
    [ntriangles] — where on the walls a change of the coefficients changes this decay at this microphone; entry t belongs to triangle t of
    the scene given to set_scene.  Needs a trace kept with keep_paths(True, listener=True).  Leaves the context re-shaded with `table`.
    The map is that of the diffuse records: ValueError for which != IR_DIFFUSE (the image sources have no per-triangle gradient)."""
    if which != capi.IR_DIFFUSE:
        raise ValueError("decay_sensitivity_map: which must be IR_DIFFUSE (rvb_reshade_grad_map takes the diffuse records only)")
    loss, _, weights = _forward(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, True)
    per_triangle = ctx.reshade_grad_map(predelay, sample_rate, nbins, weights.data_ptr())
    return loss, np.ascontiguousarray(per_triangle.cpu().numpy()).view(SURFACE).reshape(-1)


def surface_sums(map, triangles, nsurfaces):
    """The binary64 sums [nsurfaces][16] of a sensitivity map's entries over the triangles of every surface (`triangles`: the scene's
    triangle array): up to rounding the gradient per surface, coefficients(grad_surfaces) of decay_loss_and_grad."""
    out = np.zeros((int(nsurfaces), 16), np.float64)
    np.add.at(out, np.asarray(triangles["surface"], np.int64), coefficients(np.ascontiguousarray(map)).astype(np.float64))
    return out


ARMIJO_C = 1e-4
MAX_HALVINGS = 30


def _armijo(state, steps, loss_and_grad, loss_only, steepest_of, trial_of):
    """The Armijo loop that every fit here runs, on a state the caller moves: loss_and_grad(state) -> (loss, g), loss_only(state) -> loss,
    steepest_of(g) the largest |g|, trial_of(state, g, t) -> (trial state, descent = g.(theta - theta(t))).  A trial is accepted when
    descent > 0 and L(trial) <= L - c descent, c = 1e-4; t halves until then, at most 30 times, and a step that is never accepted ends
    the loop.  The first t is 0.25 / steepest; later steps start from twice the last accepted t.  Returns (state, record)."""
    record = []
    t = None
    for _ in range(int(steps)):
        loss, g = loss_and_grad(state)
        steepest = steepest_of(g)
        if not steepest > 0 or not np.isfinite(steepest):
            break
        t = 0.25 / steepest if t is None else 2.0 * t
        accepted = None
        for halvings in range(MAX_HALVINGS + 1):
            trial, descent = trial_of(state, g, t)
            trial_loss = loss_only(trial)
            if descent > 0 and trial_loss <= loss - ARMIJO_C * descent:
                accepted = (trial, trial_loss, descent, halvings)
                break
            t *= 0.5
        if accepted is None:
            break
        state = accepted[0]
        record.append({"loss_before": loss, "loss": accepted[1], "step": t, "halvings": accepted[3], "descent": accepted[2]})
    return state, record


def _fit(ctx, table, air, free, steps, lower, upper, loss_and_grad, loss_only):
    """The projected-gradient / Armijo loop of fit_decay and fit_params: loss_and_grad(table) -> (loss, grad_surfaces),
    loss_only(table) -> loss."""
    table = aligned_copy(np.ascontiguousarray(table, dtype=SURFACE))
    free = np.asarray(free, dtype=bool).reshape(table.shape[0], 16)

    def masked(candidate):
        loss, grads = loss_and_grad(candidate)
        return loss, np.where(free, coefficients(np.ascontiguousarray(grads)), np.float32(0.0)).astype(np.float64)

    def trial_of(current, g, t):
        theta = coefficients(current)
        trial = aligned_copy(current)
        moved = np.clip(theta.astype(np.float64) - t * g, lower, upper).astype(np.float32)
        coefficients(trial)[free] = moved[free]
        return trial, float((g * (theta.astype(np.float64) - coefficients(trial).astype(np.float64))).sum())

    table, record = _armijo(table, steps, masked, loss_only, lambda g: np.abs(g).max(), trial_of)
    ctx.reshade(table, air)
    return table, record


def fit_decay(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, free, steps, lower=0.01, upper=0.99,
              normalised=True, which=capi.IR_DIFFUSE, remove_direct=False):
    """Projected gradient descent on the coefficients of `table` that the boolean array `free` ([nsurfaces][16], the layout of
    `coefficients`) marks; every other entry keeps its bits.  A step from theta with gradient g tries theta(t) = clip(theta - t g, lower,
    upper) and halves t until the Armijo condition L(theta(t)) <= L(theta) - c g.(theta - theta(t)) holds, c = 1e-4 (without clipping
    that is L - c t |g|^2); a step that never satisfies it within 30 halvings ends the fit.  Only steps that satisfy it are taken.  The
    first t moves the steepest coefficient by 0.25; later steps start from twice the last accepted t.

    Returns (table, record): the fitted table (a copy) and one dict per accepted step — loss_before, loss, step (the accepted t),
    halvings, descent (g.(theta - theta(t))).  The air is held fixed.  Scope: see the module text."""
    args = (air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised)
    return _fit(ctx, table, air, free, steps, lower, upper,
                lambda candidate: _evaluate(ctx, candidate, *args, True, which, remove_direct)[:2],
                lambda candidate: _evaluate(ctx, candidate, *args, False, which, remove_direct)[0])


# ---- fitting to a table of measured room acoustic parameters (rvb_decay_params_loss) ------------------------------------------------

def _params_forward(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, want_weights, which=capi.IR_DIFFUSE,
                    remove_direct=False):
    """The evaluation up to the loss: (loss, params, weights), weights = dL/dH as a tensor [nchannels][8][nbins], or None."""
    import torch
    hist, curve = _histogram_and_curve(ctx, table, air, mic, speakers, sample_rate, predelay, nbins, which, remove_direct)
    weights = torch.empty_like(hist) if want_weights else None
    shape = (ctx.nchannels * 8, capi.DECAY_NPARAMS)
    loss_rows, params = ctx.decay_params_loss(hist.data_ptr(), curve.data_ptr(), ctx.nchannels * 8, nbins, sample_rate,
                                              np.asarray(targets, dtype=np.float32).reshape(shape),
                                              np.asarray(param_weights, dtype=np.float32).reshape(shape), weights.data_ptr() if want_weights else None)
    return float(loss_rows.sum()), params.reshape(ctx.nchannels, 8, capi.DECAY_NPARAMS), weights


def _evaluate_params(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, want_grad, which=capi.IR_DIFFUSE,
                     remove_direct=False):
    loss, params, weights = _params_forward(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, want_grad, which,
                                            remove_direct)
    if not want_grad:
        return loss, None, None, params
    grads, grad_air = _gradient(ctx, mic, speakers, predelay, sample_rate, nbins, weights, which, remove_direct)
    return loss, grads, grad_air, params


def params_loss_and_grad(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, which=capi.IR_DIFFUSE,
                         remove_direct=False):
    """(loss, grad_surfaces, grad_air, params) of the kept trace in `ctx` under the surface table `table` and the air coefficients `air`
    against a measured table: targets and param_weights are [nchannels][8][7] (columns capi.DECAY_EDT .. capi.DECAY_TS: EDT, T20, T30 in
    seconds, C50, C80 in dB, D50, Ts in seconds); loss = sum over the rows and parameters of param_weights (model - targets)^2
    (rvb_decay_params_loss: a weight of 0 leaves a parameter out, 1 / target^2 gives relative errors, a parameter that the model's curve
    does not yield adds nothing), its gradient as a SURFACE array and a float32[8] (rvb_reshade_grad), and the model's parameters, float32
    [nchannels][8][7], NaN where not available.  speakers = (directions, coefficients).  Leaves the context re-shaded with `table`.

    SCOPE: see the module text.  By default (which=IR_DIFFUSE) the diffuse records only: the early-energy parameters C50, C80, D50 and Ts
    are then those of the DIFFUSE response, without the direct sound and the image sources that a measurement's early energy holds.
    which=IR_ALL puts them into the model's curve (remove_direct: without the direct sound) and into the gradient
    (rvb_reshade_grad_images): what a fit to measured clarity, definition or EDT wants."""
    return _evaluate_params(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, True, which, remove_direct)


def params_loss(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, which=capi.IR_DIFFUSE, remove_direct=False):
    """The loss of params_loss_and_grad alone (no weights, no gradient), bit for bit: what a line search evaluates."""
    return _evaluate_params(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, False, which, remove_direct)[0]


def fit_params(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, free, steps, lower=0.01, upper=0.99,
               which=capi.IR_DIFFUSE, remove_direct=False):
    """fit_decay's loop — projected gradient descent with Armijo steps on the coefficients that `free` marks, the same record — on the
    loss of params_loss_and_grad: calibrates materials to a table of measured T30, EDT, C80, ...  Returns (table, record).  The air is
    held fixed.  Scope: see params_loss_and_grad."""
    args = (air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins)
    return _fit(ctx, table, air, free, steps, lower, upper,
                lambda candidate: _evaluate_params(ctx, candidate, *args, True, which, remove_direct)[:2],
                lambda candidate: _evaluate_params(ctx, candidate, *args, False, which, remove_direct)[0])


# ---- fitting to a target speech transmission index (include/rvb_capi_speech.h) --------------------------------------------------------

def _histogram(ctx, table, air, mic, speakers, sample_rate, predelay, nbins, which, remove_direct):
    """_histogram_and_curve without the curve: re-shade, bin exactly."""
    import torch
    assert which in (capi.IR_DIFFUSE, capi.IR_IMAGES, capi.IR_ALL)
    ctx.reshade(table, air)
    _configure(ctx, mic, speakers, which, remove_direct)
    hist = torch.zeros((ctx.nchannels, 8, int(nbins)), dtype=torch.float32, device="cuda")
    ctx.ir_accumulate_tensor(predelay, sample_rate, nbins, capi.IR_EXACT, hist)      # (waits for torch's stream: the zero fill)
    return hist


def _sti_forward(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, want_weights, which, remove_direct):
    """(loss, sti, hist, weights): L = sum_c channel_weights_c (STI_c - targets_c)^2 and, if wanted, w = dL/dH as a tensor of H's shape:
    dL/dm = 2 weight (STI - target) dSTI/dm per channel (rvb_speech_index), then rvb_mtf_adjoint."""
    import torch
    hist = _histogram(ctx, table, air, mic, speakers, sample_rate, predelay, nbins, which, remove_direct)
    m = speech.mtf_rows(ctx, hist, sample_rate)
    targets = np.asarray(targets, dtype=np.float64).reshape(ctx.nchannels)
    channel_weights = np.asarray(channel_weights, dtype=np.float64).reshape(ctx.nchannels)
    if not want_weights:
        sti = speech.index_of_rows(m, snr_db)
        return float((channel_weights * (sti - targets) ** 2).sum()), sti, hist, None
    sti, derivative = speech.index_of_rows(m, snr_db, want_derivative=True)
    coeffs = (2.0 * channel_weights * (sti - targets))[:, None, None] * derivative.reshape(ctx.nchannels, 8, -1)
    weights = torch.empty_like(hist)
    ctx.mtf_adjoint(hist.data_ptr(), ctx.nchannels * 8, nbins, sample_rate, speech.STI_FREQS, coeffs, weights.data_ptr())
    return float((channel_weights * (sti - targets) ** 2).sum()), sti, hist, weights


def _evaluate_sti(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, want_grad, which, remove_direct):
    loss, sti, _, weights = _sti_forward(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, want_grad,
                                         which, remove_direct)
    if not want_grad:
        return loss, None, None, sti
    grads, grad_air = _gradient(ctx, mic, speakers, predelay, sample_rate, nbins, weights, which, remove_direct)
    return loss, grads, grad_air, sti


def sti_loss_and_grad(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db=None, which=capi.IR_ALL,
                      remove_direct=False):
    """(loss, grad_surfaces, grad_air, sti) of the kept trace in `ctx` under the surface table `table` and the air coefficients `air`:
    loss = sum_c channel_weights_c (STI_c - targets_c)^2 over the channels, STI_c the speech transmission index of channel c
    (speech.sti: male-speech weights, snr_db seven signal-to-noise ratios in dB or None), its gradient as a SURFACE array and a
    float32[8], and the model's indices float64 [nchannels].  The chain: dSTI/dm (rvb_speech_index), rvb_mtf_adjoint, then the
    gradient of params_loss_and_grad.  The whole response by default (which=IR_ALL): an index without the direct sound is not the
    seat's.  A channel with an empty band has a NaN index and makes the loss NaN.  Leaves the context re-shaded with `table`.
    SCOPE: see the module text."""
    return _evaluate_sti(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, True, which, remove_direct)


def sti_loss(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db=None, which=capi.IR_ALL,
             remove_direct=False):
    """The loss of sti_loss_and_grad alone (no weights, no gradient), bit for bit: what a line search evaluates."""
    return _evaluate_sti(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, False, which, remove_direct)[0]


def fit_sti(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, free, steps, lower=0.01, upper=0.99,
            snr_db=None, which=capi.IR_ALL, remove_direct=False):
    """fit_decay's loop — projected gradient descent with Armijo steps on the coefficients that `free` marks, the same record — on the
    loss of sti_loss_and_grad: materials toward a target speech transmission index.  Returns (table, record).  The air is held fixed."""
    args = (air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db)
    return _fit(ctx, table, air, free, steps, lower, upper,
                lambda candidate: _evaluate_sti(ctx, candidate, *args, True, which, remove_direct)[:2],
                lambda candidate: _evaluate_sti(ctx, candidate, *args, False, which, remove_direct)[0])


def sti_sensitivity_map(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db=None, which=capi.IR_DIFFUSE):
    """(loss, map): the loss of sti_loss_and_grad(which=IR_DIFFUSE), bit for bit, and its gradient per TRIANGLE (rvb_reshade_grad_map) as
    a SURFACE array [ntriangles] — where on the walls treatment buys intelligibility at this microphone.  Needs a trace kept with
    keep_paths(True, listener=True).  The map is that of the diffuse records: ValueError for which != IR_DIFFUSE."""
    if which != capi.IR_DIFFUSE:
        raise ValueError("sti_sensitivity_map: which must be IR_DIFFUSE (rvb_reshade_grad_map takes the diffuse records only)")
    loss, _, _, weights = _sti_forward(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, True,
                                       capi.IR_DIFFUSE, False)
    per_triangle = ctx.reshade_grad_map(predelay, sample_rate, nbins, weights.data_ptr())
    return loss, np.ascontiguousarray(per_triangle.cpu().numpy()).view(SURFACE).reshape(-1)


# ---- the source end: aim and polar pattern (include/rvb_capi_source_grad.h) ------------------------------------------------------------

def source_gradient(ctx, weights, mic, speakers, sample_rate, predelay, nbins, which=capi.IR_DIFFUSE, want_pattern=False, want_rows=False):
    """dL/d(source gain) of L = sum weights * H for the configuration that an evaluation here left (the context configured with `which`,
    weights = dL/dH a float32 CUDA tensor [nchannels][8][nbins]): a dict with "rays" — capi.Context.source_grad's result, "grad" [nrays][8]
    and, if asked, "rows" — for the diffuse part (None for which=IR_IMAGES), "images" — source_grad_images' result with "depart" — for
    which != IR_DIFFUSE (None otherwise), and "pattern" {"shape" float64 [8], "direction" float64 [3]}: the parts' pattern gradients added in
    binary64 (want_pattern; the direction is the derivative for a free 3-vector).  For IR_ALL the image part is taken first, under the
    merged configuration; the context is left configured with IR_DIFFUSE then, as the material gradients leave it."""
    out = {"rays": None, "images": None, "pattern": None}
    parts = []
    if which != capi.IR_DIFFUSE:
        out["images"] = ctx.source_grad_images(predelay, sample_rate, nbins, weights.data_ptr(), want_depart=True, want_rows=want_rows, want_pattern=want_pattern)
        parts.append(out["images"]["pattern"])
        if which == capi.IR_ALL:
            ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
    if which != capi.IR_IMAGES:
        out["rays"] = ctx.source_grad(predelay, sample_rate, nbins, weights.data_ptr(), want_rows=want_rows, want_pattern=want_pattern)
        parts.append(out["rays"]["pattern"])
    if want_pattern:
        out["pattern"] = {k: sum(p[k].astype(np.float64) for p in parts) for k in ("shape", "direction")}
    return out


def _aim_forward(ctx, kind, direction, shapes, table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, want_weights, which, remove_direct):
    """set_source_pattern + the evaluation of loss `kind` up to the loss, through the forward of the material fits: (loss, weights, extra),
    extra the times' place holder None ("decay"), the parameters ("params") or the indices ("sti")."""
    ctx.set_source_pattern(direction, shapes)
    if kind == "decay":
        target, mask, normalised = loss_args
        loss, _, weights = _forward(ctx, table, air, mic, speakers, target, mask, sample_rate, predelay, nbins, normalised, want_weights, which, remove_direct)
        return loss, weights, None
    if kind == "params":
        targets, param_weights = loss_args
        loss, params, weights = _params_forward(ctx, table, air, mic, speakers, targets, param_weights, sample_rate, predelay, nbins, want_weights, which,
                                                remove_direct)
        return loss, weights, params
    if kind == "sti":
        targets, channel_weights, snr_db = loss_args
        loss, sti, _, weights = _sti_forward(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, want_weights,
                                             which, remove_direct)
        return loss, weights, sti
    raise ValueError("aim: kind must be 'decay', 'params' or 'sti'")


def aim_loss(ctx, kind, direction, shapes, table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, which=capi.IR_ALL, remove_direct=False):
    """The loss of aim_loss_and_grad alone, bit for bit: what a line search evaluates."""
    return _aim_forward(ctx, kind, direction, shapes, table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, False, which, remove_direct)[0]


def aim_loss_and_grad(ctx, kind, direction, shapes, table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, which=capi.IR_ALL,
                      remove_direct=False):
    """(loss, grad_direction float64 [3], grad_shapes float64 [8], extra) of the kept trace in `ctx` with the polar pattern (direction,
    shapes — a scalar or eight values) on the source, under the table `table` and the air `air`.  kind and loss_args name the loss:
    "decay" (target, mask, normalised) — decay_loss_and_grad's —, "params" (targets, param_weights) — params_loss_and_grad's —, "sti"
    (targets, channel_weights, snr_db) — sti_loss_and_grad's; extra is None, the parameters or the indices.  grad_direction is the
    derivative for the pattern's unit vector taken as a free 3-vector (rvb_source_pattern_grad): project it onto the tangent plane of the
    direction to turn the source.  One evaluation costs the forward and one or two gradient sweeps, whatever the number of free
    parameters.  Leaves the pattern set and the context re-shaded with it."""
    loss, weights, extra = _aim_forward(ctx, kind, direction, shapes, table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, True, which,
                                        remove_direct)
    pattern = source_gradient(ctx, weights, mic, speakers, sample_rate, predelay, nbins, which, want_pattern=True)["pattern"]
    return loss, pattern["direction"], pattern["shape"], extra


def _unit(v):
    v = np.asarray(v, dtype=np.float64).reshape(3)
    return v / np.sqrt((v * v).sum())


def fit_aim(ctx, kind, direction, shapes, table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, steps, free_direction=True,
            free_shapes=False, which=capi.IR_ALL, remove_direct=False):
    """Projected gradient descent with fit_decay's Armijo loop on the polar pattern of the source: the direction (free_direction) moves
    along the gradient's projection onto its tangent plane and is renormalised after each step, the shapes (free_shapes) are clipped to
    [0, 1].  Each trial is set_source_pattern + reshade + the loss of aim_loss_and_grad.  Returns (direction float64 [3], shapes float64
    [8], record), the record as fit_decay's; leaves the fitted pattern set and the context re-shaded with it."""
    args = (table, air, mic, speakers, loss_args, sample_rate, predelay, nbins, which, remove_direct)
    state = (_unit(direction), np.broadcast_to(np.asarray(shapes, dtype=np.float64).reshape(-1), (8,)).copy())

    def loss_and_grad(current):
        n, shape = current
        loss, gd, gs, _ = aim_loss_and_grad(ctx, kind, n, shape, *args)
        tangent = gd - (gd * n).sum() * n if free_direction else np.zeros(3)
        return loss, np.concatenate([tangent, gs if free_shapes else np.zeros(8)])

    def trial_of(current, g, t):
        n, shape = current
        trial = (_unit(n - t * g[:3]), np.clip(shape - t * g[3:], 0.0, 1.0))
        return trial, float((g[:3] * (n - trial[0])).sum() + (g[3:] * (shape - trial[1])).sum())

    (n, shape), record = _armijo(state, steps, loss_and_grad, lambda current: aim_loss(ctx, kind, current[0], current[1], *args),
                                 lambda g: np.abs(g).max(), trial_of)
    aim_loss(ctx, kind, n, shape, *args)
    return n, shape, record


def sti_source_balloon(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db=None, which=capi.IR_ALL,
                       remove_direct=False):
    """(loss, sti, balloon): the loss and the indices of sti_loss_and_grad for a source with the TABLE set on the context
    (set_source_table), and balloon float64 [360][180][8] = dL/dtable[a][e][b]: what a change of the loudspeaker's gain in every departure
    cell and band does to the loss (targets of 1 make it "which cells carry the intelligibility of this seat").  The rays' and the images'
    gain derivatives are added up by table row (directivity.balloon_gradient); cells that no ray or image leaves through are 0."""
    from .directivity import balloon_gradient
    loss, sti, _, weights = _sti_forward(ctx, table, air, mic, speakers, targets, channel_weights, sample_rate, predelay, nbins, snr_db, True, which,
                                         remove_direct)
    parts = source_gradient(ctx, weights, mic, speakers, sample_rate, predelay, nbins, which, want_rows=True)
    balloon = np.zeros((360, 180, 8), dtype=np.float64)
    for part in (parts["images"], parts["rays"]):
        if part is not None:
            balloon += balloon_gradient(part["grad"], part["rows"])
    return loss, sti, balloon
