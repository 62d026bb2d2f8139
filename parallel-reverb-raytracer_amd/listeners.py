"""Decay times over a grid of listeners: the loop a user of rvb_relisten would otherwise write (include/rvb_capi.h).

One source, many microphones: the context holds ONE trace made with keep_paths(True, listener=True); per listener

    relisten(mic)                                the kept trace's records with the new microphone: no path stage
    ir_configure_speakers(..., IR_DIFFUSE)       (a relisten voids the IR configuration)
      or ir_configure_speakers_merged(which)     which = IR_ALL / IR_IMAGES: the direct sound and the image sources take part, their
                                                 merged list made on the device (include/rvb_capi_images.h)
    ir_accumulate(mode) into a zeroed H          the exact mode adds in a fixed order: the times are repeatable bit for bit
    decay_curve(H) -> E                          Schroeder integral
    decay_times(E)                               T30 (db_begin, db_end = -5, -35), EDT (0, -10), ...           (decay_map)
      or decay_params(E)                         EDT, T20, T30, C50, C80, D50, Ts in one sweep                (parameter_map)
    or, from H itself, mtf(H) and the index      the speech transmission index (include/rvb_capi_speech.h)    (sti_map)

and nothing leaves the device but eight (or 56) floats per channel.  SCOPE: that of rvb_relisten — a single-pair trace on one context
—, the speaker model, and by default the diffuse records only (which=IR_DIFFUSE; with IR_ALL the early-energy parameters are those of
the whole response, direct sound and early reflections included); the histogram starts at time 0 (no predelay), so that every listener's
bins mean the same times."""
import numpy as np

from . import capi, speech


def _histograms(ctx, mics, speakers, sample_rate, nbins, mode, which=capi.IR_DIFFUSE, remove_direct=False):
    """Per listener (i, hist): the histogram [nchannels][8][nbins] of the kept trace heard at mics[i], enqueued on the context's stream.
    One histogram serves all listeners."""
    import torch
    nchannels = len(speakers[1])
    hist = torch.empty((nchannels, 8, int(nbins)), dtype=torch.float32, device="cuda")
    for i, mic in enumerate(mics):
        ctx.relisten(mic)
        if which == capi.IR_DIFFUSE:
            ctx.ir_configure_speakers(mic, speakers[0], speakers[1], capi.IR_DIFFUSE, None)
        else:
            ctx.ir_configure_speakers_merged(mic, speakers[0], speakers[1], which, remove_direct)
        hist.zero_()
        ctx.ir_accumulate_tensor(0.0, sample_rate, nbins, mode, hist)       # (waits for torch's stream: the zero fill)
        yield i, hist


def _curves(ctx, mics, speakers, sample_rate, nbins, mode, which=capi.IR_DIFFUSE, remove_direct=False):
    """Per listener (i, curve): the decay curve [nchannels][8][nbins] of the kept trace heard at mics[i], enqueued on the context's stream.
    One histogram and one curve serve all listeners."""
    import torch
    curve = None
    for i, hist in _histograms(ctx, mics, speakers, sample_rate, nbins, mode, which, remove_direct):
        if curve is None:
            curve = torch.empty_like(hist)
        ctx.decay_curve(hist.data_ptr(), hist.shape[0] * 8, nbins, curve.data_ptr())
        yield i, curve


def decay_map(ctx, mics, speakers, sample_rate, nbins, db_begin=-5.0, db_end=-35.0, mode=capi.IR_EXACT):
    """float32 [nlisteners][nchannels][8]: the reverberation time in seconds of every (channel, band) row at every microphone of `mics`
    ([nlisteners][3]), NaN where the curve does not reach db_end within nbins bins.  speakers = (directions, coefficients).  The diffuse
    records only (its signature is pinned: parameter_map(which=IR_ALL) has the times of the whole response in its first three columns).
    Leaves the context relistened at the last microphone."""
    mics = np.asarray(mics, dtype=np.float32).reshape(-1, 3)
    nchannels = len(speakers[1])
    out = np.zeros((mics.shape[0], nchannels, 8), dtype=np.float32)
    for i, curve in _curves(ctx, mics, speakers, sample_rate, nbins, mode):
        out[i] = ctx.decay_times(curve.data_ptr(), nchannels * 8, nbins, sample_rate, db_begin, db_end).reshape(nchannels, 8)     # synchronous
    return out


def parameter_map(ctx, mics, speakers, sample_rate, nbins, mode=capi.IR_EXACT, which=capi.IR_DIFFUSE, remove_direct=False):
    """float32 [nlisteners][nchannels][8][7]: EDT, T20, T30 (seconds), C50, C80 (dB), D50 and Ts (seconds) of every (channel, band) row at
    every microphone of `mics` ([nlisteners][3]) in one sweep per listener (rvb_decay_params; columns capi.DECAY_EDT .. capi.DECAY_TS), NaN
    where a parameter is not available.  With which=IR_DIFFUSE the time columns are decay_map's for the same arguments, byte for byte; the early-energy
    parameters are those of the diffuse response unless which is IR_ALL (or IR_IMAGES): then the direct sound (unless remove_direct) and the
    image sources take part.  Leaves the context relistened at the last microphone."""
    mics = np.asarray(mics, dtype=np.float32).reshape(-1, 3)
    nchannels = len(speakers[1])
    out = np.zeros((mics.shape[0], nchannels, 8, capi.DECAY_NPARAMS), dtype=np.float32)
    for i, curve in _curves(ctx, mics, speakers, sample_rate, nbins, mode, which, remove_direct):
        out[i] = ctx.decay_params(curve.data_ptr(), nchannels * 8, nbins, sample_rate).reshape(nchannels, 8, capi.DECAY_NPARAMS)     # synchronous
    return out


def sti_map(ctx, mics, speakers, sample_rate, nbins, snr_db=None, mode=capi.IR_EXACT, which=capi.IR_ALL, remove_direct=False):
    """float64 [nlisteners][nchannels]: the speech transmission index (speech.sti, male-speech weights) at every microphone of `mics`
    ([nlisteners][3]); snr_db: seven signal-to-noise ratios in dB, or None.  The whole response by default (which=IR_ALL): an index
    without the direct sound is not the seat's.  14 float64 per row leave the device.  NaN where a band of a channel is empty.  Leaves
    the context relistened at the last microphone."""
    mics = np.asarray(mics, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((mics.shape[0], len(speakers[1])), dtype=np.float64)
    for i, hist in _histograms(ctx, mics, speakers, sample_rate, nbins, mode, which, remove_direct):
        out[i] = speech.sti(ctx, hist, sample_rate, snr_db)                  # synchronous
    return out
