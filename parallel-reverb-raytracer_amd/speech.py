"""Speech transmission index of a histogram on the device (include/rvb_capi_speech.h): the modulation transfer function of the seven
octave bands 125 Hz .. 8 kHz at the standard's 14 modulation frequencies (rvb_mtf), then the index on the host (rvb_speech_index).
Nothing leaves the device but 14 float64 per row.

The eight bands of a histogram are octaves with the edges lo, 175, 350, ..., 11200, 20000 Hz: rows c * 8 + 0..6 of channel c are the
seven STI octaves, band 7 takes no part.  Level-dependent masking and the reception threshold of IEC 60268-16 need absolute levels and
are out of scope; a signal-to-noise ratio per band can be given."""
import numpy as np

from . import capi

STI_FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)      # Hz
# The male-speech weights of IEC 60268-16 ed. 4 as remembered by the maintainer (sum alpha - sum beta = 1); callers with the standard at
# hand pass their own.
ALPHA_MALE = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
BETA_MALE = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)
assert len(STI_FREQS) == capi.STI_FREQS and len(ALPHA_MALE) == capi.STI_BANDS and len(BETA_MALE) == capi.STI_BANDS - 1


def mtf_rows(ctx, hist, sample_rate):
    """float64 [nchannels * 8][14]: the transfer values of every row of a float32 CUDA tensor [nchannels][8][nbins] at STI_FREQS.  The
    context's stream waits for what torch's current stream has done to the tensor.  Synchronous."""
    import torch
    assert hist.is_cuda and hist.is_contiguous() and hist.dtype == torch.float32 and hist.dim() == 3 and hist.shape[1] == 8
    ctx.ir_accumulate_wait_for_torch()
    return ctx.mtf(hist.data_ptr(), hist.shape[0] * 8, hist.shape[2], sample_rate, STI_FREQS)


def index_of_rows(m, snr_db=None, alpha=ALPHA_MALE, beta=BETA_MALE, want_derivative=False):
    """float64 [nchannels] from transfer values m [nchannels * 8][nfreqs]; with want_derivative (sti, dSTI/dm [nchannels * 8][nfreqs]),
    the rows of band 7 zero."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    blocks = m.reshape(-1, 8, m.shape[1])
    out = np.zeros(blocks.shape[0], dtype=np.float64)
    derivative = np.zeros(blocks.shape, dtype=np.float64)
    for c, block in enumerate(blocks):
        if want_derivative:
            out[c], _, derivative[c, :capi.STI_BANDS] = capi.speech_index(block[:capi.STI_BANDS], alpha, beta, snr_db, True)
        else:
            out[c] = capi.speech_index(block[:capi.STI_BANDS], alpha, beta, snr_db)[0]
    return (out, derivative.reshape(m.shape)) if want_derivative else out


def sti(ctx, hist, sample_rate, snr_db=None, alpha=ALPHA_MALE, beta=BETA_MALE):
    """float64 [nchannels]: the speech transmission index of every channel of a histogram, a float32 CUDA tensor [nchannels][8][nbins]
    whose bins are 1 / sample_rate apart.  snr_db: seven signal-to-noise ratios in dB, or None.  NaN for a channel with an all-zero band."""
    return index_of_rows(mtf_rows(ctx, hist, sample_rate), snr_db, alpha, beta)
