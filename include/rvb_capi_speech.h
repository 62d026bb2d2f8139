/* rvb_capi_speech.h — speech intelligibility: the modulation transfer function (MTF) of rows of bins, its adjoint, and the speech
 * transmission index (STI, IEC 60268-16) of a matrix of transfer values.  An extension of rvb_capi.h (which it includes and whose
 * types, codes and conventions it uses), exported by the same librvb_hip.so; rvb_capi.h itself is unchanged by it.  No reference
 * counterpart.  python: capi.Context.mtf / mtf_adjoint, capi.speech_index, speech.py, listeners.sti_map, fitting.fit_sti.
 *
 * WHY.  The decay calls give the ISO 3382-1 numbers of a histogram.  A room for speech — a PA, a voice alarm, a lecture room — is
 * specified by the STI, and the STI is not a function of the Schroeder curve: it comes from the modulation transfer function of the
 * squared response of each octave band, 14 complex sums over the whole row per band.  Without these calls the histogram travels to the
 * host for them, 54 MB per listener at 100 k rays x 128 reflections.  The eight bands of a histogram are octaves with the edges lo, 175,
 * 350, ..., 11200, 20000 Hz: bands 0..6 are the seven STI octaves 125 Hz .. 8 kHz.
 */
#ifndef RVB_CAPI_SPEECH_H
#define RVB_CAPI_SPEECH_H

#include "rvb_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

struct rvb_ctx;                   /* the context of rvb_capi.h */

#define RVB_MTF_MAX_FREQS 16      /* most modulation frequencies of one call */
#define RVB_STI_BANDS 7           /* octave bands 125 Hz .. 8 kHz: rows c * 8 + 0..6 of channel c of a histogram */
#define RVB_STI_FREQS 14          /* the standard's modulation frequencies 0.63 .. 12.5 Hz (the list itself is the caller's: speech.py) */

/* ---- the modulation transfer function (csrc/speech.hip, csrc/speech_kernels.hip over csrc/decay_tiles.h) ----------------------------
 * d_histogram is a device array of nrows rows of nbins floats, the caller's own, as the decay calls take it.  ALL ARITHMETIC is binary64
 * on the float32 values of H; fs is sample_rate widened to double.  Per row, with F_i = mod_freqs[i]:
 *     e_j = H_j^2 (exact in binary64),  q_i = F_i / fs,  u_ij = j * q_i (one binary64 product),
 *     S = sum_j e_j,  A_i = sum_j e_j cos(2 pi u_ij),  B_i = sum_j e_j sin(2 pi u_ij),  m_i = sqrt(A_i^2 + B_i^2) / S.
 * mtf[r][i] receives m_i; sums, if not NULL, [r][0] = S, [r][1 + 2 i] = A_i, [r][2 + 2 i] = B_i.  A row with S == 0 gives a quiet NaN in
 * every m_i.
 * THE ORDER of the sums is fixed by (tile, chunk, bin) as for the decay calls: one partial per tile of RVB_DECAY_TILE bins — per lane
 * the four bins of a chunk one after the other, the chunks of a wave by a shuffle ladder, a tile's 16 segments one after the other —,
 * then one wave per row adds the tiles in tile order.  No atomics: two calls return identical bytes, and they do not depend on nfreqs.
 * THE COSINES.  Every cos and sin value the sums use lies within tau_i = 2^-48 + 2 pi ceil(F_i nbins / fs) 2^-52 of the mathematical
 * value at the exact phase 2 pi F_i j / fs: the first term for the evaluation, the second for the roundings of q_i and u_ij.  The
 * evaluation kept is one binary64 sincospi per chunk of 4 bins — its argument 2 u is exact and the library reduces it exactly — and
 * three rotations by the constant step (cos, sin)(2 pi q_i): a 2-ulp library value and three rotations of four products and two sums
 * stay below 2^-50.  The per-bin form was not kept: it makes four library calls where this one makes one, in kernels that are bound by
 * exactly those calls (see MEASURED).
 * MECHANISM, the names those of rvb_last_timings: "mtf_sums_kernel", grid (tiles, rows), leaves 1 + 2 nfreqs partial sums per tile; the
 * frequencies are its outer loop over the 16 squares a lane holds, so a lane never holds more than eight accumulators.
 * "mtf_fold_kernel", one wave per row, adds the tiles and leaves S, A_i, B_i and m_i (and the adjoint's coefficients) per row.
 *
 * ---- the adjoint --------------------------------------------------------------------------------------------------------------------
 * For a loss L with coeffs[r][i] = c_i = dL/dm_i and M_i = sqrt(A_i^2 + B_i^2), d_weights receives w = dL/dH in H's layout:
 *     d_weights[r][j] = 2 H_j ( sum_i c_i (A_i cos_ij + B_i sin_ij) / (M_i S)  -  (sum_i c_i m_i) / S ),
 * the terms added in the order of i, a term with M_i == 0 being 0; rounded to float once; exactly 0 where H_j is 0, all zero in a row
 * with S == 0.  Every entry is written.  This is what rvb_reshade_grad, rvb_reshade_grad_images and rvb_reshade_grad_map take.
 * The call computes the sums itself — mtf_sums_kernel and mtf_fold_kernel as above, the fold leaving a_i = c_i A_i / (M_i S),
 * b_i = c_i B_i / (M_i S) and d = (sum_i c_i m_i) / S per row — and "mtf_adjoint_kernel" streams H once more: no dense intermediate
 * goes to memory.
 *
 * CALLING, both.  Synchronous.  They use of the context its device, stream, timings and a scratch block of their own (1 + 2 nfreqs
 * doubles per tile, some hundred bytes per row, grown on demand): no scene, trace or IR configuration is needed or read, and nothing of
 * the context is voided — the sort buffers, the accumulation scratch, the decay scratch and a prepared exact list stay.
 * REFUSALS, each with a text that names its condition, each before any device is touched; a failed call writes nothing, neither to the
 * host arrays nor to d_weights.  RVB_ERR_INVALID: NULL ctx; NULL d_histogram, mod_freqs, mtf (rvb_mtf), coeffs or d_weights
 * (rvb_mtf_adjoint); nrows, nbins or nfreqs 0; nfreqs above RVB_MTF_MAX_FREQS; a sample rate or a frequency that is not finite and > 0;
 * a frequency at or above fs / 2; a coefficient that is not finite; d_weights overlapping the histogram.  RVB_ERR_CAPACITY as
 * rvb_decay_curve has it: more than 4096 rows, 2^32 - 1 bins or more.
 * MEASURED: see the end of this file. */
int rvb_mtf(rvb_ctx * ctx, const void * d_histogram, uint64_t nrows, uint64_t nbins, float sample_rate,
            const double * mod_freqs /* host [nfreqs], Hz */, uint64_t nfreqs,
            double * mtf /* host [nrows][nfreqs] */, double * sums /* host [nrows][1 + 2 nfreqs]: S, A_0, B_0, A_1, ...; may be NULL */);
int rvb_mtf_adjoint(rvb_ctx * ctx, const void * d_histogram, uint64_t nrows, uint64_t nbins, float sample_rate,
                    const double * mod_freqs, uint64_t nfreqs, const double * coeffs /* host [nrows][nfreqs] = dL/dm */,
                    void * d_weights /* device float [nrows][nbins] */);

/* ---- the speech transmission index (csrc/speech_index.h) -----------------------------------------------------------------------------
 * Pure host arithmetic in binary64: no context, no device, callable without a GPU.  mtf is [RVB_STI_BANDS][nfreqs], band k in row k.
 *     1. m' = m / (1 + 10^(-snr_db[k] / 10)); snr_db == NULL, or +inf for a band: m' = m.
 *     2. SNR = 10 log10(m' / (1 - m')), clipped to [-15, 15]; m' >= 1 gives 15, m' <= 0 gives -15.
 *     3. TI = (SNR + 15) / 30.
 *     4. MTI_k = the mean of TI over i, added in the order of i.
 *     5. STI = sum_k alpha[k] MTI_k - sum_k beta[k] sqrt(MTI_k MTI_{k+1}), each sum in the order of k.
 * A NaN in mtf gives a NaN STI.  *sti receives the index, mti (if not NULL) the seven MTI_k, d_sti_d_mtf (if not NULL) dSTI/dm in mtf's
 * layout: exact almost everywhere, 0 through a clipped entry and 0 for a square-root term whose product is 0.
 * THE WEIGHTS alpha[7] and beta[6] are arguments, not constants of the library (speech.py carries the male-speech set).
 * OUT OF SCOPE: the level-dependent auditory masking and the reception threshold of the standard need absolute sound pressure levels,
 * which a histogram does not carry; what is computed is the index of the transfer values and the signal-to-noise ratios given.
 * RVB_ERR_INVALID, writing nothing: NULL mtf, alpha, beta or sti; nfreqs 0 or above RVB_MTF_MAX_FREQS. */
int rvb_speech_index(const double * mtf /* [7][nfreqs] */, uint64_t nfreqs, const double * snr_db /* [7] or NULL */,
                     const double * alpha /* [7] */, const double * beta /* [6] */,
                     double * sti, double * mti /* [7] or NULL */, double * d_sti_d_mtf /* [7][nfreqs] or NULL */);

/* MEASURED on one MI355X at 16 x 846 741 (the stereo histogram of 100 k rays x 128 reflections) and at 512 x 846 741, 14 frequencies
 * (profiles/speech_n1.txt, tools/speech_bench.py; medians of 21 repetitions in one process, host clock to the synchronisation for the
 * calls, HIP events for the kernels; floors at the 6.6 TB/s the project measured).  No time was fixed in advance.
 *     rvb_mtf            0.343 ms [0.333 .. 0.364] / 8.33 ms [8.23 .. 8.39].  mtf_sums_kernel 0.250 / 8.19 ms against a floor of 0.008 /
 *                        0.263 ms for reading H once: 30 x / 31 x.  mtf_fold_kernel 0.043 / 0.058 ms.  The sums kernel is bound by
 *                        binary64 arithmetic — per chunk of 4 bins 14 sincospi and 42 rotations, per tile 29 shuffle ladders —, not by HBM.
 *     rvb_mtf_adjoint    0.463 ms [0.454 .. 0.495] / 11.55 ms [11.46 .. 11.69], 19 x / 15 x the floor of H read twice and w written once
 *                        (0.025 / 0.788 ms); mtf_adjoint_kernel alone 0.123 / 3.75 ms, 7.5 x / 7.1 x the floor of its own pass.
 *     what they replace  in the same run: the pinned download of the histogram 0.970 / 30.4 ms, and the transfer values in numpy binary64
 *                        on 16 host threads 36.9 / 1249 ms with the cos / sin tables of the shape at hand (220 ms to make them) —
 *                        110 x / 154 x rvb_mtf.  The largest |device - numpy| over all m: 8e-16 / 1.2e-15.
 *     the evaluation     one sincospi per chunk and three rotations was kept: it makes a quarter of the library calls of the per-bin
 *                        form in a kernel that those calls bound.  The per-bin form was not measured.
 *     the older calls    rvb_decay_curve, rvb_decay_times and rvb_decay_loss of this build against a library of the commit before, the
 *                        same loop in processes that take turns (2 turns of 21): 0.076 against 0.076, 0.122 against 0.121, 0.206
 *                        against 0.205 ms at 16 rows and 0.922 against 0.916, 1.317 against 1.332, 3.897 against 3.904 ms at 512, every
 *                        difference inside the parent's own spread (0.012 .. 0.155 ms): their device code is unchanged.
 * No counter run was made. */

#ifdef __cplusplus
}
#endif

#endif
