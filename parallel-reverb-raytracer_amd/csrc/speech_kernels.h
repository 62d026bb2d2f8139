// speech_kernels.h — what csrc/speech.hip and csrc/speech_kernels.hip share: the frequency block, the per-row block and the launches of
// the modulation transfer kernels (include/rvb_capi_speech.h).
#pragma once

#include "kernels.h"
#include "../../include/rvb_capi_speech.h"

// per modulation frequency i: q = F_i / fs, and cos / sin of the phase step of one bin, 2 pi q
struct MtfFreqs {
    double q[RVB_MTF_MAX_FREQS];
    double step_cos[RVB_MTF_MAX_FREQS], step_sin[RVB_MTF_MAX_FREQS];
    uint32_t n;
};

// What mtf_fold_kernel leaves per row: the sums S, A_0, B_0, A_1, ... and the transfer values m_i, directly behind each other as the
// host downloads them; for the adjoint a_i = c_i A_i / (M_i S), b_i = c_i B_i / (M_i S) (0 where M_i or S is 0) and
// d = (sum_i c_i m_i) / S (0 where S is 0), so that dL/dH_j = 2 H_j (sum_i (a_i cos_ij + b_i sin_ij) - d).
struct MtfRow {
    double sums[1 + 2 * RVB_MTF_MAX_FREQS];
    double m[RVB_MTF_MAX_FREQS];
    double a[RVB_MTF_MAX_FREQS], b[RVB_MTF_MAX_FREQS];
    double d;
};

// `tiles` is [1 + 2 n][nrows][rvb_decay_tiles(nbins)] doubles: plane 0 the tiles' sums of H^2, planes 1 + 2 i and 2 + 2 i those of
// H^2 cos and H^2 sin at frequency i.  coeffs: device [nrows][RVB_MTF_MAX_FREQS] = dL/dm, or null (no a, b, d).
void rvb_launch_mtf_sums(const float * hist, uint64_t nrows, uint64_t nbins, const MtfFreqs & freqs, double * tiles, hipStream_t s);
void rvb_launch_mtf_fold(uint64_t nrows, uint64_t nbins, uint32_t nfreqs, const double * tiles, const double * coeffs, MtfRow * rows, hipStream_t s);
void rvb_launch_mtf_adjoint(const float * hist, uint64_t nrows, uint64_t nbins, const MtfFreqs & freqs, const MtfRow * rows, float * weights,
                            hipStream_t s);
