// speech_index.h — the arithmetic of rvb_speech_index (include/rvb_capi_speech.h) as plain host code: the speech transmission index of
// a matrix of modulation transfer values, its band indices and its derivative.  No device, no context; csrc/speech.hip calls it.
//
// Per band k = 0..6 and modulation frequency i, every step binary64:
//     m'  = m / (1 + 10^(-snr_db[k] / 10))                 (snr_db == nullptr or +inf: m' = m)
//     SNR = 10 log10(m' / (1 - m')) clipped to [-15, 15]     (m' >= 1: 15, m' <= 0: -15)
//     TI  = (SNR + 15) / 30
//     MTI_k = (TI_0 + TI_1 + ...) / nfreqs, added in the order of i
//     STI = (alpha_0 MTI_0 + ...) - (beta_0 sqrt(MTI_0 MTI_1) + ...), each sum in the order of k
// A NaN in the matrix gives NaN.  The derivative is 0 through a clipped entry and 0 for a square-root term whose product is 0.
#pragma once

#include <cmath>
#include <cstdint>

namespace speech_index {

constexpr int kBands = 7;

// sti; mti[7] and d[7][nfreqs] = dSTI/dm where not null
inline double evaluate(const double * mtf, uint64_t nfreqs, const double * snr_db, const double * alpha, const double * beta, double * mti_out,
                       double * d)
{
    const double kLog = 10.0 / std::log(10.0);            // d(10 log10 x) / d(ln x)
    double mti[kBands];
    for (int k = 0; k < kBands; ++k) {
        const bool noiseless = !snr_db || (std::isinf(snr_db[k]) && snr_db[k] > 0.0);
        const double denominator = noiseless ? 1.0 : 1.0 + std::pow(10.0, -snr_db[k] / 10.0);
        double sum = 0.0;
        for (uint64_t i = 0; i < nfreqs; ++i) {
            const double m = mtf[k * nfreqs + i];
            const double reduced = noiseless ? m : m / denominator;
            double snr, slope = 0.0;                       // slope = dTI/dm
            if (std::isnan(reduced)) snr = reduced;
            else if (reduced >= 1.0) snr = 15.0;
            else if (reduced <= 0.0) snr = -15.0;
            else {
                snr = 10.0 * std::log10(reduced / (1.0 - reduced));
                if (snr > 15.0) snr = 15.0;
                else if (snr < -15.0) snr = -15.0;
                else slope = kLog / (reduced * (1.0 - reduced)) / 30.0 / denominator;
            }
            sum = sum + (snr + 15.0) / 30.0;
            if (d) d[k * nfreqs + i] = slope;
        }
        mti[k] = sum / (double) nfreqs;
    }
    double direct = 0.0, redundancy = 0.0;
    double by_mti[kBands];
    for (int k = 0; k < kBands; ++k) {
        direct = direct + alpha[k] * mti[k];
        by_mti[k] = alpha[k];
    }
    for (int k = 0; k + 1 < kBands; ++k) {
        const double product = mti[k] * mti[k + 1];
        const double root = std::sqrt(product);
        redundancy = redundancy + beta[k] * root;
        if (product > 0.0) {
            by_mti[k] = by_mti[k] - beta[k] * mti[k + 1] / (2.0 * root);
            by_mti[k + 1] = by_mti[k + 1] - beta[k] * mti[k] / (2.0 * root);
        }
    }
    for (int k = 0; k < kBands; ++k) {
        if (mti_out) mti_out[k] = mti[k];
        if (d)
            for (uint64_t i = 0; i < nfreqs; ++i) d[k * nfreqs + i] = d[k * nfreqs + i] * by_mti[k] / (double) nfreqs;
    }
    return direct - redundancy;
}

} // namespace speech_index
