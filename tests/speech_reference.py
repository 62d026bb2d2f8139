"""The binary64 numpy restatement of include/rvb_capi_speech.h: the modulation transfer function of rows of bins, its adjoint and the
speech transmission index, with the bars the GPU tests hold the kernels to.  Nothing here is taken from what the kernels return.

THE REFERENCE VALUES are computed in x87 extended precision (np.longdouble, 64 bits of mantissa): the phase j F / fs is one extended
product and one extended quotient (2 roundings of 2^-64 relative: at 130 cycles that is 2 pi 130 2^-63 < 2^-53 in the angle, far below
tau >= 2^-48), reduced by its integer part exactly, and cos / sin of it come from the extended library; the squares of float32 values
are exact; the sums run in extended precision (nbins 2^-64 relative).  Beside the bars below the reference is exact.

THE BARS.  With eps0 = (nbins + 16) 2^-52 for a binary64 sum of nbins terms in any order with a few roundings behind it, and
tau_i = 2^-48 + 2 pi ceil(F_i nbins / fs) 2^-52, the header's condition on every cos and sin value:
    S      |gpu - ref| <= eps0 S                       (non-negative terms)
    A, B   |gpu - ref| <= eps_i S, eps_i = eps0 + tau_i  (|e cos| <= e: the sum's roundings and the cosines' errors are both relative to S)
    m      M = sqrt(A^2 + B^2) moves by at most sqrt(2) eps_i S, its own three roundings by 2^-51 M; the quotient by S adds m eps0 and
           one rounding:  |gpu - ref| <= 1.5 eps_i + m eps0 + 2^-49.
    w      w_j = 2 H_j g_j, g_j = sum_i (a_i cos_ij + b_i sin_ij) - d with a_i = c_i A_i / (M_i S), b_i likewise, d = sum_i c_i m_i / S.
           The direction (A_i, B_i) / M_i moves by at most (eps_i S + sqrt(2) eps_i S) / M_i <= 2.5 eps_i / m_i, and never by more than
           2; so  da_i = db_i = |c_i| / S (min(2.5 eps_i / m_i, 2) + eps0 + 2^-49),  dd = sum_i |c_i| (m_bar_i + m_i (eps0 + 2^-49)) / S,
           and    c_j = 2 |H_j| [ sum_i (da_i |cos_ij| + db_i |sin_ij| + (|a_i| + |b_i|) tau_i) + (2 nfreqs + 4) 2^-53 mag_j + dd ],
           mag_j = sum_i (|a_i cos_ij| + |b_i sin_ij|) + |d|.  The rounding to float is the test's own 2^-23 |w_ref| beside c_j.
    STI    see speech_index_bars."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs x87 extended precision"
PI = 4 * np.arctan(LD(1))

STI_FREQS = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)
ALPHA_MALE = (0.085, 0.127, 0.230, 0.233, 0.309, 0.224, 0.173)
BETA_MALE = (0.085, 0.078, 0.065, 0.011, 0.047, 0.095)


def tau(freqs, nbins, fs):
    f = np.asarray(freqs, np.float64)
    return 2.0 ** -48 + 2 * np.pi * np.ceil(f * nbins / float(fs)) * 2.0 ** -52


_tables = {}


def phases(nbins, fs, freqs):
    """(cos, sin) float64 [nfreqs][nbins] of 2 pi F j / fs, evaluated in extended precision and rounded to binary64 once (2^-54: far below
    tau).  The last table asked for is kept."""
    key = (int(nbins), float(fs), tuple(float(f) for f in freqs))
    if _tables.get("key") != key:
        j = np.arange(int(nbins), dtype=LD)
        c = np.empty((len(key[2]), int(nbins)), np.float64)
        s = np.empty_like(c)
        for i, f in enumerate(key[2]):
            u = j * LD(f) / LD(float(fs))
            u -= np.floor(u)
            c[i], s[i] = np.cos(2 * PI * u), np.sin(2 * PI * u)
        _tables.update(key=key, value=(c, s))
    return _tables["value"]


def mtf(h, fs, freqs):
    """The sums and the transfer values of every row of h ([nrows][nbins], any float type: the values as they are) with their bars."""
    h = np.asarray(h)
    nrows, nbins = h.shape
    c, s = phases(nbins, fs, freqs)
    e = h.astype(LD) ** 2
    total = e.sum(axis=1)
    a = np.stack([(e * c[i].astype(LD)).sum(axis=1) for i in range(len(freqs))], axis=1)
    b = np.stack([(e * s[i].astype(LD)).sum(axis=1) for i in range(len(freqs))], axis=1)
    modulus = np.sqrt(a * a + b * b)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(total[:, None] > 0, modulus / total[:, None], LD(np.nan))
    eps0 = (nbins + 16) * 2.0 ** -52
    eps = eps0 + tau(freqs, nbins, fs)
    total64 = total.astype(np.float64)
    m64 = m.astype(np.float64)
    sums = np.empty((nrows, 1 + 2 * len(freqs)), np.float64)
    sums[:, 0], sums[:, 1::2], sums[:, 2::2] = total64, a.astype(np.float64), b.astype(np.float64)
    sums_bar = np.empty_like(sums)
    sums_bar[:, 0] = eps0 * total64
    sums_bar[:, 1::2] = sums_bar[:, 2::2] = eps[None, :] * total64[:, None]
    m_bar = 1.5 * eps[None, :] + np.nan_to_num(m64) * eps0 + 2.0 ** -49
    return {"sums": sums, "sums_bar": sums_bar, "m": m64, "m_bar": np.broadcast_to(m_bar, m64.shape).copy(), "eps0": eps0, "eps": eps,
            "S": total, "A": a, "B": b, "M": modulus, "m_ld": m}


def adjoint(h, fs, freqs, coeffs, forward=None):
    """(w, c): w = dL/dH float64 [nrows][nbins] for coeffs [nrows][nfreqs] = dL/dm, and the bar c_j of every entry (module text)."""
    h = np.asarray(h)
    nrows, nbins = h.shape
    nf = len(freqs)
    fw = forward if forward is not None else mtf(h, fs, freqs)
    c, s = phases(nbins, fs, freqs)
    coeffs = np.asarray(coeffs, np.float64).reshape(nrows, nf)
    t = tau(freqs, nbins, fs)
    w = np.zeros((nrows, nbins), np.float64)
    bar = np.zeros((nrows, nbins), np.float64)
    for r in range(nrows):
        total = fw["S"][r]
        if not total > 0:
            continue
        ok = fw["M"][r] > 0
        scale = np.where(ok, coeffs[r].astype(LD) / (np.where(ok, fw["M"][r], LD(1)) * total), LD(0))
        a, b = scale * fw["A"][r], scale * fw["B"][r]
        d = (np.where(ok, coeffs[r].astype(LD) * fw["m_ld"][r], LD(0))).sum() / total
        g = -d * np.ones(nbins, LD)
        for i in range(nf):
            g = g + a[i] * c[i].astype(LD) + b[i] * s[i].astype(LD)
        w[r] = (2 * h[r].astype(LD) * g).astype(np.float64)
        a64, b64, d64, total64, m64 = np.abs(a).astype(np.float64), np.abs(b).astype(np.float64), abs(float(d)), float(total), fw["m"][r]
        with np.errstate(divide="ignore"):
            direction = np.minimum(2.5 * fw["eps"] / m64, 2.0) + fw["eps0"] + 2.0 ** -49
        da = np.abs(coeffs[r]) / total64 * direction
        dd = (np.abs(coeffs[r]) * (fw["m_bar"][r] + m64 * (fw["eps0"] + 2.0 ** -49))).sum() / total64
        abs_c, abs_s = np.abs(c), np.abs(s)
        mag = a64 @ abs_c + b64 @ abs_s + d64
        inner = da @ abs_c + da @ abs_s + ((a64 + b64) * t).sum() + (2 * nf + 4) * 2.0 ** -53 * mag + dd
        bar[r] = 2 * np.abs(h[r].astype(np.float64)) * inner
    return w, bar


def speech_index(mtf_matrix, alpha, beta, snr_db=None):
    """(sti, mti [7], dSTI/dm [7][nfreqs], scale [7][nfreqs]) of a matrix [7][nfreqs] by the five steps of the header; scale is the sum of
    the magnitudes of the derivative's terms (speech_index_bars)."""
    m = np.asarray(mtf_matrix, np.float64)
    alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
    nf = m.shape[1]
    factor = np.ones(7)
    if snr_db is not None:
        snr_db = np.asarray(snr_db, np.float64)
        finite = ~(np.isinf(snr_db) & (snr_db > 0))
        factor[finite] = 1.0 + 10.0 ** (-snr_db[finite] / 10.0)
    reduced = m / factor[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10.0 * np.log10(reduced / (1.0 - reduced))
    snr = np.where(reduced >= 1.0, 15.0, np.where(reduced <= 0.0, -15.0, snr))
    free = (reduced > 0.0) & (reduced < 1.0) & (snr <= 15.0) & (snr >= -15.0)
    snr = np.where(np.isnan(reduced), np.nan, np.clip(snr, -15.0, 15.0))
    ti = (snr + 15.0) / 30.0
    mti = np.array([sum(ti[k, i] for i in range(nf)) / nf for k in range(7)])
    product = mti[:-1] * mti[1:]
    root = np.sqrt(product)
    sti = sum(alpha[k] * mti[k] for k in range(7)) - sum(beta[k] * root[k] for k in range(6))
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = np.where(free, (10.0 / np.log(10.0)) / (reduced * (1.0 - reduced)) / 30.0 / factor[:, None], 0.0)
        up = np.where(product > 0, beta * mti[1:] / (2.0 * root), 0.0)            # d(beta_k root_k) / dMTI_k
        down = np.where(product > 0, beta * mti[:-1] / (2.0 * root), 0.0)         # d(beta_k root_k) / dMTI_{k+1}
    by_mti, by_mti_scale = alpha.copy(), np.abs(alpha)
    by_mti[:-1] -= up
    by_mti[1:] -= down
    by_mti_scale[:-1] += np.abs(up)
    by_mti_scale[1:] += np.abs(down)
    return float(sti), mti, slope * by_mti[:, None] / nf, slope * by_mti_scale[:, None] / nf


def speech_index_bars(alpha, beta, scale):
    """(bar of STI, bar of dSTI/dm) between two binary64 evaluations of the five steps.  A TI: the quotient m' / (1 - m') (the difference
    is exact or one rounding), a 1-ulp log10 with d(10 log10 x) = 4.35 dx / x, three more roundings at values <= 30: below 2^-48.  The mean
    and the weighted sums add roundings at values <= 1, the square root halves relative errors: |dSTI| <= (sum |alpha| + sum |beta|) 2^-47.
    A derivative entry is a product of about a dozen correctly rounded operations on positive terms and one signed sum of three, so it
    errs by at most 2^-48 of the sum of the magnitudes of its terms (`scale`)."""
    return (np.abs(alpha).sum() + np.abs(beta).sum()) * 2.0 ** -47, 2.0 ** -48 * np.asarray(scale) + 1e-300


def sti_of_rows(m_rows, alpha=ALPHA_MALE, beta=BETA_MALE, snr_db=None):
    """float64 [nchannels] from transfer values [nchannels * 8][nfreqs]: rows c * 8 + 0..6 of channel c, band 7 takes no part."""
    m_rows = np.asarray(m_rows, np.float64)
    blocks = m_rows.reshape(-1, 8, m_rows.shape[1])
    return np.array([speech_index(block[:7], alpha, beta, snr_db)[0] for block in blocks])
