"""The binary64 numpy statement of the three decay definitions of include/rvb_capi.h (rvb_decay_curve, rvb_decay_times, rvb_decay_loss),
and the error bars the GPU tests hold the kernels to.  Every bar is derived here from the formulas and the number formats — never from
what the kernels return.

Arrays are [nrows][nbins]; the functions take float32 or float64 and compute in float64 without rounding anything in between.

u = 2^-53 is the unit roundoff of binary64.  Two facts are used throughout: a sum of n terms in ANY order errs by at most
(n - 1) u sum |terms| to first order, and a logarithm of the device's or numpy's library is good to 2 ulp = 4 u relative (the
documented accuracy is 1 ulp for both)."""
import numpy as np

U = 2.0 ** -53


def curve(h):
    """E[r][k] = sum_{j >= k} H[r][j]^2 in float64."""
    h = np.asarray(h, dtype=np.float64)
    return np.flip(np.cumsum(np.flip(h * h, -1), -1), -1)


def ratio(db):
    """10^(db / 10) for a level given as float32, as the C-ABI takes it."""
    return 10.0 ** (float(np.float32(db)) / 10.0)


def window(e_row, db_begin, db_end):
    """(k0, k1) of one row, or None where the time is not available: k0 the first k with E <= E[0] ratio(db_begin), k1 the first k with
    E < E[0] ratio(db_end)."""
    e = np.asarray(e_row, dtype=np.float64)
    if not e[0] > 0:
        return None
    at = np.flatnonzero(e <= e[0] * ratio(db_begin))
    below = np.flatnonzero(e < e[0] * ratio(db_end))
    if at.size == 0 or below.size == 0:
        return None
    k0, k1 = int(at[0]), int(below[0])
    if k1 - k0 < 2:
        return None
    return k0, k1


def times(e, sample_rate, db_begin, db_end):
    """(seconds, rel): per row the reverberation time in float64 (NaN: not available) and the relative bar of the binary64 evaluation.

    The line: level[k] = 10 log10(E[k] / E[0]) over xc = (k - k0) - (n - 1) / 2, n = k1 - k0; slope = sum xc level / Sxx with
    Sxx = n (n^2 - 1) / 12; seconds = -60 / (slope sample_rate).
    THE BAR, for two evaluations (the kernel's and this one) of the same formula in binary64:
      - a level: the quotient's rounding moves it by (10 / ln 10) u = 4.35 u, the logarithm by 4 u |level|, the product with 10 by
        u |level|: |dlevel_k| <= 8 u (1 + |level_k|) =: dl_k with room to spare;
      - the sum: every product xc level is rounded (u) and the n terms are added in some order ((n - 1) u):
        |d sum| <= sum |xc_k| dl_k + n u sum |xc_k level_k| per evaluation;
      - Sxx in closed form, the quotient, the product with the rate and the final quotient: 8 roundings, 8 u relative per evaluation.
    rel = 2 [ sum |xc| dl + n u sum |xc level| ] / |sum xc level| + 16 u.  The test adds 2^-23 for the one rounding to float."""
    e = np.asarray(e, dtype=np.float64)
    seconds = np.full(e.shape[0], np.nan)
    rel = np.zeros(e.shape[0])
    for r in range(e.shape[0]):
        w = window(e[r], db_begin, db_end)
        if w is None:
            continue
        k0, k1 = w
        n = k1 - k0
        level = 10.0 * np.log10(e[r, k0:k1] / e[r, 0])
        xc = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
        sxy = float((xc * level).sum())
        sxx = n * (float(n) * n - 1.0) / 12.0
        slope = sxy / sxx
        seconds[r] = -60.0 / (slope * float(np.float32(sample_rate)))
        dl = 8.0 * U * (1.0 + np.abs(level))
        rel[r] = 2.0 * (float((np.abs(xc) * dl).sum()) + n * U * float(np.abs(xc * level).sum())) / abs(sxy) + 16.0 * U
    return seconds, rel


def mask_of(t, db_begin=-5.0, db_end=-35.0):
    """1.0 where the curve T lies in its own range db_begin .. db_end (the window of `times`), else 0.0; float32."""
    t = np.asarray(t, dtype=np.float64)
    m = np.zeros(t.shape, dtype=np.float32)
    for r in range(t.shape[0]):
        w = window(t[r], db_begin, db_end)
        if w is not None:
            m[r, w[0]:w[1]] = 1.0
    return m


def loss(h, e, t, m, normalised):
    """A dict with the loss of rvb_decay_loss, its adjoint and their bars, all float64:
        loss_rows [nrows]      sum_k m d^2,  d = ln E - ln T - (normalised ? ln E[0] - ln T[0] : 0) over the bins that count
        w [nrows][nbins]       2 H[j] sum_{k <= j} g[k],  g = 2 m d / E,  with the flag g[0] -= (sum_k 2 m d) / E[0]
        loss_bar [nrows], c [nrows][nbins]    the bars below.
    THE BARS, for two evaluations in binary64.  Lambda_k = |ln E_k| + |ln T_k| (+ |ln E_0| + |ln T_0| with the flag).
      - d: the logarithms err by 4 u |ln| each, the (up to three) differences by u Lambda each, on both sides:
        |dd_k| <= 2 (4 u + 3 u) Lambda_k <= 16 u Lambda_k = 2^-49 Lambda_k =: D_k;
      - g: |dg_k| <= 2 m_k D_k / E_k, and four roundings of its own, 4 u |g_k| (they join the sum's term below);
      - the normalisation term N = S / E_0, S = sum_k 2 m d over the whole row:
        |dN| <= [ sum_k 2 m_k D_k + (nbins + 16) 2 u sum_k |2 m_k d_k| ] / E_0;
      - a prefix of j + 1 terms (and N) added in some order on both sides: (j + 16) 2 u (sum_{k <= j} |g_k| + |N|);
      - c_j = 2 |H_j| [ (j + 16) 2^-52 (sum_{k <= j} |g_k| + |N|) + sum_{k <= j} 2 m_k D_k / E_k + |dN| ];
        the product with 2 H_j and the rounding to float are the test's 2^-23 |w|.
      - loss_bar = sum_k m_k (2 |d_k| D_k + D_k^2) + (nbins + 16) 2^-52 sum_k m_k d_k^2."""
    h, e, t, m = (np.asarray(x, dtype=np.float64) for x in (h, e, t, m))
    nrows, nbins = e.shape
    rows = np.ones(nrows, dtype=bool)
    shift = np.zeros(nrows)
    lam0 = np.zeros(nrows)
    if normalised:
        rows = (e[:, 0] > 0) & (t[:, 0] > 0)
        le0, lt0 = np.log(np.where(rows, e[:, 0], 1.0)), np.log(np.where(rows, t[:, 0], 1.0))
        shift, lam0 = le0 - lt0, np.abs(le0) + np.abs(lt0)
    counts = (m > 0) & (e > 0) & (t > 0) & rows[:, None]
    le, lt = np.log(np.where(counts, e, 1.0)), np.log(np.where(counts, t, 1.0))
    d = np.where(counts, (le - lt) - shift[:, None], 0.0)
    mm = np.where(counts, m, 0.0)
    safe_e = np.where(counts, e, 1.0)
    g = 2.0 * mm * d / safe_e
    lam = np.where(counts, np.abs(le) + np.abs(lt) + lam0[:, None], 0.0)
    dk = 16.0 * U * lam
    norm = np.zeros(nrows)
    dnorm = np.zeros(nrows)
    if normalised:
        e0 = np.where(rows, e[:, 0], 1.0)
        norm = np.where(rows, -(2.0 * mm * d).sum(axis=1) / e0, 0.0)
        dnorm = np.where(rows, ((2.0 * mm * dk).sum(axis=1) + (nbins + 16) * 2.0 * U * np.abs(2.0 * mm * d).sum(axis=1)) / e0, 0.0)
    prefix = np.cumsum(g, axis=1) + norm[:, None]
    w = 2.0 * h * prefix
    j = np.arange(nbins, dtype=np.float64)[None, :]
    c = 2.0 * np.abs(h) * ((j + 16.0) * 2.0 ** -52 * (np.cumsum(np.abs(g), axis=1) + np.abs(norm)[:, None])
                           + np.cumsum(2.0 * mm * dk / safe_e, axis=1) + dnorm[:, None])
    loss_rows = (mm * d * d).sum(axis=1)
    loss_bar = (mm * (2.0 * np.abs(d) * dk + dk * dk)).sum(axis=1) + (nbins + 16) * 2.0 ** -52 * loss_rows
    return {"loss_rows": loss_rows, "w": w, "c": c, "loss_bar": loss_bar, "rows": rows}
