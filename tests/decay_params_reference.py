"""The binary64 numpy statement of rvb_decay_params and rvb_decay_params_loss (include/rvb_capi.h) — EDT, T20, T30, C50, C80, D50 and Ts of
a decay curve, the weighted squared loss against a table of targets and its adjoint — and the error bars the GPU tests hold the kernels
to.  Every bar is derived here from the formulas and the number formats, in the manner of decay_reference.py — never from what the
kernels return.

Arrays are [nrows][nbins]; everything is computed in float64 on the values given (the GPU tests give the float32 curve).  U = 2^-53.
A bar always covers TWO evaluations of the same formula in binary64, the kernel's and this one, each with its own roundings; the one
rounding of a result to float, 2^-23 |result|, is added by the tests.

THE PARAMETERS, value q and bar dq (|kernel's binary64 q - this q| <= dq):
  EDT, T20, T30   decay_reference.times for (0, -10), (-5, -25), (-5, -35); dq = rel |q| with that function's rel.
  C50, C80        q = C10 (ln early - ln late), early = E[0] - E[ke], late = E[ke].  Per evaluation: early is one rounded difference
                  (relative U: ln early moves by U), each logarithm is good to 4 U |ln|, the difference and the product with C10 are
                  rounded (2 U |q|).  dq = C10 (16 U (|ln early| + |ln late|) + 4 U) + 8 U |q|, with room to spare; the first term is
                  ABSOLUTE: C passes through 0 dB, where a relative bar would vanish.
  D50             q = (E[0] - E[k50]) / E[0]: two roundings per evaluation; dq = 8 U |q|.
  Ts              q = (sum_{k >= 1} E[k]) / (fs E[0]): a sum of nbins - 1 non-negative terms in any order errs by (nbins - 2) U relative,
                  the product and the quotient by U each; dq = (nbins + 16) 2^-52 |q|.
THE LOSS.  d = q - target, loss = sum_p weight d^2 over the parameters that count (weight > 0, q finite):
  loss_bar = sum_p weight (2 |d| dq + dq^2) + 32 U loss   (the moved d; three roundings per term and up to six additions, twice).
THE ADJOINT.  c_p = 2 weight d, dc_p = 2 weight dq + 4 U |c_p|.  g[k] is a sum of TERMS, each a coefficient of the row times a function
of E[k] or a constant; the coefficient's bar propagates, the roundings of a term's own evaluation are relative to the term:
  time p          A = c K, K = 60 C10 / (s^2 fs Sxx); s errs like the time (rel), so dA = dc |K| + |A| (2 rel + 8 U);
                  term A xc_k / E[k], bar dA |xc_k| / E[k];
  C_te            at 0: c C10 / early, bar dc C10 / early; at ke: c C10 (1 / early + 1 / late), bar dc C10 (1 / early + 1 / late);
  D50             at k50: c / E[0], bar dc / E[0]; at 0: c E[k50] / E[0]^2, bar dc E[k50] / E[0]^2;
  Ts              every k >= 1: c / (fs E[0]), bar dc / (fs E[0]); at 0: c Ts / E[0], bar (dc |Ts| + |c| dq) / E[0].
  A term is at most six roundings (6 U relative) per evaluation, and a prefix of j + 1 bins is added in some order on both sides
  (2 j U of the sum of the |terms|): together at most (j + 16) 2^-52 sum_{k <= j} |terms of g_k| — the prefix's cancellation allowance.
  w_j = 2 H_j sum_{k <= j} g_k;   c_j = 2 |H_j| [ (j + 16) 2^-52 sum_{k <= j} |terms of g_k| + sum_{k <= j} (bars of the terms of g_k) ];
  the product with 2 H_j and the rounding to float are the tests' 2^-23 |w|."""
import numpy as np

import decay_reference as dref
from decay_reference import U

C10 = 10.0 / np.log(10.0)
NPARAMS = 7
EDT, T20, T30, C50, C80, D50, TS = range(NPARAMS)
LEVELS = ((0.0, -10.0), (-5.0, -25.0), (-5.0, -35.0))
EARLY = (0.05, 0.08)


def bin_of(seconds, fs, nbins):
    """(uint64_t) (seconds * fs + 0.5), or None where that bin lies behind the row's end."""
    x = seconds * fs + 0.5
    return int(x) if x < nbins else None


def row(e, sample_rate):
    """One row (float64 [nbins]): a dict with q [7] (NaN: not available), dq [7] and what the adjoint needs."""
    e = np.asarray(e, dtype=np.float64)
    nbins = e.shape[0]
    fs = float(np.float32(sample_rate))
    out = {"q": np.full(NPARAMS, np.nan), "dq": np.zeros(NPARAMS), "fs": fs, "time": [None] * 3, "ke": [bin_of(t, fs, nbins) for t in EARLY]}
    if not e[0] > 0:
        return out
    q, dq = out["q"], out["dq"]
    for p, (db_begin, db_end) in enumerate(LEVELS):
        w = dref.window(e, db_begin, db_end)
        if w is None:
            continue
        seconds, rel = dref.times(e[None, :], fs, db_begin, db_end)
        k0, k1 = w
        n = k1 - k0
        level = 10.0 * np.log10(e[k0:k1] / e[0])
        xc = np.arange(n, dtype=np.float64) - 0.5 * (n - 1)
        sxx = n * (float(n) * n - 1.0) / 12.0
        q[p], dq[p] = seconds[0], rel[0] * abs(seconds[0])
        out["time"][p] = {"k0": k0, "k1": k1, "xc": xc, "sxx": sxx, "slope": float((xc * level).sum()) / sxx, "rel": rel[0]}
    for i, ke in enumerate(out["ke"]):
        if ke is None:
            continue
        early, late = e[0] - e[ke], e[ke]
        if early > 0 and late > 0:
            le, ll = np.log(early), np.log(late)
            q[C50 + i] = C10 * (le - ll)
            dq[C50 + i] = C10 * (16.0 * U * (abs(le) + abs(ll)) + 4.0 * U) + 8.0 * U * abs(q[C50 + i])
    if out["ke"][0] is not None:
        q[D50] = (e[0] - e[out["ke"][0]]) / e[0]
        dq[D50] = 8.0 * U * abs(q[D50])
    q[TS] = e[1:].sum() / (fs * e[0])
    dq[TS] = (nbins + 16) * 2.0 ** -52 * abs(q[TS])
    return out


def params(e, sample_rate):
    """(q, dq): float64 [nrows][7] each, NaN in q where a parameter is not available."""
    rows = [row(r, sample_rate) for r in np.asarray(e, dtype=np.float64)]
    return np.array([r["q"] for r in rows]), np.array([r["dq"] for r in rows])


def row_loss(e, sample_rate, targets, weights, adjoint=True):
    """One row: a dict with loss, loss_bar, counts, and (adjoint) g, gabs, dg [nbins]: g = dL/dE, the sum of the |terms| of every bin and
    the sum of their propagated bars."""
    e = np.asarray(e, dtype=np.float64)
    nbins = e.shape[0]
    r = row(e, sample_rate)
    q, dq, fs = r["q"], r["dq"], r["fs"]
    t, wt = np.asarray(targets, dtype=np.float64), np.asarray(weights, dtype=np.float64)
    counts = (wt > 0) & np.isfinite(q)
    d = np.where(counts, np.where(counts, q, 0.0) - t, 0.0)
    wt = np.where(counts, wt, 0.0)
    dq = np.where(counts, dq, 0.0)
    loss = float((wt * d * d).sum())
    out = {"loss": loss, "loss_bar": float((wt * (2.0 * np.abs(d) * dq + dq * dq)).sum()) + 32.0 * U * loss, "counts": bool(counts.any()), "q": q}
    if not adjoint:
        return out
    c = 2.0 * wt * d
    dc = 2.0 * wt * dq + 4.0 * U * np.abs(c)
    g, gabs, dg = np.zeros(nbins), np.zeros(nbins), np.zeros(nbins)

    def add(at, term, bar):
        g[at] += term
        gabs[at] += np.abs(term)
        dg[at] += bar

    for p in range(3):
        w = r["time"][p]
        if w is None or not counts[p]:
            continue
        k = 60.0 * C10 / (w["slope"] ** 2 * fs * w["sxx"])
        a, da = c[p] * k, dc[p] * abs(k) + abs(c[p] * k) * (2.0 * w["rel"] + 8.0 * U)
        ek = e[w["k0"]:w["k1"]]
        add(slice(w["k0"], w["k1"]), a * w["xc"] / ek, da * np.abs(w["xc"]) / ek)
    for i, ke in enumerate(r["ke"]):
        if not counts[C50 + i]:
            continue
        early, late = e[0] - e[ke], e[ke]
        add(0, c[C50 + i] * C10 / early, dc[C50 + i] * C10 / early)
        add(ke, -c[C50 + i] * C10 * (1.0 / early + 1.0 / late), dc[C50 + i] * C10 * (1.0 / early + 1.0 / late))
    if counts[D50]:
        k50 = r["ke"][0]
        add(k50, -c[D50] / e[0], dc[D50] / e[0])
        add(0, c[D50] * e[k50] / e[0] ** 2, dc[D50] * e[k50] / e[0] ** 2)
    if counts[TS]:
        add(slice(1, nbins), np.full(nbins - 1, c[TS] / (fs * e[0])), np.full(nbins - 1, dc[TS] / (fs * e[0])))
        add(0, -c[TS] * q[TS] / e[0], (dc[TS] * abs(q[TS]) + abs(c[TS]) * dq[TS]) / e[0])
    out.update(g=g, gabs=gabs, dg=dg)
    return out


def loss(h, e, sample_rate, targets, weights):
    """A dict, all float64: loss_rows [nrows], loss_bar [nrows], w and c [nrows][nbins] (the adjoint and its bar without the 2^-23 |w| of
    the rounding to float), counts [nrows] (the row has a parameter that counts), q [nrows][7]."""
    h, e = np.asarray(h, dtype=np.float64), np.asarray(e, dtype=np.float64)
    nrows, nbins = e.shape
    rows = [row_loss(e[r], sample_rate, targets[r], weights[r]) for r in range(nrows)]
    j = np.arange(nbins, dtype=np.float64)[None, :]
    prefix = np.cumsum(np.array([r["g"] for r in rows]), axis=1)
    allowance = (j + 16.0) * 2.0 ** -52 * np.cumsum(np.array([r["gabs"] for r in rows]), axis=1)
    return {"loss_rows": np.array([r["loss"] for r in rows]), "loss_bar": np.array([r["loss_bar"] for r in rows]),
            "w": 2.0 * h * prefix, "c": 2.0 * np.abs(h) * (allowance + np.cumsum(np.array([r["dg"] for r in rows]), axis=1)),
            "counts": np.array([r["counts"] for r in rows]), "q": np.array([r["q"] for r in rows])}
