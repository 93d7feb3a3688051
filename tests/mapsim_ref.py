"""The numpy restatement of c3d_map_similarity's definitions (include/c3d.h, "Reproducibility of contact maps"): the clipped box mean with
the header's summation order, a stratum's kept pairs, moments and doubled average ranks (scipy.stats.rankdata times two, A and B as
Python ints), and rho_s, w_s and scc with the header's operations in its order.  Smoothing works per stratum on a band, so a large n with
few strata stays cheap.  tests/test_mapsim_ref.py holds this file to scipy and to hand-made cases; tests/test_gpu_mapsim.py holds the
device to it."""
import math

import numpy as np
from scipy.stats import rankdata


def smooth_direct(M, h):
    """definition 1 as the direct double loop over the whole map (small n only): t(r) over the column window in ascending c from the first
    term, their sum over the row window in ascending r from the first, one division"""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    X = np.empty((n, n))
    for i in range(n):
        r0, r1 = max(0, i - h), min(n - 1, i + h)
        for j in range(n):
            c0, c1 = max(0, j - h), min(n - 1, j + h)
            x = None
            for r in range(r0, r1 + 1):
                t = M[r, c0]
                for c in range(c0 + 1, c1 + 1):
                    t = t + M[r, c]
                x = t if x is None else x + t
            X[i, j] = x / float((r1 - r0 + 1) * (c1 - c0 + 1))
    return X


def _add(acc, started, val, valid):
    """acc <- val where this is the first valid term, acc + val where it is a later one"""
    acc = np.where(valid & ~started, val, np.where(valid, acc + val, acc))
    return acc, started | valid


def smooth_stratum(M, h, s):
    """X(i, i+s), i < n - s, separably: the row sums of a cell's column window once a row offset, then added down the rows — the same
    additions in the same order as smooth_direct, so the same bits"""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    i = np.arange(n - s)
    j = i + s
    x, x_on = np.zeros(n - s), np.zeros(n - s, dtype=bool)
    for dr in range(-h, h + 1):
        r = i + dr
        r_ok = (r >= 0) & (r < n)
        t, t_on = np.zeros(n - s), np.zeros(n - s, dtype=bool)
        for dc in range(-h, h + 1):
            c = j + dc
            ok = r_ok & (c >= 0) & (c < n)
            t, t_on = _add(t, t_on, M[np.clip(r, 0, n - 1), np.clip(c, 0, n - 1)], ok)
        x, x_on = _add(x, x_on, t, r_ok)
    rows = np.minimum(n - 1, i + h) - np.maximum(0, i - h) + 1
    cols = np.minimum(n - 1, j + h) - np.maximum(0, j - h) + 1
    return x / (rows * cols).astype(np.float64)


def smooth_full(M, h):
    """the whole smoothed map, separably and vectorised: the same additions in the same order once more (for a wide band of a small map)"""
    M = np.asarray(M, dtype=np.float64)
    n = M.shape[0]
    k = np.arange(n)
    t, t_on = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    for d in range(-h, h + 1):
        ok = np.broadcast_to(((k + d >= 0) & (k + d < n))[None, :], (n, n))
        t, t_on = _add(t, t_on, M[:, np.clip(k + d, 0, n - 1)], ok)
    x, x_on = np.zeros((n, n)), np.zeros((n, n), dtype=bool)
    for d in range(-h, h + 1):
        ok = np.broadcast_to(((k + d >= 0) & (k + d < n))[:, None], (n, n))
        x, x_on = _add(x, x_on, t[np.clip(k + d, 0, n - 1), :], ok)
    width = np.minimum(n - 1, k + h) - np.maximum(0, k - h) + 1
    return x / (width[:, None] * width[None, :]).astype(np.float64)


def smooth_band(M, h, lo, hi):
    """[S, n]: row s - lo holds X(i, i+s) for i < n - s, then zeros (the layout of the entry's `smoothed`); per stratum, or from the whole
    smoothed map where that is less work"""
    n = np.asarray(M).shape[0]
    out = np.zeros((hi - lo + 1, n))
    X = smooth_full(M, h) if (hi - lo + 1) * (2 * h + 1) > 2 * n else None
    for s in range(lo, hi + 1):
        out[s - lo, :n - s] = smooth_stratum(M, h, s) if X is None else np.diagonal(X, s)
    return out


def kept_pairs(x, y, keep_zeros=False):
    """definition 2: the mask of the pairs that stay in the stratum"""
    x, y = np.asarray(x), np.asarray(y)
    return np.ones(len(x), dtype=bool) if keep_zeros else ~((x == 0) & (y == 0))


def rank_sums(v):
    """definition 4 for the kept values v: N sum a^2 - T^2 with a the doubled average ranks, as a Python int"""
    N = len(v)
    if N == 0:
        return 0
    a = np.rint(2.0 * rankdata(np.asarray(v) + 0.0)).astype(np.int64)           # (+ 0.0: -0.0 ranks as 0.0)
    T = N * (N + 1)
    return N * int(np.dot(a, a)) - T * T                                          # (sum a^2 <= 4 N^3 < 2^63 up to N = 16384)


def stratum(x, y, keep_zeros=False):
    """definitions 2 to 4 for one stratum: ((Cxy, Cxx, Cyy), (N, A, B))"""
    k = kept_pairs(x, y, keep_zeros)
    xk, yk = np.asarray(x, dtype=np.float64)[k], np.asarray(y, dtype=np.float64)[k]
    N = len(xk)
    if N == 0:
        return (0.0, 0.0, 0.0), (0, 0, 0)
    dx, dy = xk - xk.sum() / N, yk - yk.sum() / N
    return (float((dx * dy).sum()), float((dx * dx).sum()), float((dy * dy).sum())), (N, rank_sums(xk), rank_sums(yk))


def rho_w(moments, counts):
    """definition 5: (rho_s, w_s) of one stratum from its moments and counts, the header's operations in its order"""
    cxy, cxx, cyy = (float(v) for v in moments)
    N, A, B = (int(v) for v in counts)
    if N >= 3 and A > 0 and B > 0 and cxx > 0 and cyy > 0:
        Nd = float(N)
        return cxy / math.sqrt(cxx * cyy), math.sqrt(float(A) * float(B)) / (((4.0 * Nd) * Nd) * Nd)
    return math.nan, 0.0


def combine(moments, counts):
    """definitions 5 and 6 for one pair: moments, counts [S, 3] -> (rho [S], w [S], scc)"""
    S = len(moments)
    rho, w = np.empty(S), np.empty(S)
    num = den = 0.0
    any_counted = False
    for s in range(S):
        rho[s], w[s] = rho_w(moments[s], counts[s])
        if not math.isnan(rho[s]):
            num += w[s] * rho[s]
            den += w[s]
            any_counted = True
    return rho, w, (num / den if any_counted else math.nan)


def pairs(Q):
    return [(p, q) for p in range(Q) for q in range(p + 1, Q)]


def map_similarity(maps, h=(0,), min_sep=0, max_sep=0, keep_zeros=False):
    """The entry restated: a dict with the outputs' shapes — "scc" [n_h, Q, Q], "rho" and "w" [n_h, P, S], "moments" [n_h, P, S, 3],
    "counts" [n_h, P, S, 3] (object: Python ints), "smoothed" [n_h, Q, S, n]."""
    maps = np.asarray(maps, dtype=np.float64)
    Q, n = maps.shape[0], maps.shape[1]
    lo, hi = min_sep, max_sep if max_sep else n - 1
    S, pr = hi - lo + 1, pairs(Q)
    H = len(h)
    out = {"scc": np.ones((H, Q, Q)), "rho": np.empty((H, len(pr), S)), "w": np.empty((H, len(pr), S)), "moments": np.empty((H, len(pr), S, 3)),
           "counts": np.empty((H, len(pr), S, 3), dtype=object), "smoothed": np.empty((H, Q, S, n))}
    for k, hk in enumerate(h):
        for m in range(Q):
            out["smoothed"][k, m] = smooth_band(maps[m], hk, lo, hi)
        for e, (p, q) in enumerate(pr):
            for s in range(lo, hi + 1):
                mo, co = stratum(out["smoothed"][k, p, s - lo, :n - s], out["smoothed"][k, q, s - lo, :n - s], keep_zeros)
                out["moments"][k, e, s - lo] = mo
                out["counts"][k, e, s - lo] = co
            out["rho"][k, e], out["w"][k, e], scc = combine(out["moments"][k, e], out["counts"][k, e])
            out["scc"][k, p, q] = out["scc"][k, q, p] = scc
    return out
