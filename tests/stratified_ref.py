"""IF against model distance inside every genomic separation, restated in numpy: the yardstick of tests/test_gpu_stratified.py
(c3d_stratified_score).  tests/test_stratified_ref.py holds it to scipy.stats.spearmanr and to Python's "%.3f".

Every definition is written as include/c3d.h gives it: stratum s holds the N = n - s pairs (i, i + s); the distance is
sqrt(((ux ux) + uy uy) + uz uz) rounded to integer thousandths as "%.3f" rounds; a and b are the doubled average ranks
(scipy.stats.rankdata, method "average", times two: integers); C, A, B are Python ints; rho and scc are formed from them with float
operations in the header's order."""
import math

import numpy as np
from scipy.stats import rankdata

FIELDS = 3
FARTHEST = 50000000          # thousandths of an A: the limit of c3d_score_replicas


def diagonal_distances(x, s):
    """d(i, i + s), i = 0 .. n - s - 1, of one model [n, 3]: every operation rounded on its own, as tests/ensemble_ref.distances"""
    x = np.asarray(x, dtype=np.float64)
    u = x[:len(x) - s] - x[s:]
    return np.sqrt(((u[:, 0] * u[:, 0]) + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def _product_error(a, b):
    """a * b - fl(a * b), exactly (Dekker's product with Veltkamp's split): what fma(a, b, -fl(a b)) gives"""
    p = a * b

    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def round_milli(d):
    """int64 thousandths of d >= 0 as sprintf("%.3f") rounds: to nearest, a tie of the exact product d x 1000 to even"""
    d = np.asarray(d, dtype=np.float64)
    k = np.float64(1000.0)
    p = d * k
    err = _product_error(d, np.broadcast_to(k, d.shape))
    r = np.rint(p)
    diff = p - r
    tie = np.abs(diff) == 0.5
    r = np.where(tie & (err > 0), np.floor(p) + 1.0, r)
    r = np.where(tie & (err < 0), np.floor(p), r)
    return r.astype(np.int64)


def doubled_ranks(v):
    """2 x the average ranks of v, as Python-int-safe int64: #{smaller} + #{not larger} + 1"""
    r2 = 2.0 * rankdata(v, method="average")
    out = np.rint(r2).astype(np.int64)
    assert np.array_equal(out.astype(np.float64), r2)
    return out


def if_ranks(if_values):
    """the doubled average ranks of a stratum of IF; -0.0 is 0.0"""
    return doubled_ranks(np.asarray(if_values, dtype=np.float64) + 0.0)


def stratum_sums(if_values, dist_milli, a=None):
    """(C, A, B) of one stratum, Python ints; a: if_ranks(if_values) where the caller has them"""
    N = len(dist_milli)
    a = if_ranks(if_values) if a is None else a
    b = doubled_ranks(dist_milli)
    assert N <= 16383                                  # every dot product below is at most 4 N^3 < 1.8e13: exact in int64
    T = N * (N + 1)
    C = N * int(np.dot(a, b)) - T * T                  # Python ints from here on
    A = N * int(np.dot(a, a)) - T * T
    B = N * int(np.dot(b, b)) - T * T
    return C, A, B


def rho_of(C, A, B):
    return float(C) / math.sqrt(float(A) * float(B)) if A > 0 and B > 0 else math.nan


def scc_of(sums, n, strata):
    """the combined coefficient from {s: (C, A, B)}: two sequential sums over ascending s"""
    num = den = 0.0
    counted = False
    for s in strata:
        C, A, B = sums[s]
        if A > 0 and B > 0:
            N = float(n - s)
            cN = N * N * N
            num += float(C) / cN
            den += math.sqrt(float(A) * float(B)) / cN
            counted = True
    return num / den if counted else math.nan


def stratified(IF, x, rng=3, max_sep=0, strata=None, cache=None):
    """{"rho": [n], "scc": float, "sums": [n, 3] int64 (every value is below 2.9e17)} of one model [n, 3]; strata: the separations to compute (default: all of
    rng .. max_sep or n - 1; a subset leaves the others NaN / 0 and scc over the subset); cache: a dict that keeps the IF ranks of a stratum from one model of a matrix to the next"""
    IF = np.asarray(IF, dtype=np.float64)
    n = len(IF)
    lo, hi = rng, (max_sep if max_sep else n - 1)
    strata = list(range(lo, hi + 1)) if strata is None else sorted(strata)
    rho = np.full(n, np.nan)
    sums = np.zeros((n, FIELDS), dtype=np.int64)
    got = {}
    for s in strata:
        q = round_milli(diagonal_distances(x, s))
        assert (q <= FARTHEST).all()
        a = None
        if cache is not None:
            if s not in cache:
                cache[s] = if_ranks(np.diagonal(IF, s))
            a = cache[s]
        got[s] = stratum_sums(np.diagonal(IF, s), q, a)
        sums[s] = got[s]
        rho[s] = rho_of(*got[s])
    return {"rho": rho, "scc": scc_of(got, n, strata), "sums": sums}
