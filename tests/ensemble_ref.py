"""The ensemble's distance map restated in numpy: the yardstick of tests/test_gpu_ensemble.py (c3d_ensemble_map, c3d_ensemble_score).

Every operation is written in the order include/c3d.h gives for it: the distance is sqrt(((ux ux) + uy uy) + uz uz) in float64 with each
product and sum rounded on its own (numpy fuses nothing), the mean is summed model after model in list order and divided once, the sd is
the two-pass population form, a contact is a strict `<`, and the Spearman coefficient comes from average ranks over the ordered pairs
|i-j| >= range."""
import numpy as np


def distances(x):
    """[n, n] float64: the pair distances of one model [n, 3]"""
    x = np.asarray(x, dtype=np.float64)
    ux, uy, uz = (x[:, None, c] - x[None, :, c] for c in range(3))          # a component at a time: contiguous n x n arrays, the same operations
    return np.sqrt(((ux * ux) + uy * uy) + uz * uz)


def ensemble_map(models, pick=None, cutoff=None):
    """(mean, sd, contact-or-None, count-or-None) over models[k] for k in pick (None: all, in index order).  count is the integer number of
    models in which the pair is closer than cutoff; contact = count / Kp."""
    pick = list(range(len(models))) if pick is None else [int(k) for k in pick]
    Kp = len(pick)
    d = {k: distances(models[k]) for k in set(pick)}
    total = np.zeros_like(d[pick[0]])
    for k in pick:                                       # list order
        total = total + d[k]
    mean = total / Kp
    dev = np.zeros_like(mean)
    for k in pick:
        e = d[k] - mean
        dev = dev + e * e
    sd = np.sqrt(dev / Kp)
    if cutoff is None:
        return mean, sd, None, None
    count = np.zeros(mean.shape, dtype=np.int64)
    for k in pick:
        count += d[k] < cutoff
    return mean, sd, count / Kp, count


def average_ranks(v):
    """average ranks 1..m of a vector, ties sharing the mean of their positions"""
    _, inv, cnt = np.unique(np.asarray(v), return_inverse=True, return_counts=True)
    below = np.cumsum(cnt) - cnt
    return (below + 0.5 * (cnt + 1.0))[inv]


def ranked_pairs(n, rng):
    """index arrays (i, j) of the ordered pairs |i-j| >= rng, row by row"""
    i, j = np.indices((n, n))
    keep = np.abs(i - j) >= rng
    return i[keep], j[keep]


def spearman(A, B, rng=3):
    """Spearman coefficient of two [n, n] matrices over the ordered pairs |i-j| >= rng (NaN when one of them is constant there)"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    i, j = ranked_pairs(len(A), rng)
    ra, rb = average_ranks(A[i, j]), average_ranks(B[i, j])
    ma = 0.5 * (len(ra) + 1.0)
    a, b = ra - ma, rb - ma
    with np.errstate(invalid="ignore", divide="ignore"):
        return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))
