"""A model's fit to the data bead by bead, restated in numpy: the yardstick of tests/test_gpu_bead.py (c3d_bead_scores).
tests/test_bead_ref.py holds it to scipy.stats.spearmanr row by row and to the reference's own assessment of the bundled models.

Every definition is written as include/c3d.h gives it.  Row i holds the partners J(i) = { j : |i-j| >= rng }; the distance is
sqrt(((ux ux) + uy uy) + uz uz) rounded to integer thousandths as "%.3f" rounds (tests/stratified_ref.round_milli); a and b are the
doubled average ranks inside the row (integers); C, A, B are Python ints; rho is formed from them with float operations in the header's
order.  The tallies run over the partners with a target t10 > 0 tenths and |i-j| >= min_sep, on both sides of i, with the reference's
comparisons in doubles (d = q / 1000.0, t = t10 / 10.0) and the deviation as an exact integer of thousandths."""
import numpy as np

from tests.stratified_ref import FARTHEST, if_ranks, rho_of, round_milli, stratum_sums

FIELDS = 3


def partners(n, i, rng):
    """J(i), ascending: the beads at least rng away from bead i"""
    return np.concatenate([np.arange(0, max(0, i - rng + 1)), np.arange(min(n, i + rng), n)])


def row_milli(x, i, js):
    """the "%.3f" distances of bead i to the beads js of one model [n, 3], int64 thousandths: every operation rounded on its own"""
    x = np.asarray(x, dtype=np.float64)
    u = x[i] - x[js]
    return round_milli(np.sqrt(((u[:, 0] * u[:, 0]) + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]))


def row_sums(IF, x, i, rng, cache=None):
    """(C, A, B) of row i, Python ints; (0, 0, 0) for a row of fewer than two partners; cache: keeps the IF ranks of a row from one model
    of a matrix to the next"""
    n = len(x)
    js = partners(n, i, rng)
    if len(js) <= 1:
        return 0, 0, 0
    q = row_milli(x, i, js)
    assert (q <= FARTHEST).all()
    a = None
    if cache is not None:
        if i not in cache:
            cache[i] = if_ranks(np.asarray(IF[i], dtype=np.float64)[js])
        a = cache[i]
    return stratum_sums(np.asarray(IF[i], dtype=np.float64)[js], q, a)


def tally(t10, min_sep, x, i):
    """(restrained, satisfied, dev_milli) of bead i, Python ints: t10 [n, n] integer tenths, 0 = no target"""
    n = len(x)
    j = np.arange(n)
    js = j[(np.abs(j - i) >= max(min_sep, 1)) & (np.asarray(t10[i]) > 0)]
    if len(js) == 0:
        return 0, 0, 0
    q = row_milli(x, i, js)
    t = np.asarray(t10[i], dtype=np.int64)[js]
    d, tv = q.astype(np.float64) / 1000.0, t.astype(np.float64) / 10.0
    sat = int((d < tv + 0.5).sum()) - int((d < tv - 0.5).sum())
    over, under = d > tv + 0.2, d < tv - 0.2
    dev = sum(int(v) for v in (q - 100 * t)[over]) + sum(int(v) for v in (100 * t - q)[under])
    return len(js), sat, dev


def bead_scores(IF, x, rng=3, beads=None, t10=None, min_sep=1, cache=None):
    """{"rho" [B], "sums" [B, 3] int64 (IF given), "restrained" [B], "satisfied" [B], "dev_milli" [B] (t10 given)} of one model [n, 3];
    beads: the indices asked for (default: every bead)"""
    n = len(x)
    beads = list(range(n)) if beads is None else [int(b) for b in beads]
    out = {}
    if IF is not None:
        sums = [row_sums(IF, x, i, rng, cache) for i in beads]
        out["sums"] = np.array(sums, dtype=np.int64).reshape(len(beads), FIELDS)
        out["rho"] = np.array([rho_of(*s) for s in sums], dtype=np.float64)
    if t10 is not None:
        t = [tally(t10, min_sep, x, i) for i in beads]
        out["restrained"] = np.array([v[0] for v in t], dtype=np.int32)
        out["satisfied"] = np.array([v[1] for v in t], dtype=np.int32)
        out["dev_milli"] = np.array([v[2] for v in t], dtype=np.int64)
    return out


def targets_of_restraints(n, ri, rj, rt10):
    """the integer tenths [n, n] a context keeps after set_restraints(n, ri, rj, rt10) (1-based rows; a later row of a pair overwrites)"""
    t = np.zeros((n, n), dtype=np.int64)
    for i, j, v in zip(ri, rj, rt10):
        if v > 0:
            t[i - 1, j - 1] = t[j - 1, i - 1] = v
    return t

