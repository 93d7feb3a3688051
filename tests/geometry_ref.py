"""A model's geometry and the distance against separation restated in numpy: the yardstick of tests/test_gpu_geometry.py
(c3d_geometry_replicas, c3d_separation_profile).

Distances come from tests/ensemble_ref.distances, sqrt(((ux ux) + uy uy) + uz uz) in float64 with every operation rounded on its own.
Every definition is written in the order include/c3d.h gives for it: a clash is `d <= cutoff` over the pairs i < j, j - i >= sep (sep = 1:
the reference's clash_count, chromosome3D.pl:693-714), a contact is a strict `d < cutoff`, every sd is the two-pass population form, the
nearest partner of a bead that has none at |i-j| >= sep is +inf."""
import numpy as np

from tests.ensemble_ref import distances

FIELDS = 6


def _two_pass(v):
    """(mean, population sd about that mean) of a vector"""
    mean = v.sum() / len(v)
    e = v - mean
    return mean, np.sqrt((e * e).sum() / len(v))


def geometry(x, cutoff=3.5, sep=1):
    """{"clashes": int, "bead_clashes": [n] int, "nearest": [n], "chain": [6]} of one model [n, 3]"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    d = distances(x)
    i, j = np.indices((n, n))
    counted = np.abs(i - j) >= sep
    hit = counted & (d <= cutoff)
    bead = hit.sum(axis=1)
    clashes = int(np.triu(hit, 1).sum())                 # the pairs i < j
    nearest = np.where(counted, d, np.inf).min(axis=1)
    bond_mean, bond_sd = _two_pass(np.array([d[a, a + 1] for a in range(n - 1)]))
    i2_mean, i2_sd = _two_pass(np.array([d[a, a + 2] for a in range(n - 2)]))
    u = x - x.sum(axis=0) / n
    rg = np.sqrt(((u * u).sum(axis=1)).sum() / n)
    extent = d.max()
    return {"clashes": clashes, "bead_clashes": bead.astype(np.int64), "nearest": nearest,
            "chain": np.array([bond_mean, bond_sd, i2_mean, i2_sd, rg, extent])}


def separation_profile(models, pick=None, cutoff=None):
    """(mean [n], sd [n], contact [n] or None, count [n] int64 or None, largest [n]) over d_k(i, i+s) for all i and k in pick (None: all
    models, in index order); count[s] is the integer number of those values below cutoff, contact = count / ((n - s) Kp); largest[s] is
    the largest of the values, which bounds every term of the sums.  s = 0: mean 0, sd 0, contact 1."""
    pick = list(range(len(models))) if pick is None else [int(k) for k in pick]
    d = {k: distances(models[k]) for k in set(pick)}
    n = len(d[pick[0]])
    mean, sd, largest = np.zeros(n), np.zeros(n), np.zeros(n)
    count = np.zeros(n, dtype=np.int64)
    for s in range(n):
        v = np.concatenate([np.diagonal(d[k], s) for k in pick])          # k in list order
        mean[s], sd[s] = _two_pass(v)
        largest[s] = v.max()
        if cutoff is not None:
            count[s] = int((v < cutoff).sum())
    if cutoff is None:
        return mean, sd, None, None, largest
    terms = (n - np.arange(n)) * len(pick)
    return mean, sd, count / terms, count, largest
