"""tests/geometry_ref.py, the numpy restatement that tests/test_gpu_geometry.py holds the device to, held in turn to what the project
already trusts: the reference's own clash counts of the seven bundled models (tests/golden/front_half_golden.json, written by the
reference's clash_count through tests/golden/make_golden.pl), tests/util.chain_stats, and the integer contact counts of
tests/ensemble_ref.ensemble_map."""
import os

import numpy as np
import pytest

from tests import ensemble_ref as E
from tests import geometry_ref as G
from tests.util import GOLD, chain_stats, golden, load_pdb_xyz, random_coil

U = 2.0 ** -53
CLASH_3P5 = {"chr13_1mb": 12, "chr19_500kb": 5, "chr1_500kb": 1022, "chr20_1mb": 1, "chr21_1mb": 0, "chr22_1mb": 0, "chr4_1mb": 117}


def test_the_golden_file_holds_the_seven_counts():
    g = golden()
    assert {cid: g[cid]["clash_3p5"] for cid in g} == CLASH_3P5


@pytest.mark.parametrize("cid", sorted(CLASH_3P5))
def test_the_restatement_reproduces_the_references_clash_count(cid):
    g = golden()[cid]
    x = load_pdb_xyz(os.path.join(GOLD, "models", g["model"]))
    assert len(x) == g["n"]
    got = G.geometry(x, 3.5, 1)
    assert got["clashes"] == g["clash_3p5"]
    assert int(got["bead_clashes"].sum()) == 2 * got["clashes"]
    d = E.distances(x)[np.triu_indices(len(x), 1)]
    assert np.abs(d - 3.5).min() > 1e-6                      # no pair at the cutoff: the count does not hang on a rounding


@pytest.mark.parametrize("n", [3, 64, 257])
def test_chain_stats_agrees_with_the_chain_fields(n):
    """Sums of n same-sign terms in two orders differ by at most 2 n 2^-53 relative; 8 n 2^-53 x the largest term covers the division, the
    square root and the mean's own error."""
    x = random_coil(n, 1000 + n).astype(np.float64)
    got = G.geometry(x)["chain"]
    want = chain_stats(x)[:5]
    d = E.distances(x)
    tol = 8 * n * U * d.max()
    for f in range(5):
        assert abs(got[f] - want[f]) <= tol, (f, got[f], want[f])
    assert got[5] == d.max()
    assert G.geometry(x, sep=n - 1)["nearest"][0] == d[0, n - 1] and (n == 3 or np.isinf(G.geometry(x, sep=n - 1)["nearest"][1]))


@pytest.mark.parametrize("pick", [None, [3, 1], [2, 0, 2]])
def test_profile_counts_are_the_diagonal_sums_of_the_ensemble_map(pick):
    models = [random_coil(70, 70 + k).astype(np.float64) for k in range(4)]
    mean, sd, contact, count, largest = G.separation_profile(models, pick, 7.6)
    mmean, msd, mcontact, mcount = E.ensemble_map(models, pick, 7.6)
    Kp = 4 if pick is None else len(pick)
    for s in range(70):
        assert count[s] == int(np.diagonal(mcount, s).sum())
        assert abs(mean[s] - np.diagonal(mmean, s).mean()) <= 8 * (70 - s) * Kp * U * largest[s]
    assert (mean[0], sd[0], contact[0]) == (0.0, 0.0, 1.0)
    assert 0 < contact[10] < 1 and (sd[1:] >= 0).all()
    assert G.separation_profile(models, pick)[2] is None
