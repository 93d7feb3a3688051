"""The numpy restatement of the ensemble's distance map (tests/ensemble_ref.py) held to facts that need no device: it is the yardstick of
tests/test_gpu_ensemble.py."""
import numpy as np
import pytest

from tests import ensemble_ref as R
from tests.util import load_if, load_pdb_xyz, model_pdb, random_coil


def _models(n, K, seed=0):
    return [random_coil(n, seed + k).astype(np.float64) for k in range(K)]


@pytest.mark.parametrize("n, rng", [(12, 1), (40, 3), (93, 3)])
def test_spearman_is_scipys_on_the_same_arrays(n, rng):
    """Continuous values and heavily tied ones (a contact map of three models has four values)."""
    stats = pytest.importorskip("scipy.stats")
    models = _models(n, 3, seed=n)
    mean, _, contact, _ = R.ensemble_map(models, cutoff=9.0)
    gen = np.random.default_rng(n)
    IF = gen.integers(0, 50, size=(n, n)).astype(np.float64)
    IF = IF + IF.T
    i, j = R.ranked_pairs(n, rng)
    assert len(i) == (n - rng) * (n - rng + 1)
    for M in (mean, contact):
        want = stats.spearmanr(IF[i, j], M[i, j]).correlation
        assert abs(R.spearman(IF, M, rng) - want) <= 1e-12
    assert len(np.unique(contact)) <= 4
    assert np.isnan(R.spearman(IF, np.ones((n, n)), rng))                       # a constant map has no ranks to correlate


def test_a_single_model_has_its_own_distances_and_no_spread():
    x = _models(57, 1)[0]
    mean, sd, contact, count = R.ensemble_map([x], cutoff=7.6)
    d = R.distances(x)
    assert np.array_equal(mean, d) and np.array_equal(sd, np.zeros_like(d))
    assert np.array_equal(count, (d < 7.6).astype(np.int64)) and np.array_equal(contact, (d < 7.6).astype(np.float64))
    assert np.array_equal(np.diag(mean), np.zeros(57)) and np.array_equal(np.diag(contact), np.ones(57))
    u = x[3] - x[11]
    assert d[3, 11] == np.sqrt(((u[0] * u[0]) + u[1] * u[1]) + u[2] * u[2]) and np.array_equal(d, d.T)


def test_a_repeated_pick_counts_twice_and_the_list_order_is_the_summation_order():
    models = _models(31, 3, seed=5)
    d = [R.distances(x) for x in models]
    mean, sd, contact, count = R.ensemble_map(models, pick=[0, 0, 1], cutoff=8.0)
    assert np.array_equal(mean, ((d[0] + d[0]) + d[1]) / 3)
    assert np.array_equal(count, 2 * (d[0] < 8.0) + (d[1] < 8.0)) and np.array_equal(contact, count / 3)
    plain = R.ensemble_map(models, pick=[0, 1])[0]
    assert np.abs(mean - plain).max() > 0.1                                      # and it is another map than that of [0, 1]
    var = (2 * (d[0] - mean) ** 2 + (d[1] - mean) ** 2) / 3
    assert np.abs(sd - np.sqrt(var)).max() <= 1e-12
    assert np.array_equal(R.ensemble_map(models)[0], R.ensemble_map(models, pick=[0, 1, 2])[0])
    assert np.array_equal(R.ensemble_map(models, pick=[2, 0])[0], (d[2] + d[0]) / 2)


@pytest.mark.parametrize("K", [2, 3, 7, 20])
def test_copies_of_one_model_have_no_spread(K):
    x = _models(64, 1, seed=9)[0] * 25.0                                         # distances up to several hundred Angstrom
    mean, sd, _, _ = R.ensemble_map([x] * K)
    d = R.distances(x)
    assert sd.max() <= 1e-12
    if K <= 7:
        assert (np.abs(mean - d) <= 2 * np.spacing(d)).all()


def test_one_bundled_model_scores_as_the_host_helper_does_up_to_its_rounding(built):
    """chr21_1mb, K = 1: rho_mean of the restatement against c3d_spearman_if_dist, which rounds every distance to 3 decimals before it
    ranks them and so ties a few pairs the exact distances keep apart.  Measured gap: 8.35e-07 (restatement -0.8446657085, helper
    -0.8446648736); asserted: 4 x that."""
    from chromosome3d_amd import pipeline
    IF = load_if("chr21_1mb")
    x = load_pdb_xyz(model_pdb("chr21_1mb"))
    mean = R.ensemble_map([x])[0]
    rho, host = R.spearman(IF, mean, 3), pipeline.spearman_IF_pdb(IF, x, 3)
    print(f"restatement {rho:.10f}, c3d_spearman_if_dist {host:.10f}, gap {abs(rho - host):.3e}")
    assert rho < -0.8 and abs(rho - host) <= 4 * 8.35e-07
