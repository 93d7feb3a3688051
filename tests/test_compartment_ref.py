"""The numpy restatement of c3d_compartments (tests/compartment_ref.py) held to numpy.linalg.eigh of numpy.corrcoef of the O/E map, to
planted two-compartment chains, to the numbers recorded for chr1_500kb and to the definition's edge cases.  No GPU: the device is held to
the restatement by tests/test_gpu_compartments.py."""
import numpy as np
import pytest

from tests import compartment_ref as R
from tests.util import load_if, load_pdb_xyz, model_pdb

FIXTURES = ("chr21_1mb", "chr22_1mb", "chr1_500kb")


def _maps(cid):
    return load_if(cid), R.distance_map(load_pdb_xyz(model_pdb(cid)))


@pytest.mark.parametrize("cid", FIXTURES)
def test_the_iteration_reaches_eigh_of_corrcoef(cid):
    for M in _maps(cid):
        _, V, share, res = R.solve_map(M, 1, 3, 200)
        w, U = R.eigh_vectors(M, 1, 3)
        for a in range(3):
            gap = 1.0 - abs(V[a] @ U[a])
            print(cid, a, "1-|v.u|", gap, "residual", res[a], "share", share[a])
            assert gap <= 1e-12
            assert res[a] <= 1e-10
        live = int((R.row_stats(R.oe(M))[1] > 0).sum())
        assert np.abs(share - w[:3] / live).max() <= 1e-12


@pytest.mark.parametrize("n", (17, 64, 257))
def test_planted_chains_give_back_every_label(n):
    x, labels = R.planted_chain(n)
    _, V, _, res = R.solve_map(R.distance_map(x), 1, 1, 200)
    v = V[0] * np.sign(V[0] @ labels)
    assert res[0] < 1e-9
    assert (np.sign(v) == labels).all()


def test_the_numbers_recorded_for_chr1_500kb():
    IF, Dm = _maps("chr1_500kb")
    out = R.compartments([IF, Dm], True, 1, 1, 200)
    print("shares", out["share"][:, 0], "agreement", out["agreement"][0, 0, 0])
    assert abs(out["share"][0, 0] - 0.359) <= 0.002
    assert abs(out["share"][1, 0] - 0.385) <= 0.002
    assert abs(out["agreement"][0, 0, 0] - 0.931) <= 0.002


def test_a_row_without_spread_gets_zero():
    x, _ = R.planted_chain(24)
    M = R.distance_map(x)
    M[5, :] = M[:, 5] = 0.0                          # X(5, j) = 0 for j != 5 ... and 1 on the diagonal: spread
    M2 = M.copy()
    X = R.oe(M2)
    assert R.row_stats(X)[1][5] > 0
    X[5, :] = X[:, 5] = 1.0                          # a row of ones: no spread
    m, q = R.row_stats(X)
    assert q[5] == 0.0
    V, _, share, _ = R.solve_operator(lambda U: U @ X, m, q, 2, 50)
    assert (V[:, 5] == 0.0).all()
    assert np.isfinite(V).all() and np.isfinite(share).all()


def test_an_expected_of_zero_gives_one():
    M = np.zeros((9, 9))
    for i in range(8):
        M[i, i + 1] = M[i + 1, i] = 2.0 + i          # only the first diagonal holds anything
    E = R.expected(M)
    assert E[0] == 0.0 and E[1] > 0.0 and (E[2:] == 0.0).all()
    X = R.oe(M, 1, E)
    i, j = np.indices(X.shape)
    assert (X[np.abs(i - j) != 1] == 1.0).all()
    assert np.array_equal(X, X.T)
    X3 = R.oe(M, 2, E)                               # min_sep = 2 switches the first diagonal off as well
    assert (X3 == 1.0).all()


def test_the_two_sign_rules():
    v = np.array([0.1, -0.7, 0.7, 0.2])
    assert np.array_equal(R.sign_largest(v), -v)                  # the first of the two largest is negative
    assert np.array_equal(R.sign_largest(-v), -v)
    f = np.array([0.5, 0.5, -0.5, -0.5])
    V = np.array([[-0.5, -0.5, 0.5, 0.5]])
    assert np.array_equal(R.sign_against(V, f[None])[0], -V[0])   # made to point along IF's vector
    orth = np.array([[0.5, -0.5, 0.5, -0.5]])
    assert orth[0] @ f == 0.0
    assert np.array_equal(R.sign_against(-orth, f[None])[0], orth[0])      # an exact 0 falls back to the largest entry (index 0) positive


def test_a_dependent_start_is_refused():
    x, _ = R.planted_chain(17)
    M = R.distance_map(x)
    s = R.start(17, 2)
    s[0] = 0.0
    s[0, 3] = 0.25                                   # a power of two along one axis: its copy projects to exactly 0
    s[1] = 4.0 * s[0]
    with pytest.raises(R.Dependent):
        R.solve_map(M, 1, 2, 3, s)
    R.solve_map(M, 1, 2, 3, R.start(17, 2))


def test_the_start_vectors_are_exact_and_spread():
    s = R.start(455, 3)
    assert s.shape == (3, 455) and (np.abs(s) < 0.5).all()
    assert np.array_equal((s + 0.5) * 4294967296.0 - 0.5, np.floor((s + 0.5) * 4294967296.0))      # (h + 0.5) / 2^32 - 0.5 with h an integer
    assert len(np.unique(s)) == s.size
    assert np.linalg.matrix_rank(s) == 3
