"""The restatement tests/mapsim_ref.py of c3d_map_similarity's definitions, held to scipy and to hand-made cases on the CPU: the smoothing
(separable against the direct double loop bit for bit, against scipy.ndimage to rounding), rho_s against scipy.stats.pearsonr, w_s
against the variance of rank/N, the degenerate strata, the both-zero rule on a worked 6 x 6 example, and a planted case in which a
replicate must score above a map of another domain structure."""
import math

import numpy as np
import pytest
from scipy import ndimage
from scipy.stats import pearsonr, rankdata

from tests import mapsim_ref as R


def _sym(rng, n, integer=True):
    A = rng.poisson(3.0, (n, n)).astype(float) if integer else rng.gamma(2.0, 1.7, (n, n))
    A = np.triu(A) + np.triu(A, 1).T
    return A


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("n,h", [(3, 0), (3, 1), (9, 1), (9, 3), (9, 20), (13, 2), (13, 4)])
def test_separable_smoothing_is_the_direct_double_loop_bit_for_bit(n, h, integer):
    rng = np.random.default_rng(100 * n + h)
    M = _sym(rng, n, integer)
    if not integer:
        M *= rng.uniform(0.5, 2.0, (n, n))                                                  # (not symmetric any more: the order is what is tested)
    X = R.smooth_direct(M, h)
    band = R.smooth_band(M, h, 0, n - 1)
    for s in range(n):
        want = np.array([X[i, i + s] for i in range(n - s)])
        assert band[s, :n - s].tobytes() == want.tobytes(), (n, h, s)                       # corners included: s = 0 and s = n - 1
        assert (band[s, n - s:] == 0).all()
    assert R.smooth_full(M, h).tobytes() == X.tobytes()                                     # and the whole map at once, vectorised
    assert all(R.smooth_stratum(M, h, s).tobytes() == np.diagonal(X, s).tobytes() for s in range(n))
    if h == 0:
        assert X.tobytes() == M.tobytes()                                                   # h = 0 is the map itself
    if h >= n - 1:                                                                          # the window is the whole map, clipped on all sides
        assert np.allclose(X, M.sum() / (n * n), rtol=1e-13, atol=0)


def test_a_window_of_negative_zeros_keeps_its_sign():
    M = np.full((5, 5), -0.0)
    assert np.signbit(R.smooth_band(M, 1, 0, 4)[:, 0]).all() and np.signbit(R.smooth_direct(M, 1)).all()


@pytest.mark.parametrize("h", [1, 2, 5])
def test_smoothing_against_ndimage(h):
    rng = np.random.default_rng(h)
    n = 40
    M = _sym(rng, n, integer=False)
    k = np.ones((2 * h + 1, 2 * h + 1))
    want = ndimage.correlate(M, k, mode="constant", cval=0.0) / ndimage.correlate(np.ones((n, n)), k, mode="constant", cval=0.0)
    band = R.smooth_band(M, h, 0, n - 1)
    for s in range(n):
        assert np.allclose(band[s, :n - s], np.diagonal(want, s), rtol=1e-13, atol=0)


def test_rho_and_weight_against_scipy():
    rng = np.random.default_rng(5)
    for N in (3, 10, 77):
        x, y = rng.poisson(4.0, N).astype(float) + 1, rng.gamma(2.0, 1.0, N) + 0.1
        mo, co = R.stratum(x, y)
        rho, w = R.rho_w(mo, co)
        assert co[0] == N and abs(rho - pearsonr(x, y)[0]) < 1e-13
        direct = N * math.sqrt(np.var(rankdata(x) / N) * np.var(rankdata(y) / N))             # HiCRep's weight: N sqrt(var(rank_x / N) var(rank_y / N))
        assert abs(w / direct - 1) < 1e-12
        A = co[1]
        assert A == round(4 * N * N * np.var(rankdata(x)))                                    # A = 4 N^2 var(rank), an integer


def test_identical_maps_and_degenerate_strata():
    rng = np.random.default_rng(6)
    x = rng.gamma(2.0, 1.0, 50)
    rho, w = R.rho_w(*R.stratum(x, x))
    assert abs(rho - 1) < 1e-14 and w > 0
    mo, co = R.stratum(np.full(9, 2.5), x[:9])                                              # equal values: no variance, no rank variance
    assert co[1] == 0 and mo[1] == 0.0
    rho, w = R.rho_w(mo, co)
    assert math.isnan(rho) and w == 0.0
    rho, w = R.rho_w(*R.stratum(x[:2], x[2:4]))                                             # N < 3
    assert math.isnan(rho) and w == 0.0
    rho_all, w_all, scc = R.combine(np.array([mo, mo]), np.array([co, co], dtype=object))
    assert np.isnan(rho_all).all() and math.isnan(scc)                                      # no stratum counts


def test_both_zero_rule_on_a_worked_example():
    """Two 6 x 6 maps, h = 0, stratum 1 (pairs (i, i+1), i = 0..4):  x = 3 0 2 0 5,  y = 1 0 4 2 0.
    Pair 1 is 0 in both and is dropped: N = 4, x = 3 2 0 5, y = 1 4 2 0, mx = 2.5, my = 1.75,
      Cxy = (.5)(-.75) + (-.5)(2.25) + (-2.5)(.25) + (2.5)(-1.75) = -6.5,  Cxx = .25 + .25 + 6.25 + 6.25 = 13,  Cyy = 8.75;
      doubled ranks of x: 6 4 2 8, of y: 4 8 6 2, sum of squares 120 both: A = B = 4 * 120 - (4 * 5)^2 = 80.
    With the zeros kept: N = 5, the two zeros of x tie at rank 1.5: doubled ranks 8 3 6 3 10, squares 218, A = 5 * 218 - 30^2 = 190; y alike."""
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for i, (a, b) in enumerate(zip((3, 0, 2, 0, 5), (1, 0, 4, 2, 0))):
        A[i, i + 1] = A[i + 1, i] = a
        B[i, i + 1] = B[i + 1, i] = b
    out = R.map_similarity([A, B], h=(0,), min_sep=1, max_sep=1)
    assert tuple(out["moments"][0, 0, 0]) == (-6.5, 13.0, 8.75) and tuple(out["counts"][0, 0, 0]) == (4, 80, 80)
    assert out["rho"][0, 0, 0] == -6.5 / math.sqrt(13.0 * 8.75) and out["scc"][0, 0, 1] == out["rho"][0, 0, 0] == out["scc"][0, 1, 0]
    assert out["w"][0, 0, 0] == math.sqrt(80.0 * 80.0) / 256.0
    kept = R.map_similarity([A, B], h=(0,), min_sep=1, max_sep=1, keep_zeros=True)
    assert tuple(kept["counts"][0, 0, 0]) == (5, 190, 190) and kept["moments"][0, 0, 0, 1] == 18.0       # x: mean 2, squares 1 4 0 4 9


def planted_maps():
    """n = 193: Poisson counts of 200 / (1 + s) x (1 + 1.5 [same block of 17 bins]), a replicate at 0.6 of the depth, a third map with
    blocks of 29"""
    rng = np.random.default_rng(2024)
    n = 193
    i = np.arange(n)
    sep = np.abs(i[:, None] - i[None, :])

    def draw(block, depth):
        lam = depth * 200.0 / (1.0 + sep) * (1.0 + 1.5 * (i[:, None] // block == i[None, :] // block))
        M = np.triu(rng.poisson(lam).astype(float))
        return M + np.triu(M, 1).T
    return np.stack([draw(17, 1.0), draw(17, 0.6), draw(29, 1.0)])


def test_a_planted_replicate_scores_above_another_domain_structure():
    maps = planted_maps()
    hs = (0, 1, 2, 4)
    out = R.map_similarity(maps, h=hs, min_sep=1, max_sep=48)
    for k, h in enumerate(hs):
        scc = out["scc"][k]
        print("h = %d: replicate %.3f, others %.3f %.3f" % (h, scc[0, 1], scc[0, 2], scc[1, 2]))
        assert scc[0, 1] > scc[0, 2] and scc[0, 1] > scc[1, 2], h
        assert (np.isfinite(out["rho"][k]).sum(axis=1) == 48).all()                         # all 48 strata count, in every pair
