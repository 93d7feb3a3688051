"""tests/stratified_ref.py, the numpy restatement that tests/test_gpu_stratified.py holds the device to, held in turn to what needs no
trust: scipy.stats.spearmanr inside every stratum of the seven bundled models, Python's own "%.3f", and HiCRep's weights written out
from their definition."""
import math
import os

import numpy as np
import pytest
from scipy.stats import rankdata, spearmanr

from tests import stratified_ref as S
from tests.util import GOLD, golden, load_if, load_pdb_xyz

CIDS = sorted(golden())


def _case(cid):
    g = golden()[cid]
    return load_if(cid), load_pdb_xyz(os.path.join(GOLD, "models", g["model"]))


_DONE = {}


def _result(cid):
    if cid not in _DONE:
        IF, x = _case(cid)
        _DONE[cid] = (IF, x, S.stratified(IF, x, 3))
    return _DONE[cid]


def test_there_are_seven_bundled_models():
    assert len(CIDS) == 7


@pytest.mark.parametrize("cid", CIDS)
def test_every_stratum_is_scipys_spearman_and_only_the_last_is_nan(cid):
    IF, x, got = _result(cid)
    n = len(IF)
    assert np.isnan(got["rho"][:3]).all() and (got["sums"][:3] == 0).all()
    worst = 0.0
    for s in range(3, n - 1):
        d = S.round_milli(S.diagonal_distances(x, s))
        want = spearmanr(np.diagonal(IF, s), d)[0]
        assert not math.isnan(got["rho"][s]), (cid, s)
        worst = max(worst, abs(got["rho"][s] - want))
    print(f"{cid}: n {n}, scc {got['scc']:.4f}, rho {np.nanmin(got['rho']):.3f} .. {np.nanmax(got['rho']):.3f}, largest gap to scipy {worst:.2e}")
    assert worst <= 1e-12
    assert math.isnan(got["rho"][n - 1]) and -1.0 < got["scc"] < 0.0             # N = 1; a good model is negative


@pytest.mark.parametrize("cid", CIDS)
def test_the_rounding_is_pythons_percent_3f(cid):
    x = _case(cid)[1]
    n = len(x)
    for s in range(1, n):
        d = S.diagonal_distances(x, s)
        assert [int(v) for v in S.round_milli(d)] == [int(("%.3f" % v).replace(".", "")) for v in d], (cid, s)


def test_the_rounding_at_ties():
    # 0.0005 is below the decimal tie (its double is 0.000500000000000000010...: "%.3f" gives 0.001), 0.0015 is below it, 2.5e-3 above
    d = np.array([0.0005, 0.0015, 0.0025, 1.0005, 4.3875, 0.5, 0.0])
    assert [int(v) for v in S.round_milli(d)] == [int(("%.3f" % v).replace(".", "")) for v in d]


def test_both_triangles_count_every_observation_twice_and_change_nothing():
    IF, x, got = _result("chr21_1mb")
    n = len(IF)
    for s in (3, 10, n - 2):
        f, d = np.diagonal(IF, s), S.round_milli(S.diagonal_distances(x, s))
        twice = S.rho_of(*S.stratum_sums(np.concatenate([f, f]), np.concatenate([d, d])))
        assert abs(twice - got["rho"][s]) <= 1e-12


def test_a_straight_chain_has_no_coefficient():
    n = 40
    x = np.zeros((n, 3))
    x[:, 0] = 1.5 * np.arange(n)
    IF = 1.0 / (1.0 + np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]))
    got = S.stratified(IF, x, 1)
    assert np.isnan(got["rho"]).all() and math.isnan(got["scc"])
    assert (got["sums"][1:, 1:] == 0).all() and (got["sums"][:, 0] == 0).all()   # A = B = 0: both sides constant in every stratum


@pytest.mark.parametrize("cid", ["chr21_1mb", "chr22_1mb"])
def test_scc_is_hicreps_weighted_mean(cid):
    """w_s = N_s sqrt(var(a / 2N) var(b / 2N)), the variances those of the normalised ranks: scc = sum w rho / sum w."""
    IF, x, got = _result(cid)
    n = len(IF)
    num = den = 0.0
    for s in range(3, n - 1):
        N = n - s
        ra = rankdata(np.diagonal(IF, s)) / N
        rb = rankdata(S.round_milli(S.diagonal_distances(x, s))) / N
        w = N * math.sqrt(ra.var() * rb.var())
        num += w * spearmanr(ra, rb)[0]
        den += w
    assert abs(got["scc"] - num / den) <= 1e-12
