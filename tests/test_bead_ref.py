"""tests/bead_ref.py, the numpy restatement that tests/test_gpu_bead.py holds the device to, held in turn to what needs no trust:
scipy.stats.spearmanr inside every row of the seven bundled models, and the reference's own assessment of its models
(tests/golden/front_half_golden.json: `satisfied`, `restraints`, `sum_dev` are count_satisfied_tbl_rows' and sum_noe_dev's output).
Every restrained pair has two ends, so each per-bead tally summed over the beads is twice the model's figure."""
import math
import os

import numpy as np
import pytest
from scipy.stats import spearmanr

from chromosome3d_amd.pipeline import SEPARATION
from oracle import oracle as O
from tests import bead_ref as Bd
from tests.util import GOLD, golden, load_if, load_pdb_xyz

CIDS = sorted(golden())


def _case(cid):
    g = golden()[cid]
    return load_if(cid), load_pdb_xyz(os.path.join(GOLD, "models", g["model"]))


@pytest.mark.parametrize("cid", CIDS)
def test_every_row_is_scipys_spearman(cid):
    IF, x = _case(cid)
    n = len(IF)
    got = Bd.bead_scores(IF, x, 3)
    worst = 0.0
    for i in range(n):
        js = Bd.partners(n, i, 3)
        assert len(js) == max(0, i - 2) + max(0, n - i - 3)
        want = spearmanr(IF[i, js], Bd.row_milli(x, i, js))[0]
        assert math.isnan(got["rho"][i]) == math.isnan(want), (cid, i)
        if not math.isnan(want):
            worst = max(worst, abs(got["rho"][i] - want))
    print(f"{cid}: n {n}, rho {np.nanmin(got['rho']):.3f} .. {np.nanmax(got['rho']):.3f}, NaN rows {int(np.isnan(got['rho']).sum())}, largest gap to scipy {worst:.2e}")
    assert worst <= 1e-12


def test_rows_of_one_and_of_no_partner_and_constant_rows():
    n = 5
    rng = np.random.default_rng(5)
    x, IF = rng.normal(size=(n, 3)) * 5.0, rng.lognormal(size=(n, n))
    got = Bd.bead_scores(IF, x, 4)                                               # N = 1, 0, 0, 0, 1
    assert (got["sums"] == 0).all() and np.isnan(got["rho"]).all()
    got = Bd.bead_scores(IF, x, 2)                                               # N = 3, 2, 2, 2, 3
    assert not np.isnan(got["rho"]).any() and set(np.abs(got["rho"][1:4])) == {1.0}
    IF[2] = 0.0
    IF[2, 4] = -0.0                                                             # an all-zero row, -0.0 in it: constant, NaN
    got = Bd.bead_scores(IF, x, 1)
    assert math.isnan(got["rho"][2]) and got["sums"][2, 1] == 0 and got["sums"][2, 2] > 0 and not np.isnan(got["rho"][[0, 1, 3, 4]]).any()
    assert np.array_equal(Bd.bead_scores(IF, x, 1, [1, 4])["sums"], got["sums"][[1, 4]])


@pytest.mark.parametrize("cid,sat,restraints,dev", [("chr21_1mb", 68, 528, "2955.67"), ("chr22_1mb", 67, 465, "2176.17")])
def test_the_tallies_add_up_to_twice_the_references_assessment(cid, sat, restraints, dev):
    g = golden()[cid]
    assert g["satisfied"] == f"{sat}/{restraints}" and g["restraints"] == restraints and "%.2f" % g["sum_dev"] == dev
    IF, x = _case(cid)
    got = Bd.bead_scores(None, x, 3, None, O.if_to_dist10(IF), SEPARATION)
    assert int(got["satisfied"].sum()) == 2 * sat and int(got["restrained"].sum()) == 2 * restraints
    total = sum(int(v) for v in got["dev_milli"])
    assert total % 2 == 0 and "%.2f" % (total / 2000) == dev


@pytest.mark.parametrize("cid", CIDS)
def test_the_tallies_of_every_bundled_model(cid):
    g = golden()[cid]
    IF, x = _case(cid)
    got = Bd.bead_scores(None, x, 3, None, O.if_to_dist10(IF), SEPARATION)
    assert f"{int(got['satisfied'].sum()) // 2}/{int(got['restrained'].sum()) // 2}" == g["satisfied"]
    assert "%.2f" % (sum(int(v) for v in got["dev_milli"]) / 2000) == "%.2f" % g["sum_dev"]


def test_targets_of_a_restraint_list():
    t = Bd.targets_of_restraints(4, [1, 2, 1], [3, 4, 3], [50, 0, 70])
    assert t[0, 2] == t[2, 0] == 70 and t.sum() == 140                           # the later row of a pair wins, a target of 0 is none
