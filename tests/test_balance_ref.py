"""The restatement tests/balance_ref.py held to things it does not compute itself, on the CPU: planted biases on matrices whose balanced
form is known, VC as one round of ICE, the closure on hand-made chains, the codes, the refusals, and a worked example on chr1_500kb.
tests/test_gpu_balance.py holds the device to the restatement."""
import os

import numpy as np
import pytest

from tests import balance_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _circulant(n, rng):
    """symmetric, non-negative, every row sum the same: S(i, j) = c[(i - j) mod n] with c[k] = c[n - k]"""
    c = rng.uniform(0.5, 2.0, n)
    c = c + np.roll(c[::-1], 1)
    i = np.arange(n)
    return c[(i[:, None] - i[None, :]) % n]


@pytest.mark.parametrize("n, masked_bins", [(12, ()), (57, (5,)), (200, (0, 77, 199))])
def test_planted_biases_are_recovered(n, masked_bins):
    rng = np.random.default_rng(n)
    S = _circulant(n, rng)
    b = np.exp(rng.normal(0.0, 0.5, n))
    A = (b[:, None] * b[None, :]) * S
    mask = np.zeros(n, dtype=np.int32)
    mask[list(masked_bins)] = 1
    # (with bins masked the kept block of a circulant has no equal row sums any more: the planted biases are then exact only without a mask)
    for target in (1.0, 3.5):
        out = R.balance(A, "ice", ignore_diags=0, min_nnz=1, mask=mask if masked_bins else None, tol=1e-12, max_iters=500, target=target)
        U = out["masked"] == 0
        assert out["converged"] and out["kept"] == n - len(masked_bins) and (out["weights"][~U] == 0).all()
        bound = np.sqrt(out["kept"] * float(out["var"]))                       # var_T = mean (r - 1)^2, so |r_i - 1| <= sqrt(|U| var_T)
        rows = out["balanced"][U][:, U].sum(axis=1)
        print("row sums: largest fraction of the bound %.3g" % (np.abs(rows / target - 1).max() / max(bound, 1e-300)))
        assert np.abs(rows / target - 1).max() <= bound + 8 * n * 2.0 ** -53
        if not masked_bins:
            wb = out["weights"] * b
            print("w b: largest fraction of the bound %.3g" % (np.abs(wb / wb.mean() - 1).max() / max(bound, 1e-300)))
            assert np.abs(wb / wb.mean() - 1).max() <= bound + 8 * n * 2.0 ** -53


def test_vc_is_ice_with_one_round_and_no_tolerance():
    rng = np.random.default_rng(3)
    A = rng.poisson(3.0, (40, 40)).astype(float)
    A = A + A.T
    vc = R.balance(A, "vc", ignore_diags=1, min_nnz=1, tol=0.5, max_iters=77)       # (tol and max_iters are forced)
    ice = R.balance(A, "ice", ignore_diags=1, min_nnz=1, tol=0.0, max_iters=1)
    for key in ("weights", "balanced", "history", "masked"):
        assert np.array_equal(vc[key], ice[key]), key
    assert vc["rounds"] == ice["rounds"] == 1 and not vc["converged"] and len(vc["history"]) == 2
    with pytest.raises(R.Refused):
        R.balance(A, "vc", w0=np.ones(40))
    with pytest.raises(R.Refused):
        R.balance(A, "sqrt-vc", w0=np.ones(40))


def test_vc_recovers_a_rank_one_bias_in_one_round_and_sqrt_vc_its_square_root():
    """On a constant matrix scaled by b b^T the row sums are b_i sum(b): one round of VC (p = 1) divides by them and recovers b exactly, so
    the second pass finds the matrix balanced.  sqrt-VC (p = 1/2) divides by their square roots: its weights are the square roots of
    VC's up to the scale, w_i^2 b_i is constant, and the matrix it leaves has row sums proportional to sqrt(b_i) sum(sqrt(b)) — it does
    not recover b itself on such a matrix, whatever the scale; that it is one update with the exponent 1/2 is what is checked."""
    rng = np.random.default_rng(4)
    n = 30
    u = 2.0 ** -53
    b = np.exp(rng.normal(0.0, 0.7, n))
    A = 5.0 * (b[:, None] * b[None, :])
    vc = R.balance(A, "vc", ignore_diags=0, min_nnz=1)
    wb = vc["weights"] * b
    assert vc["rounds"] == 1 and np.abs(wb / wb.mean() - 1).max() < 16 * u
    assert float(vc["history"][1]) < (16 * n * u) ** 2                               # balanced after the one update
    assert np.abs(vc["balanced"].sum(axis=1) - 1.0).max() < 8 * n * u
    sq = R.balance(A, "sqrt-vc", ignore_diags=0, min_nnz=1)
    w2b = sq["weights"] ** 2 * b
    assert sq["rounds"] == 1 and len(sq["history"]) == 2 and np.abs(w2b / w2b.mean() - 1).max() < 16 * u
    rows = sq["balanced"].sum(axis=1)
    assert abs(rows.mean() - 1.0) < 8 * n * u                                        # the scale: the mean row sum is the target
    want = np.sqrt(b) / np.sqrt(b).mean()
    assert np.abs(rows / want - 1).max() < 16 * n * u


def test_the_closure_on_chains():
    # a chain 0-1-2 with bin 2 listed: 0 and 1 stay
    A = np.zeros((3, 3))
    A[0, 1] = A[1, 0] = 4.0
    A[1, 2] = A[2, 1] = 2.0
    out = R.balance(A, "ice", ignore_diags=0, min_nnz=1, mask=[0, 0, 1], max_iters=5)
    assert out["masked"].tolist() == [0, 0, 1] and out["kept"] == 2 and out["masked_counts"] == [1, 0, 0]
    # 0-1, 1-2, 2-3 plus the pair 4-5: bin 3's only partner 2 is listed -> 3 gets code 3; nobody else loses a partner
    A = np.zeros((6, 6))
    for i, j in ((0, 1), (1, 2), (2, 3), (4, 5)):
        A[i, j] = A[j, i] = 1.0 + i
    out = R.balance(A, "ice", ignore_diags=0, min_nnz=1, mask=[0, 0, 1, 0, 0, 0], max_iters=5)
    assert out["masked"].tolist() == [0, 0, 1, 3, 0, 0] and out["masked_counts"] == [1, 0, 1]
    # the band takes partners away for the marginals only: 1-2 lies inside ignore_diags = 2, so both have no non-zero at all (code 2)
    A = np.zeros((7, 7))
    for i, j in ((0, 3), (3, 6), (0, 6), (1, 2)):
        A[i, j] = A[j, i] = 1.0
    out = R.balance(A, "ice", ignore_diags=2, min_nnz=0, max_iters=3)
    assert out["masked"].tolist() == [0, 2, 2, 0, 2, 2, 0] and out["kept"] == 3
    # two listed bins, each the only partner of another bin (4 of 5, 6 of 7): both fall to the closure, bin 3 has no non-zero (code 2).
    # A bin removed by the closure had no kept partner, so by symmetry no kept bin had it for a partner: nobody can lose a partner to
    # the closure itself, and the pass after the first removes nothing
    A = np.zeros((8, 8))
    for i, j in ((0, 1), (1, 2), (0, 2), (4, 5), (6, 7), (5, 7)):
        A[i, j] = A[j, i] = 2.0
    out = R.balance(A, "ice", ignore_diags=0, min_nnz=1, mask=[0, 0, 0, 0, 0, 1, 0, 1], max_iters=3)
    assert out["masked"].tolist() == [0, 0, 0, 2, 3, 1, 3, 1] and out["masked_counts"] == [2, 1, 2]
    codes = R.mask_codes(A, 1, [0, 0, 0, 0, 0, 1, 0, 1])
    kept = codes == 0
    assert ((A[kept][:, kept] > 0).sum(axis=1) > 0).all()                          # closed: every kept bin has a kept partner


def test_codes_and_too_few_bins():
    rng = np.random.default_rng(5)
    n = 20
    A = rng.poisson(2.0, (n, n)).astype(float)
    A = A + A.T
    A[7, :] = 0.0
    A[:, 7] = 0.0                                                                    # an all-zero row: code 2 whatever min_nnz is
    nnz = (R.seen_by_marginals(A, 2) > 0).sum(axis=1)
    need = int(np.sort(nnz)[n // 2])
    out = R.balance(A, "ice", ignore_diags=2, min_nnz=need, mask=(np.arange(n) == 3).astype(int), max_iters=2)
    want = np.where(np.arange(n) == 3, 1, np.where(nnz < need, 2, 0))
    assert out["masked"][7] == 2 and np.array_equal(out["masked"] != 0, want != 0) and np.array_equal(out["masked"][want != 0], want[want != 0])
    assert out["kept"] + sum(out["masked_counts"]) == n and (out["balanced"][out["masked"] != 0] == 0).all()
    with pytest.raises(R.Refused):
        R.balance(A, "ice", ignore_diags=2, min_nnz=n + 1)                           # every bin masked
    with pytest.raises(R.Refused):
        R.balance(A, "ice", ignore_diags=n)                                          # nothing left for the marginals: |U| < 2
    one_pair = R.balance(A, "ice", ignore_diags=n - 1, min_nnz=1) if A[0, n - 1] > 0 else None
    assert one_pair is None or (one_pair["kept"] == 2 and one_pair["masked"][0] == 0 and one_pair["masked"][n - 1] == 0)
    for bad in (dict(tol=-1.0), dict(max_iters=-1), dict(max_iters=R.MAX_ITERS + 1), dict(target=0.0), dict(target=np.inf), dict(method=7),
                dict(ignore_diags=-1), dict(w0=np.zeros(n)), dict(w0=np.full(n, np.nan))):
        with pytest.raises(R.Refused):
            R.balance(A, **{"method": "ice", **bad})
    for spoil in (np.nan, -1.0):
        B = A.copy()
        B[2, 5] = B[5, 2] = spoil
        with pytest.raises(R.Refused):
            R.balance(B)
    B = A.copy()
    B[2, 5] += 1.0
    with pytest.raises(R.Refused):
        R.balance(B)


def test_zero_iterations_only_evaluate_the_start_and_history_ends_at_T():
    rng = np.random.default_rng(6)
    n = 25
    A = rng.poisson(4.0, (n, n)).astype(float)
    A = A + A.T
    w0 = rng.uniform(0.5, 2.0, n)
    out = R.balance(A, "ice", ignore_diags=1, min_nnz=1, w0=w0, max_iters=0, target=2.0)
    s = w0 * (R.seen_by_marginals(A, 1) @ w0)
    assert out["rounds"] == 0 and len(out["history"]) == 1 and not out["converged"]
    assert np.allclose(out["weights"], w0 * np.sqrt(2.0 / s.mean()), rtol=1e-14, atol=0)
    assert abs(float(out["mean_marginal"]) - s.mean()) <= 1e-14 * s.mean()
    for tol in (1e-3, 1e-6):
        run = R.balance(A, "ice", ignore_diags=1, min_nnz=1, tol=tol, max_iters=300)
        T = run["rounds"]
        assert run["converged"] and len(run["history"]) == T + 1 and run["history"][T] < tol and (run["history"][:T] >= tol).all()
    capped = R.balance(A, "ice", ignore_diags=1, min_nnz=1, tol=1e-12, max_iters=2)
    assert capped["rounds"] == 2 and not capped["converged"] and len(capped["history"]) == 3
    fixed = R.balance(A, "ice", ignore_diags=1, min_nnz=1, tol=1e-6, rounds=4)
    assert fixed["rounds"] == 4 and len(fixed["history"]) == 5


def test_the_worked_example_on_chr1_500kb():
    S = np.loadtxt(os.path.join(GOLD, "all45", "txt", "chr1_500kb_matrix.txt"))
    n = S.shape[0]
    assert n == 455
    M, _ = R.worked_example(S, seed=1)
    assert (M == M.T).all() and (M == np.rint(M)).all()
    stops = {}
    for tol in (1e-5, 1e-8, 1e-10):
        out = R.balance(M, "ice", ignore_diags=2, min_nnz=1, tol=tol, max_iters=200)
        assert out["converged"] and out["kept"] == n - 1 and out["masked_counts"] == [0, 1, 0] and out["masked"][n // 3] == 2
        stops[tol] = out["rounds"]
    assert stops == {1e-5: 11, 1e-8: 22, 1e-10: 30}
    h = np.asarray(out["history"], dtype=float)
    ratio = h[1:] / h[:-1]
    print("var ratio a round, rounds 5..30: %.3f .. %.3f" % (ratio[5:].min(), ratio[5:].max()))
    assert (ratio[5:] > 0.5).all() and (ratio[5:] < 0.6).all() and h[10] / h[11] >= 1.2           # about 0.55 a round: 1.8 between stops
    # float64 against longdouble over the same T rounds
    a = R.balance(M, "ice", ignore_diags=2, min_nnz=1, rounds=11)
    b = R.balance(M, "ice", ignore_diags=2, min_nnz=1, rounds=11, dtype=np.longdouble)
    U = a["masked"] == 0
    gap = float(np.abs(a["weights"][U] / b["weights"][U] - 1).max())
    print("float64 against longdouble after 11 rounds: %.3g relative" % gap)
    assert gap < 32 * 2.0 ** -53
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        assert gap > 0                                                                             # (the two really are different arithmetic)
