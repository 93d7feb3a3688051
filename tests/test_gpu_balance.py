"""Balancing a raw contact matrix on the device (c3d_balance_matrix; csrc/c3d_score_balance.inc k_bal_*) against the numpy restatement
tests/balance_ref.py, which tests/test_balance_ref.py holds to planted biases, hand-made chains and a worked example.

The kernels' constants: the call's copy of the matrix has pitch np = n rounded up to even (an odd n takes the padded upload and the padded
read-back); a workgroup of k_bal_marginals owns 4 consecutive rows and a thread the column pairs 2t + 512k; k_bal_update and k_bal_count
walk in steps of 256; the host enqueues 16 rounds between two looks at the round record.
  sizes     n = 2, 3; 255, 256, 257; 511, 512, 513 (the column step); 1023, 1025; 455 (the worked example); n = 1, 2, 3 mod 4 among them
  bands     ignore_diags 0, 1, 2 and n - 1 (one pair left); >= n is refused through |U| < 2
  stops     T = 11 (the worked example), and 15, 16, 17: the last round of a batch, the first of the next and the one after

Bounds, u = 2^-53.  Every term of every sum is non-negative, so nothing cancels.  One round from a given w0 against the restatement's
round from the same w0: weights, relative, (4n + 12) u; history[0] and history[1], absolute, 2 e sqrt(var) + e^2 + (|U| + 2) u var with
e = (4n + 12) u max r_i.  A run is stepped through that way, the device's own weights fed back as w0, so no error hides in accumulation.
A whole run against single rounds of the device itself, the stopping round under both ways of looking, `balanced` against numpy from the
device's own weights, two calls, and calls that leave outputs out: bit for bit.  Every numeric check prints the largest observed fraction
of its bound.

The chained single rounds rescale between rounds; the comparison is made before the scale by the second of the two ways the issue
names: every call is made twice, the second time with `target` set to the mbar the first reported (report[7]), so that target / mbar is
exactly 1, its square root exactly 1 and the weights come back unscaled — the w_t of the definition.

The entry keeps no stat key (the stat table's keys are held fixed by tests/test_config_transcript.py), so no call count is asserted."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import balance_ref as R
from tests.util import GOLD, SHORT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SENT = -7.0                                                                     # no output is ever negative
C3D_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _counts(n, seed=0):
    """raw counts: a decay with the separation times b b^T, rounded to integers; symmetric bit for bit (b_i b_j is one product)"""
    rng = np.random.default_rng(1000 * seed + n)
    b = np.exp(rng.normal(0.0, 0.4, n))
    i = np.arange(n)
    S = 300.0 / (1.0 + np.abs(i[:, None] - i[None, :])) ** 0.8 + 2.0
    M = np.rint(S * (b[:, None] * b[None, :]))
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _example():
    """the worked example of tests/test_balance_ref.py and the restatement's run of it to 1e-10 (30 rounds), computed once"""
    S = np.loadtxt(os.path.join(GOLD, "all45", "txt", "chr1_500kb_matrix.txt"))
    M, _ = R.worked_example(S, seed=1)
    M.setflags(write=False)
    return M, R.balance(M, "ice", ignore_diags=2, min_nnz=1, tol=1e-10, max_iters=200)


def _call(s, M, method=0, flags=0, ignore_diags=2, min_nnz=1, mask=None, w0=None, tol=0.0, max_iters=1, target=1.0, outs="wmbhrd", n=None):
    """The entry through ctypes with every output buffer filled with a sentinel.  Returns (rc, dict): the outputs asked for by `outs`
    (w weights, m masked, b balanced, h history, r report, d device_ms), history whole (sentinels beyond T)."""
    from chromosome3d_amd import lib
    L = lib.load()
    M = np.ascontiguousarray(M, dtype=np.float64)
    n = M.shape[0] if n is None else n
    rows = M.shape[0]
    slots = max_iters + 1 if method == 0 and 0 <= max_iters <= 10000 else 2
    buf = {"w": np.full(rows, SENT), "m": np.full(rows, 77, np.int32), "b": np.full((rows, rows), SENT) if "b" in outs else None, "h": np.full(slots, SENT),
           "r": np.full(8, SENT), "d": C.c_double(SENT)}
    mk = np.ascontiguousarray(mask, dtype=np.int32) if mask is not None else None
    st = np.ascontiguousarray(w0, dtype=np.float64) if w0 is not None else None
    rc = L.c3d_balance_matrix(s._h, lib.dptr(M), n, method, flags, ignore_diags, min_nnz, lib.i32ptr(mk) if mk is not None else None,
                              lib.dptr(st) if st is not None else None, tol, max_iters, target, lib.dptr(buf["w"]) if "w" in outs else None,
                              lib.i32ptr(buf["m"]) if "m" in outs else None, lib.dptr(buf["b"]) if "b" in outs else None,
                              lib.dptr(buf["h"]) if "h" in outs else None, lib.dptr(buf["r"]) if "r" in outs else None, C.byref(buf["d"]) if "d" in outs else None)
    for k in "wmbhr":                                                           # an output that was not asked for, or a refused call: untouched
        if buf[k] is not None and (k not in outs or rc != 0):
            assert (buf[k] == (77 if k == "m" else SENT)).all(), k
    if rc != 0 or "d" not in outs:
        assert buf["d"].value == SENT
    return rc, {k: (buf[k].value if k == "d" else buf[k]) for k in outs}


def _refused(s, word, *a, **kw):
    from chromosome3d_amd import lib
    rc, _ = _call(s, *a, **kw)
    err = lib.load().c3d_last_error().decode()
    assert rc == C3D_ERR_INVALID and "c3d_balance_matrix" in err and word in err, (rc, err)


def _one_round(s, M, w0, what, worst, **kw):
    """one round from w0 on the device against the restatement's round from the same w0; returns the device's weights"""
    n = M.shape[0]
    rc, got = _call(s, M, w0=w0, tol=0.0, max_iters=1, outs="wmhr", **kw)
    assert rc == 0, what
    want = R.balance(M, "ice", w0=w0, tol=0.0, max_iters=1, want_matrix=False, **kw)
    kept = want["masked"] == 0
    assert np.array_equal(got["m"], want["masked"]) and got["r"][0] == 1.0 and got["r"][1] == 0.0 and int(got["r"][3]) == want["kept"], what
    assert (got["w"][~kept] == 0).all() and (got["w"][kept] > 0).all(), what
    gap = np.abs(got["w"][kept] / want["weights"][kept] - 1).max() / ((4 * n + 12) * U)
    worst["weights"] = max(worst["weights"], gap)
    assert gap <= 1.0, f"{what}: weights at {gap:.3g} of the bound"
    for t in (0, 1):
        var = float(want["history"][t])
        e = (4 * n + 12) * U * float(want["r_max"][t])
        bound = 2 * e * np.sqrt(var) + e * e + (want["kept"] + 2) * U * var
        frac = abs(got["h"][t] - var) / bound
        worst["history"] = max(worst["history"], frac)
        assert frac <= 1.0, f"{what}: history[{t}] at {frac:.3g} of the bound"
    assert got["r"][2] == got["h"][1]
    return got["w"]


@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 511, 512, 513, 1023, 1025])
def test_one_round_at_the_kernels_borders(ctx, n):
    M = _counts(n)
    rng = np.random.default_rng(n)
    worst = {"weights": 0.0, "history": 0.0}
    for ig in (0, 1, 2, n - 1):
        if ig >= n:
            continue
        w0 = rng.uniform(0.5, 2.0, n)
        _one_round(ctx, M, w0, f"n = {n} ignore_diags {ig}", worst, ignore_diags=ig, min_nnz=1)
        _one_round(ctx, M, None, f"n = {n} ignore_diags {ig}, no w0", worst, ignore_diags=ig, min_nnz=1)
    rc, got = _call(ctx, M, ignore_diags=n - 1, min_nnz=1, outs="mr")                 # one pair left: the two ends
    assert rc == 0 and int(got["r"][3]) == 2 and got["m"][0] == 0 and got["m"][n - 1] == 0 and (got["m"][1:n - 1] == 2).all()
    for ig in (n, n + 5):
        _refused(ctx, "|U| < 2", M, ignore_diags=ig)
    print(f"n = {n}: weights at {worst['weights']:.3g}, history at {worst['history']:.3g} of their bounds")


def test_a_run_stepped_through_round_by_round(ctx):
    """the worked example (n = 455, one unmappable bin), 8 rounds, and an odd size with a listed bin: the device's w_t fed back as w0"""
    worst = {"weights": 0.0, "history": 0.0}
    M, _ = _example()
    w = None
    for t in range(8):
        w = _one_round(ctx, M, w, f"example, round {t}", worst, ignore_diags=2, min_nnz=1)
    M = _counts(257)
    mask = (np.arange(257) % 50 == 7).astype(np.int32)
    w = None
    for t in range(6):
        w = _one_round(ctx, M, w, f"n = 257, round {t}", worst, ignore_diags=1, min_nnz=1, mask=mask)
    print(f"stepped runs: weights at {worst['weights']:.3g}, history at {worst['history']:.3g} of their bounds")


def _unscaled(s, M, **kw):
    """the call made twice, the second time with target = the mbar the first reported: the scale is then exactly 1"""
    rc, first = _call(s, M, outs="r", **kw)
    assert rc == 0
    rc, got = _call(s, M, target=float(first["r"][7]), outs="wmhr", **kw)
    assert rc == 0 and got["r"][7] == first["r"][7] and got["r"][0] == first["r"][0]
    return got


@pytest.mark.parametrize("which", ["example", "odd"])
def test_a_whole_run_is_its_single_rounds(ctx, which):
    T = 8
    M = _example()[0] if which == "example" else _counts(257)
    kw = dict(ignore_diags=2, min_nnz=1, mask=None if which == "example" else (np.arange(257) % 50 == 7).astype(np.int32))
    whole = _unscaled(ctx, M, tol=0.0, max_iters=T, **kw)
    assert int(whole["r"][0]) == T and whole["r"][1] == 0.0
    w, hist = None, []
    for t in range(T):
        one = _unscaled(ctx, M, w0=w, tol=0.0, max_iters=1, **kw)
        assert one["h"][0].tobytes() == whole["h"][t].tobytes() and one["h"][1].tobytes() == whole["h"][t + 1].tobytes(), t
        w = one["w"]
    assert w.tobytes() == whole["w"].tobytes() and np.array_equal(one["m"], whole["m"])
    # and the scaled weights of a whole run are those weights times sqrt(target / mbar), one multiplication
    rc, scaled = _call(ctx, M, tol=0.0, max_iters=T, target=2.5, outs="wr", **kw)
    assert rc == 0 and np.array_equal(scaled["w"], whole["w"] * np.sqrt(2.5 / whole["r"][7]))


@pytest.mark.parametrize("T", [11, 15, 16, 17])
def test_the_stopping_round(ctx, T):
    M, ref = _example()
    h = np.asarray(ref["history"], dtype=float)
    assert h[T - 1] / h[T] >= 1.2                                                # a condition on the input: the tolerance sits well between two rounds
    tol = float(np.sqrt(h[T - 1] * h[T]))
    kw = dict(ignore_diags=2, min_nnz=1, tol=tol)
    rc, got = _call(ctx, M, max_iters=200, **kw)
    assert rc == 0 and int(got["r"][0]) == T and got["r"][1] == 1.0 and got["r"][2] == got["h"][T] and got["h"][T] < tol <= got["h"][T - 1]
    assert (got["h"][:T + 1] > 0).all() and (got["h"][T + 1:] == SENT).all()         # nothing written beyond T
    assert np.abs(got["h"][:T + 1] / h[:T + 1] - 1).max() < 1e-6
    rc, every = _call(ctx, M, max_iters=200, flags=1, **kw)
    assert rc == 0 and all(np.asarray(got[k]).tobytes() == np.asarray(every[k]).tobytes() for k in "wmbhr")
    rc, exact = _call(ctx, M, max_iters=T, **kw)                                  # var_T < tol is asked before t == max_iters
    assert rc == 0 and int(exact["r"][0]) == T and exact["r"][1] == 1.0 and exact["w"].tobytes() == got["w"].tobytes()
    for flags in (0, 1):
        rc, short = _call(ctx, M, max_iters=T - 1, flags=flags, **kw)
        assert rc == 0 and int(short["r"][0]) == T - 1 and short["r"][1] == 0.0 and short["h"][:T].tobytes() == got["h"][:T].tobytes()
    rc, none = _call(ctx, M, max_iters=0, ignore_diags=2, min_nnz=1, tol=0.0)
    assert rc == 0 and int(none["r"][0]) == 0 and none["h"][0] == got["h"][0]        # max_iters = 0 only evaluates the start


def test_exact_outputs(ctx):
    M, ref = _example()
    n = M.shape[0]
    kw = dict(ignore_diags=2, min_nnz=1, tol=1e-5, max_iters=200)
    rc, got = _call(ctx, M, **kw)
    assert rc == 0 and got["d"] > 0
    assert np.array_equal(got["m"], ref["masked"]) and got["m"][n // 3] == 2
    assert [int(v) for v in got["r"][3:7]] == [n - 1, 0, 1, 0] and int(got["r"][0]) == 11
    w = got["w"]
    assert got["b"].tobytes() == ((w[:, None] * w[None, :]) * M).tobytes()       # numpy's two multiplications, from the device's own weights
    assert np.array_equal(got["b"], got["b"].T) and (got["b"][n // 3] == 0).all() and (got["b"][:, n // 3] == 0).all()
    rows = R.seen_by_marginals(got["b"], 2).sum(axis=1)                          # the balanced A': mean row sum = target, every row within sqrt(|U| var_T)
    kept = got["m"] == 0
    assert abs(rows[kept].mean() - 1.0) < 1e-12 and np.abs(rows[kept] - 1).max() <= np.sqrt(n * got["r"][2]) + 1e-12
    rc, again = _call(ctx, M, **kw)
    assert rc == 0 and all(np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes() for k in "wmbhr")
    for leave in "wmbhrd":                                                      # leaving out any output changes no other output
        outs = "wmbhrd".replace(leave, "")
        rc, part = _call(ctx, M, outs=outs, **kw)
        assert rc == 0 and all(np.asarray(got[k]).tobytes() == np.asarray(part[k]).tobytes() for k in outs if k != "d"), leave
    rc, nothing = _call(ctx, M, outs="", **kw)
    assert rc == 0
    # an odd n: the padded copy, read back without its pad column
    M = _counts(513)
    rc, odd = _call(ctx, M, ignore_diags=2, min_nnz=1, tol=1e-6, max_iters=100)
    assert rc == 0 and odd["r"][1] == 1.0 and odd["b"].tobytes() == ((odd["w"][:, None] * odd["w"][None, :]) * M).tobytes() and np.array_equal(odd["b"], odd["b"].T)


def test_masks(ctx):
    n = 257
    M = _counts(n).copy()
    M[40, :] = M[:, 40] = 0.0                                                   # an all-zero row
    M[90, :] = M[:, 90] = 0.0
    M[90, 91] = M[91, 90] = 5.0                                                 # bin 90 sees only bin 91, inside the band of ignore_diags 2: no non-zero left
    M[120, :] = M[:, 120] = 0.0
    M[120, 200] = M[200, 120] = 9.0                                             # bin 120's only partner is 200, which is listed: the closure takes 120
    mask = np.zeros(n, np.int32)
    mask[[7, 200]] = 1
    A = R.seen_by_marginals(M, 2)
    nnz = (A > 0).sum(axis=1)
    for min_nnz in (0, 1, int(np.sort(nnz)[n // 3]) + 1):
        rc, got = _call(ctx, M, ignore_diags=2, min_nnz=min_nnz, mask=mask, tol=1e-6, max_iters=50)
        want = R.balance(M, "ice", ignore_diags=2, min_nnz=min_nnz, mask=mask, tol=1e-6, max_iters=50)
        assert rc == 0 and np.array_equal(got["m"], want["masked"]) and [int(v) for v in got["r"][3:7]] == [want["kept"]] + want["masked_counts"]
        assert got["m"][40] == 2 and got["m"][90] == 2 and got["m"][120] == (3 if min_nnz <= 1 else 2) and got["m"][7] == 1 and got["m"][200] == 1
        assert int(got["r"][0]) == want["rounds"] and (got["w"][got["m"] != 0] == 0).all() and (got["b"][got["m"] != 0] == 0).all()
        assert np.abs(got["w"][got["m"] == 0] / want["weights"][want["masked"] == 0] - 1).max() < 1e-9
    _refused(ctx, "|U| < 2", M, ignore_diags=2, min_nnz=n + 1)                        # every bin masked
    _refused(ctx, "|U| < 2", M, ignore_diags=2, min_nnz=1, mask=np.r_[np.zeros(1, np.int32), np.ones(n - 1, np.int32)])
    # values of w0 at masked bins are not read
    w0 = np.random.default_rng(2).uniform(0.5, 2.0, n)
    rc, a = _call(ctx, M, ignore_diags=2, min_nnz=1, mask=mask, w0=w0, max_iters=3)
    w0[[7, 40, 90, 120, 200]] = (np.nan, 0.0, -1.0, np.inf, np.nan)
    rc2, b = _call(ctx, M, ignore_diags=2, min_nnz=1, mask=mask, w0=w0, max_iters=3)
    assert rc == 0 and rc2 == 0 and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in "wmbhr")


def test_vc_and_sqrt_vc(ctx):
    M = _counts(511)
    n = M.shape[0]
    rc, ice = _call(ctx, M, method=0, ignore_diags=1, tol=0.0, max_iters=1)
    rc1, vc = _call(ctx, M, method=1, ignore_diags=1, tol=0.3, max_iters=77)          # (tol and max_iters are forced to 0 and 1)
    assert rc == 0 and rc1 == 0 and all(np.asarray(ice[k]).tobytes() == np.asarray(vc[k]).tobytes() for k in "wmbhr")
    rc, sq = _call(ctx, M, method=2, ignore_diags=1)
    want = R.balance(M, "sqrt-vc", ignore_diags=1, min_nnz=1)
    gap = np.abs(sq["w"] / want["weights"] - 1).max() / ((4 * n + 12) * U)
    print(f"sqrt-VC: weights at {gap:.3g} of the one-round bound")
    assert rc == 0 and int(sq["r"][0]) == 1 and sq["r"][1] == 0.0 and gap <= 1.0 and sq["h"][0] == ice["h"][0] and sq["h"][1] != ice["h"][1]
    assert sq["b"].tobytes() == ((sq["w"][:, None] * sq["w"][None, :]) * M).tobytes()


def test_refusals(ctx):
    from chromosome3d_amd import Solver, lib
    n = 64
    M = _counts(n)
    ok = dict(ignore_diags=2, min_nnz=1, tol=1e-5, max_iters=20)
    _refused(ctx, "n < 2", M, n=1, **ok)
    _refused(ctx, "n < 2", M, n=0, **ok)
    big = np.zeros((1, 1))
    _refused(ctx, "max_beads", big, n=5121, **ok)                                 # refused before the matrix is read
    for spoil, word in ((np.nan, "not finite"), (np.inf, "not finite"), (-1.0, "negative")):
        B = M.copy()
        B[3, 40] = B[40, 3] = spoil
        _refused(ctx, word, B, **ok)
    B = M.copy()
    B[3, 40] += 1.0
    _refused(ctx, "not symmetric", B, **ok)
    B = M.copy()
    B[5, 5] = np.nan                                                            # inside the ignored band: refused all the same, `balanced` covers every diagonal
    _refused(ctx, "not finite", B, **ok)
    for bad in (0.0, np.nan, -2.0, np.inf):
        w0 = np.ones(n)
        w0[9] = bad
        _refused(ctx, "start weight", M, w0=w0, **ok)
    for method in (1, 2):
        _refused(ctx, "w0", M, method=method, w0=np.ones(n), **ok)
    for method in (-1, 3):
        _refused(ctx, "method", M, method=method, **ok)
    _refused(ctx, "flag", M, flags=2, **ok)
    _refused(ctx, "ignore_diags", M, **{**ok, "ignore_diags": -1})
    _refused(ctx, "tol", M, **{**ok, "tol": -1e-9})
    _refused(ctx, "tol", M, **{**ok, "tol": np.nan})
    _refused(ctx, "max_iters", M, **{**ok, "max_iters": -1})
    _refused(ctx, "max_iters", M, **{**ok, "max_iters": 10001})
    for target in (0.0, -1.0, np.nan, np.inf):
        _refused(ctx, "target", M, target=target, **ok)
    L = lib.load()
    assert L.c3d_balance_matrix(ctx._h, None, n, 0, 0, 2, 1, None, None, 1e-5, 20, 1.0, None, None, None, None, None, None) == C3D_ERR_INVALID
    rc, got = _call(ctx, M, **ok)                                                # and the context works
    assert rc == 0 and got["r"][1] == 1.0
    s2 = Solver(0)                                                              # the limit follows the option
    try:
        s2.set_option("max_beads", 6000)
        _refused(s2, "max_beads", big, n=6001, **ok)
    finally:
        s2.close()


def test_end_to_end_through_the_solver():
    """Solver.balance -> set_if_matrix -> a short schedule; the restraints are the positive balanced entries at |i - j| >= min_sep"""
    from chromosome3d_amd import Solver, default_model, make_stages, pipeline
    M, _ = _example()
    n = M.shape[0]
    s = Solver(0)
    try:
        out = s.balance(M, "ice", min_nnz=1)
        assert out["converged"] and out["rounds"] == 11 and out["kept"] == n - 1 and out["masked_counts"] == [0, 1, 0] and len(out["history"]) == 12
        assert out["var"] == out["history"][-1] < 1e-5 and out["device_ms"] > 0 and out["mean_marginal"] > 0
        B = out["balanced"]
        assert np.array_equal(B, pipeline.balance_if(M, solver=s, min_nnz=1)) and s.balance(M, min_nnz=1, want_matrix=False)["balanced"] is None
        model = default_model()
        s.set_model(model)
        s.set_schedule(make_stages(SHORT))
        s.set_if_matrix(B)
        i = np.arange(n)
        far = (i[None, :] - i[:, None]) >= model.min_sep
        assert s.num_restraints == int(((B > 0) & far).sum()) and s.num_restraints > 0
        assert not (B[n // 3] > 0).any()                                        # the unmappable bin carries no restraint
        s.init_replicas(2)
        s.run()
        x = s.coords()
        assert np.isfinite(x).all() and s.steps_done == 45
        assert np.array_equal(s.balance(M, "ice", min_nnz=1)["balanced"], B) and np.array_equal(s.coords(), x)      # nothing of the solve changes
    finally:
        s.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --balance ice --balance-out p on raw counts of the smallest bundled matrix: the files parse back to the doubles the entry returns"""
    from chromosome3d_amd import pipeline
    from tests.util import load_if
    S = load_if("chr21_1mb")
    n = S.shape[0]
    M, _ = R.worked_example(S, seed=3)
    raw = str(tmp_path / "raw_matrix.txt")
    with open(raw, "w") as f:
        for row in M:
            f.write(" ".join("%d" % v for v in row) + "\n")
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    prefix = str(tmp_path / "bal")
    run = subprocess.run([exe, "--if", raw, "--out", str(tmp_path / "a"), "-m", "2", "--quiet", "--balance", "ice", "--balance-min-nnz", "1", "--balance-out", prefix],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rc, got = _call(ctx, M, ignore_diags=2, min_nnz=1, tol=1e-5, max_iters=200)
    assert rc == 0
    lines = open(prefix + "_weights.txt").read().splitlines()
    assert lines[0] == "bead weight masked" and len(lines) == n + 1
    cols = [l.split() for l in lines[1:]]
    assert [int(c[0]) for c in cols] == list(range(1, n + 1))
    assert np.array([float(c[1]) for c in cols]).tobytes() == got["w"].tobytes() and np.array_equal(np.array([int(c[2]) for c in cols]), got["m"])
    assert pipeline.parse_if_file(prefix + "_matrix.txt").tobytes() == got["b"].tobytes()
    assert os.path.exists(tmp_path / "a" / "raw_matrix_1.pdb") and got["m"][n // 3] == 2
    # the run used the balanced matrix: its restraints are those of the balanced matrix
    tbl = [l for l in open(tmp_path / "a" / "contact.tbl") if l.strip()]
    i = np.arange(n)
    assert len(tbl) == int(((got["b"] > 0) & ((i[None, :] - i[:, None]) >= 5)).sum())
    bad = subprocess.run([exe, "--if", raw, "--out", str(tmp_path / "b"), "--balance", "kr"], capture_output=True, text=True)
    assert bad.returncode == 2 and "ice, vc or sqrt-vc" in bad.stderr


@functools.lru_cache(maxsize=None)
def _large(n):
    """a decay with the separation times b b^T at a size where a matrix is built in place: b_i b_j first, then the decay, both symmetric"""
    rng = np.random.default_rng(n)
    b = np.exp(rng.normal(0.0, 0.3, n))
    decay = 1.0 / (1.0 + np.arange(n)) ** 0.9 + 1e-3
    both = np.concatenate((decay[:0:-1], decay))                                # both[n - 1 + k] = decay[|k|]
    toeplitz = np.lib.stride_tricks.as_strided(both[n - 1:], shape=(n, n), strides=(-both.strides[0], both.strides[0]))
    M = np.multiply.outer(b, b)
    M *= toeplitz
    return M


def test_large():
    """8193 beads (odd: the padded copy, 512 MiB, behind max_beads) for the numbers: 2 rounds in one call with the band, the weights held
    to the one-round bound chained twice; 16384 beads (2 GiB) for one round alone.  No `balanced` read-back at either size."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        n = 8193
        M = _large(n)
        _refused(s, "max_beads", M, ignore_diags=2, min_nnz=1, outs="wmhr")
        s.set_option("max_beads", 16384)
        rc, got = _call(s, M, ignore_diags=2, min_nnz=1, tol=0.0, max_iters=2, outs="wmhrd")
        assert rc == 0 and int(got["r"][0]) == 2 and int(got["r"][3]) == n and (got["m"] == 0).all()
        want = R.balance(M, "ice", ignore_diags=2, min_nnz=1, tol=0.0, max_iters=2, want_matrix=False)
        gap = np.abs(got["w"] / want["weights"] - 1).max() / (2 * (4 * n + 12) * U)
        print(f"n = {n}: 2 rounds, weights at {gap:.3g} of the bound, device {got['d']:.2f} ms")
        assert gap <= 1.0 and np.abs(got["h"] / np.asarray(want["history"], dtype=float) - 1).max() < 1e-9
        _large.cache_clear()
        del M
        n = 16384
        M = _large(n)
        rc, got = _call(s, M, ignore_diags=0, min_nnz=1, tol=0.0, max_iters=1, outs="whrd")
        assert rc == 0 and int(got["r"][0]) == 1 and int(got["r"][3]) == n
        want = R.balance(M, "ice", ignore_diags=0, min_nnz=1, tol=0.0, max_iters=1, want_matrix=False)
        gap = np.abs(got["w"] / want["weights"] - 1).max() / ((4 * n + 12) * U)
        print(f"n = {n}: 1 round, weights at {gap:.3g} of the bound, device {got['d']:.2f} ms")
        assert gap <= 1.0
    finally:
        _large.cache_clear()
        s.close()
