"""The restatement of the L-BFGS move's rows (lbfgs_ref.move_row_ref, the expected values of tests/test_gpu_lbfgs_move_rows.py) admitted on
the CPU: on real vectors of a case of tests/lbfgs_cases.py it is lbfgs_run's own per-bead move and compact_direction's direction to
1e-12 A; every mutation of MOVE_MUTATIONS moves some row of the table by at least 100 of that row's bounds; the table's rows are what
they are meant to be (exact in their type, NaN in every slot outside the mask, the cap's edge on adjacent values, the seed's range)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import controller_ref as R
from tests import lbfgs_cases as LC
from tests import lbfgs_ref as L

MAX_STEP = 0.5          # TABLE_FIRE leaves the library's max_step


def test_table_max_step_is_the_librarys(built):
    from chromosome3d_amd import default_fire
    assert float(default_fire(**R.TABLE_FIRE).max_step) == MAX_STEP


@pytest.mark.parametrize("max_step", [None, 0.004])
def test_move_row_is_lbfgs_runs_move_and_the_compact_direction(built, max_step):
    """wrap_m5 at 96 beads, slot 0: every step's pairs, gamma and force are rebuilt from lbfgs_run's checkpoints and log, laid into a ring
    (slots outside the mask NaN), and each bead's row gives lbfgs_run's next coordinates and compact_direction's direction"""
    name, n, M = "wrap_m5", 96, L.MAX_PAIRS
    case = LC.CASES[name]
    _, _, om, of = LC.models(case, n)
    d10 = R.problem(n)[1]
    force = lambda u: O.energy_force(om, d10, u, *case.weights)[0]
    ms = float(of.max_step) if max_step is None else max_step
    x0 = LC.start(name, n, 0).astype(np.float64)
    K = 12
    _, info = L.lbfgs_run(force, x0, K, m=case.mem, g0=LC.first_length(case, n), max_step=ms, checkpoints=range(1, K + 1))
    xs = [x0] + [info["checkpoints"][k] for k in range(1, K + 1)]
    Fs = [force(x) for x in xs]
    capped = uncapped = 0
    for k, step in enumerate(info["log"]):
        assert step.branch in ("first", "kept"), step.branch            # (no rejection, no drop in this window: the pairs are the last ones)
        p = step.pairs
        S = [(xs[j + 1] - xs[j]).reshape(-1) for j in range(k - p, k)]   # age order, oldest first
        Y = [(Fs[j] - Fs[j + 1]).reshape(-1) for j in range(k - p, k)]
        F, gamma = Fs[k].reshape(-1), step.gamma
        coef, mask = np.zeros(1 + 2 * M), 0
        coef[0] = gamma
        slots = [(step.slot - (p - 1) + i) % case.mem for i in range(p)]
        ring_s, ring_y = np.full((M, n, 3), np.nan), np.full((M, n, 3), np.nan)
        if p:
            Sm, Ym, g = np.array(S), np.array(Y), -F
            Rinv = np.linalg.inv(np.triu(Sm @ Ym.T))
            ps, py = Sm @ g, Ym @ g
            top = Rinv.T @ ((np.diag(np.diag(Sm @ Ym.T)) + gamma * (Ym @ Ym.T)) @ (Rinv @ ps)) - Rinv.T @ (gamma * py)
            bot = -Rinv @ ps
            for i, sl in enumerate(slots):
                coef[1 + sl], coef[1 + M + sl] = -top[i], -gamma * bot[i]
                ring_s[sl], ring_y[sl] = S[i].reshape(n, 3), Y[i].reshape(n, 3)
                mask |= 1 << sl
        for sl in range(M):
            if not (mask >> sl) & 1:
                coef[1 + sl], coef[1 + M + sl] = 0.37, -0.21                 # a slot outside the mask: NaN vectors, a coefficient that is not 0
        d_ref = L.compact_direction(F, S, Y, gamma).reshape(n, 3)
        slot = (step.slot + 1) % case.mem
        for i in range(n):
            row = np.concatenate([xs[k][i], Fs[k][i], ring_s[:, i].reshape(-1), ring_y[:, i].reshape(-1)])
            out, _, cap = L.move_row_ref(coef, mask, slot, row, ms)
            free = L.move_row_ref(coef, mask, slot, row, np.inf)[0]
            assert np.abs(free[3:6] - d_ref[i]).max() < 1e-12, (k, i, free[3:6], d_ref[i])
            assert np.abs(out[0:3] - xs[k + 1][i]).max() < 1e-12, (k, i, out[0:3], xs[k + 1][i])
            assert np.abs(out[3:6] - (xs[k + 1][i] - xs[k][i])).max() < 1e-12 and not np.isnan(out[[0, 1, 2, 3, 4, 5, 9]]).any()
            capped, uncapped = capped + cap, uncapped + (not cap)
        assert sum(1 for s_ in info["log"][:k + 1] if s_.pairs) == max(0, k)        # every step after the first has pairs
    assert uncapped > 50 and (max_step is None or capped > 50), (capped, uncapped)        # both sides of the cap on real vectors
    assert max(s_.pairs for s_ in info["log"]) == case.mem


def _table(prec):
    for mask, slot in L.MOVE_CALLS:
        coef = L.move_coef(prec, mask)
        for r, tag in L.move_rows(prec, mask, slot, MAX_STEP):
            yield coef, mask, slot, r, tag


@pytest.mark.parametrize("prec", [32, 64])
def test_move_rows_are_what_they_are_meant_to_be(prec):
    T = np.float32 if prec == 32 else np.float64
    M = L.MAX_PAIRS
    masks = [m for m, _ in L.MOVE_CALLS]
    assert set(masks) >= {0, 0xFF, 0x55, 0xAA, 0x80} | {1 << j for j in range(M)} and len(L.MOVE_CALLS) <= 12
    assert any((m >> s) & 1 for m, s in L.MOVE_CALLS) and any(not (m >> s) & 1 for m, s in L.MOVE_CALLS)      # the slot of s in and out of the mask
    total, tags, edges = 0, {}, 0
    for mask, slot in L.MOVE_CALLS:
        coef = L.move_coef(prec, mask)
        assert np.array_equal(coef.astype(T).astype(np.float64), coef) and (coef != 0).all() and len(set(coef)) == len(coef)
        rows = L.move_rows(prec, mask, slot, MAX_STEP)
        total += len(rows)
        prev = None
        for r, tag in rows:
            tags[tag] = tags.get(tag, 0) + 1
            assert np.array_equal(r.astype(T).astype(np.float64), r, equal_nan=True), (mask, tag)
            s, y = r[6:6 + 3 * M].reshape(M, 3), r[6 + 3 * M:].reshape(M, 3)
            for j in range(M):
                assert np.isnan(s[j]).all() and np.isnan(y[j]).all() if not (mask >> j) & 1 else not (np.isnan(s[j]).any() or np.isnan(y[j]).any())
            out, scale, capped = L.move_row_ref(coef, mask, slot, r, MAX_STEP)
            if tag != "nan":
                assert not np.isnan(out[[0, 1, 2, 3, 4, 5, 9]]).any(), (mask, tag)
            l2 = float(np.sum(L.move_row_ref(coef, mask, slot, r, np.inf)[0][3:6] ** 2))
            if tag in ("capped", "seed", "beyond", "edge") and mask:
                d = L.move_row_ref(coef, mask, slot, r, np.inf)[0][3:6]
                assert np.allclose(np.abs(d), scale, rtol=1e-12), (mask, tag)                   # terms of one sign: the scale is |d|
            if tag == "edge":
                if prev is not None and prev[1] == "edge" and np.array_equal(np.delete(prev[0], 5), np.delete(r, 5), equal_nan=True):
                    lo = L.move_row_ref(coef, mask, slot, prev[0], MAX_STEP)
                    assert not lo[2] and capped and float(np.nextafter(T(prev[0][5]), T(np.inf) if r[5] > prev[0][5] else T(-np.inf))) == r[5]
                    edges += 1
            if tag == "seed":
                assert capped and (l2 > 0.99 * float(np.finfo(np.float32).max) if prec == 32 else any(abs(l2 / t - 1) < 1e-9 for t in R.SEED_EDGE_D2)), (mask, l2)
            if tag == "beyond":
                assert prec == 32 and l2 > float(np.finfo(np.float32).max) and np.isfinite(L.move_row_ref(coef, mask, slot, r, np.inf)[0][3:6].astype(T)).all()
            prev = (r, tag)
    assert 200 <= total <= 400 and edges == 2 * len(L.MOVE_CALLS), (total, edges)
    assert {"plain", "capped", "edge", "seed", "nan"} <= set(tags) and (("beyond" in tags) == (prec == 32))
    # F = 0, a -0 and a NaN; x = 0 and x beside it; a denormal move
    rows = [r for _, _, _, r, _ in _table(prec)]
    assert any(not r[3:6].any() for r in rows) and any(np.signbit(r[4]) and r[4] == 0 for r in rows) and any(np.isnan(r[4]) for r in rows)
    assert any(not r[0:3].any() for r in rows) and any(r[0:3].all() for r in rows)
    tiny = float(np.finfo(T).tiny)
    assert any(0 < abs(L.move_row_ref(L.move_coef(prec, m), m, s, r, MAX_STEP)[0][3]) < tiny for _, m, s, r, _ in _table(prec))


@pytest.mark.parametrize("prec", [32, 64])
@pytest.mark.parametrize("mut", sorted(L.MOVE_MUTATIONS))
def test_move_table_catches_every_mutation(prec, mut):
    """each mutation moves some output of some row by at least 100 of that row's bounds (or turns it into a NaN: a slot outside the mask read)"""
    worst = 0.0
    for coef, mask, slot, r, tag in _table(prec):
        if tag == "nan":
            continue
        a, scale, capped = L.move_row_ref(coef, mask, slot, r, MAX_STEP)
        b = L.move_row_ref(coef, mask, slot, r, MAX_STEP, mut=mut)[0]
        bound = L.move_row_bounds(prec, mask, r, a, scale, capped)
        for k in (0, 1, 2, 3, 4, 5, 9):
            if b[k] != b[k]:
                worst = float("inf")
            elif b[k] != a[k]:
                with np.errstate(over="ignore"):            # (a mutated row may differ by more than a double holds in units of its bound)
                    worst = max(worst, float(np.divide(abs(b[k] - a[k]), bound[k])) if bound[k] > 0 else float("inf"))
    print(f"precision {prec}, {mut} ({L.MOVE_MUTATIONS[mut]}): {worst:.3g} bounds")
    assert worst >= 100.0, worst


def test_move_row_check_refuses_a_wrong_row():
    """the device test's own assertion fails on a touched neighbour, a NaN, an s that is not x' - x at x = 0, a move.move of another vector"""
    prec, (mask, slot) = 64, L.MOVE_CALLS[9]
    coef = L.move_coef(prec, mask)
    r, tag = next((r, t) for r, t in L.move_rows(prec, mask, slot, MAX_STEP) if t == "capped" and not r[0:3].any())
    good = L.move_row_ref(coef, mask, slot, r, MAX_STEP)[0]
    assert L.move_row_check(prec, coef, mask, slot, r, tag, good, MAX_STEP) == 0.0
    for k, v in ((6, good[6] + 1e-9), (1, float("nan")), (4, good[4] * (1 + 1e-12)), (9, good[9] * (1 + 1e-12)), (0, good[0] * (1 + 1e-13))):
        bad = good.copy()
        bad[k] = v
        with pytest.raises(AssertionError):
            L.move_row_check(prec, coef, mask, slot, r, tag, bad, MAX_STEP)
