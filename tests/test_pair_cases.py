"""Admission of the pair term's tables (tests/pair_cases.py) on the CPU, before any GPU run: every branch of every potential's softsq /
repel / chain statement is taken by a stated number of rows, every edge row's two neighbours lie on opposite sides of its edge, every row
of table A is isolated (the oracle's force on it is ONE pair's closed form), Newton's third law holds across each pair, the restatement
tests/pair_ref.py equals the oracle on every row, and each of pair_ref's mutations — the ways a pair term goes wrong — moves at least one
row by 100 of the bounds the device test applies, or breaks a row that must be exactly zero."""
import numpy as np
import pytest

from tests import pair_cases as C
from tests import pair_ref as R
from tests.util import oracle_model_from


@pytest.fixture(scope="module")
def O(built):
    from oracle import oracle
    return oracle


def f32(*v):
    return tuple(float(np.float32(a)) for a in v)


def _partner(n):
    h = n // 2
    return np.concatenate([np.arange(h) + h, np.arange(h)])


# ---- layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.SIZES)
def test_partners_sweep_every_column_and_row_slot(n):
    """both beads of a pair are rows and columns: every column 0 .. n - 1 is some row's partner (so every lane and every column slot of
    every column block, the narrow last block and the left-over columns of 328 included), the rows take every row-of-wave slot, and every
    (row slot, column slot) combination a pair (p, p + n/2) can take is met"""
    cols, rows, both = C.sweep(n)
    assert cols == set(range(n)) and rows == {0, 1, 2, 3}
    assert {a for a, _ in both} == {0, 1, 2, 3} == {b for _, b in both}
    assert n % 2 == 0 and n // 2 >= 5             # min_sep


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("n", C.SIZES)
def test_table_a_is_isolated_and_clear_of_the_padding(built, n, precision):
    m, _, _ = C.model_a("shipped")
    T = C.table_for("a", n, m, precision)
    assert T["x"].dtype == (np.float32 if precision == 32 else np.float64)
    seen = set()
    for r in range(len(C.REGIMES)):
        near, pad = C.isolation(T["x"][r], _partner(n), 0.0)
        assert near > 2.0 * m.r0_rep and pad > 1000.0, (r, near, pad)
        seen |= {row[4] for row in T["meta"][r]}
    assert len(seen) == 26                        # every axis and diagonal with every sign pattern
    x = T["x"][0].astype(np.float64)
    assert np.array_equal(x[0], [0, 0, 0]) and np.array_equal(x[n // 2], [2.5, 0, 0]) and T["t10"][0, n // 2] == 25      # d = t exactly


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("variant", C.A_VARIANTS)
def test_table_a_edges_are_straddled(built, variant, precision):
    m, _, _ = C.model_a(variant)
    n = 250
    T = C.table_for("a", n, m, precision)
    h, edges = n // 2, 0
    for r, rows in enumerate(T["meta"]):
        by_edge = {}
        for p, (regime, kind, d, side, u) in enumerate(rows):
            if kind == "edge":
                got = C.dist(T["x"][r, p], T["x"][r, p + h])
                assert (got < d) if side < 0 else (got >= d), (variant, r, p, float(got), d, side)
                by_edge.setdefault((T["cls"][p], d), set()).add(side)
                edges += 1
        assert all(s == {-1, 1} for s in by_edge.values()), (variant, r, by_edge)
    assert edges >= 100


@pytest.mark.parametrize("variant", C.B_VARIANTS)
def test_table_b_edges_are_straddled(built, variant):
    m = C.model_b(variant)
    for precision in (32, 64):
        T = C.table_for("b", 250, m, precision)
        for r in range(2):
            assert len(T["edges"][r]) >= 16
            for a, b, d, side in T["edges"][r]:
                got = C.dist(T["x"][r, a], T["x"][r, b])
                assert (got < d) if side < 0 else (got >= d), (variant, r, a, b, float(got), d)
        # bond_exact: d01 == b0 to the bit on the runs whose site has a zero coordinate
        exact = sum(1 for a, length, shape in T["runs"] if shape == "bond_exact" and float(C.dist(T["x"][0, a], T["x"][0, a + 1])) == m.b0)
        assert exact >= 4, (variant, precision, exact)
        one_step = T["x"][0] != T["x"][1]
        assert one_step.sum() == len(T["edges"][0])           # the replicas differ by one step of one coordinate per edge, nothing else


# ---- branches ---------------------------------------------------------------------------------------------------------------------------
# rows (beads) a branch must be taken by, at every size
MIN_ROWS = 8


@pytest.mark.parametrize("variant", C.A_VARIANTS)
def test_every_noe_and_repel_branch_is_taken_in_table_a(built, variant):
    m, pot, gen = C.model_a(variant)
    P = R.params_from(m)
    n = 250
    T = C.table_for("a", n, m, 32)
    counts, inside, outside, coincident = {}, 0, 0, 0
    for r in range(len(C.REGIMES)):
        ref = R.energy_force(P, T["t10"], T["x"][r], *f32(*C.STAGE))
        for b in (0, 1, 2, 3):
            counts[b] = counts.get(b, 0) + int((ref["branch"] == b).sum())
        inside += int(ref["rep"].sum())
        outside += int((~ref["rep"] & (T["t10"] > 0)).sum())
        coincident += int((ref["r2"][np.arange(n), _partner(n)] == 0).sum())
    want = {0: (0, 1, 2), 1: (0, 1), 2: (0,), 3: (0, 1, 3)}[P["noe_pot"]]
    for b in want:
        assert counts[b] >= MIN_ROWS, (variant, b, counts)
    assert inside >= MIN_ROWS and outside >= MIN_ROWS and coincident >= MIN_ROWS, (variant, inside, outside, coincident)
    print(variant, "rows per NOE branch (square, upper, mirrored lower, soft lower):", counts, "repel inside", inside, "coincident", coincident)


@pytest.mark.parametrize("variant", C.B_VARIANTS)
def test_every_chain_branch_is_taken_in_table_b(built, variant):
    m = C.model_b(variant)
    P = R.params_from(m)
    n = 250
    T = C.table_for("b", n, m, 32)
    idx = np.arange(n)
    sep = np.abs(idx[:, None] - idx[None, :])
    for r in range(2):
        ref = R.energy_force(P, T["t10"], T["x"][r], *f32(*C.STAGE))
        d = np.sqrt(ref["r2"])
        took_back = int(ref["taken_back"].sum())
        at_rep_sep_inside = int(((sep == P["rep_sep"]) & ref["rep"]).sum())
        ang_on, ang_off = int(ref["ang"].sum()), int(((sep == 2) & ~ref["ang"]).sum())
        below_b0, above_b0 = int(((sep == 1) & (d < P["b0"])).sum()), int(((sep == 1) & (d >= P["b0"])).sum())
        assert at_rep_sep_inside >= MIN_ROWS and below_b0 >= MIN_ROWS and above_b0 >= MIN_ROWS, (variant, r, at_rep_sep_inside, below_b0, above_b0)
        assert took_back >= MIN_ROWS or P["rep_sep"] == 1, (variant, r, took_back)
        if P["k_ang"] == 0:
            assert ang_on == 0
        elif P["ang_mode"] == 0:
            assert ang_on >= MIN_ROWS and ang_off >= MIN_ROWS, (variant, r, ang_on, ang_off)
        else:
            assert ang_on >= MIN_ROWS and ang_off == 0
        # the first and last two beads of the chain are rows of runs; the listed pairs closer than min_sep are there
        assert T["runs"][0][0] == 0 and sum(length for _, length, _ in T["runs"]) == n
        assert len(T["listed_close"]) >= 8 and all(b - a < P["min_sep"] for a, b in T["listed_close"])
        assert not (ref["branch"][tuple(np.array(T["listed_close"]).T)] >= 0).any()
        print(variant, r, "taken back", took_back, "at rep_sep inside the radius", at_rep_sep_inside, "angle on / off", ang_on, ang_off)


# ---- the restatement against the oracle ---------------------------------------------------------------------------------------------------
def _against_oracle(O, m, T, n, label):
    P, om = R.params_from(m), oracle_model_from(m, n)
    for w in C.WEIGHTS:
        for r in range(T["x"].shape[0]):
            x = T["x"][r].astype(np.float64)
            ref = R.energy_force(P, T["t10"], x, *f32(*w))
            Fo, eo = O.energy_force(om, T["t10"], x, *f32(*w))
            tol = 1e-12 * ref["scale"]
            assert (np.abs(ref["F"] - Fo) <= tol).all(), (label, w, r, float((np.abs(ref["F"] - Fo) / np.maximum(ref["scale"], 1e-300)).max()))
            for a, b, s in zip(ref["e"], eo, ref["abs_e"]):
                assert abs(a - b) <= 1e-12 * max(s, 1e-300), (label, w, r, a, b)
            yield r, x, ref, Fo


# every variant at 250; the larger sizes' tables differ from those in the layout alone: two variants there
@pytest.mark.parametrize("variant,n", [(v, 250) for v in C.A_VARIANTS] + [(v, n) for v in ("shipped", "gen3") for n in C.SIZES[1:]])
def test_table_a_rows_are_one_pair_term_and_the_restatement_is_the_oracle(built, O, variant, n):
    m, _, _ = C.model_a(variant)
    T = C.table_for("a", n, m, 32)
    partner = _partner(n)
    idx = np.arange(n)
    for r, x, ref, Fo in _against_oracle(O, m, T, n, variant):
        single = ref["coef"][idx, partner][:, None] * (x - x[partner])
        assert (np.abs(Fo - single) <= 1e-12 * ref["scale"]).all(), (variant, n, r)          # isolated
        assert (np.abs(Fo + Fo[partner]) <= 1e-12 * ref["scale"]).all(), (variant, n, r)     # Newton's third law


@pytest.mark.parametrize("variant", C.B_VARIANTS)
def test_table_b_restatement_is_the_oracle(built, O, variant):
    m = C.model_b(variant)
    for n in (250, 328):
        T = C.table_for("b", n, m, 32)
        for r, x, ref, Fo in _against_oracle(O, m, T, n, variant):
            assert abs(Fo.sum(0)).max() <= 1e-12 * ref["scale"].sum()                          # Newton's third law, summed over the chain


# ---- sensitivity --------------------------------------------------------------------------------------------------------------------------
def _worst_in_bounds(P, T, w, mut, none_rows=None):
    """the largest |F_mutated - F| / bound over a table's rows (inf where the mutation leaves a NaN or breaks an exact zero)"""
    worst = 0.0
    for r in range(T["x"].shape[0]):
        x = T["x"][r].astype(np.float64)
        ref = R.energy_force(P, T["t10"], x, *f32(*w), guard=R.GUARD32)
        bad = R.energy_force(P, T["t10"], x, *f32(*w), mut=mut)
        if not np.isfinite(bad["F"]).all():
            return np.inf
        if none_rows is not None and (bad["F"][none_rows] != 0).any():
            return np.inf
        bound = R.force_bound(ref, 32)
        diff = np.abs(bad["F"] - ref["F"])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(diff > 0, diff / bound, 0.0))))
    return worst


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_each_mutation_moves_a_row_by_100_bounds(built, mut):
    n = 250
    worst, where = 0.0, None
    for variant in C.A_VARIANTS:
        m, _, _ = C.model_a(variant)
        T = C.table_for("a", n, m, 32)
        got = _worst_in_bounds(R.params_from(m), T, C.STAGE, mut)
        if got > worst:
            worst, where = got, ("A", variant)
    m0, _, _ = C.model_a("shipped", k_rep=0.0)       # the exact-zero rows: pairs without a target, repel off
    T = C.table_for("a", n, m0, 32)
    none = np.array(T["none"] + [p + n // 2 for p in T["none"]])
    if _worst_in_bounds(R.params_from(m0), T, C.STAGE, mut, none) == np.inf:
        worst, where = np.inf, ("A", "shipped, k_rep 0: an exact zero broken")
    for variant in C.B_VARIANTS:
        m = C.model_b(variant)
        got = _worst_in_bounds(R.params_from(m), C.table_for("b", n, m, 32), C.STAGE, mut)
        if got > worst:
            worst, where = got, ("B", variant)
    print(mut, worst, where)
    assert worst >= 100.0, (mut, worst, where)
