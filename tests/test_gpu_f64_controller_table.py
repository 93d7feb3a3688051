"""The fp64 step controller and the fp64 row update as tables.  c3d_debug_step_scalars_f64 runs c3d_f64_scalars.inc, and
c3d_debug_row_finish_f64 runs c3d_f64_row_finish.inc — the two texts every k64_step kernel includes — a thread a row on one
precision-64 context.  Expected values: the numpy float64 restatements of the oracle's statements (controller_ref.step_scalars_ref with
precision=64, controller_ref.row_finish_ref), which tests/test_controller_ref.py admits on the CPU: every branch taken, every edge row at
its edge, every mutation caught, and the row restatement equal to the oracle's own steps.

Bounds, in double ulps of the expected value, stated before any run:
  scalars          8    rcp64 / sqrt64 claim "a rounding or two" (2 ulps each), at most three are chained (1 / F.F, the product's square
                        root, times alpha), the restatement's own roundings besides
  rows, capped     8    the same for the cap's 1 / sqrt(d2), carried into a product and a sum of one sign
  rows, plain      2    products and sums only
Integer state is exact; NaN where the oracle has NaN; zero where it has zero; an infinite value where it has one.  No row is skipped.
The largest gaps seen are in profiles/r31_f64_controller_table.md."""
import numpy as np
import pytest

from tests import controller_ref as R
from tests.util import load_if

pytestmark = pytest.mark.gpu

SCALARS_CAP, CAPPED_CAP, PLAIN_CAP = 8.0, 8.0, 2.0
ROW_DT = 2.0 ** -9


@pytest.fixture(scope="module")
def ctx64():
    """one precision-64 context on chr21_1mb under the table's model and FIRE values"""
    from chromosome3d_amd import Solver, default_fire, default_model, make_stages
    s = Solver(0)
    s.set_option("precision", 64)
    m, fire = default_model(**R.TABLE_MODEL), default_fire(**R.TABLE_FIRE)
    s.set_model(m)
    s.set_if_matrix(load_if("chr21_1mb"))
    assert s.n == R.TABLE_N
    s.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]), fire)
    s.table = (R.table_consts64(m, s.n), fire)
    yield s
    s.close()


def _gap(got, want, cap, where):
    """the gap of one output in double ulps, asserted against cap"""
    if np.isnan(want):
        assert np.isnan(got), where + (got, want)
        return 0.0
    g = R.ulps(float(got), want)
    assert g <= cap, where + (float(got), want, g, cap)
    return g


@pytest.mark.parametrize("kind", R.SCALAR_KINDS)
def test_f64_step_scalars_table_equals_the_oracles_statements(ctx64, kind):
    consts, fire = ctx64.table
    rows = R.table_rows64(kind, consts[0])
    by_step = {}
    for r in rows:
        by_step.setdefault(r[:2], []).append(r)
    checked, worst = 0, 0.0
    for (dt, t_bath), group in by_step.items():                 # one launch per (kind, dt, t_bath)
        psum = np.array([g[2] for g in group], dtype=np.float64)
        state = np.array([g[3] for g in group], dtype=np.float64)
        npos = np.array([g[4] for g in group], dtype=np.int32)
        sc, so, no = ctx64.debug_step_scalars_f64(kind, dt, t_bath, psum, state, npos)
        for i in range(len(group)):
            want_sc, want_st, want_n = R.step_scalars_ref(kind, dt, t_bath, psum[i], state[i], int(npos[i]), consts, fire, precision=64)
            assert no[i] == want_n, (kind, group[i], no[i], want_n)
            for got, want in zip(list(sc[i]) + list(so[i]), list(want_sc) + list(want_st)):
                worst = max(worst, _gap(got, want, SCALARS_CAP, (kind, group[i])))
            checked += 1
    print(f"fp64 scalars kind {kind}: {checked} rows, largest gap {worst:.3g} double ulps")
    assert checked == len(rows) >= 24


@pytest.mark.parametrize("kind", R.ROW_KINDS)
def test_f64_row_finish_table_equals_the_oracles_statements(ctx64, kind):
    consts, fire = ctx64.table
    rows = R.row_finish_rows(kind, ROW_DT, consts, fire)
    out = ctx64.debug_row_finish_f64(kind, ROW_DT, np.array([r for r, _ in rows], dtype=np.float64))      # one launch per kind
    assert out.shape == (len(rows), 10)
    checked, worst = 0, {"plain": 0.0, "capped": 0.0}
    for i, (r, tag) in enumerate(rows):
        want = R.row_finish_ref(kind, ROW_DT, r, consts, fire)
        for got, w in zip(out[i], want):
            worst[tag] = max(worst[tag], _gap(got, w, CAPPED_CAP if tag == "capped" else PLAIN_CAP, (kind, i, tag, r)))
        checked += 1
    print(f"fp64 row finish kind {kind}: {checked} rows, largest gap plain {worst['plain']:.3g}, capped {worst['capped']:.3g} double ulps")
    assert checked == len(rows) >= 50
    if kind in (2, 3, 5, 6):
        assert sum(1 for _, t in rows if t == "capped") >= 20


@pytest.mark.parametrize("entry", ["scalars", "rows"])
def test_f64_tables_refuse_what_they_do_not_run(ctx64, entry):
    """a context that is not precision 64, a kind outside the entry's list, rows outside 1 .. 2^20: C3D_ERR_INVALID naming the entry"""
    from chromosome3d_amd import Solver, lib
    L = lib.load()
    plain = Solver(0)                      # a context of the default precision
    d, i = np.zeros(64, dtype=np.float64), np.zeros(4, dtype=np.int32)
    sargs = (lib.dptr(d), lib.dptr(d), lib.i32ptr(i), lib.dptr(d), lib.dptr(d), lib.i32ptr(i))
    name = "c3d_debug_step_scalars_f64" if entry == "scalars" else "c3d_debug_row_finish_f64"

    def call(h, kind, rows):
        if entry == "scalars":
            return L.c3d_debug_step_scalars_f64(h, kind, 0.0, 0.0, rows, *sargs)
        return L.c3d_debug_row_finish_f64(h, kind, 0.0, rows, lib.dptr(d), lib.dptr(d))

    bad_kinds = (4, 7, 8, 9, -1) if entry == "scalars" else (7, 8, 9, -1)
    for h, kind, rows in [(plain._h, 2, 1)] + [(ctx64._h, k, 1) for k in bad_kinds] + [(ctx64._h, 2, 0), (ctx64._h, 2, (1 << 20) + 1)]:
        assert call(h, kind, rows) == -1, (kind, rows)
        assert name.encode() in L.c3d_last_error(), (kind, rows, L.c3d_last_error())
    plain.close()
    assert call(ctx64._h, 2, 1) == 0
