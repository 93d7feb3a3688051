"""The fp32 row update as a table.  c3d_debug_row_finish runs finish_row (c3d_step_core.h) — the function every k_cluster, k_cluster_tp,
k_step and k_update_sym step calls once per row — a thread a row on one context.  Expected values: controller_ref.row_finish_ref with
precision=32, the float64 restatement of the oracle's per-bead statements on the row's float32 inputs and the host's float constants,
which tests/test_controller_ref.py admits on the CPU (branches, edges, mutations, and a float32 emulation of finish_row inside the bounds).

Bounds, in float ulps of the expected value, stated before any run (controller_ref.row_gap32 asserts them):
  rows, plain      4    the velocity takes 3 roundings (dt acc, a product, an fma), the move one fma more
  rows, capped     8    d.d carries twice the move's relative error, v_rsq_f32 is 1 ulp and halves d.d's, then one product and one fma of one
                        sign; "overflow" rows (d.d at most one float below FLT_MAX) are capped rows
Integer-like outputs are exact; NaN where the restatement has NaN; +-0 and infinities as it has them (a value beyond FLT_MAX is the float's
infinity).  No row is skipped.  Beyond the stated domain (|d| < 2^63: rows tagged beyond, beyond_s, infinite) v' and the sums are held as
everywhere and the coordinates to what DESIGN.md section 2 states: the bead stays, or is NaN where the move itself is infinite.
The largest gaps seen are in profiles/r32_row_tables.md."""
import time

import numpy as np
import pytest

from tests import controller_ref as R
from tests.util import load_if

pytestmark = pytest.mark.gpu

ROW_DT = 2.0 ** -9


@pytest.fixture(scope="module")
def ctx():
    """one fp32 context on chr21_1mb under the table's model and FIRE values"""
    from chromosome3d_amd import Solver, default_fire, default_model, make_stages
    s = Solver(0)
    m, fire = default_model(**R.TABLE_MODEL), default_fire(**R.TABLE_FIRE)
    s.set_model(m)
    s.set_if_matrix(load_if("chr21_1mb"))
    assert s.n == R.TABLE_N
    s.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]), fire)
    s.table = (R.table_consts(m, s.n), fire)
    yield s
    s.close()


@pytest.mark.parametrize("kind", R.ROW_KINDS)
def test_row_finish_table_equals_the_oracles_statements(ctx, kind):
    consts, fire = ctx.table
    rows = R.row_finish_rows32(kind, ROW_DT, consts, fire)
    table = np.array([r for r, _ in rows], dtype=np.float32)
    assert np.array_equal(table.astype(np.float64), np.array([r for r, _ in rows]), equal_nan=True)      # every input is a float
    t0 = time.perf_counter()
    out = ctx.debug_row_finish(kind, ROW_DT, table)                                                      # one launch per kind
    took = time.perf_counter() - t0
    assert out.shape == (len(rows), 10) and out.dtype == np.float32
    worst, count = {}, {}
    for i, (r, tag) in enumerate(rows):
        want = R.row_finish_ref(kind, ROW_DT, r, consts, fire, precision=32)
        worst[tag] = max(worst.get(tag, 0.0), R.row_gap32(out[i], want, tag, r))
        count[tag] = count.get(tag, 0) + 1
    print(f"fp32 row finish kind {kind}: {len(rows)} rows in {took * 1e3:.1f} ms, largest gap in float ulps "
          + ", ".join(f"{t} {worst[t]:.3g} ({count[t]} rows)" for t in R.ROW_TAGS32 if t in worst))
    assert sum(count.values()) == len(rows) >= 50
    if kind in (2, 3, 5, 6):
        assert count["capped"] >= 20 and count["overflow"] >= 1 and count["beyond"] >= 1
    if kind in (5, 6):
        assert count["infinite"] >= 1


def test_row_finish_refuses_what_it_does_not_run(ctx):
    """a kind outside 0 .. 6, rows outside 1 .. 2^20: C3D_ERR_INVALID naming the entry"""
    from chromosome3d_amd import lib
    L = lib.load()
    f = np.zeros(64, dtype=np.float32)
    for kind, rows in [(k, 1) for k in (7, 8, 9, -1)] + [(2, 0), (2, (1 << 20) + 1)]:
        assert L.c3d_debug_row_finish(ctx._h, kind, 0.0, rows, lib.fptr(f), lib.fptr(f)) == -1, (kind, rows)
        assert b"c3d_debug_row_finish:" in L.c3d_last_error(), (kind, rows, L.c3d_last_error())
    assert L.c3d_debug_row_finish(ctx._h, 2, 0.0, 1, lib.fptr(f), lib.fptr(f)) == 0
