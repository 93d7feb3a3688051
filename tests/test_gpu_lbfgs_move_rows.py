"""The rows of the L-BFGS move as a table, in both precisions.  c3d_debug_lbfgs_move_rows runs c3d_lbfgs_move_row.inc — section 3 of
k_lbfgs_move and of k64_lbfgs_move: direction over the slot mask, per-bead cap, move, s into the ring, move.move — a thread a row over a
ring in the kernels' own layout.  Expected values: lbfgs_ref.move_row_ref in float64, which tests/test_lbfgs_ref.py ties to lbfgs_run's own
move and to compact_direction on the CPU and holds to ten mutations.

Bounds (lbfgs_ref.move_row_bounds, fixed before any run; T = the context's type): a direction component (2 pairs + 2) ulps of its scale
gamma |F_c| + sum |a_j s_jc| + sum |b_j y_jc| (one fma a term, gamma F, the narrowed coefficient); a capped row — terms of one sign — the
same count in ulps of the move + 8 for the cap (the cap of both row-update tables); x' one ulp of x' more where x is not 0; move.move
twice the move's relative bound + 2 ulps, and within 2 ulps of the fma order of the stored s; the ring's s equals x' bit for bit at x = 0;
the neighbouring ring slot comes back bit for bit.  Every ring slot outside the mask holds NaN with a non-zero coefficient: no NaN may
reach an output.  Rows at and beyond the range of the cap's float seed (d.d near FLT_MAX and beyond it with d finite in fp32; 2^127 ..
1e300 in fp64) are held as capped rows.  The largest gaps seen are in profiles/r32_row_tables.md."""
import numpy as np
import pytest

from tests import controller_ref as R
from tests import lbfgs_ref as L
from tests.util import load_if

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[32, 64])
def ctx(request):
    from chromosome3d_amd import Solver, default_fire, default_model, make_stages
    s = Solver(0)
    if request.param == 64:
        s.set_option("precision", 64)
    fire = default_fire(**R.TABLE_FIRE)
    s.set_model(default_model(**R.TABLE_MODEL))
    s.set_if_matrix(load_if("chr21_1mb"))
    s.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]), fire)
    s.prec, s.max_step = request.param, float(fire.max_step)
    yield s
    s.close()


def test_lbfgs_move_rows_equal_the_restatement(ctx):
    total, worst = 0, {}
    for mask, slot in L.MOVE_CALLS:                                   # a dozen launches
        coef = L.move_coef(ctx.prec, mask)
        rows = L.move_rows(ctx.prec, mask, slot, ctx.max_step)
        out = ctx.debug_lbfgs_move_rows(coef, mask, slot, np.array([r for r, _ in rows]))
        assert out.shape == (len(rows), 10)
        for i, (r, tag) in enumerate(rows):
            worst[tag] = max(worst.get(tag, 0.0), L.move_row_check(ctx.prec, coef, mask, slot, r, tag, out[i], ctx.max_step))
        total += len(rows)
    print(f"L-BFGS move rows, precision {ctx.prec}: {total} rows in {len(L.MOVE_CALLS)} calls, largest |difference| / bound "
          + ", ".join(f"{t} {w:.3g}" for t, w in sorted(worst.items())))
    assert 200 <= total <= 400 and {"plain", "capped", "edge", "seed", "nan"} <= set(worst)


def test_lbfgs_move_rows_refuse_what_they_do_not_run(ctx):
    from chromosome3d_amd import lib
    L_ = lib.load()
    d = np.zeros(64, dtype=np.float64)
    for rows, mask, slot in ((0, 1, 0), ((1 << 16) + 1, 1, 0), (1, -1, 0), (1, 256, 0), (1, 1, -1), (1, 1, 8)):
        assert L_.c3d_debug_lbfgs_move_rows(ctx._h, rows, lib.dptr(d), mask, slot, lib.dptr(d), lib.dptr(d)) == -1, (rows, mask, slot)
        assert b"c3d_debug_lbfgs_move_rows:" in L_.c3d_last_error()
    assert L_.c3d_debug_lbfgs_move_rows(ctx._h, 1, lib.dptr(d), 0, 0, lib.dptr(d), lib.dptr(d)) == 0
