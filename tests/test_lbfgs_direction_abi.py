"""The ABI of the L-BFGS controller's table hook (c3d_debug_lbfgs_direction), as far as it can be checked without a GPU: declared, bound and
wrapped, the sizes the header states are the ones the Python side allocates; without a context or with bad arguments it returns
C3D_ERR_INVALID naming itself.  tests/test_gpu_lbfgs_direction.py holds the numbers."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1


def test_header_declares_the_entry_and_its_sizes(built):
    from chromosome3d_amd import lib
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_debug_lbfgs_direction\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+rows,\s*const\s+double\s*\*\s*sums,"
                     r"\s*const\s+int32_t\s*\*\s*state_int_in,\s*const\s+double\s*\*\s*state_dbl_in,\s*const\s+int32_t\s*\*\s*first,"
                     r"\s*const\s+int32_t\s*\*\s*mem0,\s*int32_t\s*\*\s*state_int_out,\s*double\s*\*\s*state_dbl_out,\s*double\s*\*\s*coef,"
                     r"\s*int32_t\s*\*\s*mask_slot\s*\)\s*;", h, re.M)
    pairs = int(re.search(r"^#define\s+C3D_LBFGS_MAX_PAIRS\s+(\d+)\s*$", h, re.M).group(1))
    assert re.search(r"^#define\s+C3D_LBFGS_SUMS\s+\(4 \* C3D_LBFGS_MAX_PAIRS \+ 4\)\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_LBFGS_STATE_DOUBLES\s+\(1 \+ 2 \* C3D_LBFGS_MAX_PAIRS \* C3D_LBFGS_MAX_PAIRS\)\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_LBFGS_COEFS\s+\(1 \+ 2 \* C3D_LBFGS_MAX_PAIRS\)\s*$", h, re.M)
    assert (lib.LBFGS_MAX_PAIRS, lib.LBFGS_SUMS, lib.LBFGS_STATE_DOUBLES, lib.LBFGS_COEFS) == (pairs, 4 * pairs + 4, 1 + 2 * pairs * pairs, 1 + 2 * pairs)
    from tests import lbfgs_ref
    assert (lbfgs_ref.MAX_PAIRS, lbfgs_ref.NSUMS) == (lib.LBFGS_MAX_PAIRS, lib.LBFGS_SUMS)


def test_the_entry_is_bound_and_wrapped(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_debug_lbfgs_direction" in lib.SIGNATURES and hasattr(L, "c3d_debug_lbfgs_direction")
    assert len(lib.SIGNATURES["c3d_debug_lbfgs_direction"][1]) == 11
    assert callable(Solver.debug_lbfgs_direction)


def test_the_kernels_and_the_production_moves_share_one_text(built):
    """the serial section exists once: both move kernels and both table kernels include c3d_lbfgs_serial.inc, and the statements that
    decide a step (the pair test, the doubling, the clamp) stand nowhere else in the L-BFGS sources"""
    src = os.path.join(ROOT, "chromosome3d_amd", "csrc")
    inc = open(os.path.join(src, "c3d_lbfgs_serial.inc")).read()
    for stmt in ("sy > 1e-12 * sqrt(ss * yy)", "st.gamma *= 2.0;", "st.gamma = fmin(fmax(st.gamma, 1e-7), 1e2);"):
        assert inc.count(stmt) == 1, stmt
    for name in ("c3d_lbfgs.h", "c3d_f64.hip"):
        text = open(os.path.join(src, name)).read()
        assert text.count('#include "c3d_lbfgs_serial.inc"') == 2, name
        assert "st.gamma *= 2.0" not in text and "1e-12 * sqrt" not in text, name


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    d, i = np.zeros(129, dtype=np.float64), np.zeros(4, dtype=np.int32)
    args = (lib.dptr(d), lib.i32ptr(i), lib.dptr(d), lib.i32ptr(i), lib.i32ptr(i), lib.i32ptr(i), lib.dptr(d), lib.dptr(d), lib.i32ptr(i))
    assert L.c3d_debug_lbfgs_direction(None, 1, *args) == C3D_ERR_INVALID
    assert b"c3d_debug_lbfgs_direction" in L.c3d_last_error()
