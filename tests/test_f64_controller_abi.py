"""The ABI of the fp64 controller's and row update's table hooks (c3d_debug_step_scalars_f64, c3d_debug_row_finish_f64), as far as it can be
checked without a GPU: declared, bound and wrapped; without a context they return C3D_ERR_INVALID naming themselves; the two texts they
run are the ones the step kernels include, and the deciding statements stand nowhere else.  tests/test_gpu_f64_controller_table.py holds
the numbers."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "chromosome3d_amd", "csrc")
C3D_ERR_INVALID = -1


def test_header_declares_the_entries_and_their_sizes(built):
    from chromosome3d_amd import lib
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_debug_step_scalars_f64\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+kind,\s*double\s+dt,\s*double\s+t_bath,\s*int\s+rows,"
                     r"\s*const\s+double\s*\*\s*psum,\s*const\s+double\s*\*\s*state_in,\s*const\s+int32_t\s*\*\s*npos_in,\s*double\s*\*\s*scalars,"
                     r"\s*double\s*\*\s*state_out,\s*int32_t\s*\*\s*npos_out\s*\)\s*;", h, re.M)
    assert re.search(r"^int\s+c3d_debug_row_finish_f64\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+kind,\s*double\s+dt,\s*int\s+rows,\s*const\s+double\s*\*\s*in,"
                     r"\s*double\s*\*\s*out\s*\)\s*;", h, re.M)
    n_in = int(re.search(r"^#define\s+C3D_ROW_FINISH_IN\s+(\d+)\s*$", h, re.M).group(1))
    n_out = int(re.search(r"^#define\s+C3D_ROW_FINISH_OUT\s+(\d+)\s*$", h, re.M).group(1))
    assert (lib.ROW_FINISH_IN, lib.ROW_FINISH_OUT) == (n_in, n_out) == (16, 10)


def test_the_entries_are_bound_and_wrapped(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name, nargs in (("c3d_debug_step_scalars_f64", 11), ("c3d_debug_row_finish_f64", 6)):
        assert name in lib.SIGNATURES and hasattr(L, name)
        assert len(lib.SIGNATURES[name][1]) == nargs
    assert callable(Solver.debug_step_scalars_f64) and callable(Solver.debug_row_finish_f64)


def test_without_a_context_they_refuse_and_name_themselves(built):
    from chromosome3d_amd import lib
    L = lib.load()
    d, i = np.zeros(16, dtype=np.float64), np.zeros(2, dtype=np.int32)
    args = (lib.dptr(d), lib.dptr(d), lib.i32ptr(i), lib.dptr(d), lib.dptr(d), lib.i32ptr(i))
    assert L.c3d_debug_step_scalars_f64(None, 2, 0.0, 0.0, 1, *args) == C3D_ERR_INVALID
    assert b"c3d_debug_step_scalars_f64" in L.c3d_last_error()
    assert L.c3d_debug_row_finish_f64(None, 2, 0.0, 1, lib.dptr(d), lib.dptr(d)) == C3D_ERR_INVALID
    assert b"c3d_debug_row_finish_f64" in L.c3d_last_error()


def test_the_refusals_name_the_entry():
    """every refusal the entries state (precision, kind, rows) is a C3D_ERR_INVALID that begins with the entry's name"""
    text = open(os.path.join(SRC, "c3d_debug.cpp")).read()
    for name, kinds in (("c3d_debug_step_scalars_f64", "kind is 0, 1, 2, 3, 5 or 6"), ("c3d_debug_row_finish_f64", "kind is 0, 1, 2, 3, 4, 5 or 6")):
        body = text[text.index('extern "C" int ' + name):]
        body = body[:body.index("C3D_ENTRY")]
        for what in (kinds, "rows is 1 .. 2^20", "the context's precision is not 64"):
            assert f'fail(C3D_ERR_INVALID, "{name}: {what}")' in body, (name, what)
        assert "rows < 1 || rows > (1 << 20)" in body and "c->precision != 64" in body


def test_the_kernels_and_the_tables_share_one_text():
    """each text is included exactly twice — by the step body every k64_step kernel is made of and by its table kernel — and the statements
    that decide a step stand in it once and nowhere else in the fp64 sources"""
    body, unit = open(os.path.join(SRC, "c3d_f64_step_body.inc")).read(), open(os.path.join(SRC, "c3d_f64.hip")).read()
    deciding = {
        "c3d_f64_scalars.inc": ("if (tprev < 1e-2) tprev = 1e-2;", "if (l2 < 0) l2 = 0;", "if (s0 > 0) {", "s1 > 1e-30 ? s1 : 1e-30",
                                "if (st.npos > fp.n_min)", "st.dt * fp.f_inc < fp.dt_max", "st.dt *= fp.f_dec;", "(k & 1) ? s0 * rcp64(s2) : s3 * rcp64(s0)",
                                "if (!(a >= 1e-7)) a = 1e-7;", "if (a > 1e2) a = 1e2;"),
        "c3d_f64_row_finish.inc": ("if (d2 > ms2)", "if (d2 > fp.max_step * fp.max_step)", "lam * (v0x - cm0) + acc * Fx", "keep * v0x + mix * Fx",
                                   "q0 = sx * yx + sy * yy + sz * yz;"),
    }
    for name, stmts in deciding.items():
        inc = open(os.path.join(SRC, name)).read()
        assert body.count(f'#include "{name}"') == 1 and unit.count(f'#include "{name}"') == 1, name
        for stmt in stmts:
            assert inc.count(stmt) == 1, (name, stmt)
            assert stmt not in body and stmt not in unit, (name, stmt)
    # the table kernels are the texts' second users
    assert re.search(r"void k64_step_scalars\(.*?#include \"c3d_f64_scalars.inc\"", unit, re.S)
    assert re.search(r"void k64_row_finish\(.*?#include \"c3d_f64_row_finish.inc\"", unit, re.S)
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert "c3d_f64_scalars.inc" in mk and "c3d_f64_row_finish.inc" in mk
