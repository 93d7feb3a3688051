"""The ABI of the L-BFGS move rows' table hook (c3d_debug_lbfgs_move_rows), as far as it can be checked without a GPU: declared, bound and
wrapped, the sizes the header states are the Python side's; without a context it returns C3D_ERR_INVALID naming itself; every refusal
names the entry; both move kernels and both table kernels include the one text, and its statements stand nowhere else.
tests/test_gpu_lbfgs_move_rows.py holds the numbers."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "chromosome3d_amd", "csrc")
C3D_ERR_INVALID = -1


def test_header_declares_the_entry_and_its_sizes(built):
    from chromosome3d_amd import lib
    from tests import lbfgs_ref
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_debug_lbfgs_move_rows\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+rows,\s*const\s+double\s*\*\s*coef,\s*int\s+mask,"
                     r"\s*int\s+slot,\s*const\s+double\s*\*\s*in,\s*double\s*\*\s*out\s*\)\s*;", h, re.M)
    assert re.search(r"^#define\s+C3D_LBFGS_MOVE_ROW_IN\s+\(6 \+ 6 \* C3D_LBFGS_MAX_PAIRS\)\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_LBFGS_MOVE_ROW_OUT\s+10\s*$", h, re.M)
    assert (lib.LBFGS_MOVE_ROW_IN, lib.LBFGS_MOVE_ROW_OUT) == (6 + 6 * lib.LBFGS_MAX_PAIRS, 10) == (lbfgs_ref.MOVE_ROW_IN, lbfgs_ref.MOVE_ROW_OUT)


def test_the_entry_is_bound_and_wrapped(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_debug_lbfgs_move_rows" in lib.SIGNATURES and hasattr(L, "c3d_debug_lbfgs_move_rows")
    assert len(lib.SIGNATURES["c3d_debug_lbfgs_move_rows"][1]) == 7
    assert callable(Solver.debug_lbfgs_move_rows)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    d = np.zeros(54, dtype=np.float64)
    assert L.c3d_debug_lbfgs_move_rows(None, 1, lib.dptr(d), 0, 0, lib.dptr(d), lib.dptr(d)) == C3D_ERR_INVALID
    assert b"c3d_debug_lbfgs_move_rows:" in L.c3d_last_error()


def test_the_refusals_name_the_entry():
    text = open(os.path.join(SRC, "c3d_debug.cpp")).read()
    body = text[text.index('extern "C" int c3d_debug_lbfgs_move_rows('):]
    body = body[:body.index("C3D_ENTRY")]
    for what in ("bad arguments", "rows is 1 .. 2^16", "mask is 0 .. 255", "slot is 0 .. 7"):
        assert f'fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_move_rows: {what}")' in body, what
    assert "rows < 1 || rows > (1 << 16)" in body and "mask < 0 || mask > 255" in body and "slot < 0 || slot >= c3d::kLbfgsMaxPairs" in body


def test_the_move_kernels_and_the_tables_share_one_text():
    """c3d_lbfgs_move_row.inc is included twice by each unit — by its move kernel and by its table kernel, under one definition of the
    type and the cap — and the statements of a row stand in it once and nowhere else in the L-BFGS sources"""
    inc = open(os.path.join(SRC, "c3d_lbfgs_move_row.inc")).read()
    stmts = ("dx = C3D_LBFGS_FMA(a, s[0], C3D_LBFGS_FMA(b, y[0], dx));", "if (!(mask & (1 << j))) continue;", "sn[0] = dx; sn[np] = dy; sn[2 * np] = dz;",
             "xout[ix] = xin[ix] + dx;", "d2 = C3D_LBFGS_FMA(dx, dx, C3D_LBFGS_FMA(dy, dy, dz * dz));", "C3D_LBFGS_T* sn = hs + (size_t)3 * shi[1] * np;")
    for stmt in stmts:
        assert inc.count(stmt) == 1, stmt
    assert inc.index("C3D_LBFGS_CAP") < inc.index("xout[ix] = xin[ix] + dx;") < inc.index("sn[0] = dx;") < inc.index("d2 = C3D_LBFGS_FMA(dx, dx")
    for name, move, table in (("c3d_lbfgs.h", "k_lbfgs_move", "k_lbfgs_move_rows"), ("c3d_f64.hip", "k64_lbfgs_move", "k64_lbfgs_move_rows")):
        text = open(os.path.join(SRC, name)).read()
        assert text.count('#include "c3d_lbfgs_move_row.inc"') == 2, name
        assert text.count("#define C3D_LBFGS_CAP") == 1 and text.count("#define C3D_LBFGS_T ") == 1, name
        for stmt in ("sn[0] = dx", "xout[ix] = xin[ix]", "fma(a, s[0]", "fmaf(a, s[0]"):
            assert stmt not in text, (name, stmt)
        assert re.search(r"void %s\(.*?#include \"c3d_lbfgs_move_row.inc\".*?void %s\(.*?#include \"c3d_lbfgs_move_row.inc\"" % (move, table), text, re.S), name
    mk = open(os.path.join(SRC, "Makefile")).read()
    assert mk.count("c3d_lbfgs_move_row.inc") == 2
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    assert "hipError_t launch_lbfgs_move_rows(" in stub and "hipError_t launch_lbfgs_move_rows64(" in stub
