"""The ABI of the controller's table hook (c3d_debug_step_scalars), as far as it can be checked without a GPU: declared, bound and wrapped;
without a context or with bad arguments it returns C3D_ERR_INVALID naming itself.  tests/test_gpu_controllers.py holds the numbers."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1


def test_header_declares_the_entry(built):
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_debug_step_scalars\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+kind,\s*float\s+dt,\s*float\s+t_bath,\s*int\s+rows,"
                     r"\s*const\s+float\s*\*\s*psum,\s*const\s+float\s*\*\s*state_in,\s*const\s+int32_t\s*\*\s*npos_in,\s*float\s*\*\s*scalars,"
                     r"\s*float\s*\*\s*state_out,\s*int32_t\s*\*\s*npos_out\s*\)\s*;", h, re.M)


def test_the_entry_is_bound_and_wrapped(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_debug_step_scalars" in lib.SIGNATURES and hasattr(L, "c3d_debug_step_scalars")
    assert callable(Solver.debug_step_scalars)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    f, i = np.zeros(8, dtype=np.float32), np.zeros(2, dtype=np.int32)
    args = (lib.fptr(f), lib.fptr(f), lib.i32ptr(i), lib.fptr(f), lib.fptr(f), lib.i32ptr(i))
    assert L.c3d_debug_step_scalars(None, 2, 0.0, 0.0, 1, *args) == C3D_ERR_INVALID
    assert b"c3d_debug_step_scalars" in L.c3d_last_error()
