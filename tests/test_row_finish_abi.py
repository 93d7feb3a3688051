"""The ABI of the fp32 row update's table hook (c3d_debug_row_finish), as far as it can be checked without a GPU: declared, bound and
wrapped; without a context it returns C3D_ERR_INVALID naming itself; every refusal names the entry; the table kernel calls finish_row
itself, the one definition every fp32 step kernel calls.  tests/test_gpu_row_finish_table.py holds the numbers."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "chromosome3d_amd", "csrc")
C3D_ERR_INVALID = -1


def test_header_declares_the_entry(built):
    from chromosome3d_amd import lib
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_debug_row_finish\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+kind,\s*float\s+dt,\s*int\s+rows,\s*const\s+float\s*\*\s*in,"
                     r"\s*float\s*\*\s*out\s*\)\s*;", h, re.M)
    assert (lib.ROW_FINISH_IN, lib.ROW_FINISH_OUT) == (16, 10)
    assert "|d| < 2^63" in h[h.index("Test hook: the fp32 row update"):h.index("int c3d_debug_row_finish(")]      # the stated domain


def test_the_entry_is_bound_and_wrapped(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_debug_row_finish" in lib.SIGNATURES and hasattr(L, "c3d_debug_row_finish")
    assert len(lib.SIGNATURES["c3d_debug_row_finish"][1]) == 6
    assert callable(Solver.debug_row_finish)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    f = np.zeros(16, dtype=np.float32)
    assert L.c3d_debug_row_finish(None, 2, 0.0, 1, lib.fptr(f), lib.fptr(f)) == C3D_ERR_INVALID
    assert b"c3d_debug_row_finish:" in L.c3d_last_error()


def test_the_refusals_name_the_entry():
    text = open(os.path.join(SRC, "c3d_debug.cpp")).read()
    body = text[text.index('extern "C" int c3d_debug_row_finish('):]
    body = body[:body.index("C3D_ENTRY")]
    for what in ("bad arguments", "kind is 0, 1, 2, 3, 4, 5 or 6", "rows is 1 .. 2^20"):
        assert f'fail(C3D_ERR_INVALID, "c3d_debug_row_finish: {what}")' in body, what
    assert "rows < 1 || rows > (1 << 20)" in body and "kind < 0 || kind > 6" in body and "!c ||" in body


def test_the_table_kernel_calls_the_step_kernels_function():
    """finish_row is defined once, in c3d_step_core.h; k_row_finish calls it, as k_update_sym, k_step's body and k_cluster's do; the host builds
    its arguments with the functions every launch uses; the sanitizer unit's stub of the launcher is there"""
    core, sym = open(os.path.join(SRC, "c3d_step_core.h")).read(), open(os.path.join(SRC, "c3d_sym.hip")).read()
    assert len(re.findall(r"void finish_row\(", core)) == 1
    for name in os.listdir(SRC):
        if name != "c3d_step_core.h":
            assert "void finish_row(" not in open(os.path.join(SRC, name)).read(), name
    kernel = sym[sym.index("__global__ void k_row_finish("):]
    kernel = kernel[:kernel.index("hipError_t launch_row_finish(")]
    assert kernel.count("finish_row(m, p, fp, sc, st,") == 1
    for stmt in ("rsqf", "fmaf(", "max_step"):                      # none of the row update's own statements stands in the table kernel
        assert stmt not in kernel, stmt
    for user in ("c3d_step_body.inc", "c3d_cluster.hip"):
        assert "finish_row(m, p" in open(os.path.join(SRC, user)).read(), user
    run = open(os.path.join(SRC, "c3d_debug.cpp")).read()
    assert "c3d::launch_row_finish(dev_model(c), dev_step(c, kind, dt, 1.0f, 1.0f, 0.85f, 0.0f), dev_fire(c), rows," in run
    assert "hipError_t launch_row_finish(" in open(os.path.join(SRC, "c3d_internal.h")).read()
    assert "hipError_t launch_row_finish(" in open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
