"""The ABI of device scoring for large maps, as far as it can be checked without a GPU: the hook c3d_debug_if_ranks and the scratch budget
are declared and bound; without a context the calls return
C3D_ERR_INVALID as c3d.h documents; with a device the names are accepted and bad values refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1


def test_header_declares_the_hook_and_the_budget(built):
    """what a binding needs from c3d.h: the hook's prototype and the scratch budget as a macro with a value"""
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_debug_if_ranks\s*\(", h, re.M)
    assert re.search(r"^#define\s+C3D_SCORE_SCRATCH_BYTES\s+\S", h, re.M)


def test_the_hook_is_bound_and_refuses_null_arguments(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_debug_if_ranks" in lib.SIGNATURES and hasattr(Solver, "debug_if_ranks")
    IF = np.ones((4, 4))
    rank = np.empty((4, 4))
    saa, m = C.c_double(), C.c_size_t()
    assert L.c3d_debug_if_ranks(None, lib.dptr(IF), 3, lib.dptr(rank), C.byref(saa), C.byref(m)) == C3D_ERR_INVALID
    assert b"c3d_debug_if_ranks" in L.c3d_last_error()
    v = C.c_double()
    assert L.c3d_set_option(None, b"device_ranks", 1.0) == C3D_ERR_INVALID
    assert L.c3d_get_stat(None, b"device_rank_runs", C.byref(v)) == C3D_ERR_INVALID
    assert L.c3d_get_stat(None, b"score_wide_runs", C.byref(v)) == C3D_ERR_INVALID


def test_names_are_accepted_on_a_context(built):
    """With a device: the option takes -1, 0 and 1 and nothing else, and both stats start at 0.  Without one c3d_create itself fails
    (C3D_ERR_NO_DEVICE), which is all a context-bound name can be asked here: on a CPU box this test says nothing about the names —
    the context code that takes them runs there under the fake HIP layer of tools/sanitize only; tests/test_gpu_score_large.py sets
    and reads every one of them."""
    from chromosome3d_amd import C3DError, Solver, lib
    L = lib.load()
    if L.c3d_device_count() <= 0:
        h = C.c_void_p()
        assert L.c3d_create(0, C.byref(h)) == -2 and b"no HIP device" in L.c3d_last_error()
        return
    s = Solver(0)
    try:
        for v in (-1, 1, 0):
            s.set_option("device_ranks", v)
        for bad in (2, -2, 0.5):
            with pytest.raises(C3DError, match="device_ranks"):
                s.set_option("device_ranks", bad)
        assert s.stat("device_rank_runs") == 0 and s.stat("score_wide_runs") == 0
    finally:
        s.close()
