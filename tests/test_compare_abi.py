"""The ABI of the on-device model comparison (c3d_compare_replicas, hook c3d_debug_distance_ranks), as far as it can be checked without a
GPU: both are declared with the model limit, bound and wrapped; without a context they return C3D_ERR_INVALID naming themselves, as c3d.h
documents.  tests/test_gpu_compare.py holds the numbers."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1


def test_header_declares_both_entries_and_the_model_limit(built):
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_compare_replicas\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*double\s*\*\s*spearman,"
                     r"\s*double\s*\*\s*rmsd\s*\)\s*;", h, re.M)
    assert re.search(r"^int\s+c3d_debug_distance_ranks\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+replica,\s*double\s*\*\s*rank\s*\)\s*;", h, re.M)
    assert re.search(r"^#define\s+C3D_COMPARE_MAX_MODELS\s+256\s*$", h, re.M)


def test_both_entries_are_bound_and_wrapped(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name in ("c3d_compare_replicas", "c3d_debug_distance_ranks"):
        assert name in lib.SIGNATURES and hasattr(L, name)
    assert callable(Solver.compare) and callable(Solver.debug_distance_ranks) and callable(pipeline.compare_models)


def test_without_a_context_both_refuse_and_name_themselves(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out = np.zeros(9)
    assert L.c3d_compare_replicas(None, None, 0, lib.dptr(out), lib.dptr(out)) == C3D_ERR_INVALID
    assert b"c3d_compare_replicas" in L.c3d_last_error()
    assert L.c3d_debug_distance_ranks(None, 0, lib.dptr(out)) == C3D_ERR_INVALID
    assert b"c3d_debug_distance_ranks" in L.c3d_last_error()
    v = C.c_double()
    assert L.c3d_get_stat(None, b"compare_runs", C.byref(v)) == C3D_ERR_INVALID


def test_the_cli_lists_the_option(built):
    import subprocess
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--similarity" in out.stderr
