"""The ABI of the ensemble's distance map (c3d_ensemble_map, c3d_ensemble_score), as far as it can be checked without a GPU: declared,
bound with the header's argument list, wrapped and exported; without a context they refuse and name themselves; the stat keys are known
to c3d_get_stat's list; the CLI lists its options.  (tests/test_superpose_abi.py links the fake-HIP harness, which needs the new launchers'
stubs.)  tests/test_gpu_ensemble.py holds the numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32),
         "int": C.c_int, "double": C.c_double}


def _declared(name):
    """the ctypes argument list of `name` as include/c3d.h declares it"""
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    m = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, h, re.M)
    assert m, name
    args = []
    for a in m.group(1).split(","):
        kind = re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", "* ", a.strip())).rsplit(" ", 1)[0].strip()
        args.append(CTYPE[kind])
    return args


def test_header_declares_both_entries_as_the_issue_gives_them(built):
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_ensemble_map\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*const\s+int32_t\s*\*\s*pick,\s*int\s+n_pick,"
                     r"\s*double\s+cutoff,\s*double\s*\*\s*mean,\s*double\s*\*\s*sd,\s*double\s*\*\s*contact\s*\)\s*;", h, re.M)
    assert re.search(r"^int\s+c3d_ensemble_score\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*IF,\s*int\s+range,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,"
                     r"\s*const\s+int32_t\s*\*\s*pick,\s*int\s+n_pick,\s*double\s+cutoff,\s*double\s*\*\s*rho_mean,\s*double\s*\*\s*rho_contact\s*\)\s*;", h, re.M)
    assert "NO host ranking" in h                                                # the header says that there is no fallback
    assert '"ensemble_map_runs"' in h and '"ensemble_score_runs"' in h


def test_prototypes_match_the_header_and_the_symbols_are_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name in ("c3d_ensemble_map", "c3d_ensemble_score"):
        assert name in lib.SIGNATURES and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int and args == _declared(name), name
    assert callable(Solver.ensemble_map) and callable(Solver.ensemble_score) and callable(pipeline.ensemble_maps)


def test_without_a_context_both_refuse_and_name_themselves(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out = np.zeros(4)
    assert L.c3d_ensemble_map(None, None, 0, None, 0, 7.6, lib.dptr(out), None, None) == C3D_ERR_INVALID
    assert b"c3d_ensemble_map" in L.c3d_last_error()
    assert L.c3d_ensemble_score(None, lib.dptr(out), 3, None, 0, None, 0, 7.6, lib.dptr(out), None) == C3D_ERR_INVALID
    assert b"c3d_ensemble_score" in L.c3d_last_error()
    v = C.c_double()
    for key in (b"ensemble_map_runs", b"ensemble_score_runs"):
        assert L.c3d_get_stat(None, key, C.byref(v)) == C3D_ERR_INVALID
    from tests.util import stub_context_knows_stat
    for key in ("ensemble_map_runs", "ensemble_score_runs"):                     # and c3d_get_stat knows the keys
        assert stub_context_knows_stat(key)


def test_the_cli_lists_the_options(built):
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--ensemble <prefix>", "--ensemble-top", "--ensemble-cutoff", "convention"):
        assert opt in out.stderr, opt


def test_the_launchers_have_their_stubs():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    for name in ("launch_ensemble_map", "launch_ensemble_corr"):
        assert re.search(r"^hipError_t %s\(" % name, internal, re.M) and re.search(r"^hipError_t %s\(" % name, stub, re.M)
