"""The ABI of c3d_stratified_score, as far as it can be checked without a GPU: declared with the argument list of the issue, bound with the
header's argument list, wrapped and exported; without a context it refuses and names itself; the stat key is known to c3d_get_stat; the
CLI lists its options; the launchers have their stubs in the fake-HIP harness.  tests/test_gpu_stratified.py holds the numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "int64_t*": C.POINTER(C.c_int64), "int": C.c_int}


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


def test_header_declares_the_entry_as_the_issue_gives_it():
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^#define\s+C3D_STRATUM_FIELDS\s+3\s*$", h, re.M)
    assert re.search(r"^int\s+c3d_stratified_score\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*IF,\s*int\s+range,\s*int\s+max_sep,\s*const\s+double\s*\*\s*extra_xyz,"
                     r"\s*int\s+n_extra,\s*double\s*\*\s*rho,\s*double\s*\*\s*scc,\s*int64_t\s*\*\s*sums\s*\)\s*;", h, re.M)
    for phrase in ("#{smaller} + #{not larger} + 1", "C = N sum a_i b_i - T^2", "rho[k][s] = (double)C / sqrt((double)A * (double)B) when A > 0 and B > 0",
                   "in ascending s, each sum one sequential chain", "scc[k] = num / den, or NaN when no stratum counts", '"stratified_runs"'):
        assert phrase in h, phrase                                               # the definition stands above the prototype


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    name = "c3d_stratified_score"
    assert name in lib.SIGNATURES and hasattr(L, name)
    res, args = lib.SIGNATURES[name]
    assert res is C.c_int and args == _declared(name)
    assert lib.STRATUM_FIELDS == 3
    assert callable(Solver.stratified_score) and callable(pipeline.stratified_report)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, IF = np.zeros(8), np.zeros((2, 2))
    assert L.c3d_stratified_score(None, lib.dptr(IF), 1, 0, None, 0, lib.dptr(out), None, None) == C3D_ERR_INVALID
    assert b"c3d_stratified_score" in L.c3d_last_error()
    v = C.c_double()
    assert L.c3d_get_stat(None, b"stratified_runs", C.byref(v)) == C3D_ERR_INVALID
    from tests.util import stub_context_knows_stat
    assert stub_context_knows_stat("stratified_runs")                           # and c3d_get_stat knows the key
    assert "stratified_runs" in open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_ctx.h")).read()


def test_the_cli_lists_the_options(built):
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--stratified <prefix>", "--stratified-max-sep <S>", "_scc.txt", "_strata.txt", "`nan`"):
        assert opt in out.stderr, opt


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    for name in ("launch_stratified_if", "launch_stratified_models"):
        assert re.search(r"^hipError_t %s\(" % name, internal, re.M) and re.search(r"^hipError_t %s\(" % name, stub, re.M)
    assert "c3d_stratified_score(" in open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
