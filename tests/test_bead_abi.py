"""The ABI of c3d_bead_scores, as far as it can be checked without a GPU: declared with the argument list of the issue, bound with the
header's argument list, wrapped and exported; without a context it refuses and names itself; the stat key is known to c3d_get_stat; the
CLI lists its option; the launchers have their stubs in the fake-HIP harness.  tests/test_gpu_bead.py holds the numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "int64_t*": C.POINTER(C.c_int64),
         "const int32_t*": C.POINTER(C.c_int32), "int32_t*": C.POINTER(C.c_int32), "int": C.c_int}


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
    assert re.search(r"^#define\s+C3D_BEAD_FIELDS\s+3\s*$", h, re.M)
    proto = re.search(r"^int\s+c3d_bead_scores\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*IF,\s*int\s+range,\s*const\s+int32_t\s*\*\s*beads,\s*int\s+n_beads,"
                      r"\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*double\s*\*\s*rho,\s*int64_t\s*\*\s*sums,\s*int32_t\s*\*\s*restrained,"
                      r"\s*int32_t\s*\*\s*satisfied,\s*int64_t\s*\*\s*dev_milli\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definition stands above the prototype
    for phrase in ("J(i) = { j : |i-j| >= range }", "N_i = max(0, i-range+1) + max(0, n-i-range)", "#{smaller} + #{not larger} + 1",
                   "C = N sum a_j b_j - T^2", "rho[k*B + b] = (double)C / sqrt((double)A * (double)B) when A > 0 and B > 0", "strictly ascending",
                   "+1 if d < t + 0.5, -1 if d < t - 0.5", "(q - 100 t10) if d > t + 0.2", "(100 t10 - q) if d < t - 0.2", "4 B n", '"bead_runs"'):
        assert phrase in above, phrase


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    name = "c3d_bead_scores"
    assert name in lib.SIGNATURES and hasattr(L, name)
    res, args = lib.SIGNATURES[name]
    assert res is C.c_int and args == _declared(name)
    assert lib.BEAD_FIELDS == 3
    assert callable(Solver.bead_scores) and callable(pipeline.bead_report)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, IF = np.full(8, 7.0), np.zeros((2, 2))
    assert L.c3d_bead_scores(None, lib.dptr(IF), 1, None, 0, None, 0, lib.dptr(out), None, None, None, None) == C3D_ERR_INVALID
    assert b"c3d_bead_scores" in L.c3d_last_error() and (out == 7.0).all()
    v = C.c_double()
    assert L.c3d_get_stat(None, b"bead_runs", C.byref(v)) == C3D_ERR_INVALID
    from tests.util import stub_context_knows_stat
    for key in ("bead_runs", "bead_if_ms", "bead_models_ms"):
        assert stub_context_knows_stat(key)                                      # and c3d_get_stat knows the keys
    assert "bead_runs" in open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_ctx.h")).read()


def test_the_cli_lists_the_option_and_refuses_it_without_a_matrix(built, tmp_path):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--per-bead <prefix>", "_beads.txt", "bead restrained rho_1 satisfied_1 dev_1", "`nan`"):
        assert opt in out.stderr, opt
    tbl = os.path.join(ROOT, "tests", "golden", "chr21_1mb.contact.tbl")         # refused while the options are read: no device is opened
    no_if = subprocess.run([exe, "--tbl", tbl, "--n", "37", "--out", str(tmp_path / "o"), "--per-bead", str(tmp_path / "b")], capture_output=True, text=True)
    assert no_if.returncode == 2 and "--per-bead needs --if" in no_if.stderr and not os.path.exists(tmp_path / "o")


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    for name in ("launch_bead_if", "launch_bead_models"):
        assert re.search(r"^hipError_t %s\(" % name, internal, re.M) and re.search(r"^hipError_t %s\(" % name, stub, re.M)
    assert "c3d_bead_scores(" in open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
