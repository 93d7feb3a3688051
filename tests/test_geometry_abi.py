"""The ABI of the model-geometry entries (c3d_geometry_replicas, c3d_separation_profile), as far as it can be checked without a GPU:
declared with the argument lists of the issue, bound with the header's argument list, wrapped and exported; without a context they refuse
and name themselves; the stat keys are known to c3d_get_stat; the CLI lists its options; the launchers have their stubs in the fake-HIP
harness that tests/test_superpose_abi.py links.  tests/test_gpu_geometry.py holds the numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32),
         "int32_t*": C.POINTER(C.c_int32), "int64_t*": C.POINTER(C.c_int64), "int": C.c_int, "double": C.c_double}


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


def test_header_declares_both_entries_as_the_issue_gives_them():
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^#define\s+C3D_GEOMETRY_FIELDS\s+6\s*$", h, re.M)
    assert re.search(r"^int\s+c3d_geometry_replicas\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*double\s+cutoff,\s*int\s+sep,"
                     r"\s*int64_t\s*\*\s*clashes,\s*int32_t\s*\*\s*bead_clashes,\s*double\s*\*\s*nearest,\s*double\s*\*\s*chain\s*\)\s*;", h, re.M)
    assert re.search(r"^int\s+c3d_separation_profile\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*const\s+int32_t\s*\*\s*pick,"
                     r"\s*int\s+n_pick,\s*double\s+cutoff,\s*double\s*\*\s*mean,\s*double\s*\*\s*sd,\s*double\s*\*\s*contact\s*\)\s*;", h, re.M)
    assert "ON PURPOSE not the `<=` of the clash count" in h                     # the header says why the two comparisons differ
    assert '"geometry_runs"' in h and '"separation_runs"' in h


def test_prototypes_match_the_header_and_the_symbols_are_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name in ("c3d_geometry_replicas", "c3d_separation_profile"):
        assert name in lib.SIGNATURES and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int and args == _declared(name), name
    assert lib.GEOMETRY_FIELDS == 6
    assert callable(Solver.geometry) and callable(Solver.separation_profile) and callable(pipeline.geometry_report)


def test_without_a_context_both_refuse_and_name_themselves(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out = np.zeros(8)
    cl = np.zeros(1, np.int64)
    assert L.c3d_geometry_replicas(None, None, 0, 3.5, 1, cl.ctypes.data_as(C.POINTER(C.c_int64)), None, None, lib.dptr(out)) == C3D_ERR_INVALID
    assert b"c3d_geometry_replicas" in L.c3d_last_error()
    assert L.c3d_separation_profile(None, None, 0, None, 0, 7.6, lib.dptr(out), None, None) == C3D_ERR_INVALID
    assert b"c3d_separation_profile" in L.c3d_last_error()
    v = C.c_double()
    for key in (b"geometry_runs", b"separation_runs"):
        assert L.c3d_get_stat(None, key, C.byref(v)) == C3D_ERR_INVALID
    from tests.util import stub_context_knows_stat
    for key in ("geometry_runs", "separation_runs"):                             # and c3d_get_stat knows the keys
        assert stub_context_knows_stat(key)


def test_the_cli_lists_the_options(built):
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--geometry <prefix>", "--clash-cutoff", "--clash-sep", "_geometry.txt", "_separation.txt", "default 3.5"):
        assert opt in out.stderr, opt


def test_the_launchers_have_their_stubs():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    for name in ("launch_geometry", "launch_separation_profile"):
        assert re.search(r"^hipError_t %s\(" % name, internal, re.M) and re.search(r"^hipError_t %s\(" % name, stub, re.M)
