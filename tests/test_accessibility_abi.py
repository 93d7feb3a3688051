"""The ABI of c3d_accessibility and c3d_sphere_points, as far as it can be checked without a GPU: declared with the argument lists of the
issue, bound with the header's argument lists, wrapped and exported; the lattice is the restatement's; without a context the entry refuses
and names itself; the CLI lists its options; the launcher has its stub in the fake-HIP harness.  tests/test_gpu_accessibility.py holds the
numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import accessibility_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "int32_t*": C.POINTER(C.c_int32), "int": C.c_int,
         "double": C.c_double}


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


def test_header_declares_the_entries_as_the_issue_gives_them():
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^#define\s+C3D_ACCESS_MAX_POINTS\s+1024\s*$", h, re.M)
    assert re.search(r"^int\s+c3d_sphere_points\s*\(\s*int\s+n_points,\s*double\s*\*\s*u\s*\)\s*;", h, re.M)
    proto = re.search(r"^int\s+c3d_accessibility\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*double\s+radius,\s*double\s+probe,"
                      r"\s*const\s+double\s*\*\s*points,\s*int\s+n_points,\s*int32_t\s*\*\s*exposed,\s*double\s*\*\s*device_ms\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definition, the refusals and the scratch stand above the prototype
    for phrase in ("R = radius + probe, R2 = R * R", "c = x_i + R u_p", "((ex ex) + ey ey) + ez ez < R2", "left out by index, not by distance",
                   "z = 1 - (2k+1)/P, r = sqrt(1 - z z), phi = k pi (3 - sqrt 5)", "within 1e-9 of 1", "[0.01, 1e5]", "28 n K + 24 P",
                   "0.26 MB at 455 beads x 20 models", "9.2 MB at 16384 x 20", "C3D_ERR_NOMEM"):
        assert phrase in above, phrase


def test_prototypes_match_the_header_and_the_symbols_are_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name in ("c3d_sphere_points", "c3d_accessibility"):
        assert name in lib.SIGNATURES and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int and args == _declared(name), name
    assert lib.ACCESS_MAX_POINTS == 1024
    assert callable(Solver.accessibility) and callable(pipeline.accessibility_report)


def test_the_lattice_of_the_library_is_the_restatements(built):
    from chromosome3d_amd import lib
    L = lib.load()
    for P in (1, 2, 63, 96, 1024):
        u = np.full((P, 3), 7.0)
        assert L.c3d_sphere_points(P, lib.dptr(u)) == 0
        assert np.abs(u - A.lattice(P)).max() <= 1e-15, P
    u = np.full((4, 3), 7.0)
    for P in (0, -1, 1025):
        assert L.c3d_sphere_points(P, lib.dptr(u)) == C3D_ERR_INVALID and b"c3d_sphere_points" in L.c3d_last_error()
    assert L.c3d_sphere_points(4, None) == C3D_ERR_INVALID and b"c3d_sphere_points" in L.c3d_last_error()
    assert (u == 7.0).all()


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, ms = np.full(8, 7, np.int32), C.c_double(7.0)
    assert L.c3d_accessibility(None, None, 0, 1.965, 1.965, None, 96, lib.i32ptr(out), C.byref(ms)) == C3D_ERR_INVALID
    assert b"c3d_accessibility" in L.c3d_last_error() and (out == 7).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--accessibility <prefix>", "_accessibility.txt", "--bead-radius <A>", "--probe-radius <A>", "--sphere-points <P>", "bead mean f_1 ... f_M"):
        assert opt in out.stderr, opt


def test_the_launcher_has_its_stub_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    assert re.search(r"^hipError_t launch_accessibility\(", internal, re.M) and re.search(r"^hipError_t launch_accessibility\(", stub, re.M)
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_accessibility(") >= 2 and "C3D_ERR_INVALID" in storm[storm.index("c3d_accessibility("):]
