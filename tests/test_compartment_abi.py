"""The ABI of c3d_compartments and c3d_compartment_start, as far as it can be checked without a GPU: declared with the argument lists of
the issue under the definitions, bound with the header's argument lists, wrapped and exported; the start vectors are the restatement's bit
for bit; without a context the entry refuses and names itself; the CLI lists its options; the launchers have their stubs in the fake-HIP
harness and the storm calls the entry.  tests/test_gpu_compartments.py holds the numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import compartment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32), "int": C.c_int}
LAUNCHERS = ("launch_compartment_if_check", "launch_compartment_build", "launch_compartment_round", "launch_compartment_finish", "launch_compartment_fit")


def _header():
    return open(os.path.join(ROOT, "include", "c3d.h")).read()


def _declared(name):
    """the ctypes argument list of `name` as include/c3d.h declares it"""
    m = re.search(r"^int\s+%s\s*\(([^;]*)\)\s*;" % name, _header(), re.M)
    assert m, name
    args = []
    for a in m.group(1).split(","):
        kind = re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", "* ", a.strip())).rsplit(" ", 1)[0].strip()
        args.append(CTYPE[kind])
    return args


def test_header_declares_the_entries_as_the_issue_gives_them():
    h = _header()
    assert re.search(r"^#define\s+C3D_COMPARTMENT_MAX_VECTORS\s+3\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_COMPARTMENT_MAX_ITERS\s+10000\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_COMPARTMENT_CONSENSUS\s+1\b", h, re.M)
    assert re.search(r"^int\s+c3d_compartment_start\s*\(\s*int\s+n,\s*int\s+n_vec,\s*double\s*\*\s*start\s*\)\s*;", h, re.M)
    proto = re.search(r"^int\s+c3d_compartments\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*IF,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,"
                      r"\s*const\s+int32_t\s*\*\s*pick,\s*int\s+n_pick,\s*int\s+flags,\s*int\s+min_sep,\s*int\s+n_vec,\s*int\s+iters,\s*const\s+double\s*\*\s*start,"
                      r"\s*double\s*\*\s*expected,\s*double\s*\*\s*vectors,\s*double\s*\*\s*share,\s*double\s*\*\s*residual,"
                      r"\s*double\s*\*\s*agreement,\s*double\s*\*\s*same_side,\s*double\s*\*\s*device_ms\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definitions, the refusals and the scratch stand above the prototype
    for phrase in ("E[s] = mean over i of M(i, i+s)", "E[0] = 0", "X(i,j) = M(i,j) / E[|i-j|]", "the two-pass form", "live = the number of rows with q_i > 0",
                   "w = X (D v) - (m^T D v) 1", "C v = D (X w - m (1^T w)) / n", "modified Gram-Schmidt in index order", "share = lambda_a / live",
                   "dependent start vectors", "the entry of largest magnitude is positive (lowest index on", "|Pearson r|", "an exact count divided once",
                   "h *= 0x85EBCA6B", "no atomics", "two calls return the same bytes", "C3D_ERR_NOMEM", "8 n^2 bytes per map in flight", "C3D_SCORE_SCRATCH_BYTES",
                   "one 2 GiB slot at 16384", "at 455 beads x 20 models"):
        assert phrase in above, phrase


def test_prototypes_match_the_header_and_the_symbols_are_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name in ("c3d_compartment_start", "c3d_compartments"):
        assert name in lib.SIGNATURES and hasattr(L, name)
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int and args == _declared(name), name
    assert (lib.COMPARTMENT_MAX_VECTORS, lib.COMPARTMENT_MAX_ITERS, lib.COMPARTMENT_CONSENSUS) == (3, 10000, 1)
    assert callable(Solver.compartments) and callable(pipeline.compartment_report)


def test_the_start_vectors_of_the_library_are_the_restatements_bit_for_bit(built):
    from chromosome3d_amd import lib
    L = lib.load()
    for n, nv in ((3, 1), (3, 2), (4, 3), (455, 3), (16384, 3)):
        s = np.full((nv, n), 7.0)
        assert L.c3d_compartment_start(n, nv, lib.dptr(s)) == 0
        assert s.tobytes() == R.start(n, nv).tobytes(), (n, nv)
    s = np.full((3, 8), 7.0)
    for n, nv in ((2, 1), (0, 1), (-5, 1), (8, 0), (8, 4), (3, 3), (8, -1)):
        assert L.c3d_compartment_start(n, nv, lib.dptr(s)) == C3D_ERR_INVALID and b"c3d_compartment_start" in L.c3d_last_error(), (n, nv)
    assert L.c3d_compartment_start(8, 2, None) == C3D_ERR_INVALID and b"c3d_compartment_start" in L.c3d_last_error()
    assert (s == 7.0).all()


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, ms = np.full(64, 7.0), C.c_double(7.0)
    p = lib.dptr(out)
    assert L.c3d_compartments(None, None, None, 0, None, 0, 0, 1, 1, 10, None, p, p, p, p, None, None, C.byref(ms)) == C3D_ERR_INVALID
    assert b"c3d_compartments" in L.c3d_last_error() and (out == 7.0).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--compartments <prefix>", "_compartments.txt", "--compartment-vectors <1..3>", "--compartment-iters <k>", "--compartment-min-sep <s>",
                "bead IF consensus pc1_1 ... pc1_M"):
        assert opt in out.stderr, opt


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    kernels = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_compartment.inc")).read()
    for name in LAUNCHERS:
        for text in (internal, stub, kernels):
            assert re.search(r"^hipError_t %s\(" % name, text, re.M), name
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_compartments(") >= 2 and "C3D_ERR_INVALID" in storm[storm.index("c3d_compartments("):]
