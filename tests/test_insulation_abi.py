"""The ABI of c3d_insulation, as far as it can be checked without a GPU: declared with the argument list of the issue under the definitions,
bound with the header's argument list, wrapped and exported; without a context the entry refuses and names itself; the CLI lists its
options; the launchers have their stubs in the fake-HIP harness and the storm calls the entry.  tests/test_gpu_insulation.py holds the
numbers and the refusals that need replicas."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32),
         "int32_t*": C.POINTER(C.c_int32), "int": C.c_int, "double": C.c_double}
LAUNCHERS = ("launch_insulation_band", "launch_insulation_squares", "launch_insulation_profile", "launch_insulation_fit")


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


def test_header_declares_the_entry_as_the_issue_gives_it():
    h = _header()
    assert re.search(r"^#define\s+C3D_INSULATION_MAX_WINDOW\s+128\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_INSULATION_MAX_WINDOWS\s+8\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_INSULATION_CONSENSUS\s+1\b", h, re.M)
    assert re.search(r"^#define\s+C3D_INSULATION_CONTACT\s+2\b", h, re.M)
    proto = re.search(r"^int\s+c3d_insulation\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*IF,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,"
                      r"\s*const\s+int32_t\s*\*\s*pick,\s*int\s+n_pick,\s*int\s+flags,\s*const\s+int32_t\s*\*\s*windows,\s*int\s+n_win,\s*double\s+cutoff,"
                      r"\s*double\s+min_strength,\s*int\s+tol,\s*double\s*\*\s*mean,\s*double\s*\*\s*score,\s*int32_t\s*\*\s*boundary,\s*double\s*\*\s*strength,"
                      r"\s*double\s*\*\s*fit_r,\s*int32_t\s*\*\s*fit_counts,\s*double\s*\*\s*device_ms\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definitions, the refusals and the scratch stand above the prototype
    for phrase in ("w <= i <= n-1-w", "a in [i-w, i-1] and b in [i+1, i+w]", "2 <= b-a <= 2 w_max", "divided once by Kp", "#{cells: d < cutoff} / w^2",
                   "#{(k, cell): d_k < cutoff} / (w^2 Kp)", "the < is strict", "log2(mean_i / mbar)", "y = -score for IF and for contact maps",
                   "scipy.signal.peak_prominences", "strength = y_i - max(left minimum, right minimum)", "the means first, then the centred sums",
                   "{n_IF, n_map, IF_matched, map_matched}", "r = max(i-a, b-i) = 1..w", "no atomics", "no prefix sums", "two calls return the same bytes",
                   "listed alone or with others", "2w + 1 > n", "C3D_ERR_NOMEM", "16 n w_max per band", "at 455 beads x 20 models", "at 16384 x 20"):
        assert phrase in above, phrase


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_insulation" in lib.SIGNATURES and hasattr(L, "c3d_insulation")
    res, args = lib.SIGNATURES["c3d_insulation"]
    assert res is C.c_int and args == _declared("c3d_insulation")
    assert (lib.INSULATION_MAX_WINDOW, lib.INSULATION_MAX_WINDOWS, lib.INSULATION_CONSENSUS, lib.INSULATION_CONTACT) == (128, 8, 1, 2)
    assert callable(Solver.insulation) and callable(pipeline.insulation_report)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, marks, ms = np.full(64, 7.0), np.full(64, 7, np.int32), C.c_double(7.0)
    w = np.array([1, 2], np.int32)
    p = lib.dptr(out)
    rc = L.c3d_insulation(None, None, None, 0, None, 0, 0, lib.i32ptr(w), 2, 0.0, 0.0, 1, p, p, lib.i32ptr(marks), p, None, None, C.byref(ms))
    assert rc == C3D_ERR_INVALID and b"c3d_insulation" in L.c3d_last_error()
    assert (out == 7.0).all() and (marks == 7).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--insulation <prefix>", "_insulation.txt", "--insulation-windows <a,b,c>", "--insulation-contact <cutoff>", "--insulation-tol <beads>",
                "window bead IF consensus IF_boundary IF_strength consensus_boundary consensus_strength models"):
        assert opt in out.stderr, opt
    run = subprocess.run([exe, "--tbl", "x.tbl", "--out", "nowhere", "--insulation", "p"], capture_output=True, text=True)
    assert run.returncode == 2 and "--insulation needs --if" in run.stderr


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    kernels = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_insulation.inc")).read()
    for name in LAUNCHERS:
        for text in (internal, stub, kernels):
            assert re.search(r"^hipError_t %s\(" % name, text, re.M), name
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_insulation(") >= 3 and "C3D_ERR_INVALID" in storm[storm.index("c3d_insulation("):]
    make = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "Makefile")).read()
    assert "c3d_score_insulation.inc" in make
