"""The ABI of c3d_loops, as far as it can be checked without a GPU: declared with the argument list of the issue under the definitions,
bound with the header's argument list, wrapped and exported; without a context the entry refuses and names itself; the CLI lists its
options; the launchers have their stubs in the fake-HIP harness and the storm calls the entry.  tests/test_gpu_loops.py holds the
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
LAUNCHERS = ("launch_loop_expected", "launch_loop_scan", "launch_loop_peaks", "launch_loop_list", "launch_loop_apa")


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
    assert re.search(r"^#define\s+C3D_LOOP_MAX_WINDOW\s+20\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_LOOP_MAX_BAND\s+1024\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_LOOP_MAX_LIST\s+65536\s*$", h, re.M)
    assert re.search(r"^#define\s+C3D_LOOP_CONSENSUS\s+1\b", h, re.M)
    assert re.search(r"^#define\s+C3D_LOOP_REPORT\s+4\s*$", h, re.M)
    ptr = lambda t, name: r"\s*%s\s*\*\s*%s" % (t.replace(" ", r"\s+"), name)
    val = lambda t, name: r"\s*%s\s+%s" % (t, name)
    args = [ptr("c3d_ctx", "ctx"), ptr("const double", "IF"), ptr("const double", "extra_xyz"), val("int", "n_extra"), ptr("const int32_t", "pick"), val("int", "n_pick"),
            val("int", "flags"), ptr("const int32_t", "mask"), val("int", "p"), val("int", "w"), val("int", "min_sep"), val("int", "max_sep"), ptr("const double", "thr"),
            val("double", "min_obs"), val("int", "merge"), val("int", "corner"), ptr("const int32_t", "list_in"), val("int", "n_list"), val("int", "max_peaks"),
            ptr("double", "expected"), ptr("double", "ratio"), ptr("int32_t", "peaks"), ptr("int32_t", "report"), ptr("double", "at"), ptr("int32_t", "closed"),
            ptr("double", "apa"), ptr("double", "p2ll"), ptr("double", "device_ms")]
    proto = re.search(r"^int\s+c3d_loops\s*\(" + ",".join(args) + r"\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definitions, the refusals and the scratch stand above the prototype
    for phrase in ("divided once by Kp", "sqrt(((ux ux) + uy uy) + uz uz)", "live when neither a nor b is masked", "0 <= p < w <= C3D_LOOP_MAX_WINDOW",
                   "min_sep >= 2w + 1", "s_lo = min_sep - 2w", "s_hi = min(max_sep + 2w, n - 1)", "inside when i >= w", "j + w <= n - 1",
                   "donut: not P, a != 0, b != 0", "lower-left: not P, a >= 1, b <= -1", "horizontal: |a| <= 1, |b| > p", "vertical: |b| <= 1, |a| > p",
                   "row-major order: a ascending, then b ascending", "r_x = M(i,j) / ((SM_x / SE_x) * E[s])", "three roundings in that order",
                   "[x][s - min_sep][i]", "NaN wherever i + s > n - 1", "r_x >= thr[x]", "M(i,j) >= min_obs", "Chebyshev distance `merge`",
                   "lexicographically smaller (i, j)", "ascending (i, j) order", "min(found, max_peaks)", "{M(i,j), E[s], r_donut, r_ll, r_h, r_v}",
                   "same bytes as `ratio`", "> 1 for IF, < 1 for models and the consensus", "thread t takes the pixels t, t + 256, ...",
                   "a in [w - corner + 1, w]", "b in [-w, -w + corner - 1]", "No atomics on floating-point data", "no floating-point prefix sums",
                   "two calls return the same bytes", "alone or among others", "an integer scan", "C3D_ERR_NOMEM", "8 n S per band", "at 455 beads x 20 models",
                   "at 16384 x 20"):
        assert phrase in above, phrase


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_loops" in lib.SIGNATURES and hasattr(L, "c3d_loops")
    res, args = lib.SIGNATURES["c3d_loops"]
    assert res is C.c_int and args == _declared("c3d_loops") and len(args) == 28
    assert (lib.LOOP_MAX_WINDOW, lib.LOOP_MAX_BAND, lib.LOOP_MAX_LIST, lib.LOOP_CONSENSUS, lib.LOOP_REPORT) == (20, 1024, 65536, 1, 4)
    assert callable(Solver.loops) and callable(pipeline.loop_report)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, marks, ms = np.full(64, 7.0), np.full(64, 7, np.int32), C.c_double(7.0)
    thr = np.array([1.75, 1.75, 1.5, 1.5])
    p, ip = lib.dptr(out), lib.i32ptr(marks)
    rc = L.c3d_loops(None, None, None, 0, None, 0, 0, None, 2, 5, 11, 20, lib.dptr(thr), 0.0, 2, 3, None, 0, 4, p, p, ip, ip, p, ip, p, p, C.byref(ms))
    assert rc == C3D_ERR_INVALID and b"c3d_loops" in L.c3d_last_error()
    assert (out == 7.0).all() and (marks == 7).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--loops <prefix>", "_loops.txt", "--loop-window <w>", "--loop-peak <p>", "--loop-sep <MIN:MAX>", "--loop-thr <a,b,c,d>", "--loop-list <FILE>",
                "1.75,1.75,1.5,1.5", "i j IF r_donut r_ll r_h r_v consensus_d consensus_r_donut consensus_r_ll models_closed"):
        assert opt in out.stderr, opt
    run = subprocess.run([exe, "--tbl", "x.tbl", "--out", "nowhere", "--loops", "p"], capture_output=True, text=True)
    assert run.returncode == 2 and "--loops needs --if" in run.stderr


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    kernels = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_loop.inc")).read()
    assert len(LAUNCHERS) >= 4 and "struct LoopJob" in internal
    for name in LAUNCHERS:
        for text in (internal, stub, kernels):
            assert re.search(r"^hipError_t %s\(" % name, text, re.M), name
    for kernel in ("k_loop_band", "k_loop_expected", "k_loop_scan", "k_loop_list", "k_loop_apa"):
        assert re.search(r"void %s\(" % kernel, kernels), kernel
    for helper in ("block_reduce<2>", "cmp_dist(", "cpt_mean_dist("):
        assert helper in kernels, helper
    assert "atomic" not in kernels.replace("no atomics", "").replace("no\n// atomics", "")
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_loops(") >= 3 and "C3D_ERR_INVALID" in storm[storm.index("c3d_loops("):]
    make = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "Makefile")).read()
    assert "c3d_score_loop.inc" in make
    score = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score.hip")).read()
    assert score.count('#include "c3d_score_loop.inc"') == 1
