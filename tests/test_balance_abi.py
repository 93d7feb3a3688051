"""The ABI of c3d_balance_matrix, as far as it can be checked without a GPU: declared with the argument list of the issue under the
definitions, bound with the header's argument list, wrapped and exported; without a context the entry refuses and names itself; the CLI
lists its options; the launchers have their stubs in the fake-HIP harness and the storm calls the entry.  tests/test_gpu_balance.py holds
the numbers and the refusals that need a device."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32),
         "int32_t*": C.POINTER(C.c_int32), "int": C.c_int, "double": C.c_double}
LAUNCHERS = ("launch_balance_count", "launch_balance_round", "launch_balance_apply")


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
    for name, value in (("C3D_BALANCE_ICE", 0), ("C3D_BALANCE_VC", 1), ("C3D_BALANCE_SQRT_VC", 2), ("C3D_BALANCE_CHECK_EVERY_ROUND", 1),
                        ("C3D_BALANCE_MAX_ITERS", 10000), ("C3D_BALANCE_REPORT", 8)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, value), h, re.M), name
    proto = re.search(r"^int\s+c3d_balance_matrix\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*M,\s*int\s+n,\s*int\s+method,\s*int\s+flags,\s*int\s+ignore_diags,"
                      r"\s*int\s+min_nnz,\s*const\s+int32_t\s*\*\s*mask_in,\s*const\s+double\s*\*\s*w0,\s*double\s+tol,\s*int\s+max_iters,\s*double\s+target,"
                      r"\s*double\s*\*\s*weights,\s*int32_t\s*\*\s*masked,\s*double\s*\*\s*balanced,\s*double\s*\*\s*history,\s*double\s*\*\s*report,"
                      r"\s*double\s*\*\s*device_ms\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definitions, the refusals and the scratch stand above the prototype
    above = above[above.rindex("/* Balancing a raw contact matrix"):]
    for phrase in ("A'(i,j) = M(i,j) if |i-j| >= ignore_diags, else 0", "nnz_i = #{ j : A'(i,j) > 0 }", "nnz_i >= max(min_nnz, 1)",
                   "O = { i in U : A'(i,j) == 0 for every j in U }", "until O is empty", "1 for one listed in mask_in, 2 for too few non-zeros, 3 for one removed by the closure",
                   "|U| < 2", "w_i = 0 off U", "s_i = w_i * sum_j A'(i,j) w_j", "mbar = (sum_{i in U} s_i) / |U|", "r_i = s_i / mbar",
                   "var_t = sum_{i in U} (r_i - 1)^2 / |U|", "history[t] = var_t", "if var_t < tol: stop converged with T = t",
                   "else if t == max_iters: stop unconverged with T = max_iters", "w_i <- w_i / r_i^p", "w_i / sqrt(r_i)", "max_iters + 1 marginal passes",
                   "max_iters = 0 only evaluates w0", "max_iters forced to 1 and tol forced to 0", "refuse w0 != NULL", "C3D_ERR_DIVERGED",
                   "w_i <- w_i * sqrt(target / mbar)", "fl(fl(w_i * w_j) * M(i,j))", "symmetric bit for bit", "(w[:,None] * w[None,:]) * M", "never a fused form",
                   "entries beyond T are not written", "{ T, converged (1 / 0), var_T, |U|, #masked by 1, #masked by 2, #masked by 3, mbar of the last pass before scaling }",
                   "no atomics", "the mean first, then the centred sum", "Two calls return the same bytes", "the stop word", "batches of 16",
                   "C3D_BALANCE_CHECK_EVERY_ROUND", "changes no state of the solve", "C3D_ERR_NOMEM", "8 n np bytes", "np = n rounded up to even",
                   "formed in place over that copy", "at 455", "at 16384 beads"):
        assert phrase in above, phrase


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_balance_matrix" in lib.SIGNATURES and hasattr(L, "c3d_balance_matrix")
    res, args = lib.SIGNATURES["c3d_balance_matrix"]
    assert res is C.c_int and args == _declared("c3d_balance_matrix")
    assert (lib.BALANCE_ICE, lib.BALANCE_VC, lib.BALANCE_SQRT_VC, lib.BALANCE_CHECK_EVERY_ROUND, lib.BALANCE_MAX_ITERS, lib.BALANCE_REPORT) == (0, 1, 2, 1, 10000, 8)
    assert callable(Solver.balance) and callable(pipeline.balance_if)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    n = 4
    M = np.ones((n, n))
    out, big, codes, ms = np.full(16, 7.0), np.full((n, n), 7.0), np.full(n, 7, np.int32), C.c_double(7.0)
    p = lib.dptr(out)
    rc = L.c3d_balance_matrix(None, lib.dptr(M), n, 0, 0, 0, 1, None, None, 1e-5, 10, 1.0, p, lib.i32ptr(codes), lib.dptr(big), p, p, C.byref(ms))
    assert rc == C3D_ERR_INVALID and b"c3d_balance_matrix" in L.c3d_last_error()
    assert (out == 7.0).all() and (big == 7.0).all() and (codes == 7).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--balance <ice|vc|sqrt-vc>", "--balance-ignore-diags <k>", "--balance-min-nnz <m>", "--balance-tol <v>", "--balance-iters <k>",
                "--balance-out <prefix>", "_weights.txt", "bead weight masked", "_matrix.txt"):
        assert opt in out.stderr, opt
    run = subprocess.run([exe, "--tbl", "x.tbl", "--out", "nowhere", "--balance", "ice"], capture_output=True, text=True)
    assert run.returncode == 2 and "--balance needs --if" in run.stderr
    assert not os.path.exists("nowhere")


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    kernels = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_balance.inc")).read()
    for name in LAUNCHERS:
        for text in (internal, stub, kernels):
            assert re.search(r"^hipError_t %s\(" % name, text, re.M), name
    for kernel in ("k_bal_count", "k_bal_marginals", "k_bal_update", "k_bal_apply"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kernels), kernel
    assert "atomic" not in kernels.split("constexpr int kBalRows")[1]                 # (the comment above the kernels says "No atomics")
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_balance_matrix(") >= 3 and "C3D_ERR_INVALID" in storm[storm.index("c3d_balance_matrix("):]
    make = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "Makefile")).read()
    assert "c3d_score_balance.inc" in make
    assert '#include "c3d_score_balance.inc"' in open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score.hip")).read()


def test_the_host_side_against_the_fake_device_agrees_with_the_restatement():
    """c3d_analysis.cpp's entry linked against the fake-HIP layer, whose launchers are plain loops over the definitions: the mask with its
    closure, the batches, the padded pitch of an odd n and every output, on the CPU."""
    from tests.util import link_fake_hip
    tmp = tempfile.mkdtemp(prefix="c3d_balance_abi_")
    src = os.path.join(tmp, "main.cpp")
    with open(src, "w") as f:
        f.write(r'''
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "%s/include/c3d.h"
int main(int argc, char** argv) {
    const int n = atoi(argv[1]), flags = atoi(argv[2]);
    std::vector<double> M((size_t)n * n), w(n), bal((size_t)n * n), hist(41, -1.0), rep(C3D_BALANCE_REPORT);
    std::vector<int32_t> mask(n, 0), code(n);
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(M.data(), 8, M.size(), f) != M.size()) return 3;
    fclose(f);
    mask[2] = 1;
    c3d_ctx* c = nullptr;
    if (c3d_create(0, &c) != C3D_OK) return 4;
    const int rc = c3d_balance_matrix(c, M.data(), n, C3D_BALANCE_ICE, flags, 2, 3, mask.data(), nullptr, 1e-9, 40, 2.0, w.data(), code.data(), bal.data(), hist.data(),
                                      rep.data(), nullptr);
    if (rc != C3D_OK) { fprintf(stderr, "%%s\n", c3d_last_error()); return 5; }
    f = fopen(argv[4], "wb");
    fwrite(w.data(), 8, n, f); fwrite(code.data(), 4, n, f); fwrite(bal.data(), 8, bal.size(), f); fwrite(hist.data(), 8, 41, f); fwrite(rep.data(), 8, rep.size(), f);
    fclose(f);
    c3d_destroy(c);
    return 0;
}
''' % ROOT)
    try:
        exe = link_fake_hip(tmp, [(src, "main.o", [])], "balance_host")
        if exe is None:
            import pytest
            pytest.skip("no host C++ compiler")
        _host_runs(exe, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _host_runs(exe, tmp):
    from tests import balance_ref as R
    rng = np.random.default_rng(11)
    outs = {}
    for n in (24, 25):
        A = rng.poisson(1.5, (n, n)).astype(float)
        A = A + A.T
        A[5, :] = A[:, 5] = 0.0
        A[7, :] = A[:, 7] = 0.0
        A[7, 2] = A[2, 7] = 3.0                                                    # bin 7's only partner is the listed bin 2: the closure takes it
        A.tofile(os.path.join(tmp, "m.bin"))
        want = R.balance(A, "ice", ignore_diags=2, min_nnz=3, mask=(np.arange(n) == 2).astype(int), tol=1e-9, max_iters=40, target=2.0)
        assert want["masked"][7] in (2, 3) and want["masked"][5] == 2
        for flags in (0, 1):
            res = os.path.join(tmp, "out_%d_%d.bin" % (n, flags))
            run = subprocess.run([exe, str(n), str(flags), os.path.join(tmp, "m.bin"), res], capture_output=True, text=True)
            assert run.returncode == 0, run.stderr
            raw = open(res, "rb").read()
            w = np.frombuffer(raw, np.float64, n, 0)
            code = np.frombuffer(raw, np.int32, n, 8 * n)
            bal = np.frombuffer(raw, np.float64, n * n, 12 * n).reshape(n, n)
            hist = np.frombuffer(raw, np.float64, 41, 12 * n + 8 * n * n)
            rep = np.frombuffer(raw, np.float64, 8, 12 * n + 8 * n * n + 8 * 41)
            T = int(rep[0])
            assert np.array_equal(code, want["masked"]) and T == want["rounds"] and rep[1] == 1.0 and int(rep[3]) == want["kept"]
            assert [int(x) for x in rep[4:7]] == want["masked_counts"]
            assert np.allclose(w, want["weights"], rtol=1e-12, atol=0) and np.allclose(hist[:T + 1], want["history"], rtol=1e-9, atol=1e-24)
            assert (hist[T + 1:] == -1.0).all()                                    # untouched beyond T
            assert np.array_equal(bal, (w[:, None] * w[None, :]) * A) and np.array_equal(bal, bal.T)
            outs[(n, flags)] = raw
        assert outs[(n, 0)] == outs[(n, 1)]
