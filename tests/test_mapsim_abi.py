"""The ABI of c3d_map_similarity, as far as it can be checked without a GPU: declared with the argument list of the issue under the
definitions, bound with the header's argument list, wrapped and exported; without a context the entry refuses and names itself; the CLI
lists its options; the launchers have their twins in the fake-HIP harness and the storm calls the entry; pipeline.choose_smoothing on
hand-made tables; and the host side of the entry, linked against the fake device, against the restatement.
tests/test_gpu_mapsim.py holds the numbers and the refusals that need a device."""
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
         "int64_t*": C.POINTER(C.c_int64), "int": C.c_int, "double": C.c_double}
LAUNCHERS = ("launch_mapsim_smooth", "launch_mapsim_strata")


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
    for name, value in (("C3D_MAPSIM_KEEP_ZEROS", 1), ("C3D_MAPSIM_MAX_MAPS", 16), ("C3D_MAPSIM_MAX_H", 20), ("C3D_MAPSIM_MAX_WIDTHS", 8)):
        assert re.search(r"^#define\s+%s\s+%d\b" % (name, value), h, re.M), name
    proto = re.search(r"^int\s+c3d_map_similarity\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*maps,\s*int\s+n_maps,\s*int\s+n,\s*const\s+int32_t\s*\*\s*h,\s*int\s+n_h,"
                      r"\s*int\s+min_sep,\s*int\s+max_sep,\s*int\s+flags,\s*double\s*\*\s*scc,\s*double\s*\*\s*rho,\s*double\s*\*\s*moments,\s*int64_t\s*\*\s*counts,"
                      r"\s*double\s*\*\s*smoothed,\s*double\s*\*\s*device_ms\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definitions, the refusals and the scratch stand above the prototype
    above = above[above.rindex("/* Reproducibility of contact maps"):]
    for phrase in ("2 <= n_maps <= C3D_MAPSIM_MAX_MAPS", "3 <= n <= the max_beads in force", "M(i,j) == M(j,i) exactly", "with the map's index in the message",
                   "before any other kernel", "strictly ascending", "0 <= min_sep <= max_sep <= n - 1", "max_sep == 0 means n - 1",
                   "r in [max(0,i-h), min(n-1,i+h)]", "c in [max(0,j-h), min(n-1,j+h)]", "in ascending c, starting from the first", "(double)(rows x cols)",
                   "one IEEE division", "h = 0 is the map itself", "Pair i is kept unless x_i == 0 and y_i == 0", "C3D_MAPSIM_KEEP_ZEROS all pairs are kept",
                   "mx = (sum x) / N", "Cxy = sum (x - mx)(y - my)", "block_reduce", "i = t + 256k in ascending k", "an unkept pair brings 0",
                   "#{smaller} + #{not larger} + 1", "-0.0 ranks as 0.0", "A = N sum a^2 - T^2", "T = N(N+1)", "exact in int64", "neither sort keeps an index",
                   "take the pad", "rho_s = Cxy / sqrt(Cxx * Cyy)", "w_s = sqrt((double)A * (double)B) / (4 N^3)", "HiCRep's weights",
                   "N >= 3, A > 0, B > 0, Cxx > 0 and Cyy > 0", "rho_s is NaN and w_s is 0", "scc(p,q) = (sum w_s rho_s) / (sum w_s)",
                   "sequential over ascending counted s", "scc(p,p) = 1.0, written by the host", "(0,1), (0,2), ..., (1,2), ...", "[n_h][n_maps][n_maps]",
                   "[n_h][P][S][3]", "[n_h][n_maps][S][n]", "then zeros", "There are no atomics", "Two calls return the same bytes",
                   "permutes the outputs and changes no bit", "unknown flag bits", "C3D_ERR_NOMEM", "8 n_maps n^2 bytes", "8 n_maps S n bytes",
                   "diagonal-major", "no second n x n", "changes no state", "no stat key and no option key",
                   "Out of scope: HiCRep's depth down-sampling, its variance estimate, and sparse input"):
        assert phrase in above, phrase


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_map_similarity" in lib.SIGNATURES and hasattr(L, "c3d_map_similarity")
    res, args = lib.SIGNATURES["c3d_map_similarity"]
    assert res is C.c_int and args == _declared("c3d_map_similarity")
    assert (lib.MAPSIM_KEEP_ZEROS, lib.MAPSIM_MAX_MAPS, lib.MAPSIM_MAX_H, lib.MAPSIM_MAX_WIDTHS) == (1, 16, 20, 8)
    assert callable(Solver.map_similarity) and callable(pipeline.map_similarity_report) and callable(pipeline.choose_smoothing)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    n = 4
    maps = np.ones((2, n, n))
    out, cnt, ms = np.full(64, 7.0), np.full(64, 7, np.int64), C.c_double(7.0)
    h = np.zeros(1, np.int32)
    p = lib.dptr(out)
    rc = L.c3d_map_similarity(None, lib.dptr(maps), 2, n, lib.i32ptr(h), 1, 0, 0, 0, p, p, p, cnt.ctypes.data_as(C.POINTER(C.c_int64)), p, C.byref(ms))
    assert rc == C3D_ERR_INVALID and b"c3d_map_similarity" in L.c3d_last_error()
    assert (out == 7.0).all() and (cnt == 7).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--map-similarity <file>", "--map-similarity-h <list>", "--map-similarity-sep <lo>:<hi>", "--map-similarity-out <prefix>", "_scc.txt", "_strata.txt",
                "before any --balance"):
        assert opt in out.stderr, opt
    run = subprocess.run([exe, "--tbl", "x.tbl", "--out", "nowhere", "--map-similarity", "other.txt"], capture_output=True, text=True)
    assert run.returncode == 2 and "--map-similarity needs --if" in run.stderr
    assert not os.path.exists("nowhere")


def test_the_launchers_have_their_twins_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    kernels = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_mapsim.inc")).read()
    for name in LAUNCHERS:
        for text in (internal, stub, kernels):
            assert re.search(r"^hipError_t %s\(" % name, text, re.M), name
    for kernel in ("k_sim_smooth", "k_sim_stratum"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kernels), kernel
    code = kernels.split("constexpr int kSimTile")[1]
    assert "atomic" not in code                                                        # (the comment above the kernels says "No atomics")
    for shared in ("str_sort(", "rank_key(", "str_launch_classes(", "block_reduce("):
        assert shared in code, shared
    assert "hipFuncSetAttribute" not in code                                           # the allowance is set where str_prepare_unit sets the others
    strat = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_stratified.inc")).read()
    assert "k_sim_stratum" in strat[strat.index("static hipError_t str_prepare_unit"):]
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_map_similarity(") >= 3 and "C3D_ERR_INVALID" in storm[storm.index("c3d_map_similarity("):]
    make = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "Makefile")).read()
    assert "c3d_score_mapsim.inc" in make
    assert '#include "c3d_score_mapsim.inc"' in open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score.hip")).read()


def test_choose_smoothing_on_hand_made_tables():
    from chromosome3d_amd.pipeline import choose_smoothing
    assert choose_smoothing({0: 0.50, 1: 0.60, 2: 0.65, 3: 0.655, 4: 0.70}) == 2          # 3 gains 0.005 over 2: the first step below the gain
    assert choose_smoothing([(2, 0.65), (0, 0.50), (1, 0.60)]) == 2                       # every step gains: the largest listed; pairs in any order
    assert choose_smoothing({0: 0.9, 5: 0.905}) == 0
    assert choose_smoothing({0: 0.9, 5: 0.905}, gain=0.001) == 5
    assert choose_smoothing({3: 0.7}) == 3
    assert choose_smoothing({0: 0.8, 1: 0.7, 2: 0.9}) == 0                                # a loss is less than the gain


def test_the_host_side_against_the_fake_device_agrees_with_the_restatement():
    """c3d_analysis.cpp's entry linked against the fake-HIP layer, whose launchers are plain loops over the definitions: the argument checks,
    the check per map, the loop over the half-widths, rho, w and scc on the host and every output's layout, on the CPU."""
    from tests.util import link_fake_hip
    tmp = tempfile.mkdtemp(prefix="c3d_mapsim_abi_")
    src = os.path.join(tmp, "main.cpp")
    with open(src, "w") as f:
        f.write(r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "%s/include/c3d.h"
int main(int argc, char** argv) {
    const int n = atoi(argv[1]), Q = 3, H = 2, lo = atoi(argv[2]), hi = atoi(argv[3]), flags = atoi(argv[4]);
    const int S = (hi ? hi : n - 1) - lo + 1, P = 3;
    std::vector<double> maps((size_t)Q * n * n), scc(H * Q * Q, -7.0), rho((size_t)H * P * S, -7.0), mom((size_t)H * P * S * 3, -7.0), sm((size_t)H * Q * S * n, -7.0);
    std::vector<int64_t> cnt((size_t)H * P * S * 3, -7);
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(maps.data(), 8, maps.size(), f) != maps.size()) return 3;
    fclose(f);
    const int32_t h[2] = {0, 2}, hbad[2] = {2, 1};
    c3d_ctx* c = nullptr;
    if (c3d_create(0, &c) != C3D_OK) return 4;
    double ms = -7.0;
    if (c3d_map_similarity(c, maps.data(), Q, n, hbad, H, lo, hi, flags, scc.data(), nullptr, nullptr, nullptr, nullptr, &ms) != C3D_ERR_INVALID || scc[0] != -7.0 || ms != -7.0) return 6;
    if (c3d_map_similarity(c, maps.data(), Q, n, h, H, lo, hi, 2, scc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != C3D_ERR_INVALID) return 7;
    if (c3d_map_similarity(c, maps.data(), Q, n, h, H, lo, n, flags, scc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != C3D_ERR_INVALID) return 8;
    if (c3d_map_similarity(c, maps.data(), 1, n, h, H, lo, hi, flags, scc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != C3D_ERR_INVALID) return 9;
    maps[(size_t)n * n + 1] += 1.0;                 // map 1 loses its symmetry
    if (c3d_map_similarity(c, maps.data(), Q, n, h, H, lo, hi, flags, scc.data(), nullptr, nullptr, nullptr, nullptr, nullptr) != C3D_ERR_INVALID || !strstr(c3d_last_error(), "map 1") ||
        scc[0] != -7.0) return 10;
    maps[(size_t)n * n + 1] -= 1.0;
    const int rc = c3d_map_similarity(c, maps.data(), Q, n, h, H, lo, hi, flags, scc.data(), rho.data(), mom.data(), cnt.data(), sm.data(), &ms);
    if (rc != C3D_OK) { fprintf(stderr, "%%s\n", c3d_last_error()); return 5; }
    f = fopen(argv[6], "wb");
    fwrite(scc.data(), 8, scc.size(), f); fwrite(rho.data(), 8, rho.size(), f); fwrite(mom.data(), 8, mom.size(), f); fwrite(cnt.data(), 8, cnt.size(), f);
    fwrite(sm.data(), 8, sm.size(), f);
    fclose(f);
    c3d_destroy(c);
    return 0;
}
''' % ROOT)
    try:
        exe = link_fake_hip(tmp, [(src, "main.o", [])], "mapsim_host")
        if exe is None:
            import pytest
            pytest.skip("no host C++ compiler")
        _host_runs(exe, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _host_runs(exe, tmp):
    from tests import mapsim_ref as R
    rng = np.random.default_rng(13)
    n, Q, H, P = 21, 3, 2, 3
    maps = []
    for m in range(Q):
        A = np.triu(rng.poisson(1.2, (n, n)).astype(float))
        maps.append(A + np.triu(A, 1).T)
    maps = np.stack(maps)
    maps[:, 4, :] = maps[:, :, 4] = 0.0                                              # an empty bin in every map: the both-zero rule bites at h = 0
    maps.tofile(os.path.join(tmp, "m.bin"))
    for lo, hi, flags in ((0, 0, 0), (1, 9, 0), (1, 9, 1)):
        top = hi if hi else n - 1
        S = top - lo + 1
        res = os.path.join(tmp, "out.bin")
        run = subprocess.run([exe, str(n), str(lo), str(hi), str(flags), os.path.join(tmp, "m.bin"), res], capture_output=True, text=True)
        assert run.returncode == 0, (run.returncode, run.stderr)
        raw = open(res, "rb").read()
        sizes = [H * Q * Q, H * P * S, H * P * S * 3, H * P * S * 3, H * Q * S * n]
        offs = np.concatenate([[0], np.cumsum(sizes)]) * 8
        scc = np.frombuffer(raw, np.float64, sizes[0], offs[0]).reshape(H, Q, Q)
        rho = np.frombuffer(raw, np.float64, sizes[1], offs[1]).reshape(H, P, S)
        mom = np.frombuffer(raw, np.float64, sizes[2], offs[2]).reshape(H, P, S, 3)
        cnt = np.frombuffer(raw, np.int64, sizes[3], offs[3]).reshape(H, P, S, 3)
        sm = np.frombuffer(raw, np.float64, sizes[4], offs[4]).reshape(H, Q, S, n)
        want = R.map_similarity(maps, h=(0, 2), min_sep=lo, max_sep=hi, keep_zeros=bool(flags))
        assert sm.tobytes() == want["smoothed"].tobytes()
        assert (cnt == want["counts"].astype(np.int64)).all()
        assert np.allclose(mom, want["moments"], rtol=1e-12, atol=1e-12)
        if not flags:
            assert (cnt[0, :, :, 0] < n - np.arange(lo, top + 1)[None, :]).any()          # some pair was dropped
        for k in range(H):
            for e, (p, q) in enumerate(R.pairs(Q)):
                r, w, s = R.combine(mom[k, e], cnt[k, e])
                assert rho[k, e].tobytes() == r.tobytes()                               # bit for bit from the returned moments and counts
                assert scc[k, p, q] == s == scc[k, q, p] or (np.isnan(s) and np.isnan(scc[k, p, q]) and np.isnan(scc[k, q, p]))
            assert (np.diagonal(scc[k]) == 1.0).all()
        assert np.allclose(scc, want["scc"], rtol=1e-10, atol=1e-12, equal_nan=True)
