"""The ABI of c3d_entanglement, as far as it can be checked without a GPU: declared with the argument list of the issue under the definitions,
bound with the header's argument list, wrapped and exported; without a context the entry refuses and names itself; the CLI lists its
options; the launchers have their stubs in the fake-HIP harness and the storm calls the entry.  tests/test_gpu_entanglement.py holds the
numbers and the refusals that need replicas."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
CTYPE = {"c3d_ctx*": C.c_void_p, "const double*": C.POINTER(C.c_double), "double*": C.POINTER(C.c_double), "const int32_t*": C.POINTER(C.c_int32), "int": C.c_int}
LAUNCHERS = ("launch_entangle_rows", "launch_entangle_table")


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
    assert re.search(r"^#define\s+C3D_ENTANGLE_MAX_DOMAINS\s+256\s*$", h, re.M)
    ptr = lambda t, name: r"\s*%s\s*\*\s*%s" % (t.replace(" ", r"\s+"), name)
    val = lambda t, name: r"\s*%s\s+%s" % (t, name)
    args = [ptr("c3d_ctx", "ctx"), ptr("const double", "extra_xyz"), val("int", "n_extra"), val("int", "min_sep"), val("int", "max_sep"), ptr("const int32_t", "bounds"),
            val("int", "n_domains"), ptr("double", "writhe"), ptr("double", "acn"), ptr("double", "seg_writhe"), ptr("double", "seg_acn"), ptr("double", "link"),
            ptr("double", "link_abs"), ptr("double", "ms")]
    proto = re.search(r"^int\s+c3d_entanglement\s*\(" + ",".join(args) + r"\s*\)\s*;", h, re.M)
    assert proto
    above = h[:proto.start()]                                                    # the definitions, the refusals and the scratch stand above the prototype
    for phrase in ("K = n_replicas + n_extra", "exactly as c3d_geometry_replicas takes them", "S = n - 1 segments", "the entry needs n >= 4",
                   "a = x[t]   - x[s]        c = x[t+1] - x[s]", "d = x[t]   - x[s+1]      b = x[t+1] - x[s+1]",
                   "T(u,v,w) = 2 atan2( u.(v x w),  |u||v||w| + (u.v)|w| + (u.w)|v| + (v.w)|u| )", "g(s,t)   = ( T(a,b,c) + T(a,d,b) ) / (4 pi)",
                   "Van Oosterom-Strackee", "numerator 0 and denominator 0 contributes 0", "g(s,t) := 0 for", "min_sep <= |s-t| <= max_sep", "2 <= min_sep <= S-1",
                   "max_sep = 0 means S-1", "seg_writhe[k S + s]", "seg_acn[k S + s]", "the writhe of the open chain", "the average crossing number",
                   "link[(k D + p) D + q]", "bounds[0] = 0", "bounds[D] = S", "1 <= D <= C3D_ENTANGLE_MAX_DOMAINS", "the Gauss linking integral",
                   "the domain's own writhe", "symmetric bit for bit", "sum to writhe[k]", "c3d_insulation reports", "No floating-point atomics",
                   "follows from n, min_sep, max_sep and bounds alone", "Two calls on the same state return the same bits", "leave the replicas' entries",
                   "negates seg_writhe, writhe and link exactly", "numerators negate, denominators keep their bits", "n < 4", "every output NULL", "bad bounds",
                   "bounds == NULL with a table asked for", "C3D_ERR_NOMEM", "one allocation per call", "No state of the solve changes"):
        assert phrase in above[above.rindex("/* Entanglement"):], phrase


def test_prototype_matches_the_header_and_the_symbol_is_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    assert "c3d_entanglement" in lib.SIGNATURES and hasattr(L, "c3d_entanglement")
    res, args = lib.SIGNATURES["c3d_entanglement"]
    assert res is C.c_int and args == _declared("c3d_entanglement") and len(args) == 14
    assert lib.ENTANGLE_MAX_DOMAINS == 256
    assert callable(Solver.entanglement) and callable(pipeline.entanglement_report)


def test_without_a_context_it_refuses_and_names_itself(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out, ms = np.full(64, 7.0), C.c_double(7.0)
    bounds = np.array([0, 3, 9], np.int32)
    p = lib.dptr(out)
    rc = L.c3d_entanglement(None, None, 0, 2, 0, lib.i32ptr(bounds), 2, p, p, p, p, p, p, C.byref(ms))
    assert rc == C3D_ERR_INVALID and b"c3d_entanglement" in L.c3d_last_error()
    assert (out == 7.0).all() and ms.value == 7.0


def test_the_cli_lists_the_options(built):
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert out.returncode == 0
    for opt in ("--entanglement <prefix>", "_entanglement.txt", "_segments.txt", "--entangle-sep <a:b>", "--entangle-bounds <FILE>", "_link.txt",
                "rank model writhe acn acn_per_segment", "model segment seg_writhe seg_acn", "model p q link link_abs"):
        assert opt in out.stderr, opt


def test_the_launchers_have_their_stubs_and_the_storm_calls_the_entry():
    stub = open(os.path.join(ROOT, "tools", "sanitize", "hip_stub.cpp")).read()
    internal = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_internal.h")).read()
    kernels = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score_entangle.inc")).read()
    for name in LAUNCHERS:
        for text in (internal, stub, kernels):
            assert re.search(r"^hipError_t %s\(" % name, text, re.M), name
    for kernel in ("k_ent_pairs", "k_ent_model", "k_ent_table"):
        assert re.search(r"void %s\(" % kernel, kernels), kernel
    for helper in ("block_reduce<2>", "dist3(", "atan2("):                       # dist3 is c3d_score_core.h's: its products pass through cmp_rounded
        assert helper in kernels, helper
    code = "\n".join(line.split("//")[0] for line in kernels.splitlines())
    assert "atomic" not in code and "asm" not in code
    analysis = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_analysis.cpp")).read()
    assert "struct EntangleScratch : Carve" in analysis and analysis.count('LAUNCH_TRY("entanglement launch"') == 2
    storm = open(os.path.join(ROOT, "tools", "sanitize", "executor_tsan_main.cpp")).read()
    assert storm.count("c3d_entanglement(") >= 3 and "C3D_ERR_INVALID" in storm[storm.index("c3d_entanglement("):]
    make = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "Makefile")).read()
    assert "c3d_score_entangle.inc" in make
    score = open(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_score.hip")).read()
    assert score.count('#include "c3d_score_entangle.inc"') == 1


def test_the_stub_twins_compute_the_definitions(built):
    """The fake-HIP twins are the definitions in plain loops: the storm's program links them, and here the same source is held to the
    restatement through the stand-alone harness of tests/util.link_fake_hip — no device, nothing loaded into Python."""
    import tempfile
    from tests import entangle_ref as E
    from tests.util import link_fake_hip, random_coil
    tmp = tempfile.mkdtemp(prefix="c3d_entangle_stub_")
    main = os.path.join(tmp, "main.cpp")
    x = random_coil(40, 3).astype(np.float64)
    with open(main, "w") as f:
        f.write('#include <cstdio>\n#include <vector>\n#include "c3d_internal.h"\nint main() {\n  const int n = 40, S = 39; std::vector<double> x(3 * n), sw(S), sa(S), w(1), a(1), l(9), la(9);\n'
                '  for (double& v : x) if (scanf("%lf", &v) != 1) return 2;\n  const int b[4] = {0, 10, 11, 39};\n'
                '  c3d::launch_entangle_rows(x.data(), n, 1, 2, S - 1, sw.data(), sa.data(), w.data(), a.data(), nullptr);\n'
                '  c3d::launch_entangle_table(x.data(), n, 1, 2, S - 1, b, 3, l.data(), la.data(), nullptr);\n'
                '  printf("%.17g %.17g\\n", w[0], a[0]); for (int s = 0; s < S; ++s) printf("%.17g %.17g\\n", sw[s], sa[s]);\n'
                '  for (int q = 0; q < 9; ++q) printf("%.17g %.17g\\n", l[q], la[q]);\n  return 0;\n}\n')
    try:
        exe = link_fake_hip(tmp, [(main, "main.o", ["-I" + os.path.join(ROOT, "chromosome3d_amd", "csrc"), "-I" + os.path.join(ROOT, "include")])], "entangle_stub")
        assert exe is not None, "no host C++ compiler"
        run = subprocess.run([exe], input=" ".join("%.17g" % v for v in x.reshape(-1)), capture_output=True, text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    assert run.returncode == 0, run.stderr
    got = np.array([[float(v) for v in line.split()] for line in run.stdout.splitlines()])
    r = E.entanglement(x, bounds=[0, 10, 11, 39])
    U = 2.0 ** -53
    assert abs(got[0, 0] - r["writhe"]) <= 8 * U * r["kappa"] and abs(got[0, 1] - r["acn"]) <= 8 * U * r["kappa"]
    assert (np.abs(got[1:40, 0] - r["seg_writhe"]) <= 8 * U * r["seg_kappa"]).all() and (np.abs(got[1:40, 1] - r["seg_acn"]) <= 8 * U * r["seg_kappa"]).all()
    assert (np.abs(got[40:, 0].reshape(3, 3) - r["link"]) <= 8 * U * r["link_kappa"] + U).all() and np.array_equal(got[40:, 0].reshape(3, 3), got[40:, 0].reshape(3, 3).T)
