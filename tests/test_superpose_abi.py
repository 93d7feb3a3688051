"""The ABI of the on-device superposition (c3d_superpose_replicas, c3d_rmsd_table), as far as it can be checked without a GPU: declared
with both flags, bound, wrapped and exported; without a context they refuse and name themselves; the CLI lists its options; the fake-HIP
harness of tools/sanitize still links against the launchers.  tests/test_gpu_superpose.py holds the numbers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1


def test_header_declares_both_entries_and_both_flags(built):
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert re.search(r"^int\s+c3d_superpose_replicas\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*int\s+reference,\s*const\s+double\s*\*\s*ref_xyz,\s*int\s+flags,\s*int\s+iters,"
                     r"\s*double\s*\*\s*rmsd,\s*int32_t\s*\*\s*mirrored,\s*double\s*\*\s*mean_xyz,\s*double\s*\*\s*rmsf\s*\)\s*;", h, re.M)
    assert re.search(r"^int\s+c3d_rmsd_table\s*\(\s*c3d_ctx\s*\*\s*ctx,\s*const\s+double\s*\*\s*extra_xyz,\s*int\s+n_extra,\s*int\s+flags,\s*double\s*\*\s*rmsd,"
                     r"\s*int32_t\s*\*\s*mirrored\s*\)\s*;", h, re.M)
    assert re.search(r"^#define\s+C3D_SUPERPOSE_MIRROR\s+1\b", h, re.M) and re.search(r"^#define\s+C3D_SUPERPOSE_APPLY\s+2\b", h, re.M)
    assert re.search(r"^#define\s+C3D_SUPERPOSE_MAX_ITERS\s+50\s*$", h, re.M)


def test_both_entries_are_bound_wrapped_and_exported(built):
    from chromosome3d_amd import lib, pipeline
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    for name in ("c3d_superpose_replicas", "c3d_rmsd_table"):
        assert name in lib.SIGNATURES and hasattr(L, name)
    assert (lib.SUPERPOSE_MIRROR, lib.SUPERPOSE_APPLY) == (1, 2)
    assert callable(Solver.superpose) and callable(Solver.rmsd_table)
    assert callable(pipeline.superpose_models) and callable(pipeline.rmsd_table)


def test_without_a_context_both_refuse_and_name_themselves(built):
    from chromosome3d_amd import lib
    L = lib.load()
    out = np.zeros(9)
    assert L.c3d_superpose_replicas(None, 0, None, 1, 0, lib.dptr(out), None, None, None) == C3D_ERR_INVALID
    assert b"c3d_superpose_replicas" in L.c3d_last_error()
    assert L.c3d_rmsd_table(None, None, 0, 1, lib.dptr(out), None) == C3D_ERR_INVALID
    assert b"c3d_rmsd_table" in L.c3d_last_error()
    v = C.c_double()
    for key in (b"superpose_runs", b"rmsd_table_runs"):
        assert L.c3d_get_stat(None, key, C.byref(v)) == C3D_ERR_INVALID


def test_the_cli_lists_the_options(built):
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--superpose" in out.stderr and "--rmsf" in out.stderr


def test_the_fake_hip_harness_still_links(built, tmp_path):
    """tools/sanitize/hip_stub.cpp stands in for every launcher the host units call: the context code and the stub link into one program
    (no sanitizer here: tools/sanitize/run.sh builds the same objects with them)."""
    from tests.util import link_fake_hip
    san = os.path.join(ROOT, "tools", "sanitize")
    exe = link_fake_hip(str(tmp_path), [(os.path.join(ROOT, "chromosome3d_amd", "csrc", "c3d_batch_main.cpp"), "batch.o", ["-Dmain=c3d_batch_main"]),
                                        (os.path.join(san, "executor_tsan_main.cpp"), "main.o", [])], "executor")
    if exe is None:
        pytest.skip("no host C++ compiler")
    assert os.path.exists(exe)
