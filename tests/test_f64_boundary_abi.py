"""The ABI of a precision-64 context's boundary in doubles (c3d_get_coords_f64, c3d_get_velocities_f64, c3d_set_coords_f64, c3d_eval_f64), as
far as it can be checked without a GPU: declared in c3d.h, exported, bound with prototypes that match the header, wrapped by Solver; without
a context they return C3D_ERR_INVALID and name themselves.  tests/test_gpu_f64_boundary.py holds the numbers."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3D_ERR_INVALID = -1
ENTRIES = ("c3d_get_coords_f64", "c3d_get_velocities_f64", "c3d_set_coords_f64", "c3d_eval_f64")
CTYPES = {"c3d_ctx*": C.c_void_p, "double*": C.POINTER(C.c_double), "const double*": C.POINTER(C.c_double), "double": C.c_double}


def _declaration(h, name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^)]*)\)\s*;", h, re.M)
    assert m, name
    args = []
    for a in m.group(1).split(","):
        a = re.sub(r"\s*\*\s*", "* ", a.strip())           # "double* F"
        args.append(a.rsplit(" ", 1)[0].strip())           # the type without the parameter's name
    return args


def test_header_declares_the_four_entries(built):
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    assert _declaration(h, "c3d_get_coords_f64") == ["c3d_ctx*", "double*"]
    assert _declaration(h, "c3d_get_velocities_f64") == ["c3d_ctx*", "double*"]
    assert _declaration(h, "c3d_set_coords_f64") == ["c3d_ctx*", "const double*"]
    assert _declaration(h, "c3d_eval_f64") == ["c3d_ctx*", "double", "double", "double", "double*", "double*"]
    assert "f64_evals" in h


def test_the_entries_are_exported_bound_as_declared_and_wrapped(built):
    from chromosome3d_amd import lib
    from chromosome3d_amd.solver import Solver
    L = lib.load()
    h = open(os.path.join(ROOT, "include", "c3d.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        res, args = lib.SIGNATURES[name]
        assert res is C.c_int
        assert args == [CTYPES[t] for t in _declaration(h, name)], name
    for method in ("coords64", "velocities64", "set_coords64", "eval64"):
        assert callable(getattr(Solver, method))


def test_without_a_context_they_refuse_and_name_themselves(built):
    """NULL is the only context there is where no device exists (c3d_create fails there), and a caller's possible mistake everywhere"""
    from chromosome3d_amd import lib
    L = lib.load()
    if L.c3d_device_count() == 0:
        h = C.c_void_p()
        assert L.c3d_create(0, C.byref(h)) != 0 and not h.value
    out = np.zeros(12)
    for name, call in (("c3d_get_coords_f64", lambda: L.c3d_get_coords_f64(None, None)),
                       ("c3d_get_velocities_f64", lambda: L.c3d_get_velocities_f64(None, None)),
                       ("c3d_set_coords_f64", lambda: L.c3d_set_coords_f64(None, None)),
                       ("c3d_eval_f64", lambda: L.c3d_eval_f64(None, 1.0, 1.0, 0.85, None, None)),
                       ("c3d_get_coords_f64", lambda: L.c3d_get_coords_f64(None, lib.dptr(out))),
                       ("c3d_eval_f64", lambda: L.c3d_eval_f64(None, 1.0, 1.0, 0.85, lib.dptr(out), lib.dptr(out)))):
        assert call() == C3D_ERR_INVALID, name
        msg = L.c3d_last_error()
        assert name.encode() in msg and len(msg) > len(name), (name, msg)
    v = C.c_double()
    assert L.c3d_get_stat(None, b"f64_evals", C.byref(v)) == C3D_ERR_INVALID
