"""A model's fit to the data bead by bead on the device (c3d_bead_scores; csrc/c3d_score_bead.inc k_bead_if, k_bead_model) against the
numpy restatement tests/bead_ref.py, which tests/test_bead_ref.py holds to scipy's spearmanr row by row and to the reference's own
assessment of its bundled models.

The kernels' constants are the stratified family's (tests/test_gpu_stratified.py): a workgroup of 256 threads sorts one row's N_i keys,
padded to P, in LDS (64-bit keys for IF, 32-bit for the distances), 4 consecutive keys a thread in registers, 16-byte vectors above that.
Unlike there a call has ONE P, str_slots(n - range), the longest row's; N_i = max(0, i-range+1) + max(0, n-i-range).
  n5      2 replicas, ranges 1, 2, 4: N = 4 | 3, 2 | 1, 0, all in the smallest network (P = 8); rows of one and of no pair sort nothing
  n131    2 replicas, range 1: N = 130 everywhere (P = 256); range 2: N = 129 at the ends, 128 inside, the 256 | 128 edge from above
          (P = 256, half of it pad); range 3: N = 128, 127, 126 in P = 128: a row of exactly P keys and no pad beside rows of one and two
  n2052   2 replicas + 1 extra fp64 model that no float holds, range 3: N = 2049, 2048, 2047 in P = 4096 with one real key past half; a
          thread owns several chunks and several comparator vectors on both key widths
  n16384  1 replica, analytic coordinates: (range 1, beads 0, 8000, 16383) N = 16383, P = 16384 (128 KiB of 64-bit keys);
          (range 8192, beads 0, 1, 8191, 8192, 16383) N = 8192, 8191, 1, 1, 8192 in P = 8192; the picked rows alone are restated
The tie cases (two IF values a row, an all-zero row, -0.0 beside 0.0, a lattice model, the straight chain) run at n131.

Bounds.  sums (C, A, B), restrained, satisfied and dev_milli are exact integers: ==.  rho is formed on the host of the library by IEEE
operations (int64 -> double, x, sqrt, /) from equal integers in the order the restatement uses: bitwise equal, NaN where and only where
the restatement has NaN."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import bead_ref as Bd
from tests import stratified_ref as S
from tests.util import GOLD, SHORT, golden, load_if, load_pdb_xyz, random_coil, shared_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TALLIES = ("restrained", "satisfied", "dev_milli")


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def ctx_sep1():
    """a context of its own for the model with min_sep = 1: a context keeps the min_sep its first targets were built with"""
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _context(s, n, nrep, min_sep=None, seed=7):
    """a context of n beads with a random restraint set of partners 1..11 apart and nrep replicas; returns (t10 [n, n], min_sep)"""
    from chromosome3d_amd import default_model, make_stages
    rng = np.random.default_rng(seed)
    R = max(1, min(3 * n, n * (n - 1) // 2))
    i = rng.integers(1, n, size=R)
    j = np.minimum(i + rng.integers(1, 12, size=R), n)
    keep = j > i
    i, j, t = i[keep].astype(np.int32), j[keep].astype(np.int32), rng.integers(30, 120, size=int(keep.sum())).astype(np.int32)
    model = default_model() if min_sep is None else default_model(min_sep=min_sep)
    s.set_model(model)
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, i, j, t)
    s.init_replicas(nrep)
    return Bd.targets_of_restraints(n, i, j, t), int(model.min_sep)


def _noisy_if(n, seed):
    """a matrix without structure to spare and NOT symmetric (a row is read from the row alone): distinct positive values"""
    rng = np.random.default_rng(seed)
    return rng.lognormal(size=(n, n)) / (1.0 + np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]))


def _host(IF, models, rng, tm, beads=None):
    cache = {}
    return [Bd.bead_scores(IF, m, rng, beads, tm[0], tm[1], cache) for m in models]


def _check(got, host, what):
    """sums and tallies ==, rho bitwise, NaN exactly where the restatement has it"""
    assert len(got["satisfied"]) == len(host)
    for k, h in enumerate(host):
        if "sums" in h:
            assert np.array_equal(got["sums"][k], h["sums"]), (what, k)
            assert np.array_equal(np.isnan(got["rho"][k]), np.isnan(h["rho"])), (what, k)
            assert got["rho"][k].tobytes() == h["rho"].tobytes(), (what, k)
        assert np.array_equal(got["restrained"], h["restrained"]), (what, k)
        assert np.array_equal(got["satisfied"][k], h["satisfied"]), (what, k)
        assert np.array_equal(got["dev_milli"][k], h["dev_milli"]), (what, k)
        assert got["satisfied"].dtype == np.int32 and got["dev_milli"].dtype == np.int64
    if "rho" in got:
        print(f"{what}: rows with a coefficient {[int((~np.isnan(r)).sum()) for r in got['rho']]} of {got['rho'].shape[1]}, restrained {int(got['restrained'].sum())}, "
              f"satisfied {[int(v.sum()) for v in got['satisfied']]}")


@pytest.mark.parametrize("rng", [1, 2, 4])
def test_the_smallest_network_and_rows_of_one_and_no_pair(ctx_sep1, rng):
    ctx, n = ctx_sep1, 5
    x = np.stack([random_coil(n, 50 + r) for r in range(2)])
    tm = _context(ctx, n, 2, min_sep=1)
    assert tm[0].sum() > 0
    ctx.set_coords(x)
    IF = _noisy_if(n, 5)
    got = ctx.bead_scores(IF, rng)
    _check(got, _host(IF, [m.astype(np.float64) for m in x], rng, tm), f"n5 range {rng}")
    N = np.maximum(0, np.arange(n) - rng + 1) + np.maximum(0, n - np.arange(n) - rng)
    assert list(N) == {1: [4] * 5, 2: [3, 2, 2, 2, 3], 4: [1, 0, 0, 0, 1]}[rng]
    assert (got["sums"][:, N <= 1] == 0).all() and np.isnan(got["rho"][:, N <= 1]).all() and (got["sums"][:, N > 1, 1] > 0).all()
    assert got["restrained"].sum() > 0


@pytest.mark.parametrize("rng", [1, 2, 3])
def test_rows_around_128_keys(ctx, rng):
    n = 131
    x = np.stack([random_coil(n, 1310 + r) for r in range(2)])
    tm = _context(ctx, n, 2)
    ctx.set_coords(x)
    IF = _noisy_if(n, 131)
    got = ctx.bead_scores(IF, rng)
    _check(got, _host(IF, [m.astype(np.float64) for m in x], rng, tm), f"n131 range {rng}")
    N = np.maximum(0, np.arange(n) - rng + 1) + np.maximum(0, n - np.arange(n) - rng)
    assert sorted(set(N)) == {1: [130], 2: [128, 129], 3: [126, 127, 128]}[rng]
    assert not np.isnan(got["rho"]).any() and got["restrained"].sum() > 0


def _lattice(n, seed, step=3.0):
    rng = np.random.default_rng(seed)
    d = np.zeros((n, 3))
    d[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-step, step], n)
    return np.cumsum(d, axis=0).astype(np.float32)


def test_ties_on_either_side(ctx):
    n = 131
    chain = np.zeros((n, 3), np.float32)
    chain[:, 0] = 1.5 * np.arange(n)
    x = np.stack([_lattice(n, 7), chain])
    tm = _context(ctx, n, 2)
    ctx.set_coords(x)
    models = [m.astype(np.float64) for m in x]
    i, j = np.indices((n, n))
    two = ((j // 7) % 2).astype(np.float64) + 1.0                               # two values a row
    zero = _noisy_if(n, 9)
    zero[40] = 0.0                                                              # an all-zero row (an unmappable bin): constant, NaN
    zero[41, ::2] = 0.0
    zero[41, 1::4] = -0.0                                                       # -0.0 beside 0.0: equal, and tied
    for name, IF in (("two values", two), ("zero row", zero), ("distinct", _noisy_if(n, 11))):
        for rng in (1, 3):
            got = ctx.bead_scores(IF, rng)
            _check(got, _host(IF, models, rng, tm), f"ties, IF {name}, range {rng}")
    got = ctx.bead_scores(zero, 1)
    assert np.isnan(got["rho"][:, 40]).all() and (got["sums"][:, 40, 1] == 0).all() and (got["sums"][:, 40, 2] > 0).all()
    assert not np.isnan(np.delete(got["rho"], 40, axis=1)).any()
    q = Bd.row_milli(models[0], 60, Bd.partners(n, 60, 1))
    assert len(np.unique(q)) < len(q) * 3 // 4                                  # the lattice model ties its distances
    q = Bd.row_milli(models[1], 60, Bd.partners(n, 60, 1))
    assert len(np.unique(q)) == 70                                              # the chain: every distance below bead 60 has its twin above


def test_past_2048_keys_with_an_extra_model(ctx):
    n = 2052
    x = np.stack([random_coil(n, 20520 + r) for r in range(2)])
    rng = np.random.default_rng(2052)
    extra = random_coil(n, 20529).astype(np.float64) * 1.5 + rng.normal(scale=1e-3, size=(n, 3))
    assert not np.array_equal(extra, extra.astype(np.float32))
    tm = _context(ctx, n, 2)
    ctx.set_coords(x)
    IF = _noisy_if(n, n)
    got = ctx.bead_scores(IF, 3, None, extra)
    _check(got, _host(IF, [m.astype(np.float64) for m in x] + [extra], 3, tm), "n2052")
    N = np.maximum(0, np.arange(n) - 2) + np.maximum(0, n - np.arange(n) - 3)
    assert sorted(set(N)) == [2047, 2048, 2049] and not np.isnan(got["rho"]).any()


def test_the_largest_network_and_the_8192_edge():
    """16384 beads on a Lissajous curve, IF = (i + j) mod 1021: 1021 values a row (ties throughout), both sides vary along every row.  Only
    the picked rows are sorted, on the device and on the host."""
    from chromosome3d_amd import Solver, default_model, make_stages
    n = 16384
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        model = default_model()
        s.set_model(model)
        s.set_schedule(make_stages(SHORT))
        rows = (np.array([1, 1, 8001], np.int32), np.array([11, 16384, 16384], np.int32), np.array([100, 457, 300], np.int32))
        s.set_restraints(n, *rows)
        tm = (_SparseTargets(n, *rows), int(model.min_sep))
        i = np.arange(n, dtype=np.float64)
        IF = np.add.outer(i, i)
        np.fmod(IF, 1021.0, out=IF)
        x = np.zeros((1, n, 3), np.float32)
        x[0, :, 0] = 50.0 * np.cos(0.37 * i) + 0.01 * i
        x[0, :, 1] = 50.0 * np.sin(0.21 * i)
        x[0, :, 2] = 30.0 * np.cos(0.113 * i + 1.0)
        s.init_replicas(1, 82364, 0)
        s.set_coords(x)
        xd = s.coords()[0].astype(np.float64)
        for rng, beads, N in ((1, [0, 8000, 16383], [16383] * 3), (8192, [0, 1, 8191, 8192, 16383], [8192, 8191, 1, 1, 8192])):
            assert [len(Bd.partners(n, b, rng)) for b in beads] == N
            got = s.bead_scores(IF, rng, beads)
            _check(got, _host(IF, [xd], rng, tm, beads), f"n16384 range {rng} beads {beads}")
            few = np.array(N) <= 1
            assert not np.isnan(got["rho"][0, ~few]).any() and np.isnan(got["rho"][0, few]).all() and (got["sums"][0, few] == 0).all()
            assert list(got["restrained"]) == [2 if b in (0, 16383) else 1 if b == 8000 else 0 for b in beads]
    finally:
        s.close()


@pytest.mark.parametrize("cid", ["chr21_1mb", "chr4_1mb"])
def test_the_tallies_against_the_references_assessment(ctx, cid):
    """Targets from the matrix itself (K1).  The bundled model's tallies add up to twice the reference's own figures; on a lattice model —
    coordinates that are multiples of 0.125 A, exact in float and under the "%.3f" rounding of c3d_score_replicas — the satisfied counts
    add up to exactly twice c3d_score_replicas' and the deviation to twice its fp64 sum within that sum's rounding: R terms of at most
    d_max + t_max <= 3 d_max ... each added to a partial sum of at most sum_dev, half an ulp of the running sum a step."""
    from chromosome3d_amd import default_model, make_stages
    g = golden()[cid]
    n = g["n"]
    IF = load_if(cid)
    bundled = load_pdb_xyz(os.path.join(GOLD, "models", g["model"]))
    model = default_model()
    ctx.set_model(model)
    ctx.set_schedule(make_stages(SHORT))
    ctx.set_if_matrix(IF)
    tm = (ctx.dist10().astype(np.int64), int(model.min_sep))
    ctx.init_replicas(2)
    x = ctx.coords()
    x[1] = _lattice(n, 11, 0.125 * 40)
    assert np.array_equal(x[1] / 0.125, np.rint(x[1] / 0.125))
    ctx.set_coords(x)
    got = ctx.bead_scores(IF, 3, None, bundled)
    _check(got, _host(IF, [m.astype(np.float64) for m in x] + [bundled], 3, tm), cid)
    alone = ctx.bead_scores(None)                                               # the tallies alone, no matrix: the same bytes
    assert sorted(alone) == sorted(TALLIES) and alone["restrained"].tobytes() == got["restrained"].tobytes()
    assert alone["satisfied"].tobytes() == got["satisfied"][:2].tobytes() and alone["dev_milli"].tobytes() == got["dev_milli"][:2].tobytes()
    sat, R = (int(v) for v in g["satisfied"].split("/"))
    assert R == g["restraints"] and int(got["restrained"].sum()) == 2 * R and int(got["satisfied"][2].sum()) == 2 * sat
    total = sum(int(v) for v in got["dev_milli"][2])
    assert total % 2 == 0 and "%.2f" % (total / 2000) == "%.2f" % g["sum_dev"]
    k6_sat, k6_dev, _ = ctx.score(IF, 3)
    assert int(got["satisfied"][1].sum()) == 2 * int(k6_sat[1])
    lattice_dev = sum(int(v) for v in got["dev_milli"][1]) / 2000
    d_max = float(S.round_milli(np.linalg.norm(x[1].astype(np.float64)[:, None] - x[1].astype(np.float64)[None], axis=-1)).max()) / 1000.0
    bound = R * (3.0 * d_max + k6_dev[1]) * 2.0 ** -52
    print(f"{cid}: bundled {sat}/{R}, {total / 2000:.3f} A; lattice satisfied {int(k6_sat[1])}, dev {lattice_dev!r} against c3d_score_replicas {k6_dev[1]!r}, bound {bound:.3g}")
    assert abs(lattice_dev - k6_dev[1]) <= bound


def test_f64_state_is_scored_in_doubles():
    """A precision-64 context: sums and tallies follow the fp64 state, not its float rounding.  Coordinates near 9000 A, where a float's last
    place is 1e-3 A: rounding them to float moves the "%.3f" distances of a lattice model's many near-ties."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        n = 96
        tm = _context(s, n, 3)
        rng = np.random.default_rng(96)
        x = np.stack([_lattice(n, 960 + r).astype(np.float64) + 9000.0 for r in range(3)]) + rng.normal(scale=2e-3, size=(3, n, 3))
        IF = _noisy_if(n, 96)
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x)
        got = s.bead_scores(IF, 2)
        _check(got, _host(IF, list(x), 2, tm), "f64")
        rounded = _host(IF, list(x.astype(np.float32).astype(np.float64)), 2, tm)
        assert all(not np.array_equal(got["sums"][k], rounded[k]["sums"]) for k in range(3))
    finally:
        s.close()


class _SparseTargets:
    """the integer tenths of a restraint list as rows on demand: t[i] is row i of tests/bead_ref.targets_of_restraints, which at 16384 beads
    would take 2 GiB"""

    def __init__(self, n, ri, rj, rt10):
        self.n, self.rows = n, list(zip(ri, rj, rt10))

    def __getitem__(self, i):
        row = np.zeros(self.n, dtype=np.int64)
        for a, b, v in self.rows:
            if v > 0 and i in (a - 1, b - 1):
                row[(b - 1) if i == a - 1 else (a - 1)] = v
        return row


def _raw(ctx, IF, rng, beads, extra, K, B, want):
    """one call of the C entry with the outputs of `want` alone; returns {name: array}"""
    from chromosome3d_amd import lib
    shape = {"rho": ((K, B), np.float64), "sums": ((K, B, 3), np.int64), "restrained": ((B,), np.int32), "satisfied": ((K, B), np.int32), "dev_milli": ((K, B), np.int64)}
    kind = {np.float64: C.c_double, np.int64: C.c_int64, np.int32: C.c_int32}
    out = {k: np.full(shape[k][0], 7, shape[k][1]) for k in want}
    ptr = [out[k].ctypes.data_as(C.POINTER(kind[shape[k][1]])) if k in out else None for k in ("rho", "sums") + TALLIES]
    b = None if beads is None else np.ascontiguousarray(beads, np.int32)
    rc = ctx._L.c3d_bead_scores(ctx._h, lib.dptr(IF) if IF is not None else None, rng, lib.i32ptr(b) if b is not None else None, 0 if b is None else len(b),
                                lib.dptr(extra) if extra is not None else None, 0 if extra is None else len(extra), *ptr)
    return rc, out


def test_two_calls_return_the_same_bytes_and_nothing_of_the_solve_changes(ctx):
    x, extra = shared_models("n257")
    n = 257
    tm = _context(ctx, n, 5)
    ctx.set_coords(x)
    IF = _noisy_if(n, 257)
    ctx.run_steps(20)                                                           # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    runs = ctx.stat("bead_runs")
    a, b = ctx.bead_scores(IF, 3, None, extra), ctx.bead_scores(IF, 3, None, extra)
    assert sorted(a) == sorted(("rho", "sums") + TALLIES)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    alone = ctx.bead_scores(IF, 3)                                              # without the extra models: the replicas keep their bits
    for k in a:
        assert alone[k].tobytes() == (a[k] if k == "restrained" else a[k][:5]).tobytes(), k
    _check(a, _host(IF, [m.astype(np.float64) for m in before[0]] + list(extra), 3, tm), "n257 mid-solve")
    beads = [0, 1, 2, 100, 128, 254, 256]                                       # a bead list: the matching rows of the full call
    some = ctx.bead_scores(IF, 3, beads, extra)
    for k in a:
        assert some[k].tobytes() == np.ascontiguousarray(a[k][..., beads] if k not in ("sums",) else a[k][:, beads]).tobytes(), k
    for k in ("rho", "sums") + TALLIES:                                         # each output alone: the same bytes
        rc, out = _raw(ctx, IF if k in ("rho", "sums") else None, 3, None, extra, 7, n, (k,))
        assert rc == 0 and out[k].tobytes() == a[k].tobytes(), k
    assert ctx.stat("bead_runs") == runs + 9 and ctx.stat("bead_models_ms") > 0
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    assert ctx.run_steps(5) == 5                                                # and the solve goes on


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name; none counts as a run or writes an output; the context
    works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    n, M = 64, 2
    x = np.stack([random_coil(n, 640 + r) for r in range(M)])
    tm = _context(ctx, n, M)
    ctx.set_coords(x)
    IF = _noisy_if(n, 64)
    runs, state = ctx.stat("bead_runs"), ctx.coords().tobytes()
    good = x.astype(np.float64)
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows
    every = ("rho", "sums") + TALLIES

    def refused(IF_, rng, beads, extra, want=every, nb=None):
        K, B = M + (0 if extra is None else len(extra)), n if beads is None else max(len(beads), 1)
        if nb is None:
            rc, out = _raw(ctx, IF_, rng, beads, extra, K, B, want)
        else:                                                                   # a bead count that is not the list's length
            out = {"rho": np.full((K, n), 7.0)}
            b = None if beads is None else np.ascontiguousarray(beads, np.int32)
            rc = ctx._L.c3d_bead_scores(ctx._h, lib.dptr(IF_), rng, lib.i32ptr(b) if b is not None else None, nb, None, 0, lib.dptr(out["rho"]), None, None, None, None)
        assert rc == -1 and b"c3d_bead_scores" in ctx._L.c3d_last_error(), (rng, beads, want)
        assert all((v == 7).all() for v in out.values()), (rng, beads, want)     # nothing written

    refused(IF, 0, None, None)                                                  # range < 1
    refused(IF, -2, None, None)
    refused(IF, n, None, None)                                                  # range > n-1
    refused(None, 3, None, None)                                                # rho and sums without IF
    refused(None, 3, None, None, ("rho",) + TALLIES)
    refused(None, 3, None, None, ("sums",))
    refused(IF, 3, None, None, ())                                              # every output NULL
    refused(IF, 3, [0, n], None)                                                # a bead out of range
    refused(IF, 3, [-1, 5], None)
    refused(IF, 3, [5, 5], None)                                                # not strictly ascending
    refused(IF, 3, [7, 3], None)
    refused(IF, 3, [3], None, nb=0)                                             # a list with n_beads <= 0
    refused(IF, 3, [3], None, nb=-1)
    refused(IF, 3, None, None, nb=4)                                            # beads = NULL with n_beads != 0
    rho = np.full((M + 1, n), 7.0)
    assert ctx._L.c3d_bead_scores(ctx._h, lib.dptr(IF), 3, None, 0, None, 1, lib.dptr(rho), None, None, None, None) == -1      # n_extra > 0 without coordinates
    assert ctx._L.c3d_bead_scores(ctx._h, lib.dptr(IF), 3, None, 0, lib.dptr(good), -1, lib.dptr(rho), None, None, None, None) == -1 and (rho == 7.0).all()
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(IF, 3, None, e)
    refused(IF, 3, None, big)                                                   # K = 257
    # found by the first pass: a value that is not finite, in a row that was asked for only
    for bad in (np.nan, np.inf, -np.inf):
        e = IF.copy()
        e[7, 30] = bad
        refused(e, 3, None, None)
        assert b"not finite" in ctx._L.c3d_last_error()
        refused(e, 3, [7], None)
        assert _raw(ctx, e, 3, [6, 8, 30], None, M, 3, every)[0] == 0           # row 7 is not asked for (and IF[30][7] is fine: no symmetry)
        e[7, 30], e[7, 8] = IF[7, 30], bad                                      # inside the band |i-j| < range: not a member of the row
        assert _raw(ctx, e, 3, None, None, M, n, every)[0] == 0
    # found by the second pass: a model wider than 50 000 A
    far = good.copy()
    far[1, n - 1, 0] = 60000.0
    refused(IF, 3, None, far)
    assert b"50000" in ctx._L.c3d_last_error()
    refused(None, 3, None, far, TALLIES)
    assert ctx.stat("bead_runs") == runs + 6 and ctx.coords().tobytes() == state
    # 256 models are accepted, exactly 50 000 A too, and the context works
    wide = good[:1].copy()
    wide[0, :, :] = 0.0
    wide[0, :, 0] = np.linspace(0.0, 50000.0, n)
    many = np.concatenate([big[:-2] + good[0], wide])
    got = ctx.bead_scores(IF, 3, None, many)
    full = _host(IF, list(good), 3, tm)
    _check({k: (v if k == "restrained" else v[:2]) for k, v in got.items()}, full, "n64")
    assert got["sums"][254].tobytes() == got["sums"][0].tobytes() and got["rho"][254].tobytes() == got["rho"][0].tobytes()
    assert got["dev_milli"][254].tobytes() == got["dev_milli"][0].tobytes()
    end = _host(IF, [wide[0]], 3, tm)[0]                                        # 50 000.000 A between its ends: the limit itself is inside
    assert np.array_equal(got["sums"][255], end["sums"]) and np.array_equal(got["dev_milli"][255], end["dev_milli"])
    assert Bd.row_milli(wide[0], 0, [n - 1])[0] == Bd.FARTHEST
    assert ctx.stat("bead_runs") == runs + 7
    # no replicas; 2 beads: two rows of one pair
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_bead_scores.*c3d_init_replicas"):
            s2.bead_scores(np.ones((2, 2)), 1)
        s2.init_replicas(2)
        two = s2.bead_scores(np.ones((2, 2)), 1)
        assert np.isnan(two["rho"]).all() and (two["sums"] == 0).all() and (two["restrained"] == 0).all() and s2.stat("bead_runs") == 1
        with pytest.raises(C3DError, match="c3d_bead_scores.*range"):
            s2.bead_scores(np.ones((2, 2)), 2)
    finally:
        s2.close()


def _bounds(C_, A, B, dC, dB):
    """the interval of C' / sqrt(A B') over |C' - C| <= dC, |B' - B| <= dB (A > 0, B - dB > 0)"""
    corners = [c / np.sqrt(float(A) * float(b)) for c in (C_ - dC, C_ + dC) for b in (B - dB, B + dB)]
    return min(corners), max(corners)


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --per-bead on the smallest bundled matrix: rows 1..37, 2 + 3 M columns, `restrained` the restatement's, and coefficients
    that are the written models'.  A written coordinate is rounded to 3 decimals, so a written distance lies within sqrt(3) 1e-3 A of the
    one the run ranked and its thousandths within 2 of the run's: two distances of a row keep their order (and stay apart) when their
    written thousandths differ by more than 4.  Where that holds for a whole row the ranks are the run's and rho equals the written
    model's to its printed digits.  Elsewhere an element with c partners within 4 thousandths moves its doubled rank b by at most 2 c,
    which bounds the change of sum a b and sum b^2, and the file's number lies between the extremes (the bracket of
    tests/test_gpu_stratified.py::test_from_the_command_line)."""
    from chromosome3d_amd import default_model
    cid, M, n, rng = "chr21_1mb", 4, 37, 3
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "pb")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--per-bead", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = open(prefix + "_beads.txt").read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split() for l in lines if not l.startswith("#")]
    assert head and lines[:len(head)] == head                                   # header lines first, each with its `#`
    order = [int(v) for v in next(l for l in head if l.startswith("# models:")).split()[2:]]
    assert sorted(order) == [1, 2, 3, 4]
    assert [int(r[0]) for r in rows] == list(range(1, n + 1)) and all(len(r) == 2 + 3 * M for r in rows)
    IF = load_if(cid)
    ctx.set_model(default_model())
    ctx.set_if_matrix(IF)
    t10, min_sep = ctx.dist10().astype(np.int64), int(default_model().min_sep)
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r}.pdb") for r in order])
    host = _host(IF, list(x), rng, (t10, min_sep))
    assert [int(r[1]) for r in rows] == list(host[0]["restrained"])
    exact = bracketed = 0
    for col in range(M):
        for i in range(n):
            printed, sat, dev = rows[i][2 + 3 * col], int(rows[i][3 + 3 * col]), rows[i][4 + 3 * col]
            assert abs(sat) <= int(rows[i][1]) and float(dev) >= 0.0 and len(dev.split(".")[1]) == 3
            js = Bd.partners(n, i, rng)
            N = len(js)
            Cs, A, B = (int(v) for v in host[col]["sums"][i])
            assert A > 0 and printed != "nan" and len(printed.split(".")[1]) == 6
            q = Bd.row_milli(x[col], i, js)
            c = (np.abs(q[:, None] - q[None, :]) <= 4).sum(1) - 1
            a, b = S.if_ranks(IF[i, js]), S.doubled_ranks(q)
            dC, dB = N * int((a * 2 * c).sum()), N * int((2 * b * 2 * c + 4 * c * c).sum())
            if dC == 0 and dB == 0:
                assert abs(float(printed) - host[col]["rho"][i]) <= 5.000001e-7, (col, i)
                exact += 1
            if B - dB > 0:
                lo, hi = _bounds(Cs, A, B, dC, dB)
                assert lo - 5.000001e-7 <= float(printed) <= hi + 5.000001e-7, (col, i, lo, printed, hi)
                bracketed += 1
    print(f"rows equal to the printed digits: {exact}, bracketed: {bracketed} of {M * n}")
    assert exact > 0 and bracketed == M * n
