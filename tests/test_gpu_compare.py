"""The models of a run against one another on the device (c3d_compare_replicas, csrc/c3d_score_compare.inc k_cmp_*; hook c3d_debug_distance_ranks).

The host side of every table is pipeline.model_similarity (c3d_model_similarity, fp64) on the replicas' float coordinates cast to double;
the host side of the hook is a numpy restatement of the average ranks over sqrt(((ux ux) + uy uy) + uz uz) in float64.

Shapes, the smallest at which each part can still go wrong (m = n(n-1)/2 pairs, sorted in 4096-key LDS tiles):
  n64      64 beads x 3     m = 2016: one tile
  n92      92 beads x 2     m = 4186 -> 8192 slots: the first global-stride pass of the sort
  n257     257 beads x 5 + 2 extra models   m = 32896 = 2^15 + 128 -> 65536 slots, several global passes; n no multiple of 64, K = 7 no
           multiple of 4 or 16; the extra models are doubles no float holds
  k17      64 beads x 17    K crosses a sixteen-model block of the table pass
  lattice  130 beads x 4    integer coordinates in [0, 6)^3: coincident beads (distance 0), heavy ties, all arithmetic exact; replica 1 is a
           copy of replica 0, replica 2 is 3 x replica 0
  f64      64 beads x 3     a precision-64 context, lattice [1, 7)^3 plus noise that no float holds: the float mirror is what is compared

Tolerances (from the arithmetic, not from the device's numbers): the ranks are equal bit for bit.  rho and rmsd differ from the host's by
the order of summation alone: a few m 2^-53, about 1e-11 at the largest m here, so |rho_dev - rho_host| <= 1e-10 and |rmsd_dev - rmsd_host|
<= 1e-10 max(1, rmsd_host).  One misplaced tie group at n = 64 would move rho by about 12 / m^3 = 1.5e-9."""
import os
import subprocess

import numpy as np
import pytest

from tests.util import GOLD, SHORT, load_if, load_pdb_xyz, model_pdb, random_coil, restrained, shared_models
from tests.util import host_ranks as _host_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10
CASES = ["n64", "n92", "n257", "k17", "lattice"]


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _models(name):
    """(replica coordinates [M, n, 3] float32, extra models [E, n, 3] float64 or None)"""
    if name == "n64":
        return np.stack([random_coil(64, 100 + r) for r in range(3)]), None
    if name == "n92":
        return np.stack([random_coil(92, 200 + r) for r in range(2)]), None
    if name in ("n257", "k17"):
        return shared_models(name)
    rng = np.random.default_rng(130)
    a, b = rng.integers(0, 6, size=(130, 3)), rng.integers(0, 6, size=(130, 3))
    assert len(np.unique(a, axis=0)) < 130                                     # coincident beads
    return np.stack([a, a, 3 * a, b]).astype(np.float32), None


_HOST = {}


def _host_tables(name, models):
    """the K x K tables of the host loop, computed once per case"""
    if name not in _HOST:
        from chromosome3d_amd import pipeline
        K = len(models)
        rho, rmsd = np.empty((K, K)), np.empty((K, K))
        for a in range(K):
            for b in range(K):
                rho[a, b], rmsd[a, b] = pipeline.model_similarity(models[a], models[b])
        rho.setflags(write=False)
        rmsd.setflags(write=False)
        _HOST[name] = (rho, rmsd)
    return _HOST[name]


def _load(ctx, name):
    """the context holding the case's replicas; returns (x, extra, all K models as doubles)"""
    x, extra = _models(name)
    restrained(ctx, x.shape[1], x.shape[0])
    ctx.set_coords(x)
    models = [m.astype(np.float64) for m in x] + ([] if extra is None else list(extra))
    return x, extra, models


def _check_tables(rho, rmsd, hrho, hrmsd, what):
    erho, ermsd = np.abs(rho - hrho).max(), (np.abs(rmsd - hrmsd) / np.maximum(1.0, hrmsd)).max()
    print(f"{what}: K {len(rho)}, max |rho - host| {erho:.3e}, max |rmsd - host| / max(1, rmsd) {ermsd:.3e}")
    assert np.isfinite(rho).all() and np.isfinite(rmsd).all()
    assert erho <= TOL, (what, erho)
    assert ermsd <= TOL, (what, ermsd)
    assert np.array_equal(np.diag(rho), np.ones(len(rho))) and np.array_equal(np.diag(rmsd), np.zeros(len(rho)))


@pytest.mark.parametrize("name", CASES)
def test_distance_ranks_are_the_hosts_bit_for_bit(ctx, name):
    """The hook against numpy for every replica: the device's distances have the host's bits and its tie groups are the host's."""
    x, _, _ = _load(ctx, name)
    for r in range(len(x)):
        dev, host = ctx.debug_distance_ranks(r), _host_ranks(x[r])
        assert dev.shape == host.shape
        bad = np.flatnonzero(dev != host)
        assert bad.size == 0, (name, r, bad.size, bad[:5], dev[bad[:5]], host[bad[:5]])
    if name == "lattice":
        assert len(np.unique(_host_ranks(x[0]))) < 200                         # heavy ties, as meant


@pytest.mark.parametrize("name", CASES)
def test_tables_equal_the_host_loop(ctx, name):
    """Both K x K tables against pipeline.model_similarity of every ordered pair, extras included; diagonals exactly 1 and 0."""
    x, extra, models = _load(ctx, name)
    hrho, hrmsd = _host_tables(name, models)
    rho, rmsd = ctx.compare(extra)
    assert rho.shape == rmsd.shape == (len(models), len(models))
    _check_tables(rho, rmsd, hrho, hrmsd, name)


def test_lattice_copies_are_exact(ctx):
    """A copy gives rho exactly 1 and rmsd exactly 0 both ways; the 3 x copy gives exactly the host's rho (1: same ranks) and rmsd <= 1e-9,
    the bound of the host's own test."""
    x, _, models = _load(ctx, "lattice")
    hrho, _ = _host_tables("lattice", models)
    rho, rmsd = ctx.compare()
    assert rho[0, 1] == 1.0 and rho[1, 0] == 1.0 and rmsd[0, 1] == 0.0 and rmsd[1, 0] == 0.0
    for a, b in ((0, 2), (2, 0), (1, 2), (2, 1)):
        assert rho[a, b] == hrho[a, b] == 1.0, (a, b, rho[a, b], hrho[a, b])
        assert rmsd[a, b] <= 1e-9, (a, b, rmsd[a, b])
    assert rho[0, 3] < 0.9 and rmsd[0, 3] > 0.1                                 # and an unrelated lattice is unrelated


def test_precision64_context_compares_its_float_mirror():
    """compare() and its hook read the floats on every context: on a precision-64 one the float mirror of the fp64 state, which is what
    coords() returns and what the host twin is fed.  64 beads x 3 (one sort tile, one table block) on the lattice [1, 7)^3 plus 1e-9 of
    noise: a float's spacing at 1 is 1.2e-7, so the mirror is the bare lattice with heavy ties (43 to 44 distinct ranks a model), while the
    doubles have none (2016 distinct ranks) and 1992 to 1994 of the 2016 ranks differ between the two."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        restrained(s, 64, 3)
        rng = np.random.default_rng(64)
        lattice, x = [], []
        for _ in range(3):
            lattice.append(rng.integers(1, 7, size=(64, 3)).astype(np.float64))
            x.append(lattice[-1] + 1e-9 * rng.normal(size=(64, 3)))
        s.set_coords64(np.stack(x))
        mirror, state = s.coords(), s.coords64()
        assert np.array_equal(mirror, np.stack(lattice)) and np.array_equal(state, np.stack(x))
        for r in range(3):
            dev, of_mirror, of_state = s.debug_distance_ranks(r), _host_ranks(mirror[r]), _host_ranks(state[r])
            differ = int((dev != of_state).sum())
            print(f"replica {r}: ranks off the mirror's {int((dev != of_mirror).sum())}, off the fp64 state's {differ} of {dev.size}, "
                  f"distinct ranks {len(np.unique(of_mirror))} / {len(np.unique(of_state))}")
            assert np.array_equal(dev, of_mirror)
            assert differ > dev.size // 2
        models = [m.astype(np.float64) for m in mirror]
        rho, rmsd = s.compare()
        _check_tables(rho, rmsd, *_host_tables("f64 mirror", models), "f64 mirror")
    finally:
        s.close()


def test_rmsd_is_not_symmetric_and_each_side_is_the_hosts(ctx):
    """rmsd[a][b] scales a onto b: two models of different mean distance differ across the diagonal, each entry equal to the host's."""
    x, extra, models = _load(ctx, "n257")
    hrho, hrmsd = _host_tables("n257", models)
    rho, rmsd = ctx.compare(extra)
    a, b = 0, len(x) + 1                                                        # a replica and the extra model scaled by 2.5
    assert hrmsd[a, b] != hrmsd[b, a] and rmsd[a, b] != rmsd[b, a]
    assert abs(rmsd[a, b] - hrmsd[a, b]) <= TOL * max(1.0, hrmsd[a, b]) and abs(rmsd[b, a] - hrmsd[b, a]) <= TOL * max(1.0, hrmsd[b, a])
    assert abs(rmsd[b, a] / rmsd[a, b] - 1.0) > 0.1


def test_extras_given_as_the_replicas_reproduce_the_replica_block(ctx):
    x, _, _ = _load(ctx, "n64")
    M = len(x)
    rho0, rmsd0 = ctx.compare()
    rho, rmsd = ctx.compare(x.astype(np.float64))
    assert rho.shape == (2 * M, 2 * M)
    for blk in (np.s_[:M, :M], np.s_[M:, M:], np.s_[:M, M:], np.s_[M:, :M]):
        assert np.array_equal(rho[blk], rho0) and np.array_equal(rmsd[blk], rmsd0)
    one = ctx.compare(x[1].astype(np.float64))                                  # a single model [n, 3]
    assert one[0].shape == (M + 1, M + 1) and one[0][1, M] == 1.0 and one[1][1, M] == 0.0
    # one output alone
    L, h = ctx._L, ctx._h
    from chromosome3d_amd import lib
    only = np.empty((M, M))
    assert L.c3d_compare_replicas(h, None, 0, lib.dptr(only), None) == 0 and np.array_equal(only, rho0)
    assert L.c3d_compare_replicas(h, None, 0, None, lib.dptr(only)) == 0 and np.array_equal(only, rmsd0)


def test_two_calls_return_the_same_bytes_and_nothing_of_the_solve_changes(ctx):
    x, extra, _ = _load(ctx, "n257")
    ctx.run_steps(20)                                                           # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done)
    runs = ctx.stat("compare_runs")
    first = ctx.compare(extra)
    second = ctx.compare(extra)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    ctx.debug_distance_ranks(0)
    assert ctx.stat("compare_runs") == runs + 2
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3] == after[3]
    assert ctx.run_steps(5) == 5                                                # and the solve goes on


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name; none counts as a run; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    x, _, models = _load(ctx, "n64")
    n, M = x.shape[1], x.shape[0]
    L, h = ctx._L, ctx._h
    runs = ctx.stat("compare_runs")
    out = np.empty(4)                                                           # never written by a refused call
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows
    good = x.astype(np.float64)

    def refused(*args):
        rc = L.c3d_compare_replicas(h, *args)
        assert rc == -1 and b"c3d_compare_replicas" in L.c3d_last_error(), (args, rc, L.c3d_last_error())

    refused(lib.dptr(good), -1, lib.dptr(out), lib.dptr(out))                   # n_extra < 0
    refused(None, 1, lib.dptr(out), lib.dptr(out))                              # extra models without coordinates
    refused(lib.dptr(big), len(big), lib.dptr(out), lib.dptr(out))              # K = 257
    refused(None, 0, None, None)                                                # both outputs NULL
    for bad in (np.nan, np.inf, -np.inf, 1e6):                                  # what check_coords_d refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(lib.dptr(e), M, lib.dptr(out), lib.dptr(out))
    rank = np.empty(n * (n - 1) // 2)
    for r in (-1, M):                                                           # replica index out of range
        assert L.c3d_debug_distance_ranks(h, r, lib.dptr(rank)) == -1 and b"c3d_debug_distance_ranks" in L.c3d_last_error()
    assert L.c3d_debug_distance_ranks(h, 0, None) == -1
    assert ctx.stat("compare_runs") == runs
    # K = 256 itself is accepted
    rho, rmsd = ctx.compare(big[:-1] + good[0])
    assert rho.shape == (256, 256) and rho[0, 255] == 1.0 and rmsd[255, 0] == 0.0
    hrho, hrmsd = _host_tables("n64", models)
    _check_tables(rho[:M, :M], rmsd[:M, :M], hrho, hrmsd, "n64 after the refusals")
    assert ctx.stat("compare_runs") == runs + 1
    # no replicas; fewer than 3 beads
    s = Solver(0)
    try:
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        for call in (s.compare, lambda: s.debug_distance_ranks(0)):
            with pytest.raises(C3DError, match="c3d_init_replicas"):
                call()
        s.init_replicas(2)
        with pytest.raises(C3DError, match="c3d_compare_replicas.*3 beads"):
            s.compare()
        with pytest.raises(C3DError, match="c3d_debug_distance_ranks.*3 beads"):
            s.debug_distance_ranks(0)
        assert s.stat("compare_runs") == 0
    finally:
        s.close()


def test_after_a_real_run_and_from_the_command_line(ctx, tmp_path):
    """The smallest bundled matrix, 4 replicas, the default schedule, the bundled model as an extra: every entry within the tolerances of the
    host loop; c3d_solve --similarity on the same matrix writes the replica block to the printed digits, and no file without the option."""
    from chromosome3d_amd import default_model, pipeline
    cid = "chr21_1mb"
    IF = load_if(cid)
    ref = load_pdb_xyz(model_pdb(cid))
    assert ref.shape == (len(IF), 3)
    ctx.set_model(default_model())
    pipeline.IF2dist_new(ctx, IF)
    x, _ = pipeline.build_models(ctx, 4)
    rho, rmsd = pipeline.compare_models(ctx, ref)
    models = [m.astype(np.float64) for m in x] + [ref]
    hrho, hrmsd = _host_tables("run", models)
    _check_tables(rho, rmsd, hrho, hrmsd, cid)
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    table = tmp_path / "similarity.txt"
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", "4", "--quiet", "--similarity", str(table)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = table.read_text().splitlines()
    assert lines[0].startswith("#") and len(lines) == 1 + 4 * 3
    want = [f"{a} {b} {rho[a, b]:.5f} {rmsd[a, b]:.5f}" for a in range(4) for b in range(4) if a != b]
    assert lines[1:] == want
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", "4", "--quiet"], capture_output=True, text=True)
    assert run.returncode == 0 and sorted(os.listdir(tmp_path / "b")) == sorted(f for f in os.listdir(tmp_path / "a"))
