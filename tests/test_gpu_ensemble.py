"""The ensemble's distance map on the device (c3d_ensemble_map, c3d_ensemble_score; csrc/c3d_score_ensemble.inc k_ens_*) against its numpy
restatement tests/ensemble_ref.py, which tests/test_ensemble_ref.py holds to scipy and to the host helper.

Shapes, the smallest at which each part can still go wrong.  k_ens_map gives a workgroup a 64 x 64 tile of the upper triangle and stages
the picked models in blocks of 16: the tile-edge shapes of the issue are the ones for that tile and block, unchanged.
  n64      64 beads x 3     one (diagonal) tile
  n65      65 beads x 2     a partial edge tile of one row / column, and the off-diagonal tile beside it
  n130     130 beads x 4    three tile rows: full off-diagonal tiles and partial ones
  n257     257 beads x 5 + 2 extra fp64 models that no float holds   n no multiple of 64, K = 7; also with the pick [6, 4, 2, 2, 0]
           (reversed, a subset, one index twice)
  k17      64 beads x 17    one model more than a staging block
  lattice  130 beads x 4    integer coordinates in [0, 6)^3: coincident beads, heavy ties, exact arithmetic; replica 1 copies replica 0
  n2049    2049 beads x 3   33 tile rows, 561 tiles, n x n outputs of 32 MiB each: no loop changes shape past five tiles, what is new is the
           size of the outputs and of the ranking below them (no other case is past 257 beads)
  ranking, range 3: n = 92 (4005 keys: one sort tile), n = 95 (4278 keys -> 8192 slots: the first global pass), n = 257, n = 2049
           (2094081 keys a triangle -> 2^22 slots)
  f64     96 beads x 3 on a precision-64 context, coordinates no float holds

Bounds, from the arithmetic and not from the device's numbers.  A distance has the host's bits, so the contact counts are exact.  The mean
is the same sum in the same order; the sd sums the same deviations, but the device may fuse a square into the sum: for |x| <= 1e3 and
K <= 20, |mean - host| <= 1e-11 max(1, host) and |sd - host| <= 1e-10.  K copies of one model: sd <= 1e-12 and |mean - d| <= 2 ulp; K = 1:
mean = d bit for bit and sd = 0.  The matrices equal their transposes bit for bit; two calls return equal bits.  The Spearman coefficients
are compared with the restatement's over the maps the DEVICE returned (so that no tie group hangs on a last bit of a mean; the maps
themselves are held to the host above): sums of at most 257^2 centred-rank products in another order, tolerance 1e-10.  n2049 keeps that
tolerance: its sums have T = 4.2e6 terms, whose worst case T 2^-53 = 4.7e-10 is above it and whose expected gap sqrt(T) 2^-53 = 2e-13 is far
below; the gaps printed on an MI355X are 1.7e-15 (mean) and 4.2e-16 (contact), and the n2049 maps differ from the host's by 0 (mean, bits
equal) and 2.8e-14 (sd)."""
import os
import subprocess

import numpy as np
import pytest

from tests import ensemble_ref as R
from tests.util import GOLD, SHORT, load_pdb_xyz, random_coil, restrained, shared_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["n64", "n65", "n130", "n257", "k17", "lattice", "n2049"]
PICK257 = [6, 4, 2, 2, 0]
CUTOFF = {"lattice": 3.0}                                                       # an integer: pairs at exactly the cutoff are no contact


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _models(name):
    """(replica coordinates [M, n, 3] float32, extra models [E, n, 3] float64 or None)"""
    if name in ("n64", "n65", "n130", "n92", "n95", "n2049"):
        n, M = {"n64": (64, 3), "n65": (65, 2), "n130": (130, 4), "n92": (92, 2), "n95": (95, 2), "n2049": (2049, 3)}[name]
        return np.stack([random_coil(n, 10 * n + r) for r in range(M)]), None
    if name in ("n257", "k17"):
        return shared_models(name)
    rng = np.random.default_rng(130)
    a, b, c = (rng.integers(0, 6, size=(130, 3)) for _ in range(3))
    assert len(np.unique(a, axis=0)) < 130                                      # coincident beads
    return np.stack([a, a, b, c]).astype(np.float32), None


def _load(ctx, name):
    """the context holding the case's replicas; returns (extra, all K models as doubles)"""
    x, extra = _models(name)
    restrained(ctx, x.shape[1], x.shape[0])
    ctx.set_coords(x)
    return extra, [m.astype(np.float64) for m in x] + ([] if extra is None else list(extra))


_HOST = {}


def _host(name, models, pick, cutoff):
    """the restatement's maps, computed once per (case, pick) and left unchanged"""
    key = (name, None if pick is None else tuple(pick), cutoff)
    if key not in _HOST:
        out = R.ensemble_map(models, pick, cutoff)
        for a in out:
            a.setflags(write=False)
        _HOST[key] = out
    return _HOST[key]


def _check_maps(got, host, Kp, what):
    hmean, hsd, hcontact, hcount = host
    mean, sd, contact = got["mean"], got["sd"], got["contact"]
    n = len(hmean)
    emean, esd = (np.abs(mean - hmean) / np.maximum(1.0, hmean)).max(), np.abs(sd - hsd).max()
    bad = int((np.rint(contact * Kp).astype(np.int64) != hcount).sum())
    print(f"{what}: n {n}, Kp {Kp}, max |mean - host| / max(1, host) {emean:.3e}, max |sd - host| {esd:.3e}, contact counts off {bad}, "
          f"mean bits equal {np.array_equal(mean, hmean)}")
    assert mean.shape == sd.shape == contact.shape == (n, n)
    assert np.isfinite(mean).all() and np.isfinite(sd).all()
    assert bad == 0 and np.array_equal(contact, hcontact)                       # an exact count, divided once
    assert emean <= 1e-11, (what, emean)
    assert esd <= 1e-10, (what, esd)
    for M in (mean, sd, contact):
        assert np.array_equal(M, M.T), what                                     # bit for bit
    assert np.array_equal(np.diag(mean), np.zeros(n)) and np.array_equal(np.diag(sd), np.zeros(n)) and np.array_equal(np.diag(contact), np.ones(n))


def _if_matrix(n, seed):
    """a symmetric matrix of counts with ties, falling with the separation"""
    rng = np.random.default_rng(seed)
    i, j = np.indices((n, n))
    m = np.rint(300.0 / (1.0 + np.abs(i - j)) * rng.lognormal(sigma=0.5, size=(n, n)))
    m = np.triu(m) + np.triu(m, 1).T
    assert np.array_equal(m, m.T) and len(np.unique(m)) < n * n // 4
    return m


@pytest.mark.parametrize("name", CASES)
def test_maps_equal_the_restatement(ctx, name):
    """All three maps of all K models — and, at n = 257, of a reversed subset with one model twice — against numpy."""
    extra, models = _load(ctx, name)
    cutoff = CUTOFF.get(name, 7.6)
    got = ctx.ensemble_map(extra, cutoff=cutoff)
    _check_maps(got, _host(name, models, None, cutoff), len(models), name)
    assert 0.0 < got["contact"].mean() < 1.0                                    # the cutoff separates something
    if name == "n257":
        got = ctx.ensemble_map(extra, pick=PICK257, cutoff=cutoff)
        _check_maps(got, _host(name, models, PICK257, cutoff), len(PICK257), name + " picked")
        other = ctx.ensemble_map(extra, pick=[0, 2, 4, 6], cutoff=cutoff)
        assert np.abs(other["mean"] - got["mean"]).max() > 1e-3                 # the repeat counts


@pytest.mark.parametrize("K", [3, 7])
def test_copies_of_one_model_have_no_spread(ctx, K):
    x = random_coil(64, 77) * np.float32(25.0)
    restrained(ctx, 64, K)
    ctx.set_coords(np.stack([x] * K))
    got = ctx.ensemble_map(cutoff=60.0)
    d = R.distances(ctx.coords()[0])
    print(f"K {K}: max sd {got['sd'].max():.3e}, max |mean - d| in ulp {(np.abs(got['mean'] - d) / np.spacing(np.maximum(d, 1e-300))).max():.2f}")
    assert got["sd"].max() <= 1e-12
    assert (np.abs(got["mean"] - d) <= 2 * np.spacing(d)).all()
    assert np.array_equal(got["contact"], (d < 60.0).astype(np.float64))


def test_one_model_is_its_own_map_and_scores_as_its_distances(ctx):
    """K = 1 at n = 92: mean = d bit for bit, sd = 0 exactly, and rho_mean = Spearman(IF, exact distances) of the restatement."""
    x = random_coil(92, 920)
    restrained(ctx, 92, 1)
    ctx.set_coords(x[None])
    got = ctx.ensemble_map(cutoff=7.6)
    d = R.distances(x)
    assert np.array_equal(got["mean"], d) and np.array_equal(got["sd"], np.zeros_like(d))
    assert np.array_equal(got["contact"], (d < 7.6).astype(np.float64))
    IF = _if_matrix(92, 92)
    rho_mean, rho_contact = ctx.ensemble_score(IF, 3, cutoff=7.6)
    want = R.spearman(IF, d, 3)
    print(f"n 92, K 1: rho_mean {rho_mean:.12f}, restatement {want:.12f}")
    assert abs(rho_mean - want) <= 1e-10 and rho_mean < 0 < rho_contact
    assert abs(rho_contact - R.spearman(IF, (d < 7.6).astype(np.float64), 3)) <= 1e-10


def test_lattice_copies_are_exact(ctx):
    """pick = [0, 1], replica 1 a copy of replica 0: mean = d and sd = 0 exactly, every contact frequency 0 or 1."""
    _, models = _load(ctx, "lattice")
    got = ctx.ensemble_map(pick=[0, 1], cutoff=3.0)
    d = R.distances(models[0])
    assert np.array_equal(got["mean"], d) and np.array_equal(got["sd"], np.zeros_like(d))
    assert set(np.unique(got["contact"])) == {0.0, 1.0} and np.array_equal(got["contact"], (d < 3.0).astype(np.float64))
    assert (d == 3.0).any()                                                      # pairs at exactly the cutoff: strict <
    assert (d == 0.0).sum() > 130                                                # coincident beads: zeros off the diagonal


@pytest.mark.parametrize("name", ["n92", "n95", "n257", "n2049"])
def test_scores_equal_the_restatement_over_the_devices_maps(ctx, name):
    extra, models = _load(ctx, name)
    n = len(models[0])
    IF = _if_matrix(n, n)
    pick = PICK257 if name == "n257" else None
    maps = ctx.ensemble_map(extra, pick=pick, cutoff=7.6, sd=False)
    assert set(maps) == {"mean", "contact"}
    rho_mean, rho_contact = ctx.ensemble_score(IF, 3, extra, pick, 7.6)
    want = R.spearman(IF, maps["mean"], 3), R.spearman(IF, maps["contact"], 3)
    print(f"{name}: rho_mean {rho_mean:.12f} (restatement {want[0]:.12f}), rho_contact {rho_contact:.12f} ({want[1]:.12f}), "
          f"gaps {abs(rho_mean - want[0]):.2e} {abs(rho_contact - want[1]):.2e}")
    assert abs(rho_mean - want[0]) <= 1e-10 and abs(rho_contact - want[1]) <= 1e-10
    assert rho_mean < 0 < rho_contact
    only_mean = ctx.ensemble_score(IF, 3, extra, pick)                          # one output alone: the same bits
    assert only_mean == (rho_mean, None)
    from chromosome3d_amd import lib
    rc = np.zeros(1)
    assert ctx._L.c3d_ensemble_score(ctx._h, lib.dptr(IF), 3, lib.dptr(extra) if extra is not None else None, 0 if extra is None else len(extra),
                                     lib.i32ptr(np.array(pick, np.int32)) if pick else None, len(pick) if pick else 0, 7.6, None, lib.dptr(rc)) == 0
    assert rc[0] == rho_contact
    if name == "n92":
        other = ctx.ensemble_score(IF, 5, cutoff=7.6)                           # another range is another set of pairs
        assert abs(other[0] - R.spearman(IF, maps["mean"], 5)) <= 1e-10 and other[0] != rho_mean
        flat = ctx.ensemble_score(IF, 3, cutoff=1e5)                            # every pair in contact: a constant map
        assert np.isnan(flat[1]) and flat[0] == rho_mean


def test_f64_state_is_mapped_in_doubles():
    """A precision-64 context: the map is that of the fp64 state, not of its float mirror."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        restrained(s, 96, 3)
        rng = np.random.default_rng(96)
        x = np.stack([random_coil(96, 960 + r).astype(np.float64) for r in range(3)]) + rng.normal(scale=1e-3, size=(3, 96, 3))
        assert not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        s.set_coords64(x)
        x64 = s.coords64()
        assert np.array_equal(x64, x)
        got = s.ensemble_map(cutoff=7.6)
        _check_maps(got, R.ensemble_map(list(x64), None, 7.6), 3, "f64")
        rounded = R.ensemble_map(list(x64.astype(np.float32).astype(np.float64)), None, 7.6)
        # the float mirror would have given another map: rounding coordinates of 10 A to float moves them by up to 5e-7 A, the distances
        # with them; 1e-8 is a thousand times what the device may differ from the host by
        assert np.abs(got["mean"] - rounded[0]).max() > 1e-8 and np.abs(got["sd"] - rounded[1]).max() > 1e-8
        IF = _if_matrix(96, 96)
        rho = s.ensemble_score(IF, 3, cutoff=7.6)
        assert abs(rho[0] - R.spearman(IF, got["mean"], 3)) <= 1e-10 and abs(rho[1] - R.spearman(IF, got["contact"], 3)) <= 1e-10
    finally:
        s.close()


def test_two_calls_return_the_same_bytes_and_nothing_of_the_solve_changes(ctx):
    extra, _ = _load(ctx, "n257")
    IF = _if_matrix(257, 257)
    ctx.run_steps(20)                                                           # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    runs = ctx.stat("ensemble_map_runs"), ctx.stat("ensemble_score_runs")
    first, second = ctx.ensemble_map(extra, PICK257, 7.6), ctx.ensemble_map(extra, PICK257, 7.6)
    for k in ("mean", "sd", "contact"):
        assert first[k].tobytes() == second[k].tobytes()
    assert ctx.ensemble_score(IF, 3, extra, PICK257, 7.6) == ctx.ensemble_score(IF, 3, extra, PICK257, 7.6)
    assert (ctx.stat("ensemble_map_runs"), ctx.stat("ensemble_score_runs")) == (runs[0] + 2, runs[1] + 2)
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    only = ctx.ensemble_map(extra, PICK257, mean=False, sd=True)                # one output alone: the same bits
    assert set(only) == {"sd"} and only["sd"].tobytes() == first["sd"].tobytes()
    assert ctx.run_steps(5) == 5                                                # and the solve goes on


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name; none counts as a run; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    extra, models = _load(ctx, "n64")
    n, M = 64, 3
    L, h = ctx._L, ctx._h
    IF = _if_matrix(n, n)
    runs = ctx.stat("ensemble_map_runs"), ctx.stat("ensemble_score_runs")
    state = ctx.coords().tobytes()
    out, rho = np.empty((n, n)), np.empty(2)
    good = np.stack(models)
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows
    i32 = lambda v: lib.i32ptr(np.array(v, np.int32))
    o, r0, r1 = lib.dptr(out), lib.dptr(rho), lib.dptr(rho[1:])

    def refused(*a):                                                            # (extra, n_extra, pick, n_pick, cutoff) common to both entries
        assert L.c3d_ensemble_map(h, *a, o, None, None if a[4] == 7.6 else o) == -1 and b"c3d_ensemble_map" in L.c3d_last_error(), a
        assert L.c3d_ensemble_score(h, lib.dptr(IF), 3, *a, r0, None if a[4] == 7.6 else r1) == -1 and b"c3d_ensemble_score" in L.c3d_last_error(), a

    refused(lib.dptr(good), -1, None, 0, 7.6)                                   # n_extra < 0
    refused(None, 1, None, 0, 7.6)                                              # extras without coordinates
    refused(lib.dptr(big), len(big), None, 0, 7.6)                              # K = 257
    refused(None, 0, i32([0]), -1, 7.6)                                         # n_pick < 0
    refused(None, 0, None, 2, 7.6)                                              # a length without a list
    refused(None, 0, i32([0]), 0, 7.6)                                          # a list without a length
    refused(None, 0, i32([0, M]), 2, 7.6)                                       # an index outside 0..K-1
    refused(None, 0, i32([0, -1]), 2, 7.6)
    refused(None, 0, i32([0] * 4097), 4097, 7.6)                                # more than 4096 picks
    for bad in (0.0, -1.0, np.nan, np.inf):                                     # contact wanted, no usable cutoff
        refused(None, 0, None, 0, bad)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(lib.dptr(e), M, None, 0, 7.6)
    assert L.c3d_ensemble_map(h, None, 0, None, 0, 7.6, None, None, None) == -1 and b"c3d_ensemble_map" in L.c3d_last_error()      # every output NULL
    assert L.c3d_ensemble_score(h, lib.dptr(IF), 3, None, 0, None, 0, 7.6, None, None) == -1 and b"c3d_ensemble_score" in L.c3d_last_error()
    assert L.c3d_ensemble_score(h, None, 3, None, 0, None, 0, 7.6, r0, r1) == -1                                                    # no matrix
    for rng in (0, -3, n):                                                      # range < 1, or one that leaves no pairs
        assert L.c3d_ensemble_score(h, lib.dptr(IF), rng, None, 0, None, 0, 7.6, r0, r1) == -1 and b"c3d_ensemble_score" in L.c3d_last_error()
    skew = IF.copy()
    skew[5, 40] += 1.0
    assert L.c3d_ensemble_score(h, lib.dptr(skew), 3, None, 0, None, 0, 7.6, r0, r1) == -1 and b"not symmetric over the ranked pairs" in L.c3d_last_error()
    skew = IF.copy()
    skew[5, 6] += 1.0                                                           # inside the band: not a ranked pair
    assert L.c3d_ensemble_score(h, lib.dptr(skew), 3, None, 0, None, 0, 7.6, r0, r1) == 0
    assert (ctx.stat("ensemble_map_runs"), ctx.stat("ensemble_score_runs")) == (runs[0], runs[1] + 1)
    assert ctx.coords().tobytes() == state
    # 4096 picks and 256 models are accepted; a mean needs no cutoff
    got = ctx.ensemble_map(pick=[1] * 4096, sd=False)
    d1 = R.distances(models[1])                                                 # 4096 equal terms added one by one: 4096 2^-53 = 4.6e-13 relative
    assert set(got) == {"mean"} and (np.abs(got["mean"] - d1) <= 1e-12 * np.maximum(1.0, d1)).all()
    got = ctx.ensemble_map(big[:-1] + good[0], pick=[0, 255], sd=True)
    assert np.array_equal(got["mean"], R.distances(models[0])) and not got["sd"].any()
    _check_maps(ctx.ensemble_map(cutoff=7.6), _host("n64", models, None, 7.6), M, "n64 after the refusals")
    # no replicas; fewer than 2 beads cannot be set up at all, 2 beads are one pair
    s = Solver(0)
    try:
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        for call in (s.ensemble_map, lambda: s.ensemble_score(np.ones((2, 2)), 1)):
            with pytest.raises(C3DError, match="c3d_ensemble_(map|score).*c3d_init_replicas"):
                call()
        s.init_replicas(2)
        two = s.ensemble_map(cutoff=1e3)
        d = R.ensemble_map([m.astype(np.float64) for m in s.coords()], None, 1e3)
        assert np.array_equal(two["mean"], d[0]) and np.array_equal(two["contact"], np.ones((2, 2)))
        assert s.stat("ensemble_map_runs") == 1 and s.stat("ensemble_score_runs") == 0
    finally:
        s.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --ensemble on the smallest bundled matrix: three maps that c3d_parse_if_file reads back, the score line, and a mean map
    that is Solver.ensemble_map's of the written models to the printed digits.  The written coordinates are rounded to 3 decimals (each
    component of a difference moves by at most 1e-3, a distance by at most sqrt(3) 1e-3) and so is the printed mean (5e-4): 2.3e-3."""
    from chromosome3d_amd import pipeline
    cid, M = "chr21_1mb", 4
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "ens")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--ensemble", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    line = [l for l in run.stdout.splitlines() if l.startswith("ensemble: ")]
    assert len(line) == 1 and line[0].startswith(f"ensemble: {M} models, Spearman(IF, mean d) = -0.") and "Spearman(IF, contact) = 0." in line[0], run.stdout
    maps = {k: pipeline.parse_if_file(f"{prefix}_{k}.txt") for k in ("mean", "sd", "contact")}
    for k, m in maps.items():
        assert m.shape == (37, 37), k
        rows = open(f"{prefix}_{k}.txt").read().split("\n")
        assert len(rows) == 38 and rows[-1] == "" and all(len(r.split(" ")) == 37 for r in rows[:-1])     # n lines of n numbers, single spaces
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r + 1}.pdb") for r in range(M)])
    restrained(ctx, 37, M)
    ctx.set_coords(x)
    got = ctx.ensemble_map(cutoff=2 * 3.8)
    gap = np.abs(maps["mean"] - got["mean"]).max()
    print(f"{line[0]}; max |file - ensemble_map of the written models| {gap:.2e}")
    assert gap <= 2.3e-3 and np.abs(maps["sd"] - got["sd"]).max() <= 2.3e-3
    assert np.array_equal(np.diag(maps["contact"]), np.ones(37)) and set(np.unique(maps["contact"])) <= {0.0, 0.25, 0.5, 0.75, 1.0}
    top = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", str(M), "--quiet", "--ensemble", str(tmp_path / "top"),
                          "--ensemble-top", "2", "--ensemble-cutoff", "0"], capture_output=True, text=True)
    assert top.returncode == 0 and "ensemble: 2 models" in top.stdout, top.stderr
    assert os.path.exists(tmp_path / "top_mean.txt") and not os.path.exists(tmp_path / "top_contact.txt")
