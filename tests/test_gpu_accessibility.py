"""Bead accessibility on the device (c3d_accessibility; csrc/c3d_score_access.inc k_access) against the numpy restatement
tests/accessibility_ref.py, which tests/test_accessibility_ref.py holds to the analytic cap of two spheres and to its own brute walk.

The kernel's constants: a workgroup of 256 threads owns a tile of 16 beads of one model and walks the model's columns in super-blocks of
1024 beads; per super-block it lists every row's neighbours (16-bit offsets, a list of 1024 a row) and tests the row's points against the
list, sixteen threads a row, point p on thread p mod 16, bit p div 16 of a 64-bit mask.
  borders   n = 2, 3 (a tile of two and three rows), 15, 16, 17 (the tile's edge), 63, 65, 131 (several tiles, a ragged last one), 1023, 1025
            (the super-block's edge from both sides), 1100 and 2052 (two and three super-blocks), one to three models, coils or relaxed
  points    P = 1 (fifteen idle threads a row), 63, 64, 65 (bits 3 and 4 of the mask), 256, 1024 (all 64 bits) at n = 131
  dense     1100 beads within 2 R of one another: every list full in both super-blocks
  tangent   three beads, the second at 2 R (1 +- 2^-k) u_p from the first: the cases that tell a tight neighbour bound from a loose one
  large     16384 beads x 1 model, 64 sampled rows: 1024 tiles, 16 super-blocks, the index arithmetic

Bounds.  exposed is an integer count that depends on no order: every comparison is ==, against the restatement fed the library's own points
(c3d_sphere_points), so that no libm difference enters.  The restatement walks every j (brute) up to 131 beads, in the dense case and in the
tangent table; beyond it leaves out beads a whole Angstrom further than any that can matter (tests/accessibility_ref.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import accessibility_ref as A
from tests.util import GOLD, SHORT, load_if, load_pdb_xyz, model_pdb, random_coil, restrained, shared_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADIUS = PROBE = 1.965                                                          # touching beads at the default bond length 3.93 A
R = RADIUS + PROBE


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _points(P):
    """the library's own lattice: what NULL points mean, and what the restatement is fed"""
    from chromosome3d_amd import lib
    u = np.empty((P, 3))
    assert lib.load().c3d_sphere_points(P, lib.dptr(u)) == 0
    u.setflags(write=False)
    return u


def _host(models, u, radius=RADIUS, probe=PROBE, rows=None, brute=False):
    return np.stack([A.exposed(m, u, radius, probe, rows, brute) for m in models])


def _state(ctx):
    return [m.astype(np.float64) for m in ctx.coords()]


@pytest.mark.parametrize("n,nrep,relaxed", [(2, 3, False), (3, 2, True), (15, 3, False), (16, 3, True), (17, 3, False), (63, 2, True), (65, 3, False), (131, 3, True),
                                            (1023, 2, False), (1025, 2, True), (1100, 1, False), (2052, 3, False)])
def test_tile_and_super_block_borders(ctx, n, nrep, relaxed):
    restrained(ctx, n, nrep)
    ctx.set_coords(np.stack([random_coil(n, 100 * n + r) for r in range(nrep)]))
    if relaxed:
        ctx.run()                                                               # the 45 steps of SHORT: a model the solver left, not a coil
    got = ctx.accessibility(None, RADIUS, PROBE, 96)
    want = _host(_state(ctx), _points(96), brute=n <= 131)
    assert got["exposed"].dtype == np.int32 and got["exposed"].shape == (nrep, n)
    print(f"n = {n} x {nrep}{' relaxed' if relaxed else ''}: exposed {want.min()}..{want.max()} of 96, beads with none {(want == 0).sum()}, device {got['device_ms']:.3f} ms")
    assert np.array_equal(got["exposed"], want)
    assert np.array_equal(got["fraction"], want / 96.0) and np.array_equal(got["area"], 4.0 * np.pi * R ** 2 * (want / 96.0))
    assert got["model_area"].shape == (nrep,) and got["mean_fraction"].shape == (n,) and got["device_ms"] > 0
    if n >= 15:
        assert want.min() < want.max()                                          # a track, not a constant


@pytest.mark.parametrize("P", [1, 63, 64, 65, 256, 1024])
def test_point_loop_borders(ctx, P):
    n = 131
    restrained(ctx, n, 2)
    ctx.set_coords(np.stack([random_coil(n, 1310 + r) for r in range(2)]))
    got = ctx.accessibility(None, RADIUS, PROBE, P)
    want = _host(_state(ctx), _points(P), brute=True)
    print(f"P = {P}: exposed {want.min()}..{want.max()}")
    assert np.array_equal(got["exposed"], want) and want.max() <= P and (P == 1 or want.min() < want.max())


def test_lists_full_in_both_super_blocks(ctx):
    """The 1100-bead coil scaled by 0.01: every bead within 2 R of every bead, so a row's list takes all 1024 columns of the first
    super-block and all 76 of the second."""
    n = 1100
    restrained(ctx, n, 1)
    ctx.set_coords((random_coil(n, 11000) * np.float32(0.01))[None])
    x = _state(ctx)[0]
    assert np.linalg.norm(x[:, None, :] - x[None, :, :], axis=-1).max() < 2.0 * R
    got = ctx.accessibility(None, RADIUS, PROBE, 96)
    want = _host([x], _points(96), brute=True)
    print(f"dense: exposed {want.min()}..{want.max()}, beads with any {(want > 0).sum()}")
    assert np.array_equal(got["exposed"], want) and 0 < (want > 0).sum() < n // 4


def test_the_tangent_table(ctx):
    """108 models of three beads as extra models of one call.  The restatement must see both outcomes — a buried point and none — or the
    table decides nothing; the device must then agree case by case."""
    u = _points(96)
    models, labels = A.tangent_table(RADIUS, PROBE, u)
    want = _host(list(models), u, brute=True)
    hit = want[:, 0] < 96
    print(f"tangent table: {int(hit.sum())} cases with a buried point, {int((~hit).sum())} without")
    assert len(models) == 108 and hit.any() and (~hit).any()
    restrained(ctx, 3, 1)
    got = ctx.accessibility(models, RADIUS, PROBE, 96)
    assert np.array_equal(got["exposed"][1:], want), [l for l, a, b in zip(labels, got["exposed"][1:], want) if not np.array_equal(a, b)]


def test_replicas_and_extra_models(ctx):
    x, extra = shared_models("n257")
    restrained(ctx, 257, 3)
    ctx.set_coords(x[:3])
    got = ctx.accessibility(extra, RADIUS, PROBE, 96)
    want = _host(_state(ctx) + list(extra), _points(96))
    assert got["exposed"].shape == (5, 257) and np.array_equal(got["exposed"], want)
    alone = ctx.accessibility(None, RADIUS, PROBE, 96)                          # without the extra models: the replicas keep their bytes
    assert alone["exposed"].tobytes() == got["exposed"][:3].tobytes()
    # the defaults: half the model's bond length each, the lattice of 96 points
    b0 = ctx.b0
    assert abs(b0 - 3.93) < 1e-6
    dflt = ctx.accessibility(extra)
    assert np.array_equal(dflt["exposed"], _host(_state(ctx) + list(extra), _points(96), 0.5 * b0, 0.5 * b0))
    # another radius and another probe, as two arguments and as their sum in either
    wide = ctx.accessibility(extra, 2.5, 3.0, 96)
    assert np.array_equal(wide["exposed"], _host(_state(ctx) + list(extra), _points(96), 2.5, 3.0))
    assert not np.array_equal(wide["exposed"], got["exposed"])
    from chromosome3d_amd import pipeline
    rep = pipeline.accessibility_report(ctx, extra, RADIUS, PROBE, 96)
    assert np.array_equal(rep["exposed"], want) and (rep["radius"], rep["probe"], rep["points"]) == (RADIUS, PROBE, 96)
    assert np.array_equal(rep["buried"], (want == 0).sum(axis=1))


def test_f64_state_is_measured_in_doubles():
    """A precision-64 context: the counts follow the fp64 state, not its float rounding.  Coordinates near 9000 A, where a float's last
    place is 1e-3 A: rounding them to float moves a bead by up to 8e-4 A, and of the 2 x 96 x 1024 points some lie that close to a sphere."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        n = 96
        restrained(s, n, 2)
        rng = np.random.default_rng(96)
        x = np.stack([random_coil(n, 960 + r).astype(np.float64) + 9000.0 for r in range(2)]) + rng.normal(scale=1e-3, size=(2, n, 3))
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x) and not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        got = s.accessibility(None, RADIUS, PROBE, 1024)
        assert np.array_equal(got["exposed"], _host(list(x), _points(1024), brute=True))
        rounded = _host(list(x.astype(np.float32).astype(np.float64)), _points(1024), brute=True)
        assert not np.array_equal(got["exposed"], rounded)
    finally:
        s.close()


@pytest.mark.parametrize("cid", ["chr21_1mb", "chr1_500kb"])
def test_the_bundled_models(ctx, cid):
    """The reference's own models as extra models of a context that holds the matrix: the track is not trivial — 21 to 77 exposed points a
    bead on chr21_1mb; 160 of 455 beads with none and one with all 96 on chr1_500kb."""
    from chromosome3d_amd import default_model, make_stages
    IF = load_if(cid)
    bundled = load_pdb_xyz(model_pdb(cid))
    ctx.set_model(default_model())
    ctx.set_schedule(make_stages(SHORT))
    ctx.set_if_matrix(IF)
    ctx.init_replicas(2)
    want = _host(_state(ctx) + [bundled], _points(96), brute=True)
    got = ctx.accessibility(bundled, RADIUS, PROBE, 96)
    assert np.array_equal(got["exposed"], want)
    e = want[2]
    if cid == "chr21_1mb":
        assert len(e) == 37 and (e.min(), e.max()) == (21, 77)
    else:
        assert len(e) == 455 and (e == 0).sum() == 160 and (e == 96).sum() == 1


def test_points_from_the_caller(ctx):
    n = 131
    restrained(ctx, n, 2)
    ctx.set_coords(np.stack([random_coil(n, 1310 + r) for r in range(2)]))
    models = _state(ctx)
    u = _points(96)
    a, b = 0.7, -1.9                                                            # a rotation about z, then about x
    rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    turned = np.ascontiguousarray(u @ (rx @ rz).T)
    assert np.abs((turned * turned).sum(axis=1) - 1.0).max() < 1e-14
    got = ctx.accessibility(None, RADIUS, PROBE, points=turned)
    want = _host(models, turned, brute=True)
    assert np.array_equal(got["exposed"], want)
    null = ctx.accessibility(None, RADIUS, PROBE, 96)
    given = ctx.accessibility(None, RADIUS, PROBE, points=u)
    assert np.array_equal(null["exposed"], _host(models, u, brute=True)) and null["exposed"].tobytes() == given["exposed"].tobytes()
    assert not np.array_equal(null["exposed"], want)                            # another lattice, other integers
    few = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [0.6, 0.0, 0.8]])        # any unit vectors will do
    assert np.array_equal(ctx.accessibility(None, RADIUS, PROBE, points=few)["exposed"], _host(models, few, brute=True))


def _begin(ctx, x):
    restrained(ctx, 257, 5)
    ctx.set_coords(x)


def test_two_calls_return_the_same_bytes_and_nothing_of_the_solve_changes(ctx):
    x, extra = shared_models("n257")
    _begin(ctx, x)
    assert ctx.run_steps(20) == 20 and ctx.run_steps(15) == 15                  # an uninterrupted run
    plain = (ctx.coords().tobytes(), ctx.velocities().tobytes())
    _begin(ctx, x)
    assert ctx.run_steps(20) == 20                                              # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    a, b = ctx.accessibility(extra, RADIUS, PROBE, 96), ctx.accessibility(extra, RADIUS, PROBE, 96)
    assert a["exposed"].tobytes() == b["exposed"].tobytes()
    assert np.array_equal(a["exposed"], _host([m.astype(np.float64) for m in before[0]] + list(extra), _points(96)))
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    assert ctx.run_steps(15) == 15                                              # and the solve goes on, to the bits of the uninterrupted run
    assert (ctx.coords().tobytes(), ctx.velocities().tobytes()) == plain


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list (n < 2 aside: no context holds fewer than two beads) is C3D_ERR_INVALID with the function's name and
    writes nothing; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    n, M = 64, 2
    restrained(ctx, n, M)
    x = np.stack([random_coil(n, 640 + r) for r in range(M)])
    ctx.set_coords(x)
    L, h = ctx._L, ctx._h
    state = ctx.coords().tobytes()
    good = x.astype(np.float64)
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows
    u = np.array(_points(96))

    def refused(extra, n_extra, radius, probe, points, P, null_out=False):
        out, ms = np.full((300, n), 7, np.int32), C.c_double(7.0)
        rc = L.c3d_accessibility(h, lib.dptr(extra) if extra is not None else None, n_extra, radius, probe, lib.dptr(points) if points is not None else None, P,
                                 None if null_out else lib.i32ptr(out), C.byref(ms))
        assert rc == -1 and b"c3d_accessibility" in L.c3d_last_error(), (n_extra, radius, probe, P)
        assert (out == 7).all() and ms.value == 7.0                             # nothing written

    refused(None, 0, RADIUS, PROBE, None, 96, null_out=True)                    # exposed NULL
    for P in (0, -3, 1025):                                                     # n_points outside 1..C3D_ACCESS_MAX_POINTS
        refused(None, 0, RADIUS, PROBE, None, P)
        refused(None, 0, RADIUS, PROBE, u, P)
    for bad in (0.0, -1.0, np.nan, np.inf):                                     # radius not finite or <= 0
        refused(None, 0, bad, PROBE, None, 96)
    for bad in (-1e-9, np.nan, np.inf, -np.inf):                                # probe not finite or < 0
        refused(None, 0, RADIUS, bad, None, 96)
    refused(None, 0, 0.004, 0.005, None, 96)                                    # radius + probe outside [0.01, 1e5]
    refused(None, 0, 6e4, 5e4, None, 96)
    for bad, at in ((np.nan, 0), (np.inf, 1), (1.0 + 1e-8, 2)):                 # a bad point: not finite, or off the sphere
        e = u.copy()
        e[40, at] = bad
        refused(None, 0, RADIUS, PROBE, e, 96)
    refused(None, 0, RADIUS, PROBE, u * np.sqrt(1.0 + 2e-9), 96)                # squared norm 1 + 2e-9
    refused(None, 0, RADIUS, PROBE, u * np.sqrt(1.0 - 2e-9), 96)
    refused(None, 1, RADIUS, PROBE, None, 96)                                   # n_extra > 0 without coordinates
    refused(good, -1, RADIUS, PROBE, None, 96)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(e, M, RADIUS, PROBE, None, 96)
    refused(big, len(big), RADIUS, PROBE, None, 96)                             # K = 257
    assert ctx.coords().tobytes() == state
    # found by the pass: a replica outside |x| < 1e6, the limit of the extra models and of the neighbour bound's proof
    far = x.copy()
    far[1, 5, 0] = 2e6
    ctx.set_coords(far)
    refused(None, 0, RADIUS, PROBE, None, 96)
    assert b"1e6" in L.c3d_last_error()
    ctx.set_coords(x)
    # what is accepted: the limits themselves, 256 models, a probe of 0, points a hair off the sphere — and the context works
    got = ctx.accessibility(big[:-1] + good[0], RADIUS, PROBE, 96)
    want = _host(list(good), u, brute=True)
    assert np.array_equal(got["exposed"][:M], want) and got["exposed"][255].tobytes() == got["exposed"][0].tobytes()
    assert np.array_equal(ctx.accessibility(None, R, 0.0, 96)["exposed"], _host(list(good), u, R, 0.0, brute=True))
    assert np.array_equal(ctx.accessibility(None, 0.005, 0.005, 96)["exposed"], _host(list(good), u, 0.005, 0.005, brute=True))
    assert np.array_equal(ctx.accessibility(None, 5e4, 5e4, 96)["exposed"], _host(list(good), u, 5e4, 5e4, brute=True))
    inside = u * np.sqrt(1.0 - 5e-10)
    assert np.array_equal(ctx.accessibility(None, RADIUS, PROBE, points=inside)["exposed"], _host(list(good), inside, brute=True))
    out = np.full((M, n), 7, np.int32)                                          # device_ms is optional
    assert L.c3d_accessibility(h, None, 0, RADIUS, PROBE, None, 96, lib.i32ptr(out), None) == 0 and np.array_equal(out, want)
    # a twin: a second bead at the same coordinates buries, the bead itself does not
    twin = good[:1].copy()
    twin[0, 1] = twin[0, 0]
    assert np.array_equal(ctx.accessibility(twin, RADIUS, PROBE, points=inside)["exposed"][M:], _host(list(twin), inside, brute=True))
    assert _host(list(twin), inside, brute=True)[0, 0] == 0
    # no replicas; 2 beads
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_accessibility.*c3d_init_replicas"):
            s2.accessibility()
        s2.init_replicas(2)
        two = s2.accessibility(None, RADIUS, PROBE, 96)
        assert np.array_equal(two["exposed"], _host(_state(s2), u, brute=True))
    finally:
        s2.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --accessibility on the smallest bundled matrix: rows 1..37, 2 + M columns, the header's R, P and areas, and counts that are
    Solver.accessibility's of the written models.  A written coordinate is rounded to 3 decimals, so a point and a bead both move by at most
    sqrt(3) 5e-4 A and their distance by at most 1.74e-3 A: a point of the written model whose distance to its nearest other bead differs
    from R by more than 4e-3 A has the fate it had in the run.  Per bead the file's count therefore differs from the written model's by at
    most the number of its points within that margin — for most beads none."""
    cid, M, n, P = "chr21_1mb", 4, 37, 96
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "acc")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--accessibility", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = open(prefix + "_accessibility.txt").read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split() for l in lines if not l.startswith("#")]
    assert head and lines[:len(head)] == head
    order = [int(v) for v in next(l for l in head if l.startswith("# models:")).split()[2:]]
    assert sorted(order) == [1, 2, 3, 4]
    assert [int(r[0]) for r in rows] == list(range(1, n + 1)) and all(len(r) == 2 + M and all(len(v.split(".")[1]) == 4 for v in r[1:]) for r in rows)
    count = np.array([[int(round(float(v) * P)) for v in r[2:]] for r in rows]).T          # [M, n] in rank order: 1 / 96 is a hundred times the print's last place
    assert np.abs(count / P - np.array([[float(v) for v in r[2:]] for r in rows]).T).max() <= 5.000001e-5
    assert np.abs(count.mean(axis=0) / P - np.array([float(r[1]) for r in rows])).max() <= 5.000001e-5
    about = next(l for l in head if l.startswith("# R = "))
    assert about.startswith("# R = 3.93 A (bead radius 1.965 + probe radius 1.965), P = 96 points")
    areas = [float(v) for v in about.split(":")[1].split()]
    assert len(areas) == M and np.abs(np.array(areas) - 4.0 * np.pi * 3.93 ** 2 * count.sum(axis=1) / P).max() <= 0.0500001 + 1e-3
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r}.pdb") for r in order])
    restrained(ctx, n, M)
    ctx.set_coords(x)
    b0 = ctx.b0
    got = ctx.accessibility(None, 0.5 * b0, 0.5 * b0, P)["exposed"]
    xs = _state(ctx)
    Rd = 0.5 * b0 + 0.5 * b0
    exact = 0
    for k in range(M):
        c = xs[k][:, None, :] + Rd * _points(P)[None, :, :]                     # [n, P, 3]
        d = np.linalg.norm(c[:, :, None, :] - xs[k][None, None, :, :], axis=-1)  # [n, P, n]
        d[np.arange(n), :, np.arange(n)] = np.inf
        unsure = (np.abs(d.min(axis=2) - Rd) <= 4e-3).sum(axis=1)
        assert (np.abs(count[k] - got[k]) <= unsure).all(), (k, count[k], got[k], unsure)
        exact += int((unsure == 0).sum())
        assert np.array_equal(count[k][unsure == 0], got[k][unsure == 0])
    print(f"beads whose count is the written model's for certain: {exact} of {M * n}")
    assert exact > M * n // 2
    other = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", "2", "--quiet", "--accessibility", str(tmp_path / "o"), "--bead-radius", "2.5",
                            "--probe-radius", "0", "--sphere-points", "64"], capture_output=True, text=True)
    assert other.returncode == 0, other.stderr
    assert "# R = 2.5 A (bead radius 2.5 + probe radius 0), P = 64 points" in open(tmp_path / "o_accessibility.txt").read()


def test_the_index_arithmetic_at_16384_beads():
    """16384 beads x 1 model, the context made the way tests/test_gpu_bead.py makes its largest: 1024 tiles and 16 super-blocks.  64 sampled
    rows — the first and last of the model, of a tile and of a super-block among them — against the restatement."""
    from chromosome3d_amd import Solver, default_model, make_stages
    n = 16384
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(n, np.array([1, 1, 8001], np.int32), np.array([11, 16384, 16384], np.int32), np.array([100, 457, 300], np.int32))
        s.init_replicas(1, 82364, 0)
        s.set_coords(random_coil(n, 16384)[None])
        x = s.coords()[0].astype(np.float64)
        rows = np.unique(np.concatenate([[0, 15, 16, 1023, 1024, 1025, 8191, 8192, 16367, 16368, 16383], np.random.default_rng(16384).integers(0, n, 53)]))
        got = s.accessibility(None, RADIUS, PROBE, 96)
        want = A.exposed(x, _points(96), RADIUS, PROBE, rows)
        print(f"n = 16384: {len(rows)} rows, exposed {want.min()}..{want.max()}, device {got['device_ms']:.3f} ms")
        assert got["exposed"].shape == (1, n) and np.array_equal(got["exposed"][0, rows], want) and want.min() < want.max()
        assert 0 <= got["exposed"].min() and got["exposed"].max() <= 96
    finally:
        s.close()
