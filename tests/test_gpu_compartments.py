"""Compartment eigenvectors on the device (c3d_compartments; csrc/c3d_score_compartment.inc k_cpt_*) against the numpy restatement
tests/compartment_ref.py, which tests/test_compartment_ref.py holds to numpy.linalg.eigh of numpy.corrcoef.

The kernels' constants: the product kernel's workgroup owns kCptRows = 8 rows and, where n is even, a thread takes column pairs in steps of
512 columns (16-byte loads), where n is odd single columns in steps of 256; the O/E map is built in 64 x 64 tiles; every other kernel walks
its entries in steps of 256; maps run in batches of floor(2^30 / 8 n^2) X slots (C3D_SCORE_SCRATCH_BYTES), one at least.
  borders   n = 3, 4, 5; 7, 8, 9 (the row tile); 63, 64, 65 (the build tile); 255, 256, 257; 455; 510, 511, 512, 513, 514 (the pair step from
            both sides, both parities); 1025; 2052; one to three models, planted (tests/compartment_ref.planted_model) as set or relaxed
            by the 45 steps of a short schedule; n_vec 1, 2, 3; iters 0, 1, 3, 200; min_sep 1, 3; with and without the consensus
  batches   2052 beads, 33 maps of 31 slots: the second batch returns the bytes of the first
  large     16384 beads x 1 model, n_vec 1, iters 2: one slot of 2 GiB, byte offsets up to 2^31

Bounds.  expected: T 2^-53 relative, T = n - s the terms of the sum.  vectors: with g the largest lambda_{a+1} / lambda_a among the requested
vectors (numpy.linalg.eigh, asserted <= 0.9), B = 64 n 2^-53 / (1 - g) per entry where the restatement's residuals are below 1e-9 and
B sqrt(n) for a run stopped earlier.  What follows from a vector perturbed by d, |d| <= e = sqrt(n) B': share (lambda / live, lambda <= live)
by 2 e; residual by 2 lambda_1 e; |Pearson r| of vectors x, y by 2 e (1 / |x_c| + 1 / |y_c|), x_c the centred vector.  same_side: exact over
the beads where both entries are further from 0 than B', so the counts differ by at most the number of the others."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import compartment_ref as R
from tests.util import GOLD, SHORT, load_if, load_pdb_xyz, model_pdb, restrained

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _planted(n, r, min_sep=1, nv=3):
    """the first planted model of bead count n (seed 10 r, 10 r + 1, ...) whose map has g <= 0.85 for nv vectors: chosen from eigh, not from the device"""
    for seed in range(10 * r, 10 * r + 10):
        x = R.planted_model(n, seed)
        if R.gap_ratio(R.distance_map(x), min_sep, nv) <= 0.85:
            return x
    raise AssertionError(f"no planted model of {n} beads with separated eigenvalues")


def _state(ctx):
    return [m.astype(np.float64) for m in ctx.coords()]


def _maps(models, IF, pick, consensus):
    order = list(range(len(models))) if pick is None else list(pick)
    maps = ([np.asarray(IF, dtype=np.float64)] if IF is not None else []) + [R.distance_map(models[k]) for k in order]
    if consensus:
        maps.append(R.consensus_map([models[k] for k in order]))
    return maps


def _check(got, maps, has_if, min_sep, nv, iters, start=None, what=""):
    """every output of a call against the restatement, to the bounds of the module's docstring; returns the restatement's dict"""
    n, Q = len(maps[0]), len(maps)
    want = R.compartments(maps, has_if, min_sep, nv, iters, start)
    assert got["expected"].shape == (Q, n) and got["vectors"].shape == (Q, nv, n) and got["share"].shape == got["residual"].shape == (Q, nv)
    worst = 0.0
    for q, M in enumerate(maps):
        g = R.gap_ratio(M, min_sep, nv)
        assert g <= 0.9, (what, q, g)
        B = 64.0 * n * U / (1.0 - g)
        Bq = B if (want["residual"][q] < 1e-9).all() else B * np.sqrt(n)
        e = np.sqrt(n) * Bq
        T = np.arange(n, 0, -1).astype(np.float64)
        rel = np.abs(got["expected"][q] - want["expected"][q]) / np.where(want["expected"][q] != 0.0, np.abs(want["expected"][q]), 1.0)
        assert got["expected"][q, 0] == 0.0 and (rel <= T * U).all(), (what, q, float((rel / (T * U)).max()))
        dv = float(np.abs(got["vectors"][q] - want["vectors"][q]).max())
        ds = float(np.abs(got["share"][q] - want["share"][q]).max())
        dr = float(np.abs(got["residual"][q] - want["residual"][q]).max())
        lam1 = float(want["share"][q, 0]) * n
        print(f"{what} map {q}: g {g:.3f} bound {Bq:.2e} vectors {dv:.2e} ({dv / Bq:.3f} of it) share {ds:.2e} residual {dr:.2e} (restatement's {want['residual'][q].max():.2e})")
        assert dv <= Bq and ds <= 2.0 * e and dr <= 2.0 * lam1 * e, (what, q)
        assert np.abs(np.einsum("aj,bj->ab", got["vectors"][q], got["vectors"][q]) - np.eye(nv)).max() <= 64.0 * n * U
        worst = max(worst, dv / Bq)
        if has_if and q > 0:
            F = want["vectors"][0]
            for a in range(nv):
                for b in range(nv):
                    xc, yc = want["vectors"][q, a] - want["vectors"][q, a].mean(), F[b] - F[b].mean()
                    tol = 2.0 * e * (1.0 / np.linalg.norm(xc) + 1.0 / np.linalg.norm(yc))
                    assert abs(got["agreement"][q - 1, a, b] - want["agreement"][q - 1, a, b]) <= tol, (what, q, a, b)
                unsure = int(((np.abs(want["vectors"][q, a]) <= Bq) | (np.abs(F[a]) <= Bq)).sum())
                assert abs(got["same_side"][q - 1, a] * n - want["same_side"][q - 1, a] * n) <= unsure + 1e-9, (what, q, a, unsure)
    want["worst"] = worst
    return want


BORDERS = [(3, 1, False, 2, 200, 1), (4, 2, False, 3, 200, 1), (5, 3, False, 3, 3, 1), (7, 1, False, 3, 200, 1), (8, 2, False, 1, 1, 1), (9, 1, False, 2, 0, 1),
           (63, 2, True, 1, 200, 1), (64, 1, False, 3, 200, 3), (65, 2, True, 1, 200, 1), (255, 2, False, 3, 200, 3), (256, 3, True, 1, 3, 1), (257, 1, False, 2, 200, 1),
           (455, 2, False, 3, 200, 1), (510, 1, False, 1, 0, 3), (511, 1, False, 2, 1, 1), (512, 1, False, 3, 200, 1), (513, 2, False, 3, 3, 3), (514, 1, False, 1, 200, 1),
           (1025, 1, True, 1, 200, 3), (2052, 2, False, 3, 200, 1)]


@pytest.mark.parametrize("n,nrep,relaxed,nv,iters,min_sep", BORDERS)
def test_tile_and_step_borders(ctx, n, nrep, relaxed, nv, iters, min_sep):
    restrained(ctx, n, nrep)
    ctx.set_coords(np.stack([_planted(n, r, min_sep, nv) for r in range(nrep)]))
    if relaxed:
        ctx.run()                                                               # the 45 steps of SHORT: a model the solver left
    consensus = nrep >= 2
    got = ctx.compartments(None, None, None, consensus, min_sep, nv, iters)
    assert got["maps"] == ["model %d" % k for k in range(nrep)] + (["consensus"] if consensus else []) and got["device_ms"] > 0
    assert "agreement" not in got and "same_side" not in got
    _check(got, _maps(_state(ctx), None, None, consensus), False, min_sep, nv, iters, None, f"n = {n} x {nrep}{' relaxed' if relaxed else ''} nv {nv} iters {iters} min_sep {min_sep}")
    at = np.abs(got["vectors"]).argmax(axis=2)                                  # the first sign rule
    assert (np.take_along_axis(got["vectors"], at[:, :, None], axis=2) > 0).all()


@pytest.mark.parametrize("cid", ["chr21_1mb", "chr1_500kb"])
def test_the_bundled_matrices_and_models(ctx, cid):
    """IF, two replicas (the bundled model scaled and jittered, so that their maps keep its separated eigenvalues), the bundled model as
    an extra model and the consensus of the three.  The consensus map is c3d_ensemble_map's mean bit for bit: given to a second call as
    its IF, that mean has the diagonal means the consensus had — the same reduction over the same doubles."""
    from chromosome3d_amd import default_model, make_stages
    IF = load_if(cid)
    bundled = load_pdb_xyz(model_pdb(cid))
    n = len(IF)
    ctx.set_model(default_model())
    ctx.set_schedule(make_stages(SHORT))
    ctx.set_if_matrix(IF)
    ctx.init_replicas(2)
    rng = np.random.default_rng(n)
    ctx.set_coords(np.stack([(bundled * (1.0 + 0.02 * (r + 1)) + rng.normal(scale=0.05, size=bundled.shape)).astype(np.float32) for r in range(2)]))
    models = _state(ctx) + [bundled]
    got = ctx.compartments(IF, bundled, None, True, 1, 3, 200)
    assert got["maps"] == ["IF", "model 0", "model 1", "model 2", "consensus"]
    want = _check(got, _maps(models, IF, None, True), True, 1, 3, 200, None, cid)
    print(cid, "shares", got["share"][:, 0], "agreement of PC1", got["agreement"][:, 0, 0], "same side", got["same_side"][:, 0])
    assert (got["vectors"][0, np.arange(3), np.abs(got["vectors"][0]).argmax(axis=1)] > 0).all()
    assert (np.einsum("qaj,aj->qa", got["vectors"][1:], got["vectors"][0]) >= 0).all()        # the second sign rule
    if cid == "chr1_500kb":
        assert abs(got["share"][0, 0] - 0.359) <= 0.002 and abs(got["share"][3, 0] - 0.385) <= 0.002
        assert abs(got["agreement"][2, 0, 0] - 0.931) <= 0.002
    mean = ctx.ensemble_map(bundled, None, None, True, False)["mean"]
    again = ctx.compartments(mean, bundled, [2], False, 1, 1, 0)
    assert again["expected"][0].tobytes() == got["expected"][4].tobytes()
    from chromosome3d_amd import pipeline
    rep = pipeline.compartment_report(ctx, IF, bundled, None, 1, 3, 200)
    assert rep["vectors"].tobytes() == got["vectors"].tobytes() and rep["converged"].all()
    assert np.array_equal(rep["calls"], np.sign(got["vectors"][:, 0, :]).astype(np.int8)) and rep["best"] == 1 + int(np.argmax(got["agreement"][:-1, 0, 0]))
    assert want["worst"] <= 1.0


def test_f64_state_is_read_in_doubles():
    """A precision-64 context whose state no float holds: coordinates near 9000 A, where a float's last place is 1e-3 A.  The diagonal
    means follow the doubles to T 2^-53 and are far from those of the state rounded to float."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        n = 96
        restrained(s, n, 2)
        rng = np.random.default_rng(96)
        x = np.stack([_planted(n, r).astype(np.float64) + 9000.0 for r in range(2)]) + rng.normal(scale=1e-3, size=(2, n, 3))
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x) and not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        got = s.compartments(None, None, None, True, 1, 2, 200)
        _check(got, _maps(list(x), None, None, True), False, 1, 2, 200, None, "fp64 state")
        rounded = R.expected(R.distance_map(x[0].astype(np.float32).astype(np.float64)))
        assert (np.abs(got["expected"][0, 1:] - rounded[1:]) > 1e3 * n * U * rounded[1:]).any()
    finally:
        s.close()


def _begin(ctx, n=257, nrep=5):
    restrained(ctx, n, nrep)
    x = np.stack([_planted(n, r) for r in range(nrep)])
    ctx.set_coords(x)
    return x


def test_start_vectors_and_continuation(ctx):
    from chromosome3d_amd import lib
    n, nv = 257, 2
    _begin(ctx, n, 2)
    maps = _maps(_state(ctx), None, None, False)
    own = np.empty((nv, n))
    assert lib.load().c3d_compartment_start(n, nv, lib.dptr(own)) == 0
    null, given = ctx.compartments(None, None, None, False, 1, nv, 5), ctx.compartments(None, None, None, False, 1, nv, 5, own)
    for k in ("expected", "vectors", "share", "residual"):
        assert null[k].tobytes() == given[k].tobytes(), k
    rng = np.random.default_rng(2570)
    mine = rng.normal(size=(nv, n))
    _check(ctx.compartments(None, None, None, False, 1, nv, 4, mine), maps, False, 1, nv, 4, mine, "caller's start, 4 rounds")
    first = ctx.compartments(None, None, None, False, 1, nv, 4, mine)
    # a start vector is one for every map: continue map by map, each from its own vectors
    for q in range(2):
        on = ctx.compartments(None, None, [q], False, 1, nv, 196, first["vectors"][q])
        _check(on, [maps[q]], False, 1, nv, 200, mine, f"4 + 196 rounds, map {q}")


def test_two_calls_same_bytes_alone_or_among_five_and_the_solve_goes_on(ctx):
    x = _begin(ctx)
    assert ctx.run_steps(20) == 20 and ctx.run_steps(15) == 15                  # an uninterrupted run
    plain = (ctx.coords().tobytes(), ctx.velocities().tobytes())
    _begin(ctx)
    assert ctx.run_steps(20) == 20                                              # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    a, b = ctx.compartments(None, None, None, True, 1, 3, 20), ctx.compartments(None, None, None, True, 1, 3, 20)
    for k in ("expected", "vectors", "share", "residual"):
        assert a[k].tobytes() == b[k].tobytes(), k
    alone = ctx.compartments(None, None, [3], False, 1, 3, 20)                  # model 3 alone: the bytes it had among five and the consensus
    for k in ("expected", "vectors", "share", "residual"):
        assert alone[k][0].tobytes() == a[k][3].tobytes(), k
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    assert ctx.run_steps(15) == 15                                              # and the solve goes on, to the bits of the uninterrupted run
    assert (ctx.coords().tobytes(), ctx.velocities().tobytes()) == plain
    assert x.shape == (5, 257, 3)


def test_a_second_batch_returns_the_bytes_of_the_first(ctx):
    """2052 beads: 31 X slots fit the 2^30 bytes, so 33 maps run as 31 + 2.  The same model 33 times: every map the same bytes."""
    n = 2052
    restrained(ctx, n, 1)
    ctx.set_coords(_planted(n, 0)[None])
    assert (1 << 30) // (8 * n * n) == 31
    got = ctx.compartments(None, None, [0] * 33, False, 1, 2, 3)
    for k in ("expected", "vectors", "share", "residual"):
        assert got[k].shape[0] == 33 and all(got[k][q].tobytes() == got[k][0].tobytes() for q in (1, 30, 31, 32)), k
    _check({k: v[:1] for k, v in got.items() if k in ("expected", "vectors", "share", "residual")}, _maps(_state(ctx), None, None, False), False, 1, 2, 3, None, "batches")


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name and writes nothing; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    n, M = 64, 2
    restrained(ctx, n, M)
    x = np.stack([_planted(n, r) for r in range(M)])
    ctx.set_coords(x)
    L, h = ctx._L, ctx._h
    state = ctx.coords().tobytes()
    good = x.astype(np.float64)
    IF = R.distance_map(good[0]) + 1.0
    big = np.zeros((256 - M + 1, n, 3))

    def refused(IF=None, extra=None, n_extra=0, pick=None, n_pick=0, flags=0, min_sep=1, nv=1, iters=5, start=None, outs="evsr", word=b""):
        buf = {k: np.full(300 * 3 * n, 7.0) for k in "evsrab"}
        ms = C.c_double(7.0)
        p = lambda k: lib.dptr(buf[k]) if k in outs else None
        rc = L.c3d_compartments(h, lib.dptr(IF) if IF is not None else None, lib.dptr(extra) if extra is not None else None, n_extra,
                                lib.i32ptr(pick) if pick is not None else None, n_pick, flags, min_sep, nv, iters, lib.dptr(start) if start is not None else None,
                                p("e"), p("v"), p("s"), p("r"), p("a"), p("b"), C.byref(ms))
        assert rc == -1 and b"c3d_compartments" in L.c3d_last_error() and word in L.c3d_last_error(), (L.c3d_last_error(), word)
        assert all((v == 7.0).all() for v in buf.values()) and ms.value == 7.0  # nothing written

    for nv in (0, -1, 4):
        refused(nv=nv, word=b"n_vec")
    for iters in (-1, 10001):
        refused(iters=iters, word=b"iters")
    for ms in (0, -2, n):
        refused(min_sep=ms, word=b"min_sep")
    refused(flags=2, word=b"flag")
    refused(flags=-1, word=b"flag")
    refused(outs="r", word=b"NULL")                                             # residual alone is not an output to ask for
    refused(outs="", word=b"NULL")
    refused(outs="eva", word=b"IF")                                             # agreement without IF
    refused(outs="evb", word=b"IF")
    one = np.array([0, 1], np.int32)
    refused(pick=one, n_pick=0)                                                 # a list without a length, a length without a list
    refused(n_pick=2)
    refused(pick=one, n_pick=-1)
    refused(pick=np.array([0, 2], np.int32), n_pick=2, word=b"pick")            # K = 2: index 2 is outside
    refused(pick=np.array([-1], np.int32), n_pick=1, word=b"pick")
    refused(pick=np.zeros(257, np.int32), n_pick=257, word=b"256")
    refused(n_extra=1)                                                          # extra models without coordinates
    refused(extra=good, n_extra=-1)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(extra=e, n_extra=M)
    refused(extra=big, n_extra=len(big))                                        # K = 257
    for bad in (np.nan, np.inf):
        s0 = R.start(n, 2)
        s0[1, 7] = bad
        refused(nv=2, start=s0, word=b"start")
    dep = np.zeros((2, n))                                                      # found by the first round: a copy projects to exactly 0
    dep[0, 3], dep[1, 3] = 0.25, 1.0
    refused(nv=2, start=dep, word=b"dependent start vectors")
    for at, bad, word in (((3, 9), np.nan, b"finite"), ((3, 9), np.inf, b"finite"), ((3, 9), -1.0, b"negative"), ((9, 3), 5.0, b"symmetric")):
        m = IF.copy()
        m[at] = bad
        if bad < 0:
            m[at[::-1]] = bad
        refused(IF=m, outs="evsrab", word=word)                                 # found by the pass over IF
    assert ctx.coords().tobytes() == state
    got = ctx.compartments(IF, None, None, True, 1, 2, 200)                     # and the context works
    _check(got, _maps(list(good), IF, None, True), True, 1, 2, 200, None, "after the refusals")
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_compartments.*c3d_init_replicas"):
            s2.compartments()
        s2.init_replicas(2)
        with pytest.raises(C3DError, match="c3d_compartments.*n < 3"):
            s2.compartments()
    finally:
        s2.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --compartments on the smallest bundled matrix against Solver.compartments of the written models.  IF's column does not
    depend on the models: the print's 5e-7 and the vectors' bound.  A written coordinate is rounded to 3 decimals, so a distance moves by at
    most 1.74e-3 A, an entry of a model's O/E map by a relative eps = 2 x 1.74e-3 / d_min (the entry and its expected); the correlation
    operator by at most about eps lambda_1 and a unit eigenvector by about eps / (1 - g): the columns of the models and the consensus are
    held to 2 eps / (1 - g) + 5e-7 with g from eigh of the written model."""
    cid, M, n = "chr21_1mb", 4, 37
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "cpt")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--compartments", prefix, "--compartment-vectors", "2"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = open(prefix + "_compartments.txt").read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split() for l in lines if not l.startswith("#")]
    assert head and lines[:len(head)] == head
    order = [int(v) for v in next(l for l in head if l.startswith("# models:")).split()[2:]]
    assert sorted(order) == [1, 2, 3, 4]
    assert [int(r[0]) for r in rows] == list(range(1, n + 1)) and all(len(r) == 3 + M for r in rows)
    cols = np.array([[float(v) for v in r[1:]] for r in rows]).T               # IF, consensus, the models in rank order
    IF = load_if(cid)
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r}.pdb") for r in order])
    restrained(ctx, n, M)
    ctx.set_coords(x)
    got = ctx.compartments(IF, None, None, True, 1, 2, 200)
    assert np.abs(cols[0] - got["vectors"][0, 0]).max() <= 5.000001e-7 + 64 * n * U / (1 - 0.9)
    models = _state(ctx)
    for col, q, Mq in [(1, M + 1, R.consensus_map(models))] + [(2 + k, 1 + k, R.distance_map(models[k])) for k in range(M)]:
        d = Mq[np.triu_indices(n, 1)]
        eps, g = 2.0 * 1.74e-3 / d.min(), R.gap_ratio(Mq, 1, 1)
        gap = np.abs(cols[col] - got["vectors"][q, 0]).max()
        print(f"column {col}: g {g:.3f} eps {eps:.2e} gap {gap:.2e}")
        assert g < 1.0 and gap <= 2.0 * eps / (1.0 - g) + 5.000001e-7
    line = next(l for l in head if l.startswith("# IF:")).split()[2:]
    assert len(line) == 4 and abs(float(line[0]) - got["share"][0, 0]) <= 5.1e-7 and abs(float(line[2]) - got["share"][0, 1]) <= 5.1e-7
    assert len(next(l for l in head if l.startswith("# consensus:")).split()) == 2 + 8 and sum(l.startswith("# model ") for l in head) == M
    other = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", "2", "--quiet", "--compartments", str(tmp_path / "o"), "--compartment-iters", "7",
                            "--compartment-min-sep", "3"], capture_output=True, text=True)
    assert other.returncode == 0, other.stderr
    assert "# 1 vector(s), 7 rounds, min_sep 3;" in open(tmp_path / "o_compartments.txt").read()


def test_the_index_arithmetic_at_16384_beads():
    """16384 beads x 1 model, n_vec 1, iters 2: one X slot of 2 GiB, 2048 row tiles, 256 x 256 build tiles, byte offsets up to 2^31.  The
    restatement forms the map in row blocks and never holds it.  The run is stopped early (the case is about indices, not convergence):
    B sqrt(n) with g from a subspace estimate is not available without eigh of a 16384 x 16384 matrix, so g is bounded from the
    restatement itself — after the two rounds the Rayleigh quotient lambda and the residual r give lambda_2 <= lambda_1 only; the bound is
    taken at g = 0.9, the largest the inputs of this module may have."""
    from chromosome3d_amd import Solver, default_model, make_stages
    n = 16384
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(n, np.array([1, 1, 8001], np.int32), np.array([11, 16384, 16384], np.int32), np.array([100, 457, 300], np.int32))
        s.init_replicas(1, 82364, 0)
        s.set_coords(R.planted_model(n, 0)[None])
        x = s.coords()[0].astype(np.float64)
        got = s.compartments(None, None, None, False, 1, 1, 2)
        ref = R.BlockedMap(x, 1)
        T = np.arange(n, 0, -1).astype(np.float64)
        rel = np.abs(got["expected"][0] - ref.E) / np.where(ref.E != 0.0, ref.E, 1.0)
        assert got["expected"][0, 0] == 0.0 and (rel <= T * U).all(), float((rel / (T * U)).max())
        V, _, share, res = R.solve_operator(ref.dot, ref.m, ref.q, 1, 2)
        v = R.sign_largest(V[0])
        Bq = 64.0 * n * U / (1.0 - 0.9) * np.sqrt(n)
        dv = float(np.abs(got["vectors"][0, 0] - v).max())
        print(f"n = 16384: bound {Bq:.2e} vectors {dv:.2e} share {got['share'][0, 0]:.6f} residual {got['residual'][0, 0]:.3e} device {got['device_ms']:.1f} ms")
        assert dv <= Bq and abs(got["share"][0, 0] - share[0]) <= 2.0 * np.sqrt(n) * Bq and abs(got["residual"][0, 0] - res[0]) <= 2.0 * share[0] * n * np.sqrt(n) * Bq
        assert abs(np.linalg.norm(got["vectors"][0, 0]) - 1.0) <= 64.0 * n * U
    finally:
        s.close()
