"""Insulation profiles and domain boundaries on the device (c3d_insulation; csrc/c3d_score_insulation.inc k_ins_*) against the numpy
restatement tests/insulation_ref.py, which tests/test_insulation_ref.py holds to scipy.signal and to planted chains.

The kernels' constants: a workgroup of k_ins_squares owns kInsTile = 32 consecutive beads of one map; a thread takes the cells t, t + 256,
... of a bead's nested squares, so w = 16 is exactly one cell a thread; every walk computes its distances from the tile's coordinates in LDS, and
with C3D_INSULATION_STAGE, up to w_max = kInsStageMax = 40, a model's tile stages its (31 + w_max)^2 distances in LDS instead; the reduction is instantiated
for lists of 1, 2, 3..4 and 5..8 windows; the score, boundary and fit kernels walk a row in steps of 256.
  small     n = 3 (w = 1), 4, 5; n = 2w + 1 and 2w + 2 for w = 1, 2, 40 (the largest staged) and 128 (the largest)
  tiles     n = 31, 32, 33, 65; 255, 256, 257 (the row step)
  windows   lists of 1, 2, 3, 5 and 8 windows with 15, 16, 17 (the cell step), 40, 41 (the staging limit) and 128, at n = 257, 455, 1025
  models    one to three planted chains (tests/insulation_ref.planted_domains), as set or relaxed by the 45 steps of a short schedule
  large     16384 beads x 1 model, windows {1, 128}: every 97th bead and the beads at the tile borders

Bounds, u = 2^-53.  mean, relative: (w^2 + 2) u for IF and model maps, (w^2 + Kp + 2) u for the consensus; contact maps and the NaN
pattern bit for bit.  score, absolute: S = ((2 w^2 + Kp + n + 8) u) / ln 2 + 2 u |score|.  boundary and strength: the restatement's
step 4 on the device's own score bytes, bit for bit; and the restatement's own wherever its y-margins exceed 2 S (strength then within
2 S), the beads left out at most 2 % of a row.  fit_counts: exact from the device's boundary and strength.  fit_r: within
2 e (1 / |x_c| + 1 / |y_c|), e = sqrt(n) S.  Every check prints the largest observed fraction of its bound."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import insulation_ref as R
from tests.util import GOLD, SHORT, load_if, load_pdb_xyz, restrained

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
CUT = 30.0                                                                      # A: inside a planted domain every pair is a contact, across a boundary about half
KEYS = ("mean", "score", "boundary", "strength")


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _planted(n, r):
    return R.planted_domains(n, max(3, min(41, n // 9)), 100 + r).astype(np.float32)


def _if_of(x):
    """a symmetric non-negative matrix with the domains of x: 1 / d, zero on the diagonal"""
    x = np.asarray(x, dtype=np.float64)
    u = x[:, None, :] - x[None, :, :]
    d = np.sqrt((u * u).sum(axis=2))
    m = 1.0 / np.where(d > 0, d, 1.0)
    np.fill_diagonal(m, 0.0)
    return np.maximum(m, m.T)


def _state(ctx):
    return [m.astype(np.float64) for m in ctx.coords()]


def _maps(models, IF, pick, consensus):
    order = list(range(len(models))) if pick is None else list(pick)
    maps = ([("if", np.asarray(IF, dtype=np.float64))] if IF is not None else []) + [("model", models[k]) for k in order]
    if consensus:
        maps.append(("consensus", [models[k] for k in order]))
    return maps


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def _check(got, maps, n, windows, cutoff=None, min_strength=0.0, tol=1, what="", beads=None):
    """every output of a call against the restatement, to the bounds of the module's docstring; returns the largest fractions"""
    Q, W = len(maps), len(windows)
    want = R.insulation(maps, n, windows, cutoff, min_strength, tol, beads)
    for k in KEYS:
        assert got[k].shape == (Q, W, n), k
    worst = {"mean": 0.0, "score": 0.0, "strength": 0.0, "fit_r": 0.0, "left out": 0.0}
    for q, (kind, src) in enumerate(maps):
        Kp = len(src) if kind == "consensus" else 0
        exact = cutoff is not None and kind != "if"
        for k, w in enumerate(windows):
            gm, wm = got["mean"][q, k], want["mean"][q, k]
            at = f"{what} map {q} ({kind}) window {w}"
            if beads is not None:                                               # a sample of the beads: the restatement has the others as NaN
                inside = np.array([b for b in beads if w <= b <= n - 1 - w])
                assert np.isnan(gm[:w]).all() and np.isnan(gm[n - w:]).all() and not np.isnan(gm[w:n - w]).any(), at
                rel = np.abs(gm[inside] - wm[inside]) / wm[inside]
                assert (rel <= (w * w + Kp + 2) * U).all(), (at, float(rel.max() / U))
                worst["mean"] = max(worst["mean"], float(rel.max() / ((w * w + Kp + 2) * U)))
                continue
            assert _same_nan(gm, wm), at
            if exact:
                assert gm.tobytes() == wm.tobytes(), at
            else:
                ok = ~np.isnan(wm) & (wm != 0.0)
                assert (gm[~np.isnan(wm) & (wm == 0.0)] == 0.0).all(), at
                rel = np.abs(gm[ok] - wm[ok]) / wm[ok]
                if len(rel):
                    assert (rel <= (w * w + Kp + 2) * U).all(), (at, float(rel.max() / U))
                    worst["mean"] = max(worst["mean"], float(rel.max() / ((w * w + Kp + 2) * U)))
            gs, ws = got["score"][q, k], want["score"][q, k]
            assert _same_nan(gs, ws), at
            S = (2 * w * w + Kp + n + 8) * U / np.log(2.0) + 2.0 * U * np.abs(np.nan_to_num(ws))
            valid = ~np.isnan(ws)
            if valid.any():
                frac = np.abs(gs[valid] - ws[valid]) / S[valid]
                assert (frac <= 1.0).all(), (at, float(frac.max()))
                worst["score"] = max(worst["score"], float(frac.max()))
            minima = kind == "if" or cutoff is not None
            mark, strength = R.boundaries(gs, minima)                           # step 4 on the device's own score bytes
            assert np.array_equal(got["boundary"][q, k], mark) and got["strength"][q, k].tobytes() == strength.tobytes(), at
            rmark, rstrength, margin = R.boundaries(ws, minima, True, wm if exact else None)
            Smax = float(S.max())
            sure = margin > 2.0 * Smax
            left = float((valid & ~sure).sum()) / n
            assert left <= 0.02, (at, left)
            worst["left out"] = max(worst["left out"], left)
            assert np.array_equal(got["boundary"][q, k][sure], rmark[sure]), at
            ds = np.abs(got["strength"][q, k][sure] - rstrength[sure])
            assert (ds <= 2.0 * Smax).all(), (at, float(ds.max()))
            if len(ds):
                worst["strength"] = max(worst["strength"], float(ds.max() / (2.0 * Smax)))
            if q > 0 and maps[0][0] == "if":
                fs = got["score"][0, k]
                counts = R.match_counts(got["boundary"][0, k], got["strength"][0, k], got["boundary"][q, k], got["strength"][q, k], min_strength, tol)
                assert np.array_equal(got["fit_counts"][q - 1, k], counts), (at, got["fit_counts"][q - 1, k], counts)
                r, wr = got["fit_r"][q - 1, k], want["fit_r"][q - 1, k]
                assert np.isnan(r) == np.isnan(wr), (at, r, wr)
                if not np.isnan(wr):
                    both = ~np.isnan(ws) & ~np.isnan(want["score"][0, k])
                    xc, yc = ws[both] - ws[both].mean(), want["score"][0, k][both] - want["score"][0, k][both].mean()
                    Sif = (2 * w * w + n + 8) * U / np.log(2.0) + 2.0 * U * float(np.abs(np.nan_to_num(fs)).max())
                    bound = 2.0 * np.sqrt(n) * max(Smax, Sif) * (1.0 / np.linalg.norm(xc) + 1.0 / np.linalg.norm(yc))
                    assert abs(r - wr) <= bound, (at, r, wr, bound)
                    worst["fit_r"] = max(worst["fit_r"], abs(r - wr) / bound)
    if maps[0][0] == "if":
        assert got["fit_r"].shape == (Q - 1, W) and got["fit_counts"].shape == (Q - 1, W, 4)
    else:
        assert "fit_r" not in got and "fit_counts" not in got
    print(f"{what}: largest fraction of the bound — " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


def _set(ctx, n, nrep, relaxed=False):
    restrained(ctx, n, nrep)
    ctx.set_coords(np.stack([_planted(n, r) for r in range(nrep)]))
    if relaxed:
        ctx.run()                                                               # the 45 steps of SHORT: a model the solver left
    return _state(ctx)


SMALL = [(3, [1]), (4, [1]), (5, [1, 2]), (6, [1, 2]), (81, [2, 40]), (82, [40]), (257, [128]), (258, [1, 128])]


@pytest.mark.parametrize("n,windows", SMALL)
def test_small_sizes(ctx, n, windows):
    models = _set(ctx, n, 2)
    IF = _if_of(R.planted_domains(n, max(3, n // 9), 7))
    got = ctx.insulation(IF, None, None, True, windows)
    assert got["maps"] == ["IF", "model 0", "model 1", "consensus"] and got["windows"] == windows and got["device_ms"] > 0
    _check(got, _maps(models, IF, None, True), n, windows, None, 0.0, 1, f"n = {n} windows {windows}")
    for k, w in enumerate(windows):
        if n == 2 * w + 1:                                                      # one inside bead: score 0, no boundary
            assert (got["score"][:, k, w] == 0.0).all() and got["boundary"][:, k].sum() == 0


BORDERS = [(31, 1, False, [1, 5, 15]), (32, 2, False, [3]), (33, 3, True, [2, 16]), (65, 2, False, [1, 17, 32]), (255, 1, False, [16]), (256, 2, True, [15, 41]),
           (257, 1, False, [1, 2, 3, 15, 16, 17, 40, 128]), (257, 2, False, [40]), (455, 3, True, [5, 10, 25]), (455, 1, False, [1, 16, 41, 100, 128]),
           (1025, 1, True, [16, 128]), (1025, 2, False, [2, 3, 5, 8, 13, 21, 34, 40])]


@pytest.mark.parametrize("n,nrep,relaxed,windows", BORDERS)
def test_tile_step_and_window_borders(ctx, n, nrep, relaxed, windows):
    models = _set(ctx, n, nrep, relaxed)
    consensus = nrep >= 2
    got = ctx.insulation(None, None, None, consensus, windows)
    assert got["maps"] == ["model %d" % k for k in range(nrep)] + (["consensus"] if consensus else [])
    worst = _check(got, _maps(models, None, None, consensus), n, windows, None, 0.0, 1, f"n = {n} x {nrep}{' relaxed' if relaxed else ''} windows {windows}")
    assert worst["score"] <= 1.0
    if not relaxed and n >= 455 and 16 in windows:                              # domains of 41 beads: the planted boundaries are found
        L, k = max(3, min(41, n // 9)), windows.index(16)
        strong = np.flatnonzero((got["boundary"][0, k] == 1) & (got["strength"][0, k] >= 1.0))
        assert all(any(abs(int(s) - b) <= 1 for s in strong) for b in range(L, n, L) if 16 <= b <= n - 17)


@pytest.mark.parametrize("contact", [False, True])
def test_if_consensus_contacts_picks_and_extra_models(ctx, contact):
    """IF, three replicas and two extra models, a pick list with a repeat, the consensus, with and without the contact flag; the fit's
    counts at a threshold and tolerance that are not the defaults."""
    n, windows = 455, [5, 16, 25]
    state = _set(ctx, n, 3)
    extra = np.stack([R.planted_domains(n, 41, 100 + r) + 0.25 for r in (5, 7)])
    models = state + list(extra)
    pick = [4, 0, 0, 3, 2]
    IF = _if_of(_planted(n, 0))
    cutoff = CUT if contact else None
    got = ctx.insulation(IF, extra, pick, True, windows, cutoff, 0.25, 2)
    assert got["maps"] == ["IF"] + ["model %d" % k for k in pick] + ["consensus"]
    _check(got, _maps(models, IF, pick, True), n, windows, cutoff, 0.25, 2, "contacts" if contact else "distances")
    for k in KEYS:
        assert got[k][2].tobytes() == got[k][3].tobytes(), k                    # the repeated pick
    r = got["fit_r"][1, 1]                                                       # model 0, whose domains IF has: the sign as it comes
    assert r > 0.8 if contact else r < -0.8, r
    assert got["fit_counts"][1, 1, 0] > 0 and got["fit_counts"][1, 1, 2] >= got["fit_counts"][1, 1, 0] - 1
    from chromosome3d_amd import pipeline
    rep = pipeline.insulation_report(ctx, IF, extra, pick, [5, 16, 25, 300], cutoff, 0.25, 2)
    assert rep["windows"] == windows and all(rep[k].tobytes() == got[k].tobytes() for k in KEYS) and rep["fit_r"].tobytes() == got["fit_r"].tobytes()
    assert rep["support"].shape == (3, n) and rep["support"].max() <= len(pick) and rep["best"][1] in (2, 3)


def test_the_staged_and_the_recompute_form_return_the_same_bytes(ctx):
    n = 455
    models = _set(ctx, n, 2)
    for windows in ([3], [16, 40], [1, 2, 5, 39]):
        again, staged = ctx.insulation(None, None, None, True, windows, None), ctx.insulation(None, None, None, True, windows, None, 0.0, 1, True)
        for k in KEYS:
            assert staged[k].tobytes() == again[k].tobytes(), (windows, k)
        again, staged = ctx.insulation(None, None, None, True, windows, CUT), ctx.insulation(None, None, None, True, windows, CUT, 0.0, 1, True)
        for k in KEYS:
            assert staged[k].tobytes() == again[k].tobytes(), (windows, k, "contacts")
    _check(ctx.insulation(None, None, None, True, [16, 40], None, 0.0, 1, True), _maps(models, None, None, True), n, [16, 40], None, 0.0, 1, "staged")
    beyond = ctx.insulation(None, None, None, True, [16, 41], None, 0.0, 1, True)          # w_max = 41 does not fit: the flag changes nothing
    assert all(beyond[k].tobytes() == ctx.insulation(None, None, None, True, [16, 41])[k].tobytes() for k in KEYS)


def test_f64_state_is_read_in_doubles():
    """A precision-64 context whose state no float holds: coordinates near 9000 A, where a float's last place is 1e-3 A.  The means
    follow the doubles to (w^2 + 2) u and are far from those of the state rounded to float."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        n, windows = 96, [4, 9]
        restrained(s, n, 2)
        rng = np.random.default_rng(96)
        x = np.stack([_planted(n, r).astype(np.float64) + 9000.0 for r in range(2)]) + rng.normal(scale=1e-3, size=(2, n, 3))
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x) and not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        got = s.insulation(None, None, None, True, windows)
        _check(got, _maps(list(x), None, None, True), n, windows, None, 0.0, 1, "fp64 state")
        rounded = R.mean_row("model", x[0].astype(np.float32).astype(np.float64), n, 4)
        assert (np.abs(got["mean"][0, 0, 4:n - 4] - rounded[4:n - 4]) > 1e3 * 18 * U * rounded[4:n - 4]).any()
    finally:
        s.close()


def test_two_calls_same_bytes_alone_or_among_others_and_the_solve_goes_on(ctx):
    n, nrep, windows = 257, 5, [3, 16, 41]
    _set(ctx, n, nrep)
    assert ctx.run_steps(20) == 20 and ctx.run_steps(15) == 15                  # an uninterrupted run
    plain = (ctx.coords().tobytes(), ctx.velocities().tobytes())
    _set(ctx, n, nrep)
    assert ctx.run_steps(20) == 20                                              # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    IF = _if_of(_planted(n, 0))
    a, b = ctx.insulation(IF, None, None, True, windows, None, 0.1, 1), ctx.insulation(IF, None, None, True, windows, None, 0.1, 1)
    for k in KEYS + ("fit_r", "fit_counts"):
        assert a[k].tobytes() == b[k].tobytes(), k
    _check(a, _maps(_state(ctx), IF, None, True), n, windows, None, 0.1, 1, "mid-solve")
    alone = ctx.insulation(None, None, [3], False, windows)                     # model 3 alone: the bytes it had among five, IF and the consensus
    for k in KEYS:
        assert alone[k][0].tobytes() == a[k][4].tobytes(), k
    for j, w in enumerate(windows):                                             # a window alone: the bytes it had in the list (w_max, and so the form, differ)
        one = ctx.insulation(IF, None, None, True, [w], None, 0.1, 1)
        for k in KEYS:
            assert one[k][:, 0].tobytes() == a[k][:, j].tobytes(), (k, w)
        assert one["fit_r"][:, 0].tobytes() == a["fit_r"][:, j].tobytes() and one["fit_counts"][:, 0].tobytes() == a["fit_counts"][:, j].tobytes()
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    assert ctx.run_steps(15) == 15                                              # and the solve goes on, to the bits of the uninterrupted run
    assert (ctx.coords().tobytes(), ctx.velocities().tobytes()) == plain


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name and writes nothing; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    n, M = 64, 2
    models = _set(ctx, n, M)
    L, h = ctx._L, ctx._h
    state = ctx.coords().tobytes()
    good = np.stack(models)
    IF = _if_of(good[0])
    big = np.zeros((256 - M + 1, n, 3))

    def refused(IF=None, extra=None, n_extra=0, pick=None, n_pick=0, flags=0, windows=(2, 5), n_win=None, cutoff=0.0, min_strength=0.0, tol=1, outs="msbt", word=b""):
        buf = {k: np.full(300 * 3 * n, 7.0) for k in "mstr"}
        ibuf = {k: np.full(300 * 3 * n, 7, np.int32) for k in "bc"}
        ms = C.c_double(7.0)
        win = np.array(windows, np.int32) if windows is not None else None
        p = lambda k: lib.dptr(buf[k]) if k in outs else None
        ip = lambda k: lib.i32ptr(ibuf[k]) if k in outs else None
        rc = L.c3d_insulation(h, lib.dptr(IF) if IF is not None else None, lib.dptr(extra) if extra is not None else None, n_extra,
                              lib.i32ptr(pick) if pick is not None else None, n_pick, flags, lib.i32ptr(win) if win is not None else None,
                              len(windows) if n_win is None else n_win, cutoff, min_strength, tol, p("m"), p("s"), ip("b"), p("t"), p("r"), ip("c"), C.byref(ms))
        assert rc == -1 and b"c3d_insulation" in L.c3d_last_error() and word in L.c3d_last_error(), (L.c3d_last_error(), word)
        assert all((v == 7.0).all() for v in buf.values()) and all((v == 7).all() for v in ibuf.values()) and ms.value == 7.0      # nothing written

    refused(n_win=0, word=b"n_win")
    refused(n_win=-1, word=b"n_win")
    refused(windows=tuple(range(1, 10)), word=b"n_win")
    refused(windows=None, n_win=2, word=b"windows")
    for bad, word in (((0, 5), b"window"), ((-1,), b"window"), ((2, 129), b"window"), ((5, 2), b"ascending"), ((2, 2), b"ascending"), ((2, 32), b"2w + 1 > n")):
        refused(windows=bad, word=word)
    refused(flags=8, word=b"flag")
    refused(flags=-1, word=b"flag")
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(flags=2, cutoff=bad, word=b"cutoff")
    for bad in (-0.5, np.nan, np.inf):
        refused(min_strength=bad, word=b"min_strength")
    refused(tol=-1, word=b"tol")
    refused(outs="", word=b"NULL")
    refused(outs="msr", word=b"IF")                                             # the fit without IF
    refused(outs="c", word=b"IF")
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
    for at, bad, word in (((3, 9), np.nan, b"finite"), ((3, 9), np.inf, b"finite"), ((3, 9), -1.0, b"negative"), ((9, 3), 5.0, b"symmetric")):
        m = IF.copy()
        m[at] = bad
        if bad < 0:
            m[at[::-1]] = bad
        refused(IF=m, outs="msbtrc", word=word)                                 # found while the host packs the band
    m = IF.copy()
    m[3, 4], m[3, 30] = np.nan, -1.0                                            # outside the band 2 <= b - a <= 2 w_max that is read: accepted
    ok = ctx.insulation(m, None, None, True, [2, 5])
    assert ctx.coords().tobytes() == state
    got = ctx.insulation(IF, None, None, True, [2, 5])                          # and the context works
    _check(got, _maps(models, IF, None, True), n, [2, 5], None, 0.0, 1, "after the refusals")
    assert all(ok[k].tobytes() == got[k].tobytes() for k in KEYS)
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_insulation.*c3d_init_replicas"):
            s2.insulation(windows=[1])
        s2.init_replicas(2)
        with pytest.raises(C3DError, match="c3d_insulation.*n < 3"):
            s2.insulation(windows=[1])
    finally:
        s2.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --insulation on the smallest bundled matrix against Solver.insulation of the written models.  IF's columns do not depend
    on the models: the print's 5e-7 and the score bound.  A written coordinate is rounded to 3 decimals, so a distance moves by at most
    1.74e-3 A and so does a mean of distances; a score, the log2 of a ratio of two such means, by at most 2.02 x 1.74e-3 / (m ln 2) with
    m the smallest mean of the row."""
    cid, M, n = "chr21_1mb", 4, 37
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "ins")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--insulation", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = open(prefix + "_insulation.txt").read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    rows = [l.split() for l in lines if not l.startswith("#")]
    assert head and lines[:len(head)] == head
    order = [int(v) for v in next(l for l in head if l.startswith("# models:")).split()[2:]]
    assert sorted(order) == [1, 2, 3, 4]
    windows = [5, 10]                                                           # the default 5,10,25 clipped to 2w + 1 <= 37
    assert [(int(r[0]), int(r[1])) for r in rows] == [(w, i) for w in windows for i in range(1, n + 1)] and all(len(r) == 9 for r in rows)
    IF = load_if(cid)
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r}.pdb") for r in order])
    restrained(ctx, n, M)
    ctx.set_coords(x)
    got = ctx.insulation(IF, None, None, True, windows, None, 0.1, 1)
    cols = np.array([[float(v) for v in r] for r in rows]).reshape(2, n, 9)
    for k, w in enumerate(windows):
        S = (2 * w * w + n + 8) * U / np.log(2.0)
        assert _same_nan(cols[k, :, 2], got["score"][0, k]) and _same_nan(cols[k, :, 3], got["score"][M + 1, k])
        assert np.nanmax(np.abs(cols[k, :, 2] - got["score"][0, k])) <= 5.000001e-7 + S
        assert np.array_equal(cols[k, :, 4].astype(np.int32), got["boundary"][0, k]) and np.abs(cols[k, :, 5] - got["strength"][0, k]).max() <= 5.000001e-7 + 2 * S
        eps = 2.02 * 1.74e-3 / (np.nanmin(got["mean"][M + 1, k]) * np.log(2.0))
        gap = np.nanmax(np.abs(cols[k, :, 3] - got["score"][M + 1, k]))
        print(f"window {w}: consensus score gap {gap:.2e} of {eps + 5e-7:.2e}")
        assert gap <= eps + 5.000001e-7
        assert (cols[k, :, 8] >= 0).all() and (cols[k, :, 8] <= M).all()
        line = next(l for l in head if l.startswith(f"# window {w} consensus:")).split()
        assert len(line) == 9 and [int(v) for v in line[5:7]][0] == int(((got["boundary"][0, k] == 1) & (got["strength"][0, k] >= 0.1)).sum())
    assert sum(l.startswith("# window 5 model ") for l in head) == M and "# mean distance;" in "\n".join(head)
    other = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", "2", "--quiet", "--insulation", str(tmp_path / "o"), "--insulation-windows", "3",
                            "--insulation-contact", "60", "--insulation-tol", "2"], capture_output=True, text=True)
    assert other.returncode == 0, other.stderr
    text = open(tmp_path / "o_insulation.txt").read()
    assert "# contacts below 60.000 A;" in text and "within 2 beads" in text and sum(not l.startswith("#") for l in text.splitlines()) == n
    bad = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "c"), "-m", "2", "--quiet", "--insulation", str(tmp_path / "x"), "--insulation-windows", "30"],
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "c3d_insulation" in bad.stderr               # a window of the user's that does not fit is refused, not dropped


def test_the_index_arithmetic_at_16384_beads():
    """16384 beads x 1 model, windows {1, 128}: 512 tiles, the recompute form, a halo of 128 beads at both ends of the chain.  The means
    are checked on every 97th bead and on the beads at the tile borders; the score against the restatement's step 3 on the device's
    own means ((n + 8) u / ln 2 + 2 u |score|: the row mean and the log2), the boundaries on the device's own score bytes."""
    from chromosome3d_amd import Solver, default_model, make_stages
    n, windows = 16384, [1, 128]
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(n, np.array([1, 1, 8001], np.int32), np.array([11, 16384, 16384], np.int32), np.array([100, 457, 300], np.int32))
        s.init_replicas(1, 82364, 0)
        s.set_coords(R.planted_domains(n, 64, 3).astype(np.float32)[None])
        x = s.coords()[0].astype(np.float64)
        got = s.insulation(None, None, None, False, windows)
        beads = sorted(set(range(0, n, 97)) | {b for t in range(32, n, 2048) for b in (t - 1, t, t + 31, t + 32)} | {1, 127, 128, 129, n - 130, n - 129, n - 128, n - 2})
        _check(got, [("model", x)], n, windows, None, 0.0, 1, "n = 16384", beads)
        for k, w in enumerate(windows):
            ws = R.score_row(got["mean"][0, k])
            assert _same_nan(got["score"][0, k], ws)
            S = (n + 8) * U / np.log(2.0) + 2.0 * U * np.abs(np.nan_to_num(ws))
            frac = np.nanmax(np.abs(got["score"][0, k] - ws) / S)
            mark, strength = R.boundaries(got["score"][0, k], False)
            print(f"n = 16384 window {w}: score at {frac:.3g} of its bound, {int(mark.sum())} boundaries, device {got['device_ms']:.1f} ms")
            assert frac <= 1.0 and np.array_equal(got["boundary"][0, k], mark) and got["strength"][0, k].tobytes() == strength.tobytes()
    finally:
        s.close()
