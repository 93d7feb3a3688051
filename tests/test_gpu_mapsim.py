"""The stratum-adjusted correlation coefficient of contact maps on the device (c3d_map_similarity; csrc/c3d_score_mapsim.inc k_sim_*)
against the numpy restatement tests/mapsim_ref.py, which tests/test_mapsim_ref.py holds to scipy, a worked example and a planted case.

The kernels' constants: k_sim_smooth owns tiles of 32 x 32 cells with a halo of h on every side and launches the tile diagonals
lo / 32 .. (hi + 31) / 32; k_sim_stratum walks a stratum in steps of 256 and sorts P = 8, 16, ... 16384 64-bit keys in LDS, a thread
owning more than one comparator vector from P = 2048 on, with 128 KiB of dynamic LDS at P = 16384.
  smoothing  n = 3, 9, 31, 32, 33, 64, 65, 97 and, for the tile, 96 (three whole tiles); at n = 97 the separation windows 31..31, 32..63
             and 33..64 (the first and last tile diagonal of a launch on, before and after a tile border); h = 0, 1, 3, and 20 at n = 9
             (the window is the whole map, clipped on all sides) and at n = 97 (the widest halo); integer counts and a balanced-like map
             (w w^T) M; three masked all-zero bins at n = 97 with and without C3D_MAPSIM_KEEP_ZEROS
  strata     n = 257, 520, 1030 with min_sep 1 (every slot class up to 2048, N across the stride of 256), n = 2050 with separations 1..3
             (P = 4096), n = 8200 behind max_beads with separations 1..2 (P = 16384)

What is held bit for bit: `smoothed` against the restatement; `counts` (N, A, B) exactly; `rho` against the header's formula applied to
the returned moments and counts and `scc` against the sequential sums over the returned strata (mapsim_ref.combine); the identities.

`moments` against a yardstick: the same sums evaluated from the (bit-identical) smoothed values in exact rational arithmetic (fractions)
up to n = 97 and in numpy.longdouble beyond.  The bound, u = 2^-53, gamma(m) = m u / (1 - m u).  A thread adds its k = ceil((n - s) / 256)
terms in sequence and the tree has 8 levels, so a term passes through at most m = k + 8 additions; every x is >= 0, so the computed sum
of x is within gamma(m) of it and the mean, one division later, within em_x = gamma(m + 1) mx of mx.  A centred value fl(x_i - mx^) is
within Ex_i = em_x + u (|dx_i| + em_x) of dx_i = x_i - mx; with T_i = (|dx_i| + Ex_i)(|dy_i| + Ey_i) >= |dx^_i dy^_i| the rounded product
is within |dx_i| Ey_i + |dy_i| Ex_i + Ex_i Ey_i + u T_i of dx_i dy_i, and the sum of the rounded products within gamma(m) (1 + u) sum T_i
of their sum:
    B(u, m) = sum_i (|dx_i| Ey_i + |dy_i| Ex_i + Ex_i Ey_i + u T_i) + gamma(m) (1 + u) sum_i T_i         (Cxx, Cyy: y = x, x = y)
The longdouble yardstick is the same computation with u_l = 2^-64 and at most N additions a term, so it is within B(u_l, N) of the exact
value (about a tenth of B(u, m) at N = 16384) and the bound there is B(u, m) + B(u_l, N).  Nothing is fitted to the device's output.
Every numeric check prints the largest observed fraction of its bound.

The entry keeps no stat key (the stat table's keys are held fixed by tests/test_config_transcript.py), so no call count is asserted."""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import mapsim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
UL = float(np.finfo(np.longdouble).eps) / 2
SENT = -7.0                                                                     # no output is ever -7: scc and rho lie in [-1, 1], the rest is >= 0 or a sum of squares
C3D_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _counts(n, seed=0, depth=1.0):
    """raw counts: Poisson with a mean that decays with the separation (zeros and ties at the far diagonals), symmetric"""
    rng = np.random.default_rng(1000 * seed + n)
    i = np.arange(n)
    lam = depth * 40.0 / (1.0 + np.abs(i[:, None] - i[None, :])) ** 1.1
    M = np.triu(rng.poisson(lam).astype(float))
    M = M + np.triu(M, 1).T
    M.setflags(write=False)
    return M


def _balanced_like(M, seed):
    """(w w^T) M: non-integer, symmetric bit for bit (w_i w_j is one product)"""
    w = np.exp(np.random.default_rng(seed).normal(0.0, 0.3, M.shape[0]))
    return (w[:, None] * w[None, :]) * M


def _call(s, maps, h=(0,), lo=0, hi=0, flags=0, outs="srmcxd", n=None):
    """The entry through ctypes with every output buffer filled with a sentinel.  Returns (rc, dict): the outputs asked for by `outs`
    (s scc, r rho, m moments, c counts, x smoothed, d device_ms)."""
    from chromosome3d_amd import lib
    L = lib.load()
    maps = np.ascontiguousarray(maps, dtype=np.float64)
    Q, rows = maps.shape[0], maps.shape[1]
    n = rows if n is None else n
    hw = np.ascontiguousarray(h, dtype=np.int32)
    H, P = len(hw), Q * (Q - 1) // 2
    S = max((hi if hi else rows - 1) - lo + 1, 1)
    buf = {"s": np.full((H, Q, Q), SENT), "r": np.full((H, P, S), SENT), "m": np.full((H, P, S, 3), SENT), "c": np.full((H, P, S, 3), -7, np.int64),
           "x": np.full((H, Q, S, rows), SENT) if "x" in outs else None, "d": C.c_double(SENT)}
    ptr = lambda k: (buf[k].ctypes.data_as(C.POINTER(C.c_int64)) if k == "c" else lib.dptr(buf[k])) if k in outs else None
    rc = L.c3d_map_similarity(s._h, lib.dptr(maps), Q, n, lib.i32ptr(hw), H, lo, hi, flags, ptr("s"), ptr("r"), ptr("m"), ptr("c"), ptr("x"),
                              C.byref(buf["d"]) if "d" in outs else None)
    for k in "srmcx":                                                           # an output that was not asked for, or a refused call: untouched
        if buf[k] is not None and (k not in outs or rc != 0):
            assert (buf[k] == SENT).all(), k
    if rc != 0 or "d" not in outs:
        assert buf["d"].value == SENT
    return rc, {k: (buf[k].value if k == "d" else buf[k]) for k in outs}


def _refused(s, word, *a, **kw):
    from chromosome3d_amd import lib
    rc, _ = _call(s, *a, **kw)
    err = lib.load().c3d_last_error().decode()
    assert rc == C3D_ERR_INVALID and "c3d_map_similarity" in err and word in err, (rc, err)


def _gamma(m, u):
    return m * u / (1.0 - m * u)


def _bound(dx, dy, mx, my, m, u):
    """B(u, m) of the docstring for sum dx dy, from |dx_i|, |dy_i| and the means, in doubles"""
    ex = _gamma(m + 1, u) * mx
    ey = _gamma(m + 1, u) * my
    Ex, Ey = ex + u * (dx + ex), ey + u * (dy + ey)
    T = (dx + Ex) * (dy + Ey)
    return float((dx * Ey + dy * Ex + Ex * Ey + u * T).sum() + _gamma(m, u) * (1.0 + u) * T.sum())


def _moments_fraction(x, y, kept, N0, got):
    """the largest |device - yardstick| / bound over Cxy, Cxx, Cyy of one stratum; exact rationals up to 97 pairs, longdouble beyond"""
    xk, yk = x[kept], y[kept]
    N = len(xk)
    if N == 0:
        assert tuple(got) == (0.0, 0.0, 0.0)
        return 0.0
    m = -(-N0 // 256) + 8
    if N0 <= 97:
        # exact: every double is an integer over a power of two; with the common denominator D, N dx_i = (N x_i - sum x) / D in integers
        rx, ry = [float(v).as_integer_ratio() for v in xk], [float(v).as_integer_ratio() for v in yk]
        D = max(d for _, d in rx + ry)
        ix, iy = [a * (D // d) for a, d in rx], [a * (D // d) for a, d in ry]
        sx, sy = sum(ix), sum(iy)
        ex, ey = [N * v - sx for v in ix], [N * v - sy for v in iy]
        ND = N * D
        exact = [Fraction(sum(a * b for a, b in zip(ex, ey)), ND * ND), Fraction(sum(a * a for a in ex), ND * ND), Fraction(sum(b * b for b in ey), ND * ND)]
        dx, dy = np.array([abs(v) / ND for v in ex]), np.array([abs(v) / ND for v in ey])
        mx, my = sx / ND, sy / ND
        mx, my, extra = float(mx), float(my), None
    else:
        lx, ly = xk.astype(np.longdouble), yk.astype(np.longdouble)
        mx, my = lx.sum() / N, ly.sum() / N
        ex, ey = lx - mx, ly - my
        exact = [(ex * ey).sum(), (ex * ex).sum(), (ey * ey).sum()]
        dx, dy, mx, my, extra = np.abs(ex).astype(float), np.abs(ey).astype(float), float(mx), float(my), UL
    worst = 0.0
    for name, want, a, b, ma, mb, have in (("Cxy", exact[0], dx, dy, mx, my, got[0]), ("Cxx", exact[1], dx, dx, mx, mx, got[1]), ("Cyy", exact[2], dy, dy, my, my, got[2])):
        bound = _bound(a, b, ma, mb, m, U) + (_bound(a, b, ma, mb, N, extra) if extra else 0.0)
        gap = abs(float(type(want)(float(have)) - want))
        if bound == 0.0:
            assert gap == 0.0, name
            continue
        worst = max(worst, gap / bound)
        assert gap <= bound, f"{name}: {gap:.3g} against the bound {bound:.3g}"
    return worst


def _held(s, maps, h, lo, hi, keep, what, worst):
    """one call on the device held to the restatement and to the yardstick; returns the outputs"""
    maps = np.asarray(maps)
    Q, n = maps.shape[0], maps.shape[1]
    rc, got = _call(s, maps, h, lo, hi, 1 if keep else 0)
    assert rc == 0, what
    top = hi if hi else n - 1
    assert got["d"] >= 0.0
    for k, hk in enumerate(h):
        want = np.stack([R.smooth_band(maps[m], hk, lo, top) for m in range(Q)])
        assert got["x"][k].tobytes() == want.tobytes(), f"{what}: smoothed at h = {hk}"
        for e, (p, q) in enumerate(R.pairs(Q)):
            for sep in range(lo, top + 1):
                x, y = want[p, sep - lo, :n - sep], want[q, sep - lo, :n - sep]
                kept = R.kept_pairs(x, y, keep)
                have = tuple(int(v) for v in got["c"][k, e, sep - lo])
                assert have == (int(kept.sum()), R.rank_sums(x[kept]), R.rank_sums(y[kept])), f"{what}: counts at h = {hk}, pair {p} {q}, s = {sep}"
                worst["moments"] = max(worst["moments"], _moments_fraction(x, y, kept, n - sep, got["m"][k, e, sep - lo]))
            rho, w, scc = R.combine(got["m"][k, e], got["c"][k, e])
            assert got["r"][k, e].tobytes() == rho.tobytes(), f"{what}: rho at h = {hk}, pair {p} {q}"
            assert np.array([got["s"][k, p, q], got["s"][k, q, p]]).tobytes() == np.array([scc, scc]).tobytes(), f"{what}: scc at h = {hk}, pair {p} {q}"
        assert (np.diagonal(got["s"][k]) == 1.0).all()
    return got


@pytest.mark.parametrize("n", [3, 9, 31, 32, 33, 64, 65, 96, 97])
def test_smoothing_and_strata_at_the_tile_borders(ctx, n):
    A, B = _counts(n, 0), _counts(n, 1, 0.6)
    maps = np.stack([A, B, _balanced_like(A, n)])
    hs = (0, 1, 3, 20) if n in (9, 97) else (0, 1, 3)
    worst = {"moments": 0.0}
    windows = [(0, 0)] + ([(31, 31), (32, 63), (33, 64)] if n == 97 else [])
    if n == 97:
        maps = maps.copy()
        for b in (0, 40, 41):                                                   # three masked all-zero bins, one of them at the edge
            maps[:, b, :] = maps[:, :, b] = 0.0
    for lo, hi in windows:
        for keep in ((False, True) if n == 97 else (False,)):
            got = _held(ctx, maps, hs, lo, hi, keep, f"n = {n} separations {lo}..{hi} keep {keep}", worst)
            if n == 97 and not keep and (lo, hi) == (0, 0):
                assert (got["c"][0, :, 1:40, 0] < n - np.arange(1, 40)[None, :]).all()      # h = 0: the masked bins' pairs are dropped in every stratum they reach
            if n == 97 and keep:
                assert (got["c"][:, :, :, 0] == (n - np.arange(lo, (hi if hi else n - 1) + 1))[None, None, :]).all()
    print(f"n = {n}: moments at {worst['moments']:.3g} of the bound")


@pytest.mark.parametrize("n,lo,hi", [(257, 1, 0), (520, 1, 0), (1030, 1, 0), (2050, 1, 3)])
def test_strata_across_the_slot_classes_and_the_stride(ctx, n, lo, hi):
    maps = np.stack([_counts(n, 2), _balanced_like(_counts(n, 3, 0.7), n)])
    worst = {"moments": 0.0}
    got = _held(ctx, maps, (1,), lo, hi, False, f"n = {n}", worst)
    top = hi if hi else n - 1
    counted = int(np.isfinite(got["r"]).sum())
    assert counted >= min(top - lo + 1, 50)                                    # the near strata count; the far ones may be empty in both maps
    print(f"n = {n}: {counted} of {top - lo + 1} strata count, moments at {worst['moments']:.3g} of the bound, scc {got['s'][0, 0, 1]:.6f}")


def test_one_large_case_behind_max_beads():
    """n = 8200: P = 16384 keys, 128 KiB of dynamic LDS; two banded maps built from a handful of diagonals in a zero matrix, separations 1..2,
    h = 1, held to the band-only restatement"""
    from chromosome3d_amd import Solver
    n = 8200
    rng = np.random.default_rng(8200)
    maps = np.zeros((2, n, n))
    i = np.arange(n)
    for m in range(2):
        for d in range(0, 5):                                                   # diagonals 0..4: all that h = 1 reads for separations 1..2, and one beyond
            v = rng.poisson(30.0 / (1 + d) * (1.0 + (i[:n - d] // 50 % 2)) * (1.0 - 0.3 * m)).astype(float)
            maps[m, i[:n - d], i[:n - d] + d] = v
            maps[m, i[:n - d] + d, i[:n - d]] = v
    s = Solver(0)
    try:
        _refused(s, "max_beads", maps, (1,), 1, 2)
        s.set_option("max_beads", n)
        worst = {"moments": 0.0}
        got = _held(s, maps, (1,), 1, 2, False, "n = 8200", worst)
        assert np.isfinite(got["r"]).all() and 0.0 < got["s"][0, 0, 1] < 1.0
        print(f"n = {n}: moments at {worst['moments']:.3g} of the bound, scc {got['s'][0, 0, 1]:.6f}, device {got['d']:.2f} ms")
    finally:
        s.close()


def test_identities(ctx):
    n = 75
    A = _counts(n, 4)
    maps = np.stack([A, _counts(n, 5, 0.5), _balanced_like(_counts(n, 6), 7)])
    hs, lo, hi = (0, 2, 5), 1, 40
    rc, full = _call(ctx, maps, hs, lo, hi)
    assert rc == 0
    for k in range(len(hs)):                                                    # the table is symmetric with a unit diagonal
        assert full["s"][k].tobytes() == full["s"][k].T.copy().tobytes() and (np.diagonal(full["s"][k]) == 1.0).all()
    rc, again = _call(ctx, maps, hs, lo, hi)                                    # two calls give the same bytes
    assert rc == 0 and all(full[k].tobytes() == again[k].tobytes() for k in "srmcx")
    rc, rev = _call(ctx, maps[::-1], hs, lo, hi)                                # maps in reverse order: the permuted bytes
    assert rc == 0
    Q, pairs = 3, R.pairs(3)
    assert rev["x"][:, ::-1].tobytes() == full["x"].tobytes()
    assert rev["s"][:, ::-1, ::-1].tobytes() == full["s"].tobytes()
    for e, (p, q) in enumerate(pairs):
        f = pairs.index((Q - 1 - q, Q - 1 - p))
        assert rev["r"][:, f].tobytes() == full["r"][:, e].tobytes()
        assert rev["m"][:, f][..., [0, 2, 1]].tobytes() == full["m"][:, e].tobytes()
        assert rev["c"][:, f][..., [0, 2, 1]].tobytes() == full["c"][:, e].tobytes()
    for e, (p, q) in enumerate(pairs):                                          # a pair inside a call of three maps equals the call of the two alone
        rc, two = _call(ctx, maps[[p, q]], hs, lo, hi)
        assert rc == 0
        assert two["r"][:, 0].tobytes() == full["r"][:, e].tobytes() and two["m"][:, 0].tobytes() == full["m"][:, e].tobytes()
        assert two["c"][:, 0].tobytes() == full["c"][:, e].tobytes() and two["s"][:, 0, 1].tobytes() == full["s"][:, p, q].tobytes()
        assert two["x"].tobytes() == full["x"][:, [p, q]].tobytes()
    for k, hk in enumerate(hs):                                                 # one half-width alone equals the same one inside a list
        rc, one = _call(ctx, maps, (hk,), lo, hi)
        assert rc == 0 and all(one[key][0].tobytes() == full[key][k].tobytes() for key in "srmcx")
    for outs in ("s", "r", "mc", "x", "sd", "rmx"):                             # outputs left out change no other output
        rc, part = _call(ctx, maps, hs, lo, hi, outs=outs)
        assert rc == 0 and all(part[key].tobytes() == full[key].tobytes() for key in outs if key != "d")
    rc, same = _call(ctx, np.stack([A, A]), (0, 3), 0, 0)                       # a map against itself
    assert rc == 0
    counted = np.isfinite(same["r"])
    assert counted.any() and np.abs(same["r"][counted] - 1.0).max() <= 4 * U and abs(same["s"][0, 0, 1] - 1.0) <= (n + 4) * U      # (a weighted mean of n strata, summed in sequence)


def test_refusals_that_need_a_device(ctx):
    n = 50
    M = _counts(n, 8)
    good = np.stack([M, _counts(n, 9)])
    for spoil, word in ((np.nan, "not finite"), (np.inf, "not finite"), (-1.0, "negative")):
        bad = good.copy()
        bad[1, 3, 40] = bad[1, 40, 3] = spoil
        _refused(ctx, word, bad, (0, 1), 1, 10)
        _refused(ctx, "map 1", bad, (0, 1), 1, 10)
    bad = good.copy()
    bad[1, 3, 40] += 1.0
    _refused(ctx, "not symmetric", bad, (0, 1), 1, 10)
    _refused(ctx, "map 1", bad, (0, 1), 1, 10)
    bad = good.copy()
    bad[0, 7, 7] = -2.0
    _refused(ctx, "map 0", bad, (0,), 1, 10)
    big = np.zeros((2, 3, 3))
    _refused(ctx, "max_beads", big, (0,), 0, 0, n=5121)                          # refused before the maps are read
    for kw, word in ((dict(h=(1, 1)), "ascending"), (dict(h=(21,)), "half-width"), (dict(h=(-1,)), "half-width"), (dict(h=tuple(range(9))), "n_h"),
                     (dict(lo=n), "min_sep"), (dict(lo=5, hi=4), "max_sep"), (dict(hi=n), "max_sep"), (dict(flags=2), "flag"), (dict(n=2), "n < 3")):
        args = dict(h=(0,), lo=1, hi=10, flags=0)
        args.update(kw)
        _refused(ctx, word, good, args["h"], args["lo"], args["hi"], args["flags"], n=args.get("n"))
    _refused(ctx, "n_maps", good[:1], (0,), 1, 10)
    _refused(ctx, "n_maps", np.zeros((17, 4, 4)), (0,), 0, 0)
    rc, got = _call(ctx, good, (0, 1), 1, 10)                                     # and the context still serves
    assert rc == 0 and np.isfinite(got["s"]).all()


def test_through_the_solver_and_the_report(ctx):
    from chromosome3d_amd import pipeline
    n = 60
    maps = np.stack([_counts(n, 10), _counts(n, 10, 0.5), _counts(n, 11)])
    out = pipeline.map_similarity_report(ctx, maps, names=("a", "a_half", "b"), h=(0, 1, 2), min_sep=1, max_sep=30)
    rc, got = _call(ctx, maps, (0, 1, 2), 1, 30)
    assert rc == 0 and out["scc"].tobytes() == got["s"].tobytes() and out["rho"].tobytes() == got["r"].tobytes()
    assert out["counts"].tobytes() == got["c"].tobytes() and out["moments"].tobytes() == got["m"].tobytes()
    assert out["pairs"] == R.pairs(3) and out["h"] == [0, 1, 2] and out["device_ms"] >= 0
    assert "# h = 2" in out["text"] and "a_half" in out["text"] and "%.9f" % out["scc"][1, 0, 2] in out["text"]
    sm = ctx.map_similarity(maps, h=(1,), min_sep=1, max_sep=30, want_smoothed=True)
    assert sm["smoothed"].tobytes() == got["x"][1:2].tobytes()
    h = pipeline.choose_smoothing({hk: out["scc"][k, 0, 1] for k, hk in enumerate(out["h"])})
    assert h in (0, 1, 2)


def test_the_cli_prints_the_table_the_abi_returns(ctx, tmp_path):
    """c3d_solve --if a --map-similarity b --map-similarity c: the printed table and the files parse back to the doubles the entry returns"""
    from tests.util import load_if, write_if_text
    S = load_if("chr21_1mb")
    n = S.shape[0]
    rng = np.random.default_rng(21)
    others = [np.triu(S * rng.uniform(0.5, 1.5, S.shape)) for _ in range(2)]
    maps = np.stack([S] + [o + np.triu(o, 1).T for o in others])
    paths = [str(tmp_path / ("m%d_matrix.txt" % m)) for m in range(3)]
    for m in range(3):
        write_if_text(maps[m], paths[m])
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    prefix = str(tmp_path / "sim")
    run = subprocess.run([exe, "--if", paths[0], "--out", str(tmp_path / "a"), "-m", "2", "--quiet", "--map-similarity", paths[1], "--map-similarity", paths[2],
                          "--map-similarity-h", "0,2", "--map-similarity-sep", "1:12", "--map-similarity-out", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rc, got = _call(ctx, maps, (0, 2), 1, 12)
    assert rc == 0
    rows = [l.split() for l in run.stdout.splitlines() if l.startswith("Similarity :")]
    assert len(rows) == 6
    for row in rows:
        k, m = (0, 2).index(int(row[3])), int(row[5]) - 1
        assert np.array([float(v) for v in row[7:]]).tobytes() == got["s"][k, m].tobytes()
    lines = open(prefix + "_scc.txt").read().splitlines()
    assert lines[0] == "h map scc..." and len(lines) == 7
    assert np.array([float(v) for v in lines[6].split()[2:]]).tobytes() == got["s"][1, 2].tobytes()
    lines = open(prefix + "_strata.txt").read().splitlines()
    assert lines[0] == "h map_p map_q separation kept rho" and len(lines) == 1 + 2 * 3 * 12
    f = lines[1 + 12 + 4].split()                                               # h = 0, pair (1, 3), separation 5
    assert f[:4] == ["0", "1", "3", "5"] and int(f[4]) == got["c"][0, 1, 4, 0] and float(f[5]) == got["r"][0, 1, 4]
    bad = subprocess.run([exe, "--if", paths[0], "--out", str(tmp_path / "b"), "--map-similarity-out", prefix], capture_output=True, text=True)
    assert bad.returncode == 2 and "--map-similarity-out needs --map-similarity" in bad.stderr
