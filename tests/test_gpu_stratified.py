"""IF against model distance inside every genomic separation on the device (c3d_stratified_score; csrc/c3d_score_stratified.inc k_str_if,
k_str_model) against the numpy restatement tests/stratified_ref.py, which tests/test_stratified_ref.py holds to scipy's spearmanr and to
Python's "%.3f".

The kernels' constants.  A workgroup is kStrThreads = 256 threads and sorts one stratum's N = n - s keys, padded to P = a power of two >=
kStrMinSlots = 8, in LDS (64-bit keys for IF, 32-bit for the distances).  A thread sorts kStrChunk = 4 consecutive keys in registers: the
network's strides 1 and 2 never touch LDS a key at a time; the strides >= 4 are LDS passes of 16-byte vectors (4 keys of 32 bits, 2 of 64
bits).  So a thread owns one chunk up to P = 1024 and several from P = 2048 on, one comparator vector up to P = 1024 (64-bit) / 2048
(32-bit) and several from P = 2048 / 4096 on; at P <= 512 some threads own nothing.  Launches are grouped by P.  A single n runs every
stratum length from n - range down to 1, so few sizes cover every edge:
  n5      2 replicas, range 1: N = 4, 3, 2, 1, all in the smallest network (P = 8, two chunks, one vector pass)
  n131    2 replicas, ranges 1 and 3: every N in 1 .. 130 — each power of two 8 .. 128 with both neighbours (the launch groups' edges), the
          wave (64) and, with P = 256, the first network in which every thread of the workgroup owns a chunk
  n2100   2 replicas + 1 extra fp64 model that no float holds: N up to 2099 > 2048, so P = 4096, where a thread owns four chunks and, on
          both key widths, more than one comparator vector; P = 512 .. 2048 on the way; also max_sep 700
  n16384  1 replica, analytic coordinates, (range, max_sep) = (1, 2) and (8191, 8193): P = 16384 (N = 16383, 16382, 8193: 128 KiB of 64-bit
          keys) and the edge N = 8192 | 8191; the five diagonals alone are compared
The tie cases (two IF values a stratum, a zero band with -0.0 in it, a lattice model, the straight chain) run at n131.

Bounds.  `sums` (C, A, B) are exact integers: ==.  rho and scc are formed on the host of the library by IEEE operations (int64 -> double,
x, sqrt, /, +) from equal integers in the order the restatement uses: bitwise equal, NaN where and only where the restatement has NaN
(on the CPU: tests/test_stratified_ref.py).  Were they ever formed on the device instead, the bound would be 2 ulps a stratum, one each
for the product and the square root."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import stratified_ref as S
from tests.util import GOLD, SHORT, golden, load_if, load_pdb_xyz, random_coil, restrained, shared_models, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _context(s, n, nrep):
    if n >= 8:
        return restrained(s, n, nrep)
    from chromosome3d_amd import default_model, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
    s.init_replicas(nrep)


def _noisy_if(n, seed):
    """a symmetric matrix without structure to spare: distinct positive values, the diagonal large"""
    rng = np.random.default_rng(seed)
    m = rng.lognormal(size=(n, n)) / (1.0 + np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]))
    m = np.triu(m, 1)
    return m + m.T + np.diag(np.full(n, 100.0))


def _host(IF, models, rng, max_sep=0, strata=None):
    cache = {}
    return [S.stratified(IF, m, rng, max_sep, strata, cache) for m in models]


def _check(got, host, what, strata=None):
    """sums ==, rho and scc bitwise, NaN exactly where the restatement has it; strata: the only separations compared (n16384)"""
    for k, h in enumerate(host):
        rows = slice(None) if strata is None else list(strata)
        assert np.array_equal(got["sums"][k][rows], h["sums"][rows]), (what, k)
        assert np.array_equal(np.isnan(got["rho"][k][rows]), np.isnan(h["rho"][rows])), (what, k)
        assert got["rho"][k][rows].tobytes() == h["rho"][rows].tobytes(), (what, k)
        if strata is None:
            assert np.float64(got["scc"][k]).tobytes() == np.float64(h["scc"]).tobytes(), (what, k, got["scc"][k], h["scc"])
    print(f"{what}: scc {[float('%.4f' % v) for v in got['scc']]}, strata with a coefficient {[int((~np.isnan(r)).sum()) for r in got['rho']]}")


def test_the_smallest_network(ctx):
    n = 5
    x = np.stack([random_coil(n, 50 + r) for r in range(2)])
    _context(ctx, n, 2)
    ctx.set_coords(x)
    IF = _noisy_if(n, 5)
    got = ctx.stratified_score(IF, 1, 0, None, True)
    host = _host(IF, [m.astype(np.float64) for m in x], 1)
    _check(got, host, "n5")
    # s = 0 is not a stratum, the bonds of a random coil all print as 3.800 (a constant side), s = 4 has N = 1
    assert np.isnan(got["rho"][:, [0, 1, 4]]).all() and not np.isnan(got["rho"][:, 2:4]).any()


@pytest.mark.parametrize("rng", [1, 3])
def test_every_stratum_length_up_to_130(ctx, rng):
    n = 131
    x = np.stack([random_coil(n, 1310 + r) for r in range(2)])
    _context(ctx, n, 2)
    ctx.set_coords(x)
    IF = _noisy_if(n, 131)
    got = ctx.stratified_score(IF, rng, 0, None, True)
    _check(got, _host(IF, [m.astype(np.float64) for m in x], rng), f"n131 range {rng}")
    # (stratum 1 of a random coil is constant: every bond prints as 3.800)
    lo = max(rng, 2)
    assert not np.isnan(got["rho"][:, lo:n - 1]).any() and np.isnan(got["rho"][:, n - 1]).all() and np.isnan(got["rho"][:, :lo]).all()


def test_past_2048_keys_and_a_band(ctx):
    n = 2100
    x = np.stack([random_coil(n, 21000 + r) for r in range(2)])
    rng = np.random.default_rng(2100)
    extra = random_coil(n, 21009).astype(np.float64) * 1.5 + rng.normal(scale=1e-3, size=(n, 3))
    assert not np.array_equal(extra, extra.astype(np.float32))
    _context(ctx, n, 2)
    ctx.set_coords(x)
    IF = synthetic_if(n, seed=n)[0]
    models = [m.astype(np.float64) for m in x] + [extra]
    got = ctx.stratified_score(IF, 3, 0, extra, True)
    host = _host(IF, models, 3)
    _check(got, host, "n2100")
    band = ctx.stratified_score(IF, 3, 700, extra, True)
    _check(band, _host(IF, models, 3, 700), "n2100 max_sep 700")
    assert (band["sums"][:, 701:] == 0).all() and np.isnan(band["rho"][:, 701:]).all()
    assert np.array_equal(band["sums"][:, :701], got["sums"][:, :701])          # a band of the full call's sums: a band-limited scc needs no second call
    for k in range(3):
        assert band["scc"][k] == S.scc_of({s: tuple(int(v) for v in got["sums"][k, s]) for s in range(3, 701)}, n, range(3, 701))


def test_the_largest_network_and_the_8192_edge():
    """16384 beads on a Lissajous curve, IF = (i + j) mod 1021: symmetric, 1021 values a stratum (ties throughout), both sides vary along
    every diagonal.  Only strata 1, 2 and 8191 .. 8193 are sorted."""
    from chromosome3d_amd import Solver, default_model, make_stages
    n = 16384
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(n, np.array([1], np.int32), np.array([11], np.int32), np.array([100], np.int32))
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
        for rng, max_sep in ((1, 2), (8191, 8193)):
            strata = list(range(rng, max_sep + 1))
            got = s.stratified_score(IF, rng, max_sep, None, True)
            host = _host(IF, [xd], rng, max_sep, strata)
            _check(got, host, f"n16384 strata {strata}", strata)
            assert np.float64(got["scc"][0]).tobytes() == np.float64(host[0]["scc"]).tobytes()
            assert not np.isnan(got["rho"][0, strata]).any()
            outside = np.setdiff1d(np.arange(n), strata)
            assert (got["sums"][0, outside] == 0).all() and np.isnan(got["rho"][0, outside]).all()
    finally:
        s.close()


def _lattice(n, seed):
    rng = np.random.default_rng(seed)
    step = np.zeros((n, 3))
    step[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-3.0, 3.0], n)
    return np.cumsum(step, axis=0).astype(np.float32)


def test_ties_on_either_side(ctx):
    n = 131
    chain = np.zeros((n, 3), np.float32)
    chain[:, 0] = 1.5 * np.arange(n)
    x = np.stack([_lattice(n, 7), chain])
    _context(ctx, n, 2)
    ctx.set_coords(x)
    models = [m.astype(np.float64) for m in x]
    i, j = np.indices((n, n))
    two = ((np.minimum(i, j) // 7) % 2).astype(np.float64) + 1.0                # two values a stratum
    band = _noisy_if(n, 9)
    band[(np.abs(i - j) >= 10) & (np.abs(i - j) <= 20)] = 0.0                   # strata that are all zero: constant, NaN
    low = (np.abs(i - j) == 30) & (np.minimum(i, j) % 3 == 0)
    band[low] = 0.0
    band[low & (i < j)] = -0.0                                                  # -0.0 above the diagonal, 0.0 below: equal, and tied
    for name, IF in (("two values", two), ("zero band", band), ("distinct", _noisy_if(n, 11))):
        got = ctx.stratified_score(IF, 1, 0, None, True)
        host = _host(IF, models, 1)
        _check(got, host, f"ties, IF {name}")
        assert np.isnan(got["rho"][1]).all() and np.isnan(got["scc"][1])        # the straight chain: every stratum of distances is constant
        assert (got["sums"][1][:, [0, 2]] == 0).all()
    got = ctx.stratified_score(band, 1, 0, None, True)
    assert np.isnan(got["rho"][0, 10:21]).all() and (got["sums"][0, 10:21, 1] == 0).all() and not np.isnan(got["rho"][0, [9, 21, 30]]).any()
    d = S.round_milli(S.diagonal_distances(models[0], 5))
    assert len(np.unique(d)) < len(d) // 4                                      # the lattice model ties its distances


@pytest.mark.parametrize("cid", sorted(golden()))
def test_the_bundled_models(ctx, cid):
    g = golden()[cid]
    x = load_pdb_xyz(os.path.join(GOLD, "models", g["model"]))
    IF = load_if(cid)
    n = g["n"]
    _context(ctx, n, 1)
    got = ctx.stratified_score(IF, 3, 0, x, True)
    host = _host(IF, [ctx.coords()[0].astype(np.float64), x], 3)
    _check(got, host, cid)
    assert not np.isnan(got["rho"][1, 3:n - 1]).any() and -1.0 < got["scc"][1] < 0.0


def test_f64_state_is_ranked_in_doubles():
    """A precision-64 context: the sums follow the fp64 state, not its float rounding.  Coordinates near 9000 A, where a float's last place
    is 1e-3 A: rounding them to float moves the "%.3f" distances of a lattice model's many near-ties."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        n = 96
        restrained(s, n, 3)
        rng = np.random.default_rng(96)
        x = np.stack([_lattice(n, 960 + r).astype(np.float64) + 9000.0 for r in range(3)]) + rng.normal(scale=2e-3, size=(3, n, 3))
        IF = _noisy_if(n, 96)
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x)
        got = s.stratified_score(IF, 2, 0, None, True)
        _check(got, _host(IF, list(x), 2), "f64")
        rounded = _host(IF, list(x.astype(np.float32).astype(np.float64)), 2)
        assert all(not np.array_equal(got["sums"][k], rounded[k]["sums"]) for k in range(3))
    finally:
        s.close()


def test_two_calls_return_the_same_bytes_and_nothing_of_the_solve_changes(ctx):
    from chromosome3d_amd import lib
    x, extra = shared_models("n257")
    n = 257
    _context(ctx, n, 5)
    ctx.set_coords(x)
    IF = _noisy_if(n, 257)
    ctx.run_steps(20)                                                           # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    runs = ctx.stat("stratified_runs")
    a, b = ctx.stratified_score(IF, 3, 0, extra, True), ctx.stratified_score(IF, 3, 0, extra, True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    alone = ctx.stratified_score(IF, 3, 0, None, True)                          # without the extra models: the replicas keep their bits
    for k in a:
        assert alone[k].tobytes() == a[k][:5].tobytes(), k
    _check(a, _host(IF, [m.astype(np.float64) for m in before[0]] + list(extra), 3), "n257 mid-solve")
    # each output alone: the same bytes
    rho, scc, sums = np.empty((7, n)), np.empty(7), np.empty((7, n, 3), np.int64)
    sp = sums.ctypes.data_as(C.POINTER(C.c_int64))
    for args, out, want in (((lib.dptr(rho), None, None), rho, a["rho"]), ((None, lib.dptr(scc), None), scc, a["scc"]), ((None, None, sp), sums, a["sums"])):
        assert ctx._L.c3d_stratified_score(ctx._h, lib.dptr(IF), 3, 0, lib.dptr(extra), 2, *args) == 0
        assert out.tobytes() == want.tobytes()
    assert ctx.stat("stratified_runs") == runs + 6
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
    _context(ctx, n, M)
    ctx.set_coords(x)
    L, h = ctx._L, ctx._h
    IF = _noisy_if(n, 64)
    runs, state = ctx.stat("stratified_runs"), ctx.coords().tobytes()
    rho, scc, sums = np.full((300, n), 7.0), np.full(300, 7.0), np.full((300, n, 3), 7, np.int64)
    outs = (lib.dptr(rho), lib.dptr(scc), sums.ctypes.data_as(C.POINTER(C.c_int64)))
    good = x.astype(np.float64)
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows

    def refused(*a):
        assert L.c3d_stratified_score(h, *a) == -1 and b"c3d_stratified_score" in L.c3d_last_error(), a
        assert (rho == 7.0).all() and (scc == 7.0).all() and (sums == 7).all(), a    # nothing written

    refused(None, 3, 0, None, 0, *outs)                                         # no IF
    refused(lib.dptr(IF), 0, 0, None, 0, *outs)                                 # range < 1
    refused(lib.dptr(IF), -2, 0, None, 0, *outs)
    refused(lib.dptr(IF), 3, -1, None, 0, *outs)                                # max_sep < 0
    refused(lib.dptr(IF), 3, n, None, 0, *outs)                                 # max_sep > n-1
    refused(lib.dptr(IF), 3, 2, None, 0, *outs)                                 # 0 < max_sep < range
    refused(lib.dptr(IF), n, 0, None, 0, *outs)                                 # range > n-1
    refused(lib.dptr(IF), 3, 0, None, 0, None, None, None)                      # every output NULL
    refused(lib.dptr(IF), 3, 0, None, 1, *outs)                                 # n_extra > 0 without coordinates
    refused(lib.dptr(IF), 3, 0, lib.dptr(good), -1, *outs)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(lib.dptr(IF), 3, 0, lib.dptr(e), M, *outs)
    refused(lib.dptr(IF), 3, 0, lib.dptr(big), len(big), *outs)                 # K = 257
    # found by the first pass: asymmetry and a value that is not finite, inside the strata asked for only
    asym = IF.copy()
    asym[10, 20] += 1.0
    refused(lib.dptr(asym), 3, 0, None, 0, *outs)
    assert b"symmetric" in L.c3d_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        e = IF.copy()
        e[7, 30] = e[30, 7] = bad
        refused(lib.dptr(e), 3, 0, None, 0, *outs)
        assert b"not finite" in L.c3d_last_error()
    # found by the second pass: a model wider than 50 000 A
    far = good.copy()
    far[1, n - 1, 0] = 60000.0
    refused(lib.dptr(IF), 3, 0, lib.dptr(far), M, *outs)
    assert b"50000" in L.c3d_last_error()
    assert ctx.stat("stratified_runs") == runs and ctx.coords().tobytes() == state
    # outside the strata asked for neither matters: |i-j| = 10 and 23 are not in 3 .. 9
    e = asym.copy()
    e[7, 30] = np.nan
    host = _host(IF, list(good), 3, 9)
    _check(ctx.stratified_score(e, 3, 9, None, True), host, "n64 band 3..9")
    # 256 models are accepted, exactly 50 000 A too, and the context works
    wide = good[:1].copy()
    wide[0, :, :] = 0.0
    wide[0, :, 0] = np.linspace(0.0, 50000.0, n)
    many = np.concatenate([big[:-2] + good[0], wide])
    got = ctx.stratified_score(IF, 3, 0, many, True)
    full = _host(IF, list(good), 3)
    assert np.array_equal(got["sums"][0], full[0]["sums"]) and np.array_equal(got["sums"][254], full[0]["sums"]) and got["scc"][254] == got["scc"][0]
    end = _host(IF, [wide[0]], 3)[0]                                            # 50 000.000 A between its ends: the limit itself is inside
    assert np.array_equal(got["sums"][255], end["sums"]) and S.round_milli(S.diagonal_distances(wide[0], n - 1))[0] == S.FARTHEST
    assert ctx.stat("stratified_runs") == runs + 2
    # no replicas; 2 beads: one stratum of one pair
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_stratified_score.*c3d_init_replicas"):
            s2.stratified_score(np.ones((2, 2)), 1)
        s2.init_replicas(2)
        two = s2.stratified_score(np.ones((2, 2)), 1, 0, None, True)
        assert np.isnan(two["rho"]).all() and np.isnan(two["scc"]).all() and (two["sums"] == 0).all() and s2.stat("stratified_runs") == 1
    finally:
        s2.close()
    s1 = Solver(0)
    try:
        s1.set_model(default_model())
        s1.set_schedule(make_stages(SHORT))
        s1.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        s1.init_replicas(1)
        assert s1._L.c3d_stratified_score(s1._h, lib.dptr(np.ones((2, 2))), 1, 0, None, 0, None, None, None) == -1
    finally:
        s1.close()


def _bounds(C_, A, B, dC, dB):
    """the interval of C' / sqrt(A B') over |C' - C| <= dC, |B' - B| <= dB (A > 0, B - dB > 0)"""
    corners = [c / np.sqrt(float(A) * float(b)) for c in (C_ - dC, C_ + dC) for b in (B - dB, B + dB)]
    return min(corners), max(corners)


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --stratified on the smallest bundled matrix: both files, rows in rank order, and numbers that are Solver.stratified_score's
    of the written models.  A written coordinate is rounded to 3 decimals, so a written distance lies within sqrt(3) 1e-3 A of the one the
    run ranked and its thousandths within 2 of the run's: two distances of a stratum keep their order (and stay apart) when their written
    thousandths differ by more than 4.  Where that holds for a whole stratum the ranks are the run's and rho equals the file's to its printed
    digits.  Elsewhere an element with c partners within 4 thousandths moves its doubled rank b by at most 2 c, which bounds the change of
    sum a b and sum b^2, and the file's number lies between the extremes (as tests/test_gpu_geometry.py brackets its clash counts)."""
    cid, M = "chr21_1mb", 4
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "str")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--stratified", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = [l.split() for l in open(prefix + "_scc.txt") if not l.startswith("#")]
    assert len(rows) == M and [int(r[0]) for r in rows] == [1, 2, 3, 4] and sorted(int(r[1]) for r in rows) == [1, 2, 3, 4] and all(len(r) == 3 for r in rows)
    n = 37
    strata = [l.split() for l in open(prefix + "_strata.txt") if not l.startswith("#")]
    assert [int(r[0]) for r in strata] == list(range(3, n)) and [int(r[1]) for r in strata] == [n - s for s in range(3, n)] and all(len(r) == 2 + M for r in strata)
    assert strata[-1][2:] == ["nan"] * M                                        # N = 1, printed as nan
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r + 1}.pdb") for r in range(M)])
    IF = load_if(cid)
    restrained(ctx, n, M)
    ctx.set_coords(x)
    got = ctx.stratified_score(IF, 3, 0, None, True)
    exact = bracketed = 0
    for col, r in enumerate(rows):
        k = int(r[1]) - 1
        num, den = [0.0, 0.0], [0.0, 0.0]
        for row in strata[:-1]:
            s = int(row[0])
            N = n - s
            Cs, A, B = (int(v) for v in got["sums"][k, s])
            q = S.round_milli(S.diagonal_distances(x[k].astype(np.float64), s))
            c = (np.abs(q[:, None] - q[None, :]) <= 4).sum(1) - 1
            a, b = S.if_ranks(np.diagonal(IF, s)), S.doubled_ranks(q)
            dC, dB = N * int((a * 2 * c).sum()), N * int((2 * b * 2 * c + 4 * c * c).sum())
            printed = float(row[2 + col])
            cN = float(N) ** 3
            if dC == 0 and dB == 0:
                assert abs(printed - got["rho"][k, s]) <= 5.000001e-7, (r, s)
                exact += 1
            if B - dB > 0:
                lo, hi = _bounds(Cs, A, B, dC, dB)
                assert lo - 5.000001e-7 <= printed <= hi + 5.000001e-7, (r, s, lo, printed, hi)
                bracketed += 1
            num[0] += (Cs - dC) / cN; num[1] += (Cs + dC) / cN
            den[0] += np.sqrt(float(A) * float(max(B - dB, 0))) / cN; den[1] += np.sqrt(float(A) * float(B + dB)) / cN
        corners = [p / q_ for p in num for q_ in den if q_ > 0]
        print(f"rank {r[0]} model {r[1]}: scc {r[2]} (of the written model {got['scc'][k]:.6f}, bracket {min(corners):.6f} .. {max(corners):.6f})")
        assert min(corners) - 5.000001e-7 <= float(r[2]) <= max(corners) + 5.000001e-7
    print(f"strata equal to the printed digits: {exact}, bracketed: {bracketed} of {M * (n - 4)}")
    assert exact > 0
    band = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", str(M), "--quiet", "--stratified", str(tmp_path / "band"), "--stratified-max-sep", "12"],
                          capture_output=True, text=True)
    assert band.returncode == 0, band.stderr
    assert [int(l.split()[0]) for l in open(tmp_path / "band_strata.txt") if not l.startswith("#")] == list(range(3, 13))
    assert "separations 3..12" in open(tmp_path / "band_scc.txt").read()
    no_if = subprocess.run([exe, "--tbl", str(tmp_path / "a" / "contact.tbl"), "--n", "37", "--out", str(tmp_path / "c"), "--stratified", prefix], capture_output=True, text=True)
    assert no_if.returncode == 2 and "--stratified needs --if" in no_if.stderr
