"""The distance-geometry start (A7, csrc/c3d_embed.hip) against the fp64 oracle, at every size it accepts.

  A. the smoothed bounds (k_dg_bounds, the blocked Floyd-Warshall passes k_fw_u_12 / k_fw_u_3 / k_fw_l_12 / k_fw_l_3, k_dg_clamp) element by
     element through the hook c3d_dg_smoothed_bounds: one block (n <= 32, phases 2 and 3 never launched), one-bead last blocks (33, 65,
     1025), up to 2100 beads; K1 targets with beads that have no data, and sparse restraints whose upper bounds route through many hops
  B. the trial distances (k_dg_trial) and the eigen stage (k_dg_eig) from the device's own bounds, up to the 4549-bead limit, where the
     eigen stage runs on 160 KiB of dynamic LDS and every thread owns up to five elements of a vector
  C. replica keying and repeatability        D. the embedded start of a precision-64 context, and fp64 FIRE steps from it
  E. the unit's LDS allowance in both load modes (fresh processes)        F. the limit: 4550 beads are refused, by the library and c3d_solve

Every test runs on a context of its own (module fixture) whose schedule is set here: the lower bound of unrestrained pairs is the last
stage's repel x r0_rep."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.util import oracle_fire_from, oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 82364
FIRE10 = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0)]     # one FIRE stage: repel 0.5, so unrestrained pairs start at [0.5 r0_rep, inf)
# Tolerances of A, fp32 device against the fp64 oracle; measured worst over every case: U 1.9e-7 relative (2100 beads, sparse),
# L 1.9e-7 of max U (1025, sparse)
U_RTOL, U_ATOL = 5e-7, 1e-6                      # |U - Uo| <= U_RTOL Uo + U_ATOL
L_TOL = 5e-7                                     # |L - Lo| <= L_TOL max(Uo)


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _lower(m):
    return float(np.float32(np.float32(FIRE10[-1][5]) * np.float32(m.r0_rep)))


def _k1(s, n):
    """K1 targets of synthetic_if(n) with beads n // 3 and n - 1 left without data (all-zero rows and columns) where n >= 5;
    returns (d10, model, U0): U0 = the float32 starting upper bound on |i - j| = 1 and on restrained pairs, 0 elsewhere."""
    from chromosome3d_amd import default_model, make_stages, pipeline
    IF = synthetic_if(n, seed=n)[0]
    if n >= 5:
        IF[[n // 3, n - 1], :] = 0.0
        IF[:, [n // 3, n - 1]] = 0.0
    m = default_model()
    s.set_model(m)
    s.set_schedule(make_stages(FIRE10))
    d10 = pipeline.IF2dist_new(s, IF)
    return d10, m, _start(m, d10)


def _sparse(s, n):
    """set_restraints: a band |i - j| = 5 .. 12 and about 2n long-range pairs, targets from a coil (>= 1 A)"""
    from chromosome3d_amd import default_model, make_stages
    rng = np.random.default_rng(n)
    truth = random_coil(n, n).astype(np.float64) * 0.5
    ri = np.concatenate([np.arange(n - k) for k in range(5, 13) if k < n] + [np.zeros(0, int)])
    rj = np.concatenate([np.arange(k, n) for k in range(5, 13) if k < n] + [np.zeros(0, int)])
    li, lj = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    keep = np.abs(li - lj) > 12
    li, lj = np.minimum(li, lj)[keep][:2 * n], np.maximum(li, lj)[keep][:2 * n]
    key = np.unique(np.concatenate([ri * n + rj, li * n + lj]))    # no pair twice: the library keeps the last of duplicates
    ri, rj = key // n, key % n
    t10 = np.maximum(np.round(np.linalg.norm(truth[ri] - truth[rj], axis=1) * 10.0), 10).astype(np.int32)
    m = default_model()
    s.set_model(m)
    s.set_schedule(make_stages(FIRE10))
    s.set_restraints(n, (ri + 1).astype(np.int32), (rj + 1).astype(np.int32), t10)
    d10 = np.zeros((n, n), dtype=np.int32)
    d10[ri, rj] = t10
    d10[rj, ri] = t10
    return d10, m, _start(m, d10)


def _start(m, d10):
    n = d10.shape[0]
    sep = np.abs(np.arange(n)[:, None] - np.arange(n)[None])
    U0 = np.where((sep >= m.min_sep) & (d10 > 0), (d10 / 10.0).astype(np.float32), np.float32(0.0))
    U0[sep == 1] = np.float32(m.b0)
    return U0


# ---------------------------------------------------------------------------------------------------------------------------------
A_SIZES = [2, 3, 5, 31, 32, 33, 63, 64, 65, 96, 455, 1025, 1819, 2100]


@pytest.mark.parametrize("kind", ["k1", "sparse"])
@pytest.mark.parametrize("n", A_SIZES)
def test_smoothed_bounds_match_the_oracle(ctx, O, n, kind):
    """c3d_dg_smoothed_bounds against c3o_dg_smooth(c3o_dg_bounds(...)) element by element: U within U_RTOL relative (+ U_ATOL), L within
    L_TOL of max U; L <= U, zero diagonals, and U never above its starting bound (b0 on the chain, the target on a restrained pair; it is
    lower where a path through restraints is shorter).  A wrong tile, a skipped phase or a dropped k is off by whole Angstroms.
    Measured worst (fp32 path sums against fp64): see U_RTOL / L_TOL; these inputs' shortest paths run through restraints in a few dozen
    hops at most (a bare chain of thousands of hops rounds once per hop: test_the_limit_is_4549_beads).  The oracle's smoothing is O(n^3)
    on the host: 2100 beads take 8 s a call on the GPU machine's CPU (25 s on a slower one), most of this file's time."""
    d10, m, U0 = (_k1 if kind == "k1" else _sparse)(ctx, n)
    t0 = time.perf_counter()
    U, L = ctx.dg_bounds()
    Uo, Lo = O.dg_smooth(*O.dg_bounds(oracle_model_from(m, n), d10, _lower(m)))
    t1 = time.perf_counter()
    assert U.shape == L.shape == (n, n) and np.isfinite(U).all() and np.isfinite(L).all()
    assert (np.diag(U) == 0).all() and (np.diag(L) == 0).all()
    assert (L <= U).all()
    start = U0 > 0
    assert (U[start] <= U0[start]).all(), np.argwhere(start & (U > U0))[:5]
    eu = np.abs(U.astype(np.float64) - Uo)
    el = np.abs(L.astype(np.float64) - Lo)
    umax = Uo.max()
    assert (eu <= U_RTOL * Uo + U_ATOL).all(), (np.argwhere(eu > U_RTOL * Uo + U_ATOL)[:5], (eu / np.maximum(Uo, 1e-30)).max())
    assert el.max() <= L_TOL * umax, (np.argwhere(el > L_TOL * umax)[:5], el.max() / umax)
    off = ~np.eye(n, dtype=bool)
    print(f"n={n} {kind}: U rel {(eu[off] / Uo[off]).max():.2e}, L {el.max() / umax:.2e} of max U {umax:.1f}, "
          f"restraints {ctx.num_restraints}, {t1 - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_error(x, xo, ch=512):
    """max |d_ij - do_ij| over all pairs and max do_ij, by row blocks (no n x n x 3 array at 4549 beads)"""
    x = x.astype(np.float64)
    worst, dmax = 0.0, 0.0
    for a in range(0, x.shape[0], ch):
        dg = np.linalg.norm(x[a:a + ch, None] - x[None], axis=-1)
        do = np.linalg.norm(xo[a:a + ch, None] - xo[None], axis=-1)
        worst, dmax = max(worst, float(np.abs(dg - do).max())), max(dmax, float(do.max()))
    return worst, dmax


@pytest.mark.parametrize("n", [2, 33, 1025, 1819, 4549])
def test_trial_distances_and_eigen_stage_follow_the_oracle(ctx, O, n):
    """embed(50) of 20 replicas from first replica 7 against c3o_dg_trial_d2 + c3o_dg_embed of replica 7 + r, both from the device's
    smoothed bounds in fp64 (so this tests k_dg_trial and k_dg_eig alone): embedded pair distances of replicas 0, 1 and 19 within 2e-6 of
    the largest (measured worst 2.2e-7, at 4549 beads; test_dg_embedding_matches_oracle, which smooths in fp64 on its side, allows
    2e-3), and every replica centred to 2e-7 of its largest coordinate (measured 2.1e-8).  1819 is the first size above 64 KB of dynamic
    LDS, 4549 the last the library accepts (163 780 B).  With n < 4 the metric matrix has rank n - 1 < 3: its other eigenvectors are
    rounding noise in both implementations, so only the first n - 1 coordinates are compared there."""
    d10, m, _ = _k1(ctx, n)
    ctx.init_replicas(20, SEED, 7)
    ctx.embed(50)
    x = ctx.coords()
    U, L = (a.astype(np.float64) for a in ctx.dg_bounds())
    assert np.isfinite(x).all()
    k = min(3, n - 1)
    worst = 0.0
    for r in (0, 1, 19):
        xo = O.dg_embed(O.dg_trial_d2(U, L, SEED, 7 + r), SEED, 7 + r, 50)
        e, dmax = _pair_error(x[r][:, :k], xo[:, :k])
        assert e < 2e-6 * dmax, (r, e, dmax)
        worst = max(worst, e / dmax)
    c = np.abs(x.astype(np.float64).mean(1)).max(1) / np.abs(x).max((1, 2))
    assert (c < 2e-7).all(), c.max()
    print(f"n={n}: pair distances {worst:.2e} of the largest, centre {c.max():.2e} of max |x|")


# ---------------------------------------------------------------------------------------------------------------------------------
def test_replicas_are_keyed_by_id_and_embedding_repeats(ctx):
    """A replica's embedding depends only on (seed, first_replica + r): replica 2 of five from id 7 equals replica 0 of one from id 9, bit
    for bit; embedding twice gives the same bits.  1025 beads: the eigen stage's per-thread loops take two elements."""
    _k1(ctx, 1025)
    ctx.init_replicas(5, SEED, 7)
    ctx.embed(50)
    a = ctx.coords()
    ctx.embed(50)
    assert np.array_equal(a, ctx.coords())
    ctx.init_replicas(1, SEED, 9)
    ctx.embed(50)
    b = ctx.coords()
    assert np.array_equal(a[2], b[0])
    assert not np.array_equal(a[1], a[2])


def test_precision_64_imports_the_embedded_start(ctx, O):
    """A precision-64 context embeds with the same fp32 kernels and imports the result: its coords() equal the fp32 context's bit for bit.
    Ten fp64 FIRE steps from there follow the oracle from the same start within test_fp64_column_layouts_follow_the_oracle's tolerance."""
    from chromosome3d_amd import Solver, default_fire, make_stages
    n = 1025
    d10, m, _ = _k1(ctx, n)
    ctx.init_replicas(2, SEED, 0)
    ctx.embed(50)
    x32 = ctx.coords()
    IF = synthetic_if(n, seed=n)[0]
    IF[[n // 3, n - 1], :] = 0.0
    IF[:, [n // 3, n - 1]] = 0.0
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        s.set_model(m)
        s.set_if_matrix(IF)
        assert np.array_equal(s.dist10(), d10)
        s.set_schedule(make_stages(FIRE10), default_fire())
        s.init_replicas(2, SEED, 0)
        s.embed(50)
        x0 = s.coords()
        assert np.array_equal(x0, x32)
        assert s.run_steps(10) == 10
        assert s.step_kernel_name.startswith("c3d::k64_step<"), s.step_kernel_name
        x = s.coords()
    finally:
        s.close()
    om, of = oracle_model_from(m, n), oracle_fire_from(default_fire())
    for r in range(2):
        xo, _, ev = O.run_schedule(om, d10, O.make_stages(FIRE10), of, SEED, r, x0=x0[r].astype(np.float64))
        assert ev == 10
        xc = x[r].astype(np.float64)
        tol = max(2e-5, 1.2e-7 * np.abs(xo).max())
        e = float(np.abs(xc - xc.mean(0) - xo).max())
        assert e < tol, (r, e, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
_CHILD = r'''
import hashlib, sys
sys.path.insert(0, %r)
import numpy as np
from chromosome3d_amd import lib
from chromosome3d_amd.solver import Solver, default_model, make_stages
lib.check(lib.load().c3d_set_process_option(b"preload", float(sys.argv[1])))
s = Solver(0)
s.set_model(default_model())
s.set_schedule(make_stages([(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0)]))
s.set_if_matrix(np.load(sys.argv[2]))
s.init_replicas(3, 82364, 7)
s.embed(50)
x = s.coords()
assert np.isfinite(x).all()
print("HASH", hashlib.md5(np.ascontiguousarray(x).tobytes()).hexdigest(), int(s.stat("units_loaded")))
'''


def test_embedding_unit_loads_with_its_lds_allowance_in_both_modes(built, tmp_path):
    """2000 beads need 72 KB of dynamic LDS for k_dg_eig, allowed when the unit is loaded: in c3d_create's set (preload 1: the embedding
    is outside the default units and loads at c3d_embed_replicas) and at the first entry that needs it (preload 0).  Fresh processes in
    both modes embed and end in the same bits."""
    path = str(tmp_path / "if2000.npy")
    np.save(path, synthetic_if(2000, seed=2000)[0])
    out = []
    for flag in ("1", "0"):
        p = subprocess.run([sys.executable, "-c", _CHILD % ROOT, flag, path], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        out.append([l for l in p.stdout.splitlines() if l.startswith("HASH")][-1].split()[1])
    assert out[0] == out[1], out


# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_limit_is_4549_beads(ctx):
    """9 n + 16 floats of LDS: 4549 beads embed (test_trial_distances_and_eigen_stage_follow_the_oracle), 4550 are refused with
    C3D_ERR_INVALID and a message that names the limit, on the host, before any kernel runs; the smoothed bounds have no such limit.
    Without restraints U_ij = b0 |i - j|, summed in fp32 one hop at a time: measured largest error 0.88 A, 4.9e-5 of b0 (n - 1) (a
    sequential fp32 sum of 4549 b0 is off by 3.4e-5), allowed 1e-4 of each element."""
    from chromosome3d_amd import C3DError, default_model, make_stages
    n = 4550
    m = default_model()
    ctx.set_model(m)
    ctx.set_schedule(make_stages(FIRE10))
    IF = np.zeros((n, n))
    for k in range(1, 4):
        IF[np.arange(n - k), np.arange(k, n)] = IF[np.arange(k, n), np.arange(n - k)] = 1.0 / k
    np.fill_diagonal(IF, 10.0)
    ctx.set_if_matrix(IF)
    ctx.init_replicas(1, SEED, 0)
    with pytest.raises(C3DError, match=r"error -1: .*4549"):
        ctx.embed(50)
    assert ctx.num_restraints == 0               # |i - j| <= 3 < min_sep: the chain alone, U_ij = b0 |i - j|
    U, L = ctx.dg_bounds()
    sep = np.abs(np.arange(n)[:, None] - np.arange(n)[None])
    assert (np.abs(U - float(m.b0) * sep) <= 1e-4 * float(m.b0) * sep).all(), np.abs(U - float(m.b0) * sep).max()
    assert (L <= U).all()


def _write_banded(path, n, width=200):
    """a symmetric IF matrix that is zero for |i - j| > width (contact.tbl stays small)"""
    band = ["%.4g" % (1.0 / (1.0 + d)) for d in range(width + 1)]
    with open(path, "w") as f:
        for i in range(n):
            lo, hi = max(0, i - width), min(n, i + width + 1)
            f.write(" ".join(["0"] * lo + [band[abs(j - i)] for j in range(lo, hi)] + ["0"] * (n - hi)) + "\n")


def test_cli_embed_refuses_4550_beads(built, tmp_path):
    """c3d_solve --embed on a banded 4550-bead matrix exits non-zero and names the limit on stderr."""
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    mat = tmp_path / "banded_4550.txt"
    _write_banded(str(mat), 4550, width=8)
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, "-i", str(mat), "-o", str(out), "-m", "1", "--min-steps", "10", "--embed"], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode != 0
    assert "4549" in p.stderr, p.stderr[-2000:]
