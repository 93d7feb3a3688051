"""The distance-geometry start beyond 4549 beads: the tiled eigen stage (k_dg_matvec / k_dg_orth, csrc/c3d_embed.hip), replica batches and
the options embed_max_beads / embed_form / embed_batch.

  1. the tiled form gives k_dg_eig's bits at every size both run           2. the same bits whatever the replica batch; replica keying
  3. 4550, 8192 and 16384 beads against the fp64 oracle from the device's own smoothed bounds
  4. the smoothing (kernels unchanged, never checked beyond 4550) at 8192 beads against scipy's shortest paths
  5. options and refusals                                                   6. from the embedded start to a model, library and c3d_solve

Helpers follow tests/test_gpu_embed.py (same seeds, same targets), without the n x n arrays that file builds for its own checks."""
import os
import subprocess
import time

import numpy as np
import pytest

from tests.util import random_coil, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 82364
FIRE10 = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0)]     # one FIRE stage: repel 0.5, so unrestrained pairs start at [0.5 r0_rep, inf)
U_RTOL, U_ATOL = 5e-7, 1e-6                      # tests/test_gpu_embed.py's: |U - Uo| <= U_RTOL Uo + U_ATOL
# Test 3's bound on |d_ij - do_ij| / max do_ij.  tests/test_gpu_embed.py allows 2e-6 up to 4549 beads (measured worst 2.2e-7 there).  Rule:
# 2e-6 stays if every value measured at the new sizes is at most a quarter of it (5e-7), else 4 x the measured worst rounded up to one
# digit.  Measured on MI355X, worst over the compared replicas: 3.65e-7 at 4550 beads, 2.70e-7 at 8192, 3.12e-7 at 16384: 2e-6 stays.
PAIR_TOL = 2e-6


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    s.set_option("max_beads", 16384)
    yield s
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _options(s, **kw):
    for k, v in kw.items():
        s.set_option(k, v)


def _k1(s, n):
    """K1 targets of synthetic_if(n) with beads n // 3 and n - 1 left without data where n >= 5 (tests/test_gpu_embed.py's _k1)"""
    from chromosome3d_amd import default_model, make_stages, pipeline
    IF = synthetic_if(n, seed=n)[0]
    if n >= 5:
        IF[[n // 3, n - 1], :] = 0.0
        IF[:, [n // 3, n - 1]] = 0.0
    m = default_model()
    s.set_model(m)
    s.set_schedule(make_stages(FIRE10))
    pipeline.IF2dist_new(s, IF)
    return m


def _sparse(s, n):
    """set_restraints: a band |i - j| = 5 .. 12 and about 2n long-range pairs, targets from a coil (>= 1 A) (tests/test_gpu_embed.py's
    _sparse); returns (model, ri, rj, target in Angstrom)"""
    from chromosome3d_amd import default_model, make_stages
    rng = np.random.default_rng(n)
    truth = random_coil(n, n).astype(np.float64) * 0.5
    ri = np.concatenate([np.arange(n - k) for k in range(5, 13) if k < n] + [np.zeros(0, int)])
    rj = np.concatenate([np.arange(k, n) for k in range(5, 13) if k < n] + [np.zeros(0, int)])
    li, lj = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    keep = np.abs(li - lj) > 12
    li, lj = np.minimum(li, lj)[keep][:2 * n], np.maximum(li, lj)[keep][:2 * n]
    key = np.unique(np.concatenate([ri * n + rj, li * n + lj]))
    ri, rj = key // n, key % n
    t10 = np.maximum(np.round(np.linalg.norm(truth[ri] - truth[rj], axis=1) * 10.0), 10).astype(np.int32)
    m = default_model()
    s.set_model(m)
    s.set_schedule(make_stages(FIRE10))
    s.set_restraints(n, (ri + 1).astype(np.int32), (rj + 1).astype(np.int32), t10)
    return m, ri, rj, t10 / 10.0


def _chain_only(s, n):
    """n beads with one restraint (1, 11): the cheapest context of that size"""
    from chromosome3d_amd import default_model, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(FIRE10))
    s.set_restraints(n, np.array([1], np.int32), np.array([11], np.int32), np.array([100], np.int32))


def _pair_error(x, xo, ch=512):
    """max |d_ij - do_ij| over all pairs and max do_ij, by row blocks (tests/test_gpu_embed.py's)"""
    x = x.astype(np.float64)
    worst, dmax = 0.0, 0.0
    for a in range(0, x.shape[0], ch):
        dg = np.linalg.norm(x[a:a + ch, None] - x[None], axis=-1)
        do = np.linalg.norm(xo[a:a + ch, None] - xo[None], axis=-1)
        worst, dmax = max(worst, float(np.abs(dg - do).max())), max(dmax, float(do.max()))
    return worst, dmax


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 33, 64, 65, 1025, 1819, 4549])
def test_tiled_form_gives_k_dg_eig_bits(ctx, n):
    """embed(50) and embed(1) of 20 replicas from first replica 7 with embed_form 0 (k_dg_eig) and 1 (k_dg_matvec + k_dg_orth) on the same
    context: the same coordinates bit for bit, and the stat embed_form says which form ran.  The sizes cover one lane of a row (2, 3),
    a partial row tile (33, 65), exactly four tiles (64), two elements per thread of the vector pass (1025) and five (4549)."""
    _k1(ctx, n)
    ctx.init_replicas(20, SEED, 7)
    try:
        for iters in (50, 1):
            _options(ctx, embed_form=0)
            ctx.embed(iters)
            assert ctx.stat("embed_form") == 0
            a = ctx.coords()
            _options(ctx, embed_form=1)
            ctx.embed(iters)
            assert ctx.stat("embed_form") == 1
            b = ctx.coords()
            assert np.isfinite(a).all()
            assert np.array_equal(a, b), (iters, np.argwhere(a != b)[:5], float(np.abs(a - b).max()))
    finally:
        _options(ctx, embed_form=0)


def test_batches_do_not_change_the_bits(ctx):
    """1025 beads x 5 replicas with embed_batch 0 (the budget: one batch), 1, 2 and 5, in both forms: equal bits, and embed_batches = 1, 5,
    3, 1.  On the tiled form, in batches of two: replica 2 of five from id 7 equals replica 0 of one from id 9."""
    _k1(ctx, 1025)
    try:
        ref = None
        for form in (0, 1):
            for batch, count in ((0, 1), (1, 5), (2, 3), (5, 1)):
                ctx.init_replicas(5, SEED, 7)
                _options(ctx, embed_form=form, embed_batch=batch)
                ctx.embed(50)
                assert ctx.stat("embed_batches") == count and ctx.stat("embed_form") == form
                x = ctx.coords()
                ref = x if ref is None else ref
                assert np.array_equal(ref, x), (form, batch)
        _options(ctx, embed_form=1, embed_batch=2)
        ctx.init_replicas(1, SEED, 9)
        ctx.embed(50)
        assert ctx.stat("embed_batches") == 1
        b = ctx.coords()
        assert np.array_equal(ref[2], b[0])
        assert not np.array_equal(ref[1], ref[2])
    finally:
        _options(ctx, embed_form=0, embed_batch=0)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrep,batch,compared", [(4550, 4, 0, (0, 3)), (8192, 4, 0, (0, 3)), (16384, 2, 1, (0,))])
def test_embedding_past_4549_beads_follows_the_oracle(ctx, O, n, nrep, batch, compared):
    """embed(50) from first replica 7 against c3o_dg_trial_d2 + c3o_dg_embed of replica 7 + r, both from the device's smoothed bounds in
    fp64 (tests/test_gpu_embed.py's method): embedded pair distances within PAIR_TOL of the largest, every replica centred to 2e-7 of its
    largest coordinate; the tiled form ran, in the expected number of batches.
    Measured on MI355X (worst pair-distance error over the compared replicas, of the largest distance; allowed 2e-6 by the rule at
    PAIR_TOL; centre; c3d_embed_replicas wall; the oracle's wall per call = trial distances + eigen stage on one host thread):
         4550 x 4   3.65e-7   centre 3.7e-9   embed 0.08 s   oracle  1.6 s
         8192 x 4   2.70e-7   centre 1.9e-9   embed 0.41 s   oracle  5.2 s
        16384 x 2   3.12e-7   centre 1.9e-9   embed 3.12 s   oracle 21.1 s      (profiles/r11_embed_large.md)
    Host memory at 16384 beads: about 10 GB (U and L in fp32 and fp64: 6 GB at the peak, the oracle's D2 in fp64: 2 GB, K1's IF matrix
    and tenths before that: 3 GB)."""
    _options(ctx, embed_max_beads=16384, embed_batch=batch)
    try:
        _k1(ctx, n)
        ctx.init_replicas(nrep, SEED, 7)
        t0 = time.perf_counter()
        ctx.embed(50)
        t_embed = time.perf_counter() - t0
        assert ctx.stat("embed_form") == 1
        assert ctx.stat("embed_batches") == (nrep if batch else 1)
        x = ctx.coords()
        assert np.isfinite(x).all()
        U32, L32 = ctx.dg_bounds()
        U, L = U32.astype(np.float64), L32.astype(np.float64)
        del U32, L32
        worst, t_oracle = 0.0, 0.0
        errs = []
        for r in compared:
            t0 = time.perf_counter()
            xo = O.dg_embed(O.dg_trial_d2(U, L, SEED, 7 + r), SEED, 7 + r, 50)
            t_oracle = max(t_oracle, time.perf_counter() - t0)
            e, dmax = _pair_error(x[r], xo)
            errs.append((r, e, dmax))
            worst = max(worst, e / dmax)
        c = np.abs(x.astype(np.float64).mean(1)).max(1) / np.abs(x).max((1, 2))
        print(f"n={n}: pair distances {worst:.2e} of the largest, centre {c.max():.2e} of max |x|, embed {t_embed:.2f} s, "
              f"oracle {t_oracle:.1f} s a call")
        for r, e, dmax in errs:
            assert e < PAIR_TOL * dmax, (r, e, dmax)
        assert (c < 2e-7).all(), c.max()
    finally:
        _options(ctx, embed_batch=0, embed_max_beads=4549)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_smoothing_at_8192_beads(ctx):
    """The blocked Floyd-Warshall kernels beyond the sizes tests/test_gpu_embed.py reaches (2100 against the oracle): sparse restraints at
    8192 beads, U against scipy.sparse.csgraph.shortest_path on the graph of chain bonds and restraints in fp64 within U_RTOL / U_ATOL;
    L <= U, zero diagonals, and L never below its starting bound (the restraint, b0 on the chain, repel x r0_rep elsewhere)."""
    n = 8192
    m, ri, rj, t = _sparse(ctx, n)
    U, L = ctx.dg_bounds()
    assert np.isfinite(U).all() and np.isfinite(L).all()
    assert (np.diag(U) == 0).all() and (np.diag(L) == 0).all()
    assert (L <= U).all()
    lower = np.float32(np.float32(FIRE10[-1][5]) * np.float32(m.r0_rep))
    L0 = np.full((n, n), lower, dtype=np.float32)
    np.fill_diagonal(L0, 0.0)
    L0[ri, rj] = L0[rj, ri] = t.astype(np.float32)
    i = np.arange(n - 1)
    L0[i, i + 1] = L0[i + 1, i] = np.float32(m.b0)
    L0 = np.minimum(L0, U)                       # (a restraint longer than a path through others: the clamp L <= U wins)
    assert (L >= L0).all(), np.argwhere(L < L0)[:5]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import shortest_path
    except ImportError:
        return
    w = np.concatenate([np.full(n - 1, float(np.float32(m.b0))), t.astype(np.float32).astype(np.float64)])
    g = coo_matrix((w, (np.concatenate([i, ri]), np.concatenate([i + 1, rj]))), shape=(n, n)).tocsr()
    Uo = shortest_path(g, method="D", directed=False)
    eu = np.abs(U.astype(np.float64) - Uo)
    assert (eu <= U_RTOL * Uo + U_ATOL).all(), (np.argwhere(eu > U_RTOL * Uo + U_ATOL)[:5], eu.max())
    off = ~np.eye(n, dtype=bool)
    print(f"n={n} sparse: U rel {(eu[off] / Uo[off]).max():.2e} against scipy, {len(ri)} restraints")


# ---------------------------------------------------------------------------------------------------------------------------------
def test_options_and_refusals():
    """Defaults untouched: 4550 beads are refused naming 4549 and the option; embed_max_beads takes integers 4549 .. 16384 only; beyond
    embed_max_beads the refusal comes on the host before any launch (the stats of the last embed stay); max_beads is still what
    admits a matrix beyond 5120 beads."""
    from chromosome3d_amd import C3DError, Solver
    s = Solver(0)
    try:
        for bad in (4548, 16385, 5000.5):
            with pytest.raises(C3DError, match="error -1: .*embed_max_beads"):
                s.set_option("embed_max_beads", bad)
        for key, bad in (("embed_form", 2), ("embed_form", 0.5), ("embed_batch", -1), ("embed_batch", 1.5)):
            with pytest.raises(C3DError, match="error -1: .*" + key):
                s.set_option(key, bad)
        _chain_only(s, 4550)
        s.init_replicas(1, SEED, 0)
        with pytest.raises(C3DError, match=r"error -1: .*4549.*embed_max_beads"):
            s.embed(50)
        s.set_option("embed_max_beads", 4550)
        s.embed(50)
        assert s.stat("embed_form") == 1 and s.stat("embed_batches") == 1 and np.isfinite(s.coords()).all()
        with pytest.raises(C3DError, match="error -1: .*max_beads"):
            _chain_only(s, 5121)                 # embed_max_beads does not admit the matrix
        s.set_option("embed_max_beads", 16384)
        with pytest.raises(C3DError, match="error -1: .*max_beads"):
            _chain_only(s, 5121)
        s.set_option("max_beads", 6001)
        s.set_option("embed_max_beads", 6000)
        s.set_option("embed_batch", 1)
        _chain_only(s, 6001)
        s.init_replicas(3, SEED, 0)
        x0 = s.coords()
        with pytest.raises(C3DError, match=r"error -1: .*6001 beads.*embed_max_beads = 6000"):
            s.embed(50)
        assert s.stat("embed_batches") == 1      # still the 4550-bead embed's: nothing ran (three batches would have)
        assert np.array_equal(x0, s.coords())
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
def _banded_if(n, width=200):
    IF = np.zeros((n, n))
    for d in range(1, width + 1):
        IF[np.arange(n - d), np.arange(d, n)] = IF[np.arange(d, n), np.arange(n - d)] = 1.0 / (1.0 + d)
    np.fill_diagonal(IF, 1.0)
    return IF


def test_embedded_start_of_6000_beads_anneals(ctx):
    """6000 beads x 2 from a banded matrix: with embed_max_beads 6000 the embedded start is finite, and 60 FIRE steps from it end in finite
    energies below the start's (E_noe + E_bond + E_repel at the stage's weights, per replica)."""
    from chromosome3d_amd import default_model, make_stages
    n = 6000
    stage = (2, 60, 0.0, 1.0, 20.0, 0.5, 0.0)
    _options(ctx, embed_max_beads=6000)
    try:
        ctx.set_model(default_model())
        ctx.set_schedule(make_stages([stage]))
        ctx.set_if_matrix(_banded_if(n))
        ctx.init_replicas(2, SEED, 0)
        ctx.embed(50)
        assert ctx.stat("embed_form") == 1
        assert np.isfinite(ctx.coords()).all()
        e0 = ctx.eval(stage[3], stage[4], stage[5], forces=False)[1].sum(1)
        assert ctx.run_steps(60) == 60
        e1 = ctx.eval(stage[3], stage[4], stage[5], forces=False)[1].sum(1)
        print(f"n={n}: energy {e0} -> {e1}")
        assert np.isfinite(e0).all() and np.isfinite(e1).all() and np.isfinite(ctx.coords()).all()
        assert (e1 < e0).all(), (e0, e1)
    finally:
        _options(ctx, embed_max_beads=4549)


def _write_banded(path, n, width=200):
    """a symmetric IF matrix that is zero for |i - j| > width (contact.tbl stays small) (tests/test_gpu_embed.py's)"""
    band = ["%.4g" % (1.0 / (1.0 + d)) for d in range(width + 1)]
    with open(path, "w") as f:
        for i in range(n):
            lo, hi = max(0, i - width), min(n, i + width + 1)
            f.write(" ".join(["0"] * lo + [band[abs(j - i)] for j in range(lo, hi)] + ["0"] * (n - hi)) + "\n")


def test_cli_embeds_6000_beads_with_the_flag_only(built, tmp_path):
    """c3d_solve --embed --embed-max-beads 6000 on a banded 6000-bead matrix writes its models; without the flag it exits non-zero and
    names the 4549-bead limit."""
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    mat = tmp_path / "banded_6000.txt"
    _write_banded(str(mat), 6000)                # width 200: targets up to 1.4 A (width 8 rounds to no restraint at all)
    out = tmp_path / "out"
    out.mkdir()
    cmd = [exe, "-i", str(mat), "-o", str(out), "-m", "2", "--min-steps", "10", "--embed"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode != 0
    assert "4549" in p.stderr and "embed_max_beads" in p.stderr, p.stderr[-2000:]
    assert not list(out.glob("banded_6000_*.pdb"))
    p = subprocess.run(cmd + ["--embed-max-beads", "6000"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    models = sorted(f.name for f in out.glob("banded_6000_*.pdb"))
    assert models == ["banded_6000_1.pdb", "banded_6000_2.pdb"], (models, p.stdout[-2000:])
