"""Device scoring of large maps (csrc/c3d_score.hip, shared helpers in c3d_score_core.h): the IF ranks on the GPU (k_rank_*, option device_ranks, stat device_rank_runs, hook
c3d_debug_if_ranks) and models of any extent (the sized-histogram re-run, stat score_wide_runs).

  1. the device's ranks are the average ranks, bit for bit          2. the same scores from either rank source
  3. models wider than the fixed 262 A histogram                    4. beyond 5120 beads the device ranks at the default
  5. the ceiling, 16384 beads, once

Tolerances: satisfied is equal; sum_dev within 1e-10 relative of the host's (as tests/test_gpu_step_kernels.py has it) and bit-identical
where only the rank source differs (the distance side is the same launches); rho within RHO_TOL = 1e-9 of c3d_spearman_if_dist_batch.
RHO_TOL is derived, not measured: both sides add m <= 2.7e8 fp64 terms in different orders, worst case about m 2^-53 = 3e-8, expected
about sqrt(m) 2^-53 = 2e-12 (the existing scoring test measured 1.9e-12 at 2500 beads); measured by this file on MI355X, largest
|rho - host function|: 0 at 455 beads, 1.9e-12 at 2048 (wide), 1.8e-12 at 2500, 5.2e-13 at 6000, 7.8e-13 at 8192, |rho + 1| = 0 at 16384;
tools/score_large.py writes the difference at 6000, 8192 and 16384 beads next to its wall times (profiles/r12_score_large.md)."""
import numpy as np
import pytest

from tests.util import load_if, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

RHO_TOL = 1e-9
SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    s.set_option("max_beads", 16384)
    yield s
    s.set_option("device_ranks", 0)
    s.close()


def _chain_only(s, n):
    """n beads with one restraint (1, 11): the cheapest context of that size"""
    from chromosome3d_amd import default_model, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, np.array([1], np.int32), np.array([11], np.int32), np.array([100], np.int32))


def _k1(s, IF):
    """K1 targets of IF; returns the restraint rows pipeline.assess reads"""
    from chromosome3d_amd import default_model, make_stages, pipeline
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    return pipeline.restraints_from_dist10(pipeline.IF2dist_new(s, IF))


def _average_ranks(IF, rng):
    """(rank matrix, saa, m) of the ordered pairs |i-j| >= rng of a symmetric matrix: every upper-triangle value counted twice, a tie group
    of c values with b values below it has rank 2b + c + 0.5 (positions 2b .. 2b + 2c - 1 of the doubled list, averaged, 1-based)"""
    n = len(IF)
    i, j = np.triu_indices(n, rng)
    u, inv, cnt = np.unique(IF[i, j], return_inverse=True, return_counts=True)      # -0.0 and 0.0 are one value here, as on the host
    below = np.cumsum(cnt) - cnt
    r = 2.0 * below + cnt + 0.5
    R = np.zeros((n, n))
    R[i, j] = r[inv]
    R[j, i] = r[inv]
    m = 2 * len(i)
    saa = float(np.sum(2.0 * cnt * (r - 0.5 * (m + 1.0)) ** 2))
    return R, saa, m


def _quantised(n, seed):
    """a symmetric matrix of small integers: most values tie, a third are zero, one upper-triangle zero is -0.0"""
    rng = np.random.default_rng(seed)
    IF = np.triu(np.floor(rng.gamma(0.7, 4.0, size=(n, n))), 1)
    IF[rng.random((n, n)) < 0.3] = 0.0
    IF = np.triu(IF, 1)
    IF = IF + IF.T
    IF[10, 500] = -0.0
    IF[500, 10] = 0.0
    assert np.signbit(IF[10, 500]) and (IF == 0).mean() > 0.3 and len(np.unique(IF)) < 200
    return IF


def _rank_case(name):
    if name == "chr1_500kb":
        return load_if("chr1_500kb")
    if name == "chr21_1mb":
        IF = load_if("chr21_1mb")
        assert len(IF) == 37
        return IF
    if name == "syn2500":
        return synthetic_if(2500, seed=2500)[0]
    return _quantised(6000, 6000)


# ---------------------------------------------------------------------------------------------
# 1. the ranks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chr1_500kb", "chr21_1mb", "syn2500", "quantised6000"])
def test_device_ranks_are_the_average_ranks_bit_for_bit(ctx, name):
    """c3d_debug_if_ranks — what the device computes for c3d_score_replicas — against a numpy restatement of the average ranks over the
    doubled upper triangle: the rank matrix bit for bit (half-integers, exact in fp64), m equal, saa within 1e-12 relative; ranges 1 and 3;
    real data with many ties, a 37-bead matrix (fewer keys than one sort tile), a continuous 2500-bead matrix and a 6000-bead matrix of
    small integers with zeros and a -0.0."""
    IF = _rank_case(name)
    assert np.array_equal(IF, IF.T)
    _chain_only(ctx, len(IF))
    ctx.set_option("device_ranks", 1)
    try:
        for rng in (1, 3):
            R, saa, m = ctx.debug_if_ranks(IF, rng)
            Rn, saan, mn = _average_ranks(IF, rng)
            assert m == mn, (name, rng, m, mn)
            print(f"{name} range {rng}: m {m}, distinct ranks {len(np.unique(Rn))}, saa {saa!r} numpy {saan!r}")
            assert np.array_equal(R, Rn), (name, rng, int((R != Rn).sum()), float(np.abs(R - Rn).max()))
            assert abs(saa - saan) <= 1e-12 * saan, (name, rng, saa, saan)
    finally:
        ctx.set_option("device_ranks", 0)


def test_an_asymmetric_matrix_is_ranked_on_the_host(ctx):
    """device_ranks 1 and a matrix with IF(i,j) != IF(j,i) for one ranked pair: the call does not count as a device run and returns what
    the host path (device_ranks -1) returns, bit for bit; the hook refuses the matrix."""
    from chromosome3d_amd import C3DError
    n = 600
    IF = synthetic_if(n, seed=n)[0]
    _k1(ctx, IF)
    IF = IF.copy()
    IF[400, 17] *= 1.5
    ctx.init_replicas(2, 82364, 0)
    ctx.set_coords(random_coil(n, 5)[None].repeat(2, 0) * np.float32([[[0.25]], [[0.35]]]))
    try:
        ctx.set_option("device_ranks", 1)
        d0, h0 = ctx.stat("device_rank_runs"), ctx.stat("rank_prefetch_hits")
        dev = ctx.score(IF, 3)
        assert ctx.stat("device_rank_runs") == d0 and ctx.stat("rank_prefetch_hits") == h0
        with pytest.raises(C3DError, match="not symmetric"):
            ctx.debug_if_ranks(IF, 3)
        ctx.set_option("device_ranks", -1)
        host = ctx.score(IF, 3)
        assert ctx.stat("device_rank_runs") == d0
        for a, b in zip(dev, host):
            assert np.array_equal(a, b)
    finally:
        ctx.set_option("device_ranks", 0)


# ---------------------------------------------------------------------------------------------
# 2. either rank source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,nrep", [("chr1_500kb", 20), ("syn2500", 2)])
def test_same_scores_from_either_rank_source(ctx, name, nrep):
    """After a short anneal, device_ranks 1 against -1: satisfied and sum_dev bit-identical (the distance side is untouched), rho of both
    within RHO_TOL of the host function; at 1 the prefetched ranks are neither used nor counted and device_rank_runs rises by one per call."""
    from chromosome3d_amd import pipeline
    IF = _rank_case(name)
    rows = _k1(ctx, IF)
    ctx.init_replicas(nrep, 82364, 0)
    assert ctx.run_steps(10 ** 6) == 45
    x = ctx.coords()
    host_rho = pipeline.spearman_IF_models(IF, x)
    try:
        ctx.set_option("device_ranks", -1)
        d0 = ctx.stat("device_rank_runs")
        sat_h, dev_h, rho_h = ctx.score(IF, 3)
        assert ctx.stat("device_rank_runs") == d0
        ctx.set_option("device_ranks", 1)
        h0 = ctx.stat("rank_prefetch_hits")
        for call in (1, 2):
            sat_d, dev_d, rho_d = ctx.score(IF, 3)
            assert ctx.stat("device_rank_runs") == d0 + call and ctx.stat("rank_prefetch_hits") == h0
            assert np.array_equal(sat_d, sat_h) and np.array_equal(dev_d, dev_h)
            print(f"{name}: max |rho device ranks - host function| {np.abs(rho_d - host_rho).max():.3g}, "
                  f"|rho host ranks - host function| {np.abs(rho_h - host_rho).max():.3g}")
            assert np.abs(rho_d - host_rho).max() <= RHO_TOL and np.abs(rho_h - host_rho).max() <= RHO_TOL
    finally:
        ctx.set_option("device_ranks", 0)
    for r in range(min(nrep, 3)):
        hs, hd = pipeline.assess(x[r], rows)
        assert sat_d[r] == hs and abs(dev_d[r] - hd) <= 1e-10 * max(1.0, abs(hd)), (r, sat_d[r], hs, dev_d[r], hd)


# ---------------------------------------------------------------------------------------------
# 3. wide models
# ---------------------------------------------------------------------------------------------
def _largest_distance(x, ch=256):
    x = x.astype(np.float64)
    return max(float(np.linalg.norm(x[a:a + ch, None, :] - x[None, :, :], axis=-1).max()) for a in range(0, len(x), ch))


def test_models_wider_than_the_fixed_histogram(ctx):
    """2048 beads, a full-size random coil (wider than 262.144 A) beside a compact one: the call succeeds through the sized-histogram
    re-run (score_wide_runs + 1), both replicas equal the host (spearman_IF_models, pipeline.assess), and the compact replica's three
    numbers are, bit for bit, those of a call that scores it alone on the normal path.  A model beyond 50 000 A is refused."""
    from chromosome3d_amd import C3DError, pipeline
    n = 2048
    IF = synthetic_if(n, seed=n)[0]
    rows = _k1(ctx, IF)
    coil = random_coil(n, 5)
    x = np.stack([coil, coil * np.float32(0.25)])
    assert _largest_distance(x[0]) > 262.144 and _largest_distance(x[1]) < 262.144
    ctx.init_replicas(2, 82364, 0)
    ctx.set_coords(x)
    x = ctx.coords()
    w0 = ctx.stat("score_wide_runs")
    sat, dev, rho = ctx.score(IF, 3)
    assert ctx.stat("score_wide_runs") == w0 + 1
    host_rho = pipeline.spearman_IF_models(IF, x)
    for r in range(2):
        hs, hd = pipeline.assess(x[r], rows)
        print(f"wide replica {r}: rho {rho[r]!r} host {host_rho[r]!r} diff {rho[r] - host_rho[r]:.3g}; satisfied {sat[r]} host {hs}; sum_dev {dev[r]!r} host {hd!r}")
        assert abs(rho[r] - host_rho[r]) <= RHO_TOL, (r, rho[r] - host_rho[r])
        assert sat[r] == hs and abs(dev[r] - hd) <= 1e-10 * max(1.0, abs(hd)), (r, sat[r], hs, dev[r], hd)
    ctx.init_replicas(1, 82364, 0)
    ctx.set_coords(x[1:2])
    sat1, dev1, rho1 = ctx.score(IF, 3)
    assert ctx.stat("score_wide_runs") == w0 + 1
    assert sat1[0] == sat[1] and dev1[0] == dev[1] and rho1[0] == rho[1], (sat1, sat[1], dev1, dev[1], rho1, rho[1])
    far = coil * np.float32(60000.0 / _largest_distance(coil))
    assert _largest_distance(far) > 50000.0
    ctx.set_coords(far[None])
    with pytest.raises(C3DError, match="50000 A"):
        ctx.score(IF, 3)
    ctx.set_coords((far * np.float32(2.0))[None])      # 120 000 A: wider than the limit along one axis, refused from the bounding box alone
    with pytest.raises(C3DError, match="50000 A"):
        ctx.score(IF, 3)
    assert ctx.stat("score_wide_runs") == w0 + 1


# ---------------------------------------------------------------------------------------------
# 4. beyond 5120 beads at the default
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6000, 8192])
def test_beyond_5120_beads_the_device_ranks_by_default(ctx, n):
    """max_beads raised, device_ranks left at 0: the call ranks on the device (device_rank_runs rises), rho is within RHO_TOL of the host
    function, satisfied and sum_dev equal pipeline.assess."""
    from chromosome3d_amd import pipeline
    IF = synthetic_if(n, seed=n)[0]
    rows = _k1(ctx, IF)
    ctx.init_replicas(2, 82364, 0)
    ctx.set_coords(random_coil(n, 5)[None].repeat(2, 0) * np.float32([[[0.15]], [[0.2]]]))
    x = ctx.coords()
    d0, w0 = ctx.stat("device_rank_runs"), ctx.stat("score_wide_runs")
    sat, dev, rho = ctx.score(IF, 3)
    assert ctx.stat("device_rank_runs") == d0 + 1 and ctx.stat("score_wide_runs") == w0
    host_rho = pipeline.spearman_IF_models(IF, x)
    for r in range(2):
        hs, hd = pipeline.assess(x[r], rows)
        print(f"n {n} replica {r}: rho {rho[r]!r} host {host_rho[r]!r} diff {rho[r] - host_rho[r]:.3g}; satisfied {sat[r]} host {hs}; sum_dev {dev[r]!r} host {hd!r}")
        assert abs(rho[r] - host_rho[r]) <= RHO_TOL, (r, rho[r] - host_rho[r])
        assert sat[r] == hs and abs(dev[r] - hd) <= 1e-10 * max(1.0, abs(hd)), (r, sat[r], hs, dev[r], hd)


# ---------------------------------------------------------------------------------------------
# 5. the ceiling
# ---------------------------------------------------------------------------------------------
def test_the_ceiling_once(ctx):
    """16384 beads on a line at 0.5 A spacing, IF = 1 / |i-j|: both rank sides have the same tie structure in opposite order, so rho = -1
    within RHO_TOL; the extent is 8192 A, so the device sort (2^27 key slots) and the sized histogram (8.2 M bins) both run at full size."""
    n = 16384
    _chain_only(ctx, n)
    sep = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64)
    np.fill_diagonal(sep, 1.0)
    IF = 1.0 / sep
    del sep
    np.fill_diagonal(IF, 0.0)
    x = np.zeros((1, n, 3), np.float32)
    x[0, :, 0] = 0.5 * np.arange(n)
    ctx.init_replicas(1, 82364, 0)
    ctx.set_coords(x)
    d0, w0 = ctx.stat("device_rank_runs"), ctx.stat("score_wide_runs")
    sat, dev, rho = ctx.score(IF, 3)
    print(f"ceiling: rho + 1 = {rho[0] + 1.0:.3g}")
    assert ctx.stat("device_rank_runs") == d0 + 1 and ctx.stat("score_wide_runs") == w0 + 1
    assert abs(rho[0] + 1.0) <= RHO_TOL, rho[0] + 1.0
