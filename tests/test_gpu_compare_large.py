"""c3d_compare_replicas past one tile a chunk (csrc/c3d_score_compare.inc k_cmp_*; hook c3d_debug_distance_ranks).

k_cmp_table gives a workgroup a chunk of the m = n(n-1)/2 pairs and walks it in tiles of kCmpPairs = 64, restaging its LDS arrays behind the
loop's last barrier.  The chunk is compare_chunk_pairs(m, K) of csrc/c3d_internal.h, restated here as chunk_pairs():
    nb = ceil(K / 16),  want = max(2048 / nb^2, 64),  per = ceil(ceil(m / want) / 64) 64
In every case of tests/test_gpu_compare.py per is 64: one tile a chunk.  The cases here are the smallest at which each regime past that exists:

  case   beads x models       m        nb  per   tiles a chunk  chunks  last chunk      what it is the first of
  n513   513 x 3              131328   1   128   2              1026    128 = 64 + 64   2^18 key slots; two full tiles, no partial one
  n600   600 x 2 + 1 extra    179700   1   128   2              1404    116 = 64 + 52   the cnt < 64 tail is not the chunk's first tile
  k33    172 x 33             14706    3   128   2              115     114 = 64 + 50   a 3 x 3 grid of model blocks, the last of one model
  k81    120 x 81             7140     6   128   2              56      100 = 64 + 36   `want` on its floor of 64; grid 56 x 6 x 6
  n2049  2049 x 2 + 1 extra   2098176  1   1088  17             1929    512 = 8 x 64    2^22 slots; p beyond 2^21 in cmp_pair_of
  cube   130 x 3              8385     1   64    1              132     1               corners of a cube: the largest distance is a tie group
  point  130 x 3 + 1 extra    8385     1   64    1              132     1               a model whose beads all coincide, twice

The module asserts these figures at import from chunk_pairs(), and a test without a GPU compiles a host program that includes the header
and holds chunk_pairs() / table_chunks() to it: a change of the library's chunking fails here loudly.  The extra models are doubles that no
float holds.

Host side.  Ranks: tests/util.host_ranks (numpy average ranks of the host's distances).  Tables: pipeline.model_similarity
(c3d_model_similarity, fp64) of every ordered pair for n513, n600, k33, cube and point; for n2049 of every ordered pair a != b (the
diagonal is asserted to be exactly 1 and 0, which is what the host returns for a model and itself); for k81, whose 6561 host calls take
7 s, a numpy restatement that ranks each model once and forms both tables from the rank and distance arrays in the host's order of
operations (sequential sums by cumsum), itself held to the host function bit for bit on its first row and last column.

Bounds, from the arithmetic and never from the device's numbers.
  ranks  equal bit for bit.
  rho    n513, n600, k33, k81, cube, point: every centred rank is a multiple of 1/2, every product and partial sum a multiple of 1/4 below
         m^3 < 2^53 (the largest m^3 is 5.8e15, at n600), so the three sums of an entry are exact in any order
         (test_centred_rank_sums_are_exact_in_any_order checks that on the CPU); the device and the host then form sab / sqrt(saa sbb) by the
         same IEEE operations: rho == host bitwise, NaN where the host has NaN.
         n2049: the sums are no longer exact; |rho - host| <= 8 m 2^-53 = 1.9e-9 (two orders of m terms, the division, the square root).
  rmsd   |rmsd - host| <= 8 m 2^-53 x the largest pair distance of the two models, absolute in A: the error enters through
         scale = sums[b] / sums[a], two sums of m distances in different orders, times a distance.
One misplaced tie group moves rho by about 12 / m^3, far below any summation bound at n = 2049: hence the ranks through the hook.  A skipped
or doubled tile moves both tables by about 64 / m relative.

Largest gaps on an MI355X (printed by the tests); the ranks were the host's bit for bit in every case:
  case   rho bits equal  max |rho - host|  max |rmsd - host|  largest |rmsd - host| / bound
  n513   yes             0                 1.6e-13 A          1.1e-05
  n600   yes             0                 2.2e-13 A          9.3e-06
  k33    yes             0                 1.8e-13 A          2.0e-04
  k81    yes             0                 1.4e-13 A          2.9e-04
  n2049  no              1.4e-12           3.5e-12 A          3.6e-06          (rho bound 1.9e-9)
  cube   yes             0                 3.0e-13 A          8.0e-04          (the body diagonal ties 1043 of the 8385 pairs)
  point  yes             0                 7.8e-14 A          9.6e-05          (NaN in the 12 entries where the host has NaN)
With k_cmp_table's tile loop cut to its first iteration (a scratch build, not kept) the five table cases n513 .. n2049 fail, rho off in
the second digit, while every test of tests/test_gpu_compare.py still passes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.util import average_ranks, host_ranks, pair_distances, random_coil, restrained

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
TILE = 64                                                                       # kCmpPairs
MODEL_BLOCK = 16                                                                # kCmpModels


def chunk_pairs(m, K):
    """compare_chunk_pairs(m, K) of csrc/c3d_internal.h"""
    nb = (K + MODEL_BLOCK - 1) // MODEL_BLOCK
    want = max(2048 // (nb * nb), 64)
    return ((m + want - 1) // want + 63) // 64 * 64


def table_chunks(m, K):
    """compare_table_chunks(m, K) of csrc/c3d_internal.h"""
    per = chunk_pairs(m, K)
    return (m + per - 1) // per


# name: (beads, replicas, extra models, seed), then what the table above says of it: (m, model blocks, tiles a chunk, chunks, last chunk)
SHAPES = {"n513": (513, 3, 0, 5130), "n600": (600, 2, 1, 6000), "k33": (172, 33, 0, 1720), "k81": (120, 81, 0, 1200), "n2049": (2049, 2, 1, 20490),
          "cube": (130, 3, 0, 1301), "point": (130, 3, 1, 1302)}
FIGURES = {"n513": (131328, 1, 2, 1026, 128), "n600": (179700, 1, 2, 1404, 116), "k33": (14706, 3, 2, 115, 114), "k81": (7140, 6, 2, 56, 100),
           "n2049": (2098176, 1, 17, 1929, 512), "cube": (8385, 1, 1, 132, 1), "point": (8385, 1, 1, 132, 1)}
LARGE = ["n513", "n600", "k33", "k81", "n2049"]
EDGES = ["cube", "point"]
EXACT = ["n513", "n600", "k33", "k81", "cube", "point"]                         # m^3 < 2^53: rho bitwise


def figures(name):
    n, M, E, _ = SHAPES[name]
    m, K = n * (n - 1) // 2, M + E
    per, chunks = chunk_pairs(m, K), table_chunks(m, K)
    return m, (K + MODEL_BLOCK - 1) // MODEL_BLOCK, per // TILE, chunks, m - (chunks - 1) * per


for _name in SHAPES:
    assert figures(_name) == FIGURES[_name], (_name, figures(_name), FIGURES[_name])
    assert chunk_pairs(FIGURES[_name][0], SHAPES[_name][1] + SHAPES[_name][2]) % TILE == 0
assert all(FIGURES[c][2] >= 2 for c in LARGE)                                   # the point of the module: the tile loop runs twice at least
assert FIGURES["n600"][4] == 64 + 52 and FIGURES["k33"][4] == 64 + 50 and FIGURES["k81"][4] == 64 + 36       # a full tile, then a partial one
assert all((FIGURES[c][0] ** 3 < 2 ** 53) == (c in EXACT) for c in SHAPES)


def _models(name):
    """(replica coordinates [M, n, 3] float32, extra models [E, n, 3] float64 or None)"""
    n, M, E, seed = SHAPES[name]
    rng = np.random.default_rng(seed)
    if name == "cube":
        # corners of a cube of edge 7: distances 0, 7, 7 sqrt 2 and, for about an eighth of the pairs, the body diagonal 7 sqrt 3, the tie
        # group that ends at the last key; replica 1 an ordinary coil, replica 2 another draw of corners
        a, b = 7 * rng.integers(0, 2, size=(n, 3)), 7 * rng.integers(0, 2, size=(n, 3))
        assert len(np.unique(a, axis=0)) == 8 and len(np.unique(b, axis=0)) == 8
        return np.stack([a.astype(np.float32), random_coil(n, seed + 1), b.astype(np.float32)]), None
    if name == "point":
        # replica 1: every bead at one point; the extra model: every bead at another point, in doubles
        x = np.stack([random_coil(n, seed + 1), np.full((n, 3), 2.5, np.float32), random_coil(n, seed + 2)])
        return x, np.full((1, n, 3), -1.0 / 3.0)
    x = np.stack([random_coil(n, seed + r) for r in range(M)])
    if not E:
        return x, None
    extra = np.stack([random_coil(n, seed + M + e).astype(np.float64) * 2.5 + rng.normal(scale=1e-3, size=(n, 3)) for e in range(E)])
    assert not np.array_equal(extra, extra.astype(np.float32))
    return x, extra


_CACHE = {}


def _case(name):
    """(replicas float32, extras or None, all K models as doubles), built once"""
    if ("models", name) not in _CACHE:
        x, extra = _models(name)
        x.setflags(write=False)
        _CACHE["models", name] = (x, extra, [m.astype(np.float64) for m in x] + ([] if extra is None else list(extra)))
    return _CACHE["models", name]


def _ranks(name, k):
    """host ranks of model k of a case, computed once"""
    if ("ranks", name, k) not in _CACHE:
        r = host_ranks(_case(name)[2][k])
        r.setflags(write=False)
        _CACHE["ranks", name, k] = r
    return _CACHE["ranks", name, k]


def _numpy_tables(name):
    """both tables from one ranking and one distance array a model, in the host's order of operations: the rank sums are exact in any order
    (EXACT cases only), the distance sums are taken front to back as the host's loops take them (cumsum adds in sequence)"""
    assert name in EXACT
    models = _case(name)[2]
    K, m = len(models), FIGURES[name][0]
    C = np.stack([_ranks(name, k) for k in range(K)]) - 0.5 * (m + 1.0)
    D = np.stack([pair_distances(x) for x in models])
    S = C @ C.T
    saa = np.diag(S)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = S / np.sqrt(saa[:, None] * saa[None, :])
    sums = np.cumsum(D, axis=1)[:, -1]
    rmsd = np.empty((K, K))
    for a in range(K):
        scale = sums / sums[a] if sums[a] > 0 else np.ones(K)
        e = scale[:, None] * D[a][None, :] - D
        rmsd[a] = np.sqrt(np.cumsum(e * e, axis=1)[:, -1] / m)
    return rho, rmsd


def _host_tables(name):
    """the K x K tables of the host, computed once per case (the module docstring says by which means)"""
    if ("tables", name) not in _CACHE:
        from chromosome3d_amd import pipeline
        models = _case(name)[2]
        K = len(models)
        if name == "k81":
            rho, rmsd = _numpy_tables(name)
            for a, b in [(0, b) for b in range(K)] + [(a, K - 1) for a in range(K)]:
                h = pipeline.model_similarity(models[a], models[b])
                assert (rho[a, b], rmsd[a, b]) == h, (a, b, rho[a, b], rmsd[a, b], h)
        else:
            rho, rmsd = np.empty((K, K)), np.empty((K, K))
            for a in range(K):
                for b in range(K):
                    rho[a, b], rmsd[a, b] = (1.0, 0.0) if name == "n2049" and a == b else pipeline.model_similarity(models[a], models[b])
        rho.setflags(write=False)
        rmsd.setflags(write=False)
        _CACHE["tables", name] = (rho, rmsd)
    return _CACHE["tables", name]


def _largest(name):
    """the largest pair distance of every model of a case"""
    if ("largest", name) not in _CACHE:
        _CACHE["largest", name] = np.array([pair_distances(x).max() for x in _case(name)[2]])
    return _CACHE["largest", name]


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _load(ctx, name):
    x, extra, models = _case(name)
    restrained(ctx, x.shape[1], x.shape[0])
    ctx.set_coords(x)
    return x, extra, models


def _check_tables(name, rho, rmsd, degenerate=()):
    """rho and rmsd of the device against the host's, by the bounds of the module docstring; `degenerate` lists the models without extent"""
    hrho, hrmsd = _host_tables(name)
    m, K = FIGURES[name][0], len(hrho)
    assert rho.shape == rmsd.shape == (K, K)
    nan = np.zeros((K, K), bool)
    for k in degenerate:
        nan[k, :] = nan[:, k] = True
    assert np.array_equal(np.isnan(hrho), nan) and np.isfinite(hrmsd).all()     # what the host does with them
    assert np.array_equal(np.isnan(rho), nan), (name, np.argwhere(np.isnan(rho) != nan)[:5])
    assert np.isfinite(rmsd).all()
    big = _largest(name)
    bound = 8 * m * U * np.maximum(big[:, None], big[None, :])
    erho = np.abs(rho - hrho)[~nan].max()
    ermsd, worst = np.abs(rmsd - hrmsd).max(), (np.abs(rmsd - hrmsd) / np.where(bound > 0, bound, 1.0)).max()
    print(f"{name}: K {K}, m {m}, {FIGURES[name][2]} tiles a chunk, rho bits equal {np.array_equal(rho, hrho, equal_nan=True)}, "
          f"max |rho - host| {erho:.3e}, max |rmsd - host| {ermsd:.3e} A, largest |rmsd - host| / bound {worst:.3e}")
    if name in EXACT:
        bad = np.argwhere((rho != hrho) & ~nan)
        assert bad.size == 0, (name, len(bad), bad[:5], [(rho[a, b], hrho[a, b]) for a, b in bad[:5]])
    else:
        assert erho <= 8 * m * U, (name, erho, 8 * m * U)
    assert (np.abs(rmsd - hrmsd) <= bound).all(), (name, ermsd, worst)
    live = [k for k in range(K) if k not in degenerate]
    assert np.array_equal(np.diag(rho)[live], np.ones(len(live))) and np.array_equal(np.diag(rmsd), np.zeros(K))


def test_restated_chunking_is_the_headers(tmp_path):
    """A host program that includes csrc/c3d_internal.h prints compare_chunk_pairs and compare_table_chunks for every case here, for the
    cases of tests/test_gpu_compare.py and for the sizes at which the issue's regimes begin; chunk_pairs() and table_chunks() must agree."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    asked = sorted({(FIGURES[c][0], SHAPES[c][1] + SHAPES[c][2]) for c in SHAPES}
                   | {(2016, 3), (4186, 2), (32896, 7), (2016, 17), (8385, 4), (131072, 16), (131073, 16), (32768, 17), (32769, 17), (14528, 33),
                      (14529, 33), (4096, 81), (4097, 96), (4097, 256), (3, 1), (16384 * 16383 // 2, 256), (16384 * 16383 // 2, 1)})
    src = tmp_path / "chunks.cpp"
    src.write_text('#include <stdio.h>\n#include "c3d_internal.h"\nint main() {\n'
                   + "".join(f'    printf("%zu %d\\n", c3d::compare_chunk_pairs({m}ull, {K}), c3d::compare_table_chunks({m}ull, {K}));\n' for m, K in asked)
                   + "    return 0;\n}\n")
    exe = tmp_path / "chunks"
    build = subprocess.run([cxx, "-std=c++17", "-O0", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
                            "-I" + os.path.join(ROOT, "chromosome3d_amd", "csrc"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    got = [tuple(int(t) for t in line.split()) for line in out.stdout.splitlines()]
    assert got == [(chunk_pairs(m, K), table_chunks(m, K)) for m, K in asked]
    # the thresholds of the issue: the loop first runs twice just past these m
    assert [chunk_pairs(m, K) for m, K in ((131072, 16), (131073, 16), (32768, 17), (32769, 17), (14528, 33), (14529, 33), (4096, 81), (4097, 96))] \
        == [64, 128, 64, 128, 64, 128, 64, 128]


@pytest.mark.parametrize("name", EXACT)
def test_centred_rank_sums_are_exact_in_any_order(name):
    """The premise of the bitwise rho: sab, saa and sbb of two models' centred ranks, added front to back, back to front and pairwise (numpy's
    sum), agree exactly, and stay below 2^53 / 4."""
    m = FIGURES[name][0]
    K = len(_case(name)[2])
    for a, b in ((0, 1), (K - 1, 0)):
        ca, cb = _ranks(name, a) - 0.5 * (m + 1.0), _ranks(name, b) - 0.5 * (m + 1.0)
        assert np.array_equal(2 * ca, np.rint(2 * ca))
        for p in (ca * cb, ca * ca, cb * cb):
            assert np.array_equal(4 * p, np.rint(4 * p))
            front, back, pairwise = np.cumsum(p)[-1], np.cumsum(p[::-1])[-1], p.sum()
            assert front == back == pairwise, (name, a, b, front, back, pairwise)
            assert np.abs(np.cumsum(np.abs(p))[-1]) < 2.0 ** 51


@gpu
@pytest.mark.parametrize("name", LARGE + EDGES)
def test_distance_ranks_are_the_hosts_bit_for_bit(ctx, name):
    """The hook against numpy: every replica of n513, n600, n2049, cube and point, replica 0 of k33 and k81."""
    x, _, _ = _load(ctx, name)
    for r in range(1 if name in ("k33", "k81") else len(x)):
        dev, host = ctx.debug_distance_ranks(r), _ranks(name, r)
        assert dev.shape == host.shape == (FIGURES[name][0],)
        bad = np.flatnonzero(dev != host)
        assert bad.size == 0, (name, r, bad.size, bad[:5], dev[bad[:5]], host[bad[:5]])
    if name == "cube":
        top = _ranks(name, 0).max()
        group = int((_ranks(name, 0) == top).sum())
        print(f"cube: the body diagonal ties {group} of {FIGURES[name][0]} pairs, average rank {top}")
        assert group > 500 and top == FIGURES[name][0] - 0.5 * (group - 1)       # the group that ends at the last key
        assert len(np.unique(_ranks(name, 0))) == 4
    if name == "point":
        assert np.array_equal(_ranks(name, 1), np.full(FIGURES[name][0], 0.5 * (FIGURES[name][0] + 1.0)))   # one tie group: every pair


@gpu
@pytest.mark.parametrize("name", LARGE)
def test_tables_equal_the_host(ctx, name):
    """Both K x K tables, extras included, against the host (module docstring: which host side, which bounds); diagonals exactly 1 and 0."""
    _, extra, _ = _load(ctx, name)
    rho, rmsd = ctx.compare(extra)
    _check_tables(name, rho, rmsd)


@gpu
def test_a_tie_group_at_the_last_key(ctx):
    """cube: two models on the corners of a cube and a coil, every ordered pair against pipeline.model_similarity."""
    _, extra, _ = _load(ctx, "cube")
    rho, rmsd = ctx.compare(extra)
    _check_tables("cube", rho, rmsd)
    assert 0 < abs(rho[0, 2]) < 1 and rmsd[0, 2] > 0                            # two draws of corners are two models


@gpu
def test_models_without_extent_give_the_hosts_nan_pattern(ctx):
    """point: replica 1 and the extra model are single points: sums[a] = 0, scale 1 where they are a, 0 where they are b, rho 0 / 0.  NaN
    exactly where pipeline.model_similarity has NaN (their rows and columns, their diagonal entries included), every other entry by the bounds."""
    x, extra, models = _load(ctx, "point")
    rho, rmsd = ctx.compare(extra)
    _check_tables("point", rho, rmsd, degenerate=(1, 3))
    hrmsd = _host_tables("point")[1]
    assert rmsd[1, 3] == 0.0 and rmsd[3, 1] == 0.0 and hrmsd[1, 3] == 0.0
    assert rmsd[0, 1] == 0.0 and hrmsd[0, 1] == 0.0                             # scaled by 0 / sums[a] onto a point
    assert rmsd[1, 0] > 1.0                                                     # a point onto a coil: scale 1, the coil's rms distance


@gpu
def test_two_calls_return_the_same_bytes_with_and_without_the_extra(ctx):
    """n600: two calls return the same bytes, and the replicas' entries keep their bits when the extra model joins: the chunking does not
    depend on K below seventeen models, and no sum crosses models."""
    x, extra, _ = _load(ctx, "n600")
    M = len(x)
    first, second = ctx.compare(extra), ctx.compare(extra)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    alone = ctx.compare()
    assert alone[0].shape == (M, M)
    assert alone[0].tobytes() == first[0][:M, :M].tobytes() and alone[1].tobytes() == first[1][:M, :M].tobytes()
    assert ctx.debug_distance_ranks(1).tobytes() == ctx.debug_distance_ranks(1).tobytes()
