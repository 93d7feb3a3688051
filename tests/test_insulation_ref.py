"""The restatement tests/insulation_ref.py held to scipy.signal (find_peaks, peak_prominences) and to planted chains whose domain
boundaries are known, on the CPU.  tests/test_gpu_insulation.py holds the device to the restatement."""
import numpy as np
import pytest

from tests import insulation_ref as R


def _valid_stretches(y):
    ok = ~np.isnan(y)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], ok.astype(np.int8), [0]))))
    return list(zip(edges[::2], edges[1::2]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("minima", [False, True])
def test_boundaries_and_strengths_are_scipys_peaks_and_prominences(seed, minima):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(seed)
    n = 300
    score = np.round(rng.normal(size=n).cumsum() * 0.3, 2)                       # rounded: ties and plateaus occur
    score[:7] = np.nan
    score[-5:] = np.nan
    if seed >= 2:
        score[120:123] = np.nan                                                 # two valid stretches: a walk stops at the gap
    mark, strength = R.boundaries(score, minima)
    y = -score if minima else score
    want_mark, want_strength = np.zeros(n, np.int32), np.zeros(n)
    for lo, hi in _valid_stretches(y):
        peaks, _ = signal.find_peaks(y[lo:hi])
        strict = np.array([p for p in peaks if y[lo + p] > y[lo + p - 1] and y[lo + p] > y[lo + p + 1]], dtype=np.intp)   # find_peaks also reports a plateau's middle
        prom = signal.peak_prominences(y[lo:hi], strict)[0]
        want_mark[lo + strict] = 1
        want_strength[lo + strict] = prom
    assert want_mark.sum() >= 10
    assert np.array_equal(mark, want_mark) and strength.tobytes() == want_strength.tobytes()
    assert (strength[mark == 0] == 0.0).all() and (strength[mark == 1] > 0.0).all()


@pytest.mark.parametrize("n,L,w", [(64, 8, 3), (455, 35, 16), (1025, 41, 16)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_planted_domains_are_found(n, L, w, seed):
    x = R.planted_domains(n, L, seed)
    D = R.block_distances
    got = R.insulation([("model", x)], n, [w])
    mark, strength = got["boundary"][0, 0], got["strength"][0, 0]
    strong = np.flatnonzero((mark == 1) & (strength >= 1.0))
    planted = [b for b in range(L, n, L) if w <= b <= n - 1 - w]
    assert planted
    for b in planted:
        assert any(abs(int(s) - b) <= 1 for s in strong), (b, strong)
    for s in strong:
        assert any(abs(int(s) - b) <= 1 for b in planted), (s, planted)
    # IF = 1 / d of the same model
    u = x[:, None, :] - x[None, :, :]
    d = np.sqrt((u * u).sum(axis=2))
    IF = 1.0 / np.where(d > 0, d, 1.0)
    np.fill_diagonal(IF, 0.0)
    both = R.insulation([("if", IF), ("model", x)], n, [w], None, 1.0, 1)
    r = both["fit_r"][0, 0]
    spurious = strength[(mark == 1) & (strength < 1.0)]
    print(f"n {n} L {L} w {w} seed {seed}: weakest planted {strength[strong].min():.2f}, strongest other {spurious.max() if len(spurious) else 0.0:.2f}, fit_r {r:.3f}, counts {both['fit_counts'][0, 0]}")
    assert r < -0.9
    assert D(x, w, w).shape == (w, w)


def test_edge_cases():
    # n = 2w + 1: one inside bead, no boundary possible
    w, n = 3, 7
    x = R.planted_domains(n, 3, 0)
    got = R.insulation([("model", x)], n, [w])
    assert np.isnan(got["mean"][0, 0, [0, 1, 2, 4, 5, 6]]).all() and got["mean"][0, 0, 3] > 0
    assert got["score"][0, 0, 3] == 0.0 and got["boundary"].sum() == 0 and (got["strength"] == 0).all()
    # a constant map: score 0 wherever the square fits, no boundaries
    n = 40
    got = R.insulation([("if", np.full((n, n), 2.5))], n, [1, 4])
    for k, w in enumerate((1, 4)):
        assert (got["score"][0, k, w:n - w] == 0.0).all() and np.isnan(got["score"][0, k, :w]).all() and np.isnan(got["score"][0, k, n - w:]).all()
    assert got["boundary"].sum() == 0
    # an all-zero IF square: the bead is not valid and its neighbours cannot be boundaries
    rng = np.random.default_rng(5)
    M = rng.uniform(1.0, 2.0, size=(n, n))
    M = M + M.T
    w, z = 2, 20
    M[z - w:z, z + 1:z + w + 1] = 0.0
    M[z + 1:z + w + 1, z - w:z] = 0.0
    got = R.insulation([("if", M)], n, [w])
    assert got["mean"][0, 0, z] == 0.0 and np.isnan(got["score"][0, 0, z])
    assert got["boundary"][0, 0, z - 1] == 0 and got["boundary"][0, 0, z] == 0 and got["boundary"][0, 0, z + 1] == 0
    assert got["boundary"][0, 0].sum() > 0
    # a plateau is no strict extremum
    score = np.array([np.nan, 0.0, 1.0, 1.0, 0.0, 2.0, 0.5, np.nan])
    mark, strength = R.boundaries(score, False)
    assert mark.tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and strength[5] == 1.5
    mark, _ = R.boundaries(score, True)
    assert mark.tolist() == [0, 0, 0, 0, 1, 0, 0, 0]


def test_contact_counts_and_the_fit_counts():
    n, L, w = 96, 12, 4
    models = [R.planted_domains(n, L, s) for s in range(3)]
    got = R.insulation([("model", models[0]), ("consensus", models)], n, [w], 12.0)
    i = 40
    d = [R.block_distances(x, i, w) for x in models]
    assert got["mean"][0, 0, i] == float((d[0] < 12.0).sum()) / 16.0
    assert got["mean"][1, 0, i] == float(sum((a < 12.0).sum() for a in d)) / 48.0
    b_if, s_if = np.array([0, 1, 0, 0, 0, 1, 0, 0, 1, 0]), np.array([0, 0.5, 0, 0, 0, 0.05, 0, 0, 0.3, 0])
    b_m, s_m = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0]), np.array([0, 0, 0.2, 0, 0, 0, 0.4, 0, 0, 0])
    assert R.match_counts(b_if, s_if, b_m, s_m, 0.1, 1).tolist() == [2, 2, 1, 1]
    assert R.match_counts(b_if, s_if, b_m, s_m, 0.1, 2).tolist() == [2, 2, 2, 2]
    assert R.match_counts(b_if, s_if, b_m, s_m, 0.0, 1).tolist() == [3, 2, 2, 2]
    assert R.match_counts(b_if, s_if, b_m, s_m, 0.1, 0).tolist() == [2, 2, 0, 0]
