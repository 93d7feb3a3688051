"""tests/loop_ref.py, the numpy restatement of c3d_loops, held to a direct loop over cells and to planted inputs: the planted loops of a
contact map are exactly its peaks, the bases of a rosette are closed, the mask removes a bin from every sum, and on the planted inputs
of tests/test_gpu_loops.py at most 1 % of the pixels have a ratio within 2 S of a threshold — the cap that test relies on."""
import numpy as np
import pytest

from tests import loop_ref as R

U = 2.0 ** -53
THR = (1.75, 1.75, 1.5, 1.5)


def _direct(M, E, n, masked, p, w, s_lo, i, j, dead=()):
    """the four ratios of pixel (i, j) by a plain double loop; `dead`: bins whose cells are left out by hand"""
    if i < w or j + w > n - 1 or masked[i] or masked[j] or i in dead or j in dead or E[j - i - s_lo] == 0.0:
        return [R.NAN] * 4
    sm, se = [0.0] * 4, [0.0] * 4
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            ca, cb = i + a, j + b
            if masked[ca] or masked[cb] or ca in dead or cb in dead:
                continue
            P = abs(a) <= p and abs(b) <= p
            member = (not P and a != 0 and b != 0, not P and a >= 1 and b <= -1, abs(a) <= 1 and abs(b) > p, abs(b) <= 1 and abs(a) > p)
            for x in range(4):
                if member[x]:
                    sm[x] += M[ca, cb]
                    se[x] += E[cb - ca - s_lo]
    return [M[i, j] / ((sm[x] / se[x]) * E[j - i - s_lo]) if sm[x] != 0.0 and se[x] != 0.0 else R.NAN for x in range(4)]


@pytest.mark.parametrize("n,w,p,lo,hi,planted,cands", [(120, 5, 2, 11, 50, [(30, 60), (50, 95), (70, 90)], 27), (80, 3, 1, 7, 30, [(20, 40), (35, 60)], 16)])
def test_the_planted_loops_are_exactly_the_peaks(n, w, p, lo, hi, planted, cands):
    M = R.planted_map(n, planted)
    out = R.loops([("if", M)], n, None, p, w, lo, hi, THR, 0.0, 2, min(3, w))
    assert out["peaks"].tolist() == [list(q) for q in planted]
    assert out["report"].tolist() == [cands, len(planted), len(planted), 0]
    assert out["closed"].tolist() == [[len(planted), len(planted)]] and out["p2ll"][0] > 2.0
    assert out["margin"].min() > 1e-9                                           # no pixel sits on a threshold
    s_lo = lo - 2 * w
    masked = np.zeros(n, dtype=bool)
    for s in (lo, (lo + hi) // 2, hi):                                          # the vectorised walk against the plain loop, bit for bit
        for i in range(0, n - s, 7):
            want = _direct(M, out["expected"][0], n, masked, p, w, s_lo, i, i + s)
            assert np.array(want).tobytes() == out["ratio"][:, s - lo, i].tobytes(), (s, i)
    assert np.isnan(out["ratio"][:, hi - lo, n - hi:]).all()                    # beyond the matrix
    assert (out["at"][0, :, 2:].T.tobytes() == np.stack([out["ratio"][:, b - a - lo, a] for a, b in planted], axis=1).tobytes())


def test_the_rosettes_bases_are_closed():
    n, petal = 96, 12
    xs = [R.planted_rosette(n, petal, 1 + r) for r in range(2)]
    bases = [(petal * m, petal * (m + 1)) for m in range(1, n // petal - 1)]
    out = R.loops([("model", xs[0]), ("model", xs[1]), ("consensus", xs)], n, None, 1, 3, 7, 30, listed=bases)
    assert (out["closed"] == len(bases)).all()                                  # every base pixel scored, every one on the loop side
    assert (out["at"][:, :, 2:4] < 0.5).all() and (out["at"][:, :, 0] < 4.0).all()
    assert (out["p2ll"] < 1.0).all() and (out["apa"][:, 3, 3] < 0.5).all()
    assert np.allclose(out["at"][2, :, 0], (out["at"][0, :, 0] + out["at"][1, :, 0]) / 2.0, rtol=4 * U)


def test_the_mask_removes_a_bin_from_every_sum():
    n, w, p, lo, hi = 80, 3, 1, 7, 30
    M = R.planted_map(n, [(20, 40), (35, 60)])
    mask = np.zeros(n, np.int32)
    mask[[22, 41]] = (1, 3)                                                      # any non-zero value
    masked = mask != 0
    s_lo, s_hi = R.band_range(n, w, lo, hi)
    E = R.expected("if", M, n, masked, s_lo, s_hi)
    for s in range(s_lo, s_hi + 1):                                             # E without the bins' cells, by hand
        v = [M[i, i + s] for i in range(n - s) if i not in (22, 41) and i + s not in (22, 41)]
        assert abs(E[s - s_lo] - sum(v) / len(v)) <= (len(v) + 2) * U * E[s - s_lo]
    out = R.loops([("if", M)], n, mask, p, w, lo, hi)
    nobody = np.zeros(n, dtype=bool)
    for i, j in [(20, 40), (19, 40), (22, 40), (20, 41), (25, 44), (35, 60), (38, 45), (3, 20), (2, 20), (50, 79 - w), (50, 80 - w)]:
        want = _direct(M, out["expected"][0], n, nobody, p, w, s_lo, i, j, dead=(22, 41))
        assert np.array(want).tobytes() == out["ratio"][:, j - i - lo, i].tobytes(), (i, j)
    assert out["report"][3] == sum(1 for s in range(lo, hi + 1) for i in range(w, n - s - w) if i in (22, 41) or i + s in (22, 41))
    whole = np.zeros(n, np.int32)
    whole[30:30 + 2 * w + 1] = 1                                                 # a run of 2w + 1 bins empties whole neighbourhoods: SE = 0, NaN
    gone = R.loops([("if", M)], n, whole, p, w, lo, hi)
    assert np.isnan(gone["ratio"][:, 33 - 10 - lo, 10]).all()                    # pixel (10, 33): j is masked
    r = gone["ratio"][:, 40 - 20 - lo, 20]                                       # pixel (20, 40): its columns 37..43 are live, 30..36 are not
    assert not np.isnan(r).any()
    r = gone["ratio"][:, 26 - 10 - lo, 10]                                       # pixel (10, 26): the columns right of it, 30..36, are all gone
    want = _direct(M, gone["expected"][0], n, whole != 0, p, w, s_lo, 10, 26)
    assert np.array(want).tobytes() == r.tobytes() and not np.isnan(r).any()
    every = np.ones(n, np.int32)
    every[[10, 26]] = 0                                                          # nothing live around the pixel: SM = SE = 0 in every neighbourhood
    none = R.loops([("if", M)], n, every, p, w, lo, hi, dense=False, listed=[(10, 26)])
    assert np.isnan(none["at"][0, 0, 2:]).all() and none["at"][0, 0, 0] == M[10, 26] and none["closed"].tolist() == [[0, 0]]


def test_few_pixels_sit_near_a_threshold_on_the_inputs_of_the_gpu_tests():
    """S = (2c + 2(n + Kp + 2) + 4) u; the share of pixels whose ratio lies within 2 S (relative) of a threshold is at most 1 %"""
    for name, (n, planted, w, p, lo, hi, seps, step) in R.PLANTED_CASES.items():
        M = R.planted_map(n, planted)
        masked = np.zeros(n, dtype=bool)
        s_lo, s_hi = R.band_range(n, w, lo, hi)
        E = R.expected("if", M, n, masked, s_lo, s_hi)
        ratio = R.scan(M, E, n, masked, p, w, lo, hi, seps, step)
        S = (2 * (2 * w + 1) ** 2 + 2 * (n + 2) + 4) * U
        m = R.margins(ratio, None, THR, 0.0)
        scored = np.isfinite(m)
        share = float((m[scored] <= 2 * S).sum()) / max(1, int(scored.sum()))
        print(f"{name}: {int(scored.sum())} pixels, least margin {m.min():.3g}, share within 2 S {share:.3g}")
        assert scored.sum() > 0 and share <= 0.01
