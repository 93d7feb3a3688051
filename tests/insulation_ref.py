"""The numpy restatement of c3d_insulation (definitions 1-5 above its prototype in include/c3d.h), for tests/test_insulation_ref.py (against
scipy.signal), tests/test_gpu_insulation.py and tools/insulation.py (against the device).

A map is a pair: ("if", M) with M an n x n matrix, ("model", x) with x n x 3 coordinates, ("consensus", [x, ...]) the pick list's models.
Square sums are accumulated in numpy.longdouble and rounded once (the device of compartment_ref.expected_from_sums): any order of double
additions of the same positive terms then lies within (terms - 1) 2^-53 of them, relative.  Counts are integers.  Everything after the
means — the score row, the boundaries, the prominences, the fit — is written out as the header defines it, one operation at a time."""
import numpy as np

NAN = float("nan")


def block_distances(x, i, w):
    """the distances d(a, b), a in [i-w, i-1], b in [i+1, i+w], of a model: the host's distance operation for operation"""
    u = x[i - w:i, None, :] - x[None, i + 1:i + w + 1, :]
    return np.sqrt(((u[..., 0] * u[..., 0]) + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])


def consensus_block(models, i, w):
    """the pick list's mean distance over the square: summed in list order from 0.0 and divided once"""
    s = np.zeros((w, w))
    for x in models:
        s = s + block_distances(x, i, w)
    return s / float(len(models))


def square_mean(kind, src, i, w, cutoff=None):
    """mean[q][w][i] of a bead that is inside"""
    if kind == "if":
        cells = np.asarray(src, dtype=np.float64)[i - w:i, i + 1:i + w + 1]
    elif kind == "model":
        d = block_distances(src, i, w)
        if cutoff is not None:
            return float(int((d < cutoff).sum())) / float(w * w)
        cells = d
    else:
        if cutoff is not None:
            return float(sum(int((block_distances(x, i, w) < cutoff).sum()) for x in src)) / float(w * w * len(src))
        cells = consensus_block(src, i, w)
    return float(np.float64(cells.astype(np.longdouble).sum())) / float(w * w)


def mean_row(kind, src, n, w, cutoff=None, beads=None):
    """definition 2 for one map and window; beads: compute these beads only (the others NaN), for maps too large to walk whole"""
    if kind != "if":
        src = [np.asarray(x, dtype=np.float64) for x in src] if kind == "consensus" else np.asarray(src, dtype=np.float64)
    out = np.full(n, NAN)
    for i in (range(w, n - w) if beads is None else beads):
        if w <= i <= n - 1 - w:
            out[i] = square_mean(kind, src, i, w, cutoff)
    return out


def score_row(mean):
    """definition 3: log2(mean_i / mbar) over the valid beads (inside, mean > 0), NaN elsewhere"""
    mean = np.asarray(mean, dtype=np.float64)
    valid = mean > 0.0                                                          # NaN > 0 is False
    out = np.full(len(mean), NAN)
    if valid.any():
        mbar = float(np.float64(mean[valid].astype(np.longdouble).sum())) / float(int(valid.sum()))
        out[valid] = np.log2(mean[valid] / mbar)
    return out


def boundaries(score, minima, margins=False, same=None):
    """definition 4 on one score row: (boundary int32 [n], strength [n]); with margins=True also, per bead, the smallest |y_j - y_i| among
    the comparisons that decide the bead's entries: its two neighbours and, for a boundary, every bead its walks compare with y_i.
    same: the row's means where they are known to be the other side's bit for bit (contact maps) — beads of equal mean have equal scores
    on both sides, whatever the rounding, so their comparison is not one a margin has to cover"""
    s = np.asarray(score, dtype=np.float64)
    y = -s if minima else s
    gap = lambda i, j: np.inf if same is not None and same[i] == same[j] else abs(y[i] - y[j])
    n = len(y)
    mark, strength, margin = np.zeros(n, np.int32), np.zeros(n), np.full(n, np.inf)
    for i in range(n):
        if np.isnan(y[i]):
            continue
        for j in (i - 1, i + 1):
            if 0 <= j < n and not np.isnan(y[j]):
                margin[i] = min(margin[i], gap(i, j))
        if not (1 <= i < n - 1) or not (y[i] > y[i - 1] and y[i] > y[i + 1]):   # a NaN neighbour: False
            continue
        mins = []
        for step in (-1, 1):
            m, j = y[i], i + step
            while 0 <= j < n and y[j] <= y[i]:                                  # stops at a bead that is not valid: NaN <= y is False
                m = min(m, y[j])
                margin[i] = min(margin[i], gap(i, j))
                j += step
            if 0 <= j < n and not np.isnan(y[j]):
                margin[i] = min(margin[i], gap(i, j))                           # the comparison that stopped the walk
            mins.append(m)
        mark[i] = 1
        strength[i] = y[i] - max(mins)
    return (mark, strength, margin) if margins else (mark, strength)


def pearson(x, y):
    """definition 5's r over the beads valid in both rows: the means first, then the centred sums; NaN below 3 beads or for a constant side"""
    both = ~np.isnan(x) & ~np.isnan(y)
    if int(both.sum()) < 3:
        return NAN
    xc, yc = x[both] - x[both].mean(), y[both] - y[both].mean()
    sxx, syy = float((xc * xc).sum()), float((yc * yc).sum())
    if not (sxx > 0.0 and syy > 0.0):
        return NAN
    return float((xc * yc).sum()) / np.sqrt(sxx * syy)


def match_counts(b_if, s_if, b_map, s_map, min_strength, tol):
    """definition 5's {n_IF, n_map, IF_matched, map_matched}"""
    f = np.flatnonzero((np.asarray(b_if) == 1) & (np.asarray(s_if) >= min_strength))
    m = np.flatnonzero((np.asarray(b_map) == 1) & (np.asarray(s_map) >= min_strength))
    near = lambda a, others: int(sum(1 for i in a if len(others) and int(np.abs(others - i).min()) <= tol))
    return np.array([len(f), len(m), near(f, m), near(m, f)], np.int32)


def profile(means, minima):
    """score, boundary, strength of a stack of mean rows [W, n]"""
    score = np.stack([score_row(r) for r in means])
    bs = [boundaries(r, minima) for r in score]
    return score, np.stack([b for b, _ in bs]), np.stack([s for _, s in bs])


def insulation(maps, n, windows, cutoff=None, min_strength=0.0, tol=1, beads=None):
    """The whole call: maps as the module's docstring gives them, IF (if any) first.  A dict with the device's keys."""
    has_if = bool(maps) and maps[0][0] == "if"
    out = {k: [] for k in ("mean", "score", "boundary", "strength")}
    for kind, src in maps:
        means = np.stack([mean_row(kind, src, n, int(w), cutoff, beads) for w in windows])
        score, mark, strength = profile(means, kind == "if" or cutoff is not None)
        for k, v in zip(("mean", "score", "boundary", "strength"), (means, score, mark, strength)):
            out[k].append(v)
    out = {k: np.stack(v) for k, v in out.items()}
    if has_if:
        Q, W = len(maps), len(windows)
        out["fit_r"] = np.array([[pearson(out["score"][q, k], out["score"][0, k]) for k in range(W)] for q in range(1, Q)]).reshape(Q - 1, W)
        out["fit_counts"] = np.array([[match_counts(out["boundary"][0, k], out["strength"][0, k], out["boundary"][q, k], out["strength"][q, k], min_strength, tol)
                                       for k in range(W)] for q in range(1, Q)], np.int32).reshape(Q - 1, W, 4)
    return out


def planted_domains(n, L, seed, step=4.0, hop=30.0):
    """a chain of domains of L beads: the centre moves by `hop` in a random direction at every multiple of L, a bead scatters by `step`
    about its domain's centre.  Its distance map has a domain boundary at every multiple of L."""
    r = np.random.default_rng(seed)
    centre = np.zeros(3)
    x = np.empty((n, 3))
    for i in range(n):
        if i > 0 and i % L == 0:
            d = r.normal(size=3)
            centre = centre + hop * d / np.linalg.norm(d)
        x[i] = centre + step * r.normal(size=3)
    return x
