"""The numpy restatement of c3d_loops (include/c3d.h, "Loop enrichment"): every definition as written there, over pixels and cells in the
defined order.  A map is ("if", M [n, n]), ("model", x [n, 3]) or ("consensus", [x, ...]); a model's distance is computed with every
operation rounded on its own, ((ux ux) + uy uy) + uz uz and the root, so a distance has the device's bits and only sums can differ.  The
eight neighbourhood sums of a pixel are sequential sums in row-major order (numpy's cumsum adds in index order), as the definition
fixes them; E and the pile-up's sums are numpy's own, whose order is not the device's.  Also the two planted inputs of the tests."""
import numpy as np

NAN = float("nan")


def cells(kind, src, A, B):
    """M(A, B) of a map for index arrays of one shape"""
    if kind == "if":
        return np.asarray(src)[A, B]
    if kind == "model":
        x = np.asarray(src, dtype=np.float64)
        u = x[A] - x[B]
        q = u[..., 0] * u[..., 0]
        q = q + u[..., 1] * u[..., 1]
        q = q + u[..., 2] * u[..., 2]
        return np.sqrt(q)
    total = np.zeros(np.broadcast(A, B).shape)
    for x in src:                                                               # list order from 0.0, divided once
        total = total + cells("model", x, A, B)
    return total / float(len(src))


def band_range(n, w, min_sep, max_sep):
    s_lo, s_hi = min_sep - 2 * w, min(max_sep + 2 * w, n - 1)
    return s_lo, s_hi


def expected(kind, src, n, masked, s_lo, s_hi):
    """E[s_lo .. s_hi] of a map: the mean over the live cells of a separation, 0 where there is none"""
    E = np.zeros(s_hi - s_lo + 1)
    for s in range(s_lo, s_hi + 1):
        i = np.arange(n - s)
        live = ~masked[i] & ~masked[i + s]
        if live.any():
            E[s - s_lo] = cells(kind, src, i[live], i[live] + s).sum() / float(live.sum())
    return E


def neighbourhoods(p, w):
    """the four boolean (2w+1) x (2w+1) masks over (a, b): donut, lower-left, horizontal, vertical"""
    a = np.arange(-w, w + 1)[:, None]
    b = np.arange(-w, w + 1)[None, :]
    P = (np.abs(a) <= p) & (np.abs(b) <= p)
    return [~P & (a != 0) & (b != 0), ~P & (a >= 1) & (b <= -1), (np.abs(a) <= 1) & (np.abs(b) > p), (np.abs(b) <= 1) & (np.abs(a) > p)]


def pixels(kind, src, E, n, masked, p, w, s_lo, I, J, chunk=512):
    """[L, 6] for the pixels (I, J): M(i,j), E[s], r_donut, r_ll, r_h, r_v — the ratios NaN where the definition says so"""
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    out = np.full((len(I), 6), NAN)
    if not len(I):
        return out
    out[:, 0] = cells(kind, src, I, J)
    out[:, 1] = E[J - I - s_lo]
    ok = np.flatnonzero((I >= w) & (J + w <= n - 1) & ~masked[I] & ~masked[J] & (out[:, 1] != 0.0))
    nb = neighbourhoods(p, w)
    off = np.arange(-w, w + 1)
    for c0 in range(0, len(ok), chunk):
        k = ok[c0:c0 + chunk]
        A = (I[k][:, None, None] + off[None, :, None]) + 0 * off[None, None, :]
        Bc = (J[k][:, None, None] + off[None, None, :]) + 0 * off[None, :, None]
        live = ~masked[A] & ~masked[Bc]
        vals = cells(kind, src, A, Bc)
        Ev = E[Bc - A - s_lo]
        for x in range(4):
            sel = (live & nb[x][None]).reshape(len(k), -1)
            SM = np.cumsum(np.where(sel, vals.reshape(len(k), -1), 0.0), axis=1)[:, -1]     # row-major, one accumulator; + 0.0 changes no bit
            SE = np.cumsum(np.where(sel, Ev.reshape(len(k), -1), 0.0), axis=1)[:, -1]
            with np.errstate(divide="ignore", invalid="ignore"):
                r = out[k, 0] / ((SM / SE) * out[k, 1])
            out[k, 2 + x] = np.where((SM == 0.0) | (SE == 0.0), NAN, r)
    return out


def scan(M, E, n, masked, p, w, min_sep, max_sep, seps=None, step=1):
    """the dense scan of IF: ratio [4, B, n], NaN beyond the matrix; seps / step: only those separations and every step-th row (the
    others stay NaN)"""
    s_lo = min_sep - 2 * w
    B = max_sep - min_sep + 1
    ratio = np.full((4, B, n), NAN)
    for s in (range(min_sep, max_sep + 1) if seps is None else seps):
        I = np.arange(0, n - s, step)
        ratio[:, s - min_sep, I] = pixels("if", M, E, n, masked, p, w, s_lo, I, I + s)[:, 2:].T
    return ratio


def band_values(M, n, min_sep, max_sep):
    """[B, n]: M(i, i + s), 0 beyond the matrix"""
    out = np.zeros((max_sep - min_sep + 1, n))
    for s in range(min_sep, max_sep + 1):
        i = np.arange(n - s)
        out[s - min_sep, i] = np.asarray(M)[i, i + s]
    return out


def _shift(X, ds, di, fill):
    """Y[s, i] = X[s + ds, i + di], `fill` where that lies outside"""
    Y = np.full(X.shape, fill, dtype=X.dtype)
    B, n = X.shape
    s0, s1 = max(0, -ds), min(B, B - ds)
    i0, i1 = max(0, -di), min(n, n - di)
    if s0 < s1 and i0 < i1:
        Y[s0:s1, i0:i1] = X[s0 + ds:s1 + ds, i0 + di:i1 + di]
    return Y


def call_peaks(ratio, vals, n, masked, w, min_sep, thr, min_obs, merge, max_peaks):
    """steps 6 of the definition on given ratio bytes: (candidate flags [B, n], peak flags [B, n], peaks [written, 2], report[4])"""
    B = ratio.shape[1]
    with np.errstate(invalid="ignore"):
        cand = (vals >= min_obs)
        for x in range(4):
            cand &= ratio[x] >= thr[x]
    beaten = np.zeros_like(cand)
    for di in range(-merge, merge + 1):
        for dj in range(-merge, merge + 1):
            if di == 0 and dj == 0:
                continue
            c2, v2 = _shift(cand, dj - di, di, False), _shift(vals, dj - di, di, 0.0)
            first = di < 0 or (di == 0 and dj < 0)
            beaten |= c2 & ((v2 > vals) | ((v2 == vals) & first))
    peak = cand & ~beaten
    found = np.argwhere(peak.T)                                                 # (i, s index) ascending: ascending (i, j)
    pk = np.stack([found[:, 0], found[:, 0] + found[:, 1] + min_sep], axis=1).astype(np.int32) if len(found) else np.zeros((0, 2), np.int32)
    s = np.arange(min_sep, min_sep + B)[:, None]
    i = np.arange(n)[None, :]
    j = i + s
    inside = (i >= w) & (j + w <= n - 1)
    lost = inside & (masked[i] | masked[np.minimum(j, n - 1)])
    report = np.array([cand.sum(), len(pk), min(len(pk), max_peaks), lost.sum()], dtype=np.int32)
    return cand, peak, pk[:max_peaks], report


def margins(ratio, vals, thr, min_obs):
    """[B, n]: the least relative distance of a pixel's ratios from their thresholds (inf for a pixel with a NaN ratio: it is no
    candidate whatever the rounding).  min_obs has no margin: M(i,j) >= min_obs compares two input values, exactly."""
    with np.errstate(invalid="ignore"):
        m = np.min([np.abs(ratio[x] - thr[x]) / thr[x] for x in range(4)], axis=0)
    return np.where(np.isnan(m), np.inf, m)


def closed(at_rows, is_if):
    """{pixels whose r_donut and r_ll are both numbers, of those the ones with both on the loop side}"""
    rd, rl = at_rows[:, 2], at_rows[:, 3]
    ok = ~np.isnan(rd) & ~np.isnan(rl)
    with np.errstate(invalid="ignore"):
        side = (rd > 1.0) & (rl > 1.0) if is_if else (rd < 1.0) & (rl < 1.0)
    return np.array([ok.sum(), (ok & side).sum()], dtype=np.int32)


def apa(kind, src, E, n, masked, w, s_lo, I, J, corner):
    """the pile-up [2w+1, 2w+1] and P2LL"""
    I, J = np.asarray(I, dtype=np.int64), np.asarray(J, dtype=np.int64)
    side = 2 * w + 1
    A = np.full((side, side), NAN)
    inside = (I >= w) & (J + w <= n - 1)
    I, J = I[inside], J[inside]
    for a in range(-w, w + 1):
        for b in range(-w, w + 1):
            if not len(I):
                continue
            ca, cb = I + a, J + b
            ok = ~masked[ca] & ~masked[cb]
            e = E[cb - ca - s_lo]
            ok &= e != 0.0
            if ok.any():
                A[a + w, b + w] = (cells(kind, src, ca[ok], cb[ok]) / e[ok]).sum() / float(ok.sum())
    total = 0.0
    for a in range(w - corner + 1, w + 1):
        for b in range(-w, -w + corner):
            total += A[a + w, b + w]
    with np.errstate(divide="ignore", invalid="ignore"):
        p2ll = np.float64(A[w, w]) / np.float64(total / float(corner * corner))
    return A, float(p2ll)


def loops(maps, n, mask=None, p=2, w=5, min_sep=None, max_sep=None, thr=(1.75, 1.75, 1.5, 1.5), min_obs=0.0, merge=2, corner=3, listed=None, max_peaks=65536,
          dense=True):
    """the whole call: a dict with the entry's outputs (ratio, peaks and report only when maps[0] is IF; `dense=False` leaves them out)"""
    masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask) != 0
    min_sep = 2 * w + 1 if min_sep is None else min_sep
    max_sep = n - 1 if max_sep is None else max_sep
    s_lo, s_hi = band_range(n, w, min_sep, max_sep)
    out = {"expected": np.stack([expected(k, src, n, masked, s_lo, s_hi) for k, src in maps])}
    has_if = maps[0][0] == "if"
    if has_if and dense:
        out["ratio"] = scan(maps[0][1], out["expected"][0], n, masked, p, w, min_sep, max_sep)
        vals = band_values(maps[0][1], n, min_sep, max_sep)
        out["cand"], out["peak"], out["peaks"], out["report"] = call_peaks(out["ratio"], vals, n, masked, w, min_sep, thr, min_obs, merge, max_peaks)
        out["margin"] = margins(out["ratio"], vals, thr, min_obs)
    if listed is None and "peaks" in out:
        listed = out["peaks"]
    if listed is not None:
        listed = np.asarray(listed, dtype=np.int64).reshape(-1, 2)
        out["pixels"] = listed
        out["at"] = np.stack([pixels(k, src, out["expected"][q], n, masked, p, w, s_lo, listed[:, 0], listed[:, 1]) for q, (k, src) in enumerate(maps)])
        out["closed"] = np.stack([closed(out["at"][q], has_if and q == 0) for q in range(len(maps))])
        both = [apa(k, src, out["expected"][q], n, masked, w, s_lo, listed[:, 0], listed[:, 1], corner) for q, (k, src) in enumerate(maps)]
        out["apa"] = np.stack([a for a, _ in both])
        out["p2ll"] = np.array([v for _, v in both])
    return out


def planted_map(n, loops, amp=4, sig=1):
    """a contact map with the distance decay of a polymer, a mild per-bin bias and a Gaussian spot at every planted (a, b):
    M(i,j) = 100 / |i-j| g_i g_j, g_i = 1 + 0.05 sin(0.37 i), times 1 + amp exp(-((i-a)^2 + (j-b)^2) / (2 sig^2)) and its transpose for
    every spot, symmetrised by max.  Beyond r = 9 sig + 1 bins of a spot its factor is exactly 1.0 (amp e^-40 is below half an ulp of
    1), so only that square and its mirror image are multiplied: the same bits as over the whole matrix."""
    i = np.arange(n)
    g = 1.0 + 0.05 * np.sin(0.37 * i)
    sep = np.abs(i[:, None] - i[None, :])
    M = 100.0 / np.where(sep > 0, sep, 1) * g[:, None] * g[None, :]
    np.fill_diagonal(M, 0.0)
    r = int(np.ceil(9 * sig)) + 1
    assert amp * np.exp(-r * r / (2.0 * sig * sig)) < 2.0 ** -54
    for a, b in loops:
        ia, ib = np.arange(max(0, a - r), min(n, a + r + 1)), np.arange(max(0, b - r), min(n, b + r + 1))
        spot = 1.0 + amp * np.exp(-((ia[:, None] - a) ** 2 + (ib[None, :] - b) ** 2) / (2.0 * sig * sig))
        M[np.ix_(ia, ib)] *= spot
        M[np.ix_(ib, ia)] *= spot.T
    return np.maximum(M, M.T)


# the planted contact maps of tests/test_gpu_loops.py: n, planted loops, w, p, min_sep, max_sep, and for the restatement the separations
# and the row step it is held to (None, 1: every pixel)
PLANTED_CASES = {
    "120": (120, [(30, 60), (50, 95), (70, 90)], 5, 2, 11, 50, None, 1),
    "80": (80, [(20, 40), (35, 60)], 3, 1, 7, 30, None, 1),
    "one pixel": (6, [], 1, 0, 3, 3, None, 1),
    "one pixel, clipped": (6, [], 1, 0, 3, 5, None, 1),
    "two pixels": (7, [], 1, 0, 3, 4, None, 1),
    "largest window, p = 19": (82, [], 20, 19, 41, 41, None, 1),
    "largest window, p = 0": (83, [(21, 62)], 20, 0, 41, 42, None, 1),
    "n = 31": (31, [(8, 20)], 2, 1, 5, 30, None, 1),
    "n = 32": (32, [(8, 20)], 2, 1, 5, 31, None, 1),
    "n = 33": (33, [(8, 20), (3, 30)], 2, 1, 5, 32, None, 1),
    "n = 65": (65, [(8, 20), (30, 62), (31, 40)], 2, 1, 5, 64, None, 1),
    "B = 31": (100, [(31, 40), (32, 63), (60, 95)], 3, 1, 7, 37, None, 1),
    "B = 32": (100, [(31, 40), (32, 63), (60, 98)], 3, 1, 7, 38, None, 1),
    "B = 33": (100, [(31, 40), (32, 64), (63, 96)], 3, 1, 7, 39, None, 1),
    "B = 65": (140, [(31, 40), (32, 96), (64, 135)], 3, 1, 7, 71, None, 1),
    "B = 1024": (1060, [(10, 20), (500, 900), (20, 1040)], 1, 0, 3, 1026, None, 1),
    "4096": (4096, [(500, 560), (1000, 1041), (2048, 2150), (4000, 4060)], 20, 4, 41, 104, list(range(41, 105, 7)), 97),
}


def planted_rosette(n, petal, seed):
    """[n, 3]: a chain of closed circular petals of `petal` beads; every petal starts at its base on the z axis and returns to it, the
    bases advance by 3 A, the petals' planes turn by the golden angle, so that bead a = m petal and bead a + petal nearly coincide while
    their neighbours point apart; a seeded jitter of 0.05 A"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    m, t = k // petal, 2.0 * np.pi * (k % petal) / petal
    R = 10.0 * petal / (2.0 * np.pi)
    phi = 2.399963229728653 * m
    x = np.stack([R * (1.0 - np.cos(t)) * np.cos(phi), R * (1.0 - np.cos(t)) * np.sin(phi), 3.0 * m + R * np.sin(t)], axis=1)
    return x + rng.normal(scale=0.05, size=(n, 3))
