"""numpy restatement of c3d_entanglement (include/c3d.h): the Gauss pair term of two chain segments as the Van Oosterom-Strackee solid angle
of the parallelogram they span, its row sums (seg_writhe, seg_acn), totals (writhe, acn) and domain tables (link, link_abs), with a
conditioning weight per term.  Vectorised by rows: one row segment against all column segments at a time, never an S x S x 3 array.
Every function takes the float type `ft` (np.float64 or np.longdouble): tests/test_entangle_ref.py holds the fp64 form to the longdouble
one, to a quadrature of the integral and to the four-asin form."""
import numpy as np


def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def _cross(v, w):
    return np.stack([v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1], v[..., 2] * w[..., 0] - v[..., 0] * w[..., 2],
                     v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]], axis=-1)


def _triangle(u, v, w):
    """(atan2 of the triangle, so T / 2; its conditioning weight max(1, |u||v||w| / |den|)); 0 where numerator and denominator are both 0"""
    nu, nv, nw = np.sqrt(_dot(u, u)), np.sqrt(_dot(v, v)), np.sqrt(_dot(w, w))
    num = _dot(u, _cross(v, w))
    vol = nu * nv * nw
    den = vol + _dot(u, v) * nw + _dot(u, w) * nv + _dot(v, w) * nu
    both = (num == 0) & (den == 0)
    half = np.where(both, num.dtype.type(0), np.arctan2(num, den))
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = np.where(den == 0, np.where(vol == 0, 1.0, np.inf), np.maximum(1.0, np.abs(vol / den).astype(np.float64)))
    return half, kappa


def counted(S, s, min_sep, max_sep):
    """mask over t = 0..S-1 of the pairs (s, t) that are counted; max_sep = 0 means S - 1"""
    hi = S - 1 if max_sep == 0 else max_sep
    gap = np.abs(np.arange(S) - s)
    return (gap >= max(min_sep, 2)) & (gap <= hi)


def row_terms(x, s, min_sep=2, max_sep=0, ft=np.float64):
    """g(s, t) for t = 0..S-1 (0 where the pair is not counted) and kappa(s, t) (0 there)"""
    x = np.asarray(x, ft)
    S = len(x) - 1
    two_pi = 2 * ft(np.pi) if ft is np.float64 else 2 * np.arctan2(ft(0), ft(-1))
    m = counted(S, s, min_sep, max_sep)
    t = np.nonzero(m)[0]
    g, kappa = np.zeros(S, ft), np.zeros(S)
    if len(t) == 0:
        return g, kappa
    a, c = x[t] - x[s], x[t + 1] - x[s]
    d, b = x[t] - x[s + 1], x[t + 1] - x[s + 1]
    h1, k1 = _triangle(a, b, c)
    h2, k2 = _triangle(a, d, b)
    g[t] = (h1 + h2) / two_pi                                # (2 h1 + 2 h2) / (4 pi)
    kappa[t] = np.maximum(k1, k2)
    return g, kappa


def rows(x, min_sep=2, max_sep=0, ft=np.float64, which=None):
    """seg_writhe, seg_acn and the sum of kappa over each row's terms, for the rows `which` (all by default)"""
    S = len(x) - 1
    which = range(S) if which is None else which
    w, a, k = np.zeros(len(which), ft), np.zeros(len(which), ft), np.zeros(len(which))
    for q, s in enumerate(which):
        g, kappa = row_terms(x, s, min_sep, max_sep, ft)
        w[q], a[q], k[q] = g.sum(), np.abs(g).sum(), kappa.sum()
    return w, a, k


def entanglement(x, min_sep=2, max_sep=0, bounds=None, ft=np.float64):
    """dict of seg_writhe, seg_acn, seg_kappa (S each), writhe, acn, kappa, and with bounds link, link_abs, link_kappa (D x D)"""
    x = np.asarray(x, ft)
    S = len(x) - 1
    w, a, k = np.zeros(S, ft), np.zeros(S, ft), np.zeros(S)
    D = 0 if bounds is None else len(bounds) - 1
    link, link_abs, link_k = np.zeros((D, D), ft), np.zeros((D, D), ft), np.zeros((D, D))
    dom = None if bounds is None else np.searchsorted(np.asarray(bounds)[1:], np.arange(S), side="right")
    for s in range(S):
        g, kappa = row_terms(x, s, min_sep, max_sep, ft)
        w[s], a[s], k[s] = g.sum(), np.abs(g).sum(), kappa.sum()
        if D:
            p = dom[s]
            at = np.asarray(bounds[p:D])                         # the table is taken from the p <= q side and copied across
            link[p, p:] += np.add.reduceat(g, at)                # the sums over t in domain q = p .. D-1 (the last one runs to S = bounds[D])
            link_abs[p, p:] += np.add.reduceat(np.abs(g), at)
            link_k[p, p:] += np.add.reduceat(kappa, at)
    for p in range(D):
        for q in range(p):
            link[p, q], link_abs[p, q], link_k[p, q] = link[q, p], link_abs[q, p], link_k[q, p]
    out = {"seg_writhe": w, "seg_acn": a, "seg_kappa": k, "writhe": w.sum(), "acn": a.sum(), "kappa": k.sum()}
    if D:
        out.update(link=link, link_abs=link_abs, link_kappa=link_k)
    return out


# ---- independent forms, and shapes with known answers ------------------------------------------------------------------------------------
def asin_term(x, s, t):
    """g(s, t) in the four-asin form of Klenin & Langowski (2000), eqs. 15-16"""
    p1, p2, p3, p4 = x[s], x[s + 1], x[t], x[t + 1]
    r12, r13, r14, r23, r24, r34 = p2 - p1, p3 - p1, p4 - p1, p3 - p2, p4 - p2, p4 - p3
    unit = lambda v: v / np.sqrt(v @ v)
    n1, n2, n3, n4 = unit(np.cross(r13, r14)), unit(np.cross(r14, r24)), unit(np.cross(r24, r23)), unit(np.cross(r23, r13))
    clip = lambda v: np.arcsin(max(-1.0, min(1.0, v)))
    omega = clip(n1 @ n2) + clip(n2 @ n3) + clip(n3 @ n4) + clip(n4 @ n1)
    return omega * np.sign(np.cross(r34, r12) @ r13) / (4 * np.pi)


def quadrature_term(x, s, t, m=400):
    """(1 / 4 pi) of the double integral of (r_s - r_t) . (dr_s x dr_t) / |r_s - r_t|^3 by the midpoint rule on an m x m grid"""
    u = (np.arange(m) + 0.5) / m
    es, et = x[s + 1] - x[s], x[t + 1] - x[t]
    rs = x[s][None, :] + u[:, None] * es[None, :]
    rt = x[t][None, :] + u[:, None] * et[None, :]
    r = rs[:, None, :] - rt[None, :, :]
    return float(((r @ np.cross(es, et)) / np.sqrt((r * r).sum(-1)) ** 3).sum() / (m * m) / (4 * np.pi))


def helix(beads=120, turns=4.0, radius=10.0, pitch=3.0):
    t = np.linspace(0.0, 2 * np.pi * turns, beads)
    return np.stack([radius * np.cos(t), radius * np.sin(t), pitch * t], axis=1)


def spiral(beads=80):
    t = np.linspace(0.0, 6 * np.pi, beads)
    return np.stack([3 * t * np.cos(t), 3 * t * np.sin(t), np.zeros(beads)], axis=1)


def straight(beads=40):
    """beads at whole multiples of a direction with small dyadic components: every difference and every product of two is exact"""
    return np.arange(beads, dtype=np.float64)[:, None] * np.array([1.5, -2.0, 0.25])[None, :]


def ring(m, radius, centre, u, v, phase=0.3):
    t = phase + 2 * np.pi * np.arange(m) / m
    return np.asarray(centre)[None, :] + radius * (np.cos(t)[:, None] * np.asarray(u, float)[None, :] + np.sin(t)[:, None] * np.asarray(v, float)[None, :])


def two_rings(linked=True, m=24):
    """Two closed m-gons joined into one chain of 2 (m + 1) beads (each ring returns to its first bead), and the bounds of the three
    domains ring / joining segment / ring.  Linked: the second ring passes through the first; else it lies four radii away.  The rings
    start at a phase of 0.3, so that the joining segment lies in neither ring's plane: a segment in the plane of another that touches or
    crosses it has the origin on the parallelogram's edge, where the solid angle jumps."""
    a = ring(m, 10.0, (0.0, 0.0, 0.0), (1, 0, 0), (0, 1, 0))
    b = ring(m, 10.0, (10.0 if linked else 40.0, 0.0, 0.0), (1, 0, 0), (0, 0, 1))
    x = np.concatenate([a, a[:1], b, b[:1]])
    return x, np.array([0, m, m + 1, 2 * m + 1], np.int32)
