"""The pair term's table problems (CPU only; admitted by tests/test_pair_cases.py, run by tests/test_gpu_pair_table.py).

A. ISOLATED PAIRS (table_a).  Bonds and angles off (k_bond = k_ang = 0).  Bead p < n/2 sits on a site of a coarse lattice, its only partner
   p + n/2 at site + d u; the spacing (a power of two, per replica) exceeds twice the replica's longest d plus the repel radius, so the
   force on a bead is ONE pair term.  The pair's class p % 7 fixes its target — 2.5, 0.1, 3.9, 25, 2000 A, none or 101 A — for every replica
   (101 A puts D = 10 mrswitch of the default model at d = 1 A, where under a zero repel weight the deep term is the whole force and the bound 2 % of it); a
   replica is one REGIME of d: `zero` (d - t either side of 0 on adjacent values of one coordinate; one pair along +x from the origin with
   d = t = 2.5 exactly), `switch` (either side of +rswitch, -rswitch, -mrswitch), `deep` (D = 3 and 10 mrswitch, d = 10 t, d = 1e3 A),
   `small` (1e-2, 1e-3, 1e-4 A and two beads at one point), `repel` (r either side of repel_s r0_rep, R / 2, R / 100).  Pairs without a
   target sit 1e-3 and 1 A apart on the lattice and 50 and 1e4 A apart on a line of their own far below it.  Directions: the 26 axes and
   diagonals with every sign pattern.  Sites are dealt out by distance from the origin, the smallest targets first, so the finest rows
   have the finest coordinates.  Everything is rounded to the type under test (float32 / float64) HERE: expected values are computed
   from what the device is given.
B. CHAIN GROUPS (table_b), with table C inside.  Default k_bond, k_ang; runs of five consecutive beads (the last may be shorter) on a
   64 A lattice: `bond_edge` (d01 either side of b0), `bond_exact` (d01 = b0 to the bit wherever the site has a zero coordinate), `angle_edge` (d02 either side of a0), `compressed` (separation-2
   neighbours 3.5 A apart, inside the repel radius), `folded` (a 120-degree helix: separation 3 at 3.0 A and separation 2 at 4.3 A inside
   the radius), `listed` (at rest; restraints LISTED for its separations 2 and 4 = min_sep - 1 at delta = +3 A, which no form may feel,
   and a real one to the next run's first bead).  Replica 0 takes the lower side of every edge, replica 1 the upper.  The beads that join
   two runs carry a bond stretched to the lattice spacing; they stay in the table."""
import functools
import itertools

import numpy as np

SIZES = (250, 328, 1100)          # four columns a lane and nothing left over; one column a lane in the last block + 8 left-over columns; wide form
CLASS_T10 = (25, 1, 39, 250, 20000, 0, 1010)
NCLASS = len(CLASS_T10)
REGIMES = ("zero", "switch", "deep", "small", "repel")
STAGE = (1.0, 1.0, 0.85)          # (w_all, w_vdw, repel_s) the tables' repel edges are built for
WEIGHTS = (STAGE, (0.4, 0.0, 0.9))
DIRS = np.array([v for v in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(v)])
DIRS = DIRS / np.linalg.norm(DIRS, axis=1, keepdims=True)
SHAPES = ("bond_edge", "bond_exact", "angle_edge", "compressed", "folded", "listed")
PAD = np.array([[1e4 * (c + 1) + 16.0 * k for c in range(3)] for k in range(256)])     # where the library parks its padding beads

_LD = np.longdouble


def dist(a, b):
    """|a - b| in extended precision: the side of an edge a coordinate's last bit decides"""
    u = np.asarray(a, dtype=_LD) - np.asarray(b, dtype=_LD)
    return np.sqrt((u * u).sum())


def straddle(fixed, start, d_edge, comp, away, dtype):
    """(below, above): two points that differ by ONE step of `dtype` in coordinate `comp`, |below - fixed| < d_edge <= |above - fixed|;
    `away` = the sign of the step in that coordinate that lengthens the distance"""
    y = np.array(start, dtype=dtype)
    far = dtype(np.inf) * dtype(away)
    for _ in range(8):                              # the other coordinates' rounding, taken out in this one
        cur = dist(y, fixed)
        y[comp] = dtype(_LD(y[comp]) + (d_edge - cur) * cur / (_LD(y[comp]) - _LD(fixed[comp])))
    for _ in range(200):
        if dist(y, fixed) < d_edge:
            break
        y[comp] = np.nextafter(y[comp], -far)
    below = y.copy()
    for _ in range(200):
        above = below.copy()
        above[comp] = np.nextafter(above[comp], far)
        if dist(above, fixed) >= d_edge:
            return below, above
        below = above
    raise AssertionError("no straddle found")


def _lattice(count, spacing):
    """`count` lattice sites of a centred cube, nearest the origin first"""
    k = int(np.ceil(count ** (1.0 / 3.0)))
    k += 1 - k % 2                                  # an odd edge: the origin is a site
    g = np.arange(k) - k // 2
    pts = np.array(list(itertools.product(g, g, g)), dtype=np.float64)
    order = np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0], np.abs(pts).max(1), (pts * pts).sum(1)))
    return pts[order][:count] * spacing


def _specs(regime, t, rs, mrs, R):
    """the d of a restrained pair in a regime: ("at", d) or ("edge", d_edge) — an edge is taken from below and from above by two pairs"""
    if regime == "zero":
        return [("edge", t)]
    if regime == "switch":
        return [("edge", e) for e in (t + rs, t - rs, t - mrs) if e > 1e-3]
    if regime == "deep":
        return [("at", d) for d in (t - 3.0 * mrs, t - 10.0 * mrs, 10.0 * t, 1000.0) if 1e-3 < d <= 2000.0]
    if regime == "small":
        return [("at", d) for d in (1e-2, 1e-3, 1e-4, 0.0)]
    return [("edge", R), ("at", 0.5 * R), ("at", 0.01 * R)]


def table_a(n, P, dtype):
    """dict(ri, rj, rt10: the list for c3d_set_restraints (1-based); t10 [n, n]; x [5, n, 3] in dtype; meta: per replica and pair
    (regime, kind, d_edge or d, side); spacing per replica) for the model numbers P (pair_ref.params_from)"""
    assert n % 2 == 0
    h = n // 2
    rs, mrs, R = P["rswitch"], P["mrswitch"], STAGE[2] * P["r0_rep"]
    cls = np.arange(h) % NCLASS
    q = np.arange(h) // NCLASS
    t10 = np.zeros((n, n), dtype=np.int32)
    for p in range(h):
        t10[p, p + h] = t10[p + h, p] = CLASS_T10[cls[p]]
    keep = [p for p in range(h) if CLASS_T10[cls[p]] > 0]
    ri, rj, rt = [p + 1 for p in keep], [p + h + 1 for p in keep], [CLASS_T10[cls[p]] for p in keep]
    far_none = [p for p in range(h) if cls[p] == 5 and q[p] % 4 >= 2]          # 50 and 1e4 A: on a line of their own
    on_lattice = [p for p in range(h) if p not in far_none]
    # sites by distance from the origin: the exact pair (class 0, q 0) first, then ascending targets
    on_lattice.sort(key=lambda p: (p != 0, CLASS_T10[cls[p]] if cls[p] != 5 else 10 ** 9, q[p]))
    x = np.zeros((len(REGIMES), n, 3), dtype=dtype)
    meta, spacings = [], []
    for r, regime in enumerate(REGIMES):
        plan = {}
        for p in range(h):
            t = 0.1 * CLASS_T10[cls[p]]
            if cls[p] == 5:
                plan[p] = ("at", (1e-3, 1.0, 50.0, 1e4)[q[p] % 4], 0)
                continue
            specs = _specs(regime, t, rs, mrs, R)
            slots = [(k, d, s) for k, d in specs for s in ((-1, 1) if k == "edge" else (0,))]
            plan[p] = slots[q[p] % len(slots)]
        if regime == "zero":
            plan[0] = ("at", 2.5, 0)
        # pairs up to 300 A apart on the inner lattice, the longer ones on an outer one of 8192 A (its origin site left out)
        inner = [p for p in on_lattice if plan[p][1] <= 300.0]
        outer = [p for p in on_lattice if plan[p][1] > 300.0]
        spacing = 2.0 ** np.ceil(np.log2(2.0 * max(plan[p][1] for p in inner) + 16.0))
        site = {p: s for p, s in zip(inner, _lattice(len(inner), spacing))}
        site.update({p: s for p, s in zip(outer, _lattice(len(outer) + 1, 8192.0)[1:])})
        for k, p in enumerate(far_none):
            site[p] = np.array([0.0, 320.0 * k, -30000.0])
        rows = []
        for p in range(h):
            kind, d, side = plan[p]
            cycle = q[p] // 6
            u = DIRS[(7 * cycle + 5 * cls[p] + 3 * r + p) % 26]
            if p in far_none or (regime == "zero" and p == 0):
                u = np.array([1.0, 0.0, 0.0])
            s = site[p].astype(dtype)
            assert np.array_equal(s.astype(np.float64), site[p])
            x[r, p] = s
            start = (site[p] + d * u).astype(dtype)
            if kind == "edge":
                comp = int(np.flatnonzero(u)[0])
                below, above = straddle(s, start, d, comp, np.sign(u[comp]), dtype)
                start = below if side < 0 else above
            x[r, p + h] = start
            rows.append((regime, kind, d, side, tuple(u)))
        meta.append(rows)
        spacings.append(spacing)
    return dict(ri=np.array(ri, dtype=np.int32), rj=np.array(rj, dtype=np.int32), rt10=np.array(rt, dtype=np.int32), t10=t10, x=x, meta=meta,
                spacing=spacings, cls=cls, half=h, none=[p for p in range(h) if cls[p] == 5])


def _run_shape(shape, site, P, side, dtype, length):
    """the beads of one run: [length, 3] in dtype, and the edge it sits at (bead a, bead b, d_edge) or None"""
    b0, a0 = P["b0"], P["a0"]
    px = 1.75 if shape == "compressed" else 0.5 * a0
    py = np.sqrt(b0 * b0 - px * px)
    if shape == "folded":
        # rho^2 A1 + h^2 = b0^2 and rho^2 A3 + 9 h^2 = 3.0^2 with A1 = 2 (1 - cos 120) = 3, A3 = 2 (1 - cos 360) = 0
        rho = np.sqrt((9.0 * b0 * b0 - 9.0) / 27.0)
        hz = np.sqrt(b0 * b0 - 3.0 * rho * rho)
        pts = np.array([[rho * np.cos(k * 2.0 * np.pi / 3.0) - rho, rho * np.sin(k * 2.0 * np.pi / 3.0), k * hz] for k in range(5)])
    elif shape in ("bond_edge", "bond_exact"):      # the first bond along x, the zigzag from bead 1 on
        pts = np.array([[0.0, 0.0, 0.0]] + [[b0 + k * px, (k % 2) * py, 0.0] for k in range(4)])
        if shape == "bond_exact" and (site == 0).any():      # along a coordinate in which the site is 0: there 0 + b0 is b0 itself
            pts = np.roll(pts, int(np.flatnonzero(site == 0)[0]), axis=1)
    else:
        pts = np.array([[k * px, (k % 2) * py, 0.0] for k in range(5)])
    y = (site + pts).astype(dtype)
    edge = None
    if shape == "bond_edge" or shape == "bond_exact":
        if shape == "bond_edge":
            below, above = straddle(y[0], y[1], b0, 0, 1.0, dtype)
            y[1] = below if side < 0 else above
            edge = (0, 1, b0)
    elif shape == "angle_edge" and length >= 3:
        below, above = straddle(y[0], y[2], a0, 0, 1.0, dtype)
        y[2] = below if side < 0 else above
        edge = (0, 2, a0)
    return y[:length], edge


def table_b(n, P, dtype):
    """dict(ri, rj, rt10, t10 (what the oracle is given: WITH the listed pairs closer than min_sep, which it filters), x [2, n, 3],
    runs: [(first bead, length, shape)], edges: per replica [(bead a, bead b, d_edge, side)], listed_close: the pairs table C lists)"""
    runs = [(a, min(5, n - a), SHAPES[(a // 5) % len(SHAPES)]) for a in range(0, n, 5)]
    assert all(3 <= length <= 5 for _, length, _ in runs)
    sites = _lattice(len(runs), 64.0)
    order = np.lexsort((sites[:, 0], sites[:, 1], sites[:, 2]))          # consecutive runs on neighbouring sites, x fastest
    sites = sites[order]
    x = np.zeros((2, n, 3), dtype=dtype)
    edges = [[], []]
    for r, side in enumerate((-1, 1)):
        for k, (a, length, shape) in enumerate(runs):
            y, edge = _run_shape(shape, sites[k], P, side, dtype, length)
            x[r, a:a + length] = y
            if edge:
                edges[r].append((a + edge[0], a + edge[1], edge[2], side))
    t10 = np.zeros((n, n), dtype=np.int32)
    ri, rj, rt, close = [], [], [], []
    x0 = x[0].astype(np.float64)
    for a, length, shape in runs:
        if shape != "listed" or length < 5:
            continue
        for b in (a + 2, a + P["min_sep"] - 1):                          # table C: listed, closer than min_sep, delta = +3 A
            t = int(round(10.0 * (np.linalg.norm(x0[a] - x0[b]) - 3.0)))
            assert t > 0 and b - a < P["min_sep"]
            ri.append(a + 1); rj.append(b + 1); rt.append(t); close.append((a, b))
            t10[a, b] = t10[b, a] = t
        b = a + 5
        if b < n:                                                        # a real one: the next run's first bead, delta = 0 or +3 A
            t = int(round(10.0 * (np.linalg.norm(x0[a] - x0[b]) - (3.0 if (a // 5) % 12 >= 6 else 0.0))))
            ri.append(a + 1); rj.append(b + 1); rt.append(t)
            t10[a, b] = t10[b, a] = t
    return dict(ri=np.array(ri, dtype=np.int32), rj=np.array(rj, dtype=np.int32), rt10=np.array(rt, dtype=np.int32), t10=t10, x=x, runs=runs,
                edges=edges, listed_close=close)


def sweep(n):
    """what a size's pairs (p, p + n/2) cover, both beads being rows and columns: (columns that are some row's partner, row-of-wave slots
    i % 4 of the rows, the pairs (row slot, column slot j % 4) met)"""
    h = n // 2
    rows = np.concatenate([np.arange(h), np.arange(h) + h])
    cols = np.concatenate([np.arange(h) + h, np.arange(h)])
    return set(cols.tolist()), set((rows % 4).tolist()), set(zip((rows % 4).tolist(), (cols % 4).tolist()))


def isolation(x, partner_of, radius):
    """the smallest distance from any bead to a bead that is not itself or its partner, and to the library's padding beads, over a replica"""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    d2[np.arange(n), np.arange(n)] = np.inf
    d2[np.arange(n), partner_of] = np.inf
    pad = np.sqrt(((x[:, None, :] - PAD[None, :, :]) ** 2).sum(-1)).min()
    return float(np.sqrt(d2.min())), float(pad)


@functools.lru_cache(maxsize=None)
def cached_table(kind, n, key, precision):
    """table_a / table_b for the model numbers `key` (a sorted tuple of pair_ref.params_from's items), built once per session"""
    P = dict(key)
    return (table_a if kind == "a" else table_b)(n, P, np.float32 if precision == 32 else np.float64)


# ---- the models the tables run under -------------------------------------------------------------------------------------------------
# A: the NOE forms of tests/test_gpu_step_kernels.py's VARIANTS (its ang0 / kang0 differ from `shipped` in the chain terms only, which A
# switches off: they run in B).  B: the chain's switches.
A_VARIANTS = ("shipped", "pot0", "pot1", "pot2", "pot3_clamp", "pot3_rs1", "gen0", "gen1", "gen2", "gen3")
B_VARIANTS = {"shipped": {}, "ang0": dict(ang_mode=0, k_ang=200.0, a0=6.0), "kang0": dict(k_ang=0.0), "rep1": dict(rep_sep=1), "rep3": dict(rep_sep=3)}


def model_a(variant, **more):
    """(c3d_model, device potential, general tail) of an A variant: the variant's NOE form with bonds and angles off"""
    from chromosome3d_amd import default_model
    from tests.test_gpu_step_kernels import VARIANTS
    kw, pot, gen = VARIANTS[variant]
    return default_model(**dict(kw, k_bond=0.0, k_ang=0.0, **more)), pot, gen


def model_b(variant):
    from chromosome3d_amd import default_model
    return default_model(**B_VARIANTS[variant])


def table_for(kind, n, m, precision):
    from tests import pair_ref
    return cached_table(kind, n, tuple(sorted(pair_ref.params_from(m).items())), precision)
