"""fp64 restatement of the L-BFGS stage (stage kind 8; device kinds 9 / 8, chromosome3d_amd/csrc/c3d_lbfgs.h), step for step as the device
runs it: L-BFGS with m pairs in the compact form (Byrd-Nocedal-Schnabel) built from the projections of the CURRENT gradient, a fixed unit
step (no energy, no line search), every bead's move capped at fire.max_step, a pair kept only if s.y > 1e-12 |s| |y|, the memory dropped
when the direction is not downhill; gamma = the kind-6 first step length dt_start^2 * acc at the stage's first step, s.y / y.y after a kept
pair, doubled after a rejected one, clamped to [1e-7, 1e2].  After the first min(nsteps, final_minimiser_steps) steps FIRE finishes the
stage from a fresh state: the oracle's own FIRE (oracle.run_schedule with a kind-2 stage).  The oracle library is not changed for this."""
import numpy as np

from oracle import oracle as O


def gamma0(model, fire):
    """The first step length of kinds 6 and 9 in the device's fp32 arithmetic: (dt_start * dt_start) * (418.4 / mass)."""
    acc = np.float32(418.4) / np.float32(model.mass)
    dt = np.float32(fire.dt_start)
    return float(np.float32(dt * dt) * acc)


def compact_direction(F, S, Y, gamma):
    """d = -H g (g = -F) for H = gamma I + [S gamma Y] M [S' ; gamma Y'], S / Y in age order (oldest first)."""
    if not S:
        return -gamma * -F
    g = -F
    Sm, Ym = np.array(S), np.array(Y)
    ps, py = np.array([s_.dot(g) for s_ in S]), np.array([y_.dot(g) for y_ in Y])     # the projections of the current gradient
    SY = Sm @ Ym.T
    Rinv = np.linalg.inv(np.triu(SY))
    D = np.diag(np.diag(SY))
    YY = Ym @ Ym.T
    top = Rinv.T @ ((D + gamma * YY) @ (Rinv @ ps)) - Rinv.T @ (gamma * py)
    bot = -Rinv @ ps
    return -(gamma * g + Sm.T @ top + gamma * (Ym.T @ bot))


def rms(F):
    return float(np.sqrt((F * F).mean()))


# name -> what the mutated restatement does differently (lbfgs_run(mutate=name); tests/test_lbfgs_cases.py holds every case table to them)
MUTATIONS = {
    "accept_rejected": "a rejected pair is accepted",
    "no_doubling": "gamma is not doubled after a rejection",
    "reject_keeps_memory": "a rejection keeps the memory",
    "no_lower_clamp": "gamma is not clamped at 1e-7",
    "no_upper_clamp": "gamma is not clamped at 1e2",
    "gamma_ss_sy": "gamma = s.s / s.y",
    "evict_newest": "the newest stored pair is evicted instead of the oldest",
    "age_reversed": "the pairs enter the two solves newest first",
    "no_cap": "no per-bead cap",
    "cap_whole_vector": "the cap acts on the whole vector's norm",
    "s_before_cap": "s is stored before the cap",
    "first_no_mass": "the first length is dt_start^2 * 418.4, without / mass",
    "memory_plus_one": "one pair more than lbfgs_memory is held",
}


class LStep:
    """One step of lbfgs_run.  branch: "first" | "kept" | "rejected", + "+dropped" where the direction was not downhill; clamp: None | "lo" |
    "hi"; pairs: pairs in the direction (after a drop: 0); slot: ring slot of the newest kept pair, as the device counts it (head: mem - 1
    before the first kept pair, + 1 mod mem with every kept pair, unchanged by a rejection or a drop); ncap: beads the cap acted on;
    margin: s.y / sqrt(s.s y.y) of the pair test (None at the first step); cos: F.d / (|F| |d|) of the compact-form direction; graw / gamma:
    the length before and after the clamp."""
    __slots__ = ("it", "branch", "clamp", "pairs", "slot", "ncap", "margin", "cos", "graw", "gamma")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def lbfgs_run(force, x0, nsteps, m=5, g0=1.67e-5, max_step=0.5, gtol=0.0, clamp=True, mutate=None, round32=False, checkpoints=(), mass=1.0):
    """nsteps steps from x0 (n x 3); force(x) -> F (n x 3).  Returns (x, info): info["evals"] = force evaluations made, info["resets"] =
    memory drops (rejected pairs + dropped directions: the device's stat lbfgs_resets per replica), info["rms"] = RMS force of every
    evaluation, info["log"] = one LStep per step, info["checkpoints"] = {k: x after k steps for k in checkpoints}.  gtol > 0: stop after
    the evaluation whose RMS force is below it (that evaluation's move is not made: tools/minimiser_study.py's convention; the device and
    the oracle check after whole steps and chunks).  round32: the float32 twin — coordinates, forces and the stored pairs are rounded to
    float32 after every step, as the device holds them (the sums and the compact form stay doubles, as on the device).  mutate: one name
    of MUTATIONS (mass: the model's, for "first_no_mass")."""
    assert mutate is None or mutate in MUTATIONS, mutate
    x = np.array(x0, dtype=np.float64).reshape(-1)
    if round32:
        x = _r32(x)
    S, Y = [], []
    gamma = g0 * mass if mutate == "first_no_mass" else g0
    hold = m + 1 if mutate == "memory_plus_one" else m
    F_prev = s_prev = None
    resets, rmss, log, cps, head = 0, [], [], {}, m - 1
    for k in range(nsteps):
        F = np.asarray(force(x.reshape(-1, 3)), dtype=np.float64).reshape(-1)
        if round32:
            F = _r32(F)
        rmss.append(rms(F))
        if gtol > 0 and rmss[-1] < gtol:
            break
        branch, side, margin, graw = "first", None, None, gamma
        if k > 0:
            y = F_prev - F
            if round32:
                y = _r32(y)
            sy, yy, ss = s_prev @ y, y @ y, s_prev @ s_prev
            with np.errstate(all="ignore"):
                margin = float(sy / np.sqrt(ss * yy))
            if sy > 1e-12 * np.sqrt(ss * yy) or mutate == "accept_rejected":
                branch = "kept"
                S.append(s_prev); Y.append(y)
                if len(S) > hold:
                    at = -2 if mutate == "evict_newest" else 0
                    S.pop(at); Y.pop(at)
                head = head + 1 if head + 1 < m else 0
                gamma = (ss / sy) if mutate == "gamma_ss_sy" else sy / yy
            else:
                branch = "rejected"
                if mutate != "reject_keeps_memory":
                    S, Y = [], []
                resets += 1
                if mutate != "no_doubling":
                    gamma *= 2.0
            graw = gamma
            if clamp:
                lo = -np.inf if mutate == "no_lower_clamp" else 1e-7
                hi = np.inf if mutate == "no_upper_clamp" else 1e2
                gamma = min(max(gamma, lo), hi)
                side = "lo" if graw < 1e-7 else ("hi" if graw > 1e2 else None)
        d = compact_direction(F, S[::-1], Y[::-1], gamma) if mutate == "age_reversed" else compact_direction(F, S, Y, gamma)
        fd = F @ d
        with np.errstate(all="ignore"):
            cos = float(fd / np.sqrt((F @ F) * (d @ d)))
        if not (fd > 0):
            S, Y = [], []
            resets += 1
            d = gamma * F
            branch += "+dropped"
        step = d.reshape(-1, 3)
        ln = np.sqrt((step ** 2).sum(axis=1))
        ncap = int((ln > max_step).sum())
        if mutate == "no_cap":
            ncap = 0
        elif mutate == "cap_whole_vector":
            whole = np.sqrt((step ** 2).sum())
            step = step * (max_step / whole if whole > max_step else 1.0)
        else:
            step = step * np.where(ln > max_step, max_step / np.maximum(ln, 1e-300), 1.0)[:, None]
        if round32:
            step = _r32(step)
            xn = _r32(x + step.reshape(-1))
            s_new = step.reshape(-1)
        else:
            xn = x + step.reshape(-1)
            s_new = xn - x
        if mutate == "s_before_cap":
            s_new = d.copy()
        F_prev, s_prev = F, s_new
        x = xn
        log.append(LStep(it=k, branch=branch, clamp=side, pairs=len(S), slot=head, ncap=ncap, margin=margin, cos=cos, graw=float(graw),
                         gamma=float(gamma)))
        if k + 1 in checkpoints:
            cps[k + 1] = x.reshape(-1, 3).copy()
    return x.reshape(-1, 3), {"evals": len(rmss), "resets": resets, "rms": rmss, "log": log, "checkpoints": cps}


def lbfgs_stage(om, d10, x0, stage, fire, n_lbfgs, m=5, seed=82364, replica=0):
    """A whole stage of kind 8: `stage` = (8, nsteps, dt, w_all, w_vdw, repel_s, t_bath); L-BFGS for min(nsteps, n_lbfgs) steps, then the
    oracle's FIRE from a fresh state for the rest.  Returns (x centred, info) — the oracle centres what its schedule returns."""
    _, nsteps, _, w_all, w_vdw, repel_s, _ = stage
    force = lambda u: O.energy_force(om, d10, u, w_all, w_vdw, repel_s)[0]
    nl = min(nsteps, n_lbfgs)
    x, info = lbfgs_run(force, x0, nl, m=m, g0=gamma0(om, fire), max_step=float(fire.max_step))
    if nsteps > nl:
        x, _, ev = O.run_schedule(om, d10, O.make_stages([(2, nsteps - nl, 0.0, w_all, w_vdw, repel_s, 0.0)]), fire, seed, replica, x0=x)
        info["fire_evals"] = ev
    return x - x.mean(0), info


# ---------------------------------------------------------------------------------------------
# the serial section of a move as a table: one row of c3d_debug_lbfgs_direction, in float64
# ---------------------------------------------------------------------------------------------
MAX_PAIRS = 8
NSUMS = 4 * MAX_PAIRS + 4


def direction_row_ref(sums, state_int, state_dbl, first, mem0, g0):
    """One row of c3d_debug_lbfgs_direction, from the header comment of c3d_lbfgs.h and compact_direction above.  sums [36]: per ring slot j
    (F.s_j, F.y_j, s_j.y, y_j.y) at 4 j, then s.s, F.F; state_int = (cnt, head, mem, resets); state_dbl [129] = (gamma, S'Y [8, 8], Y'Y
    [8, 8]) by slot; g0: the first step's gamma.  Returns (state_int, state_dbl, coef [17] = gamma, a by slot, b by slot, mask, slot of
    the move's s, F.d).  Comparisons as the device writes them: a NaN fails every one."""
    M = MAX_PAIRS
    sums = np.asarray(sums, dtype=np.float64)
    cnt, head, mem, resets = (int(a) for a in state_int)
    gamma = float(state_dbl[0])
    SY = np.array(state_dbl[1:1 + M * M], dtype=np.float64).reshape(M, M)
    YY = np.array(state_dbl[1 + M * M:], dtype=np.float64).reshape(M, M)
    with np.errstate(all="ignore"):
        if first:
            cnt, mem, head, resets, gamma = 0, int(mem0), int(mem0) - 1, 0, float(g0)
        else:
            mem = min(max(mem, 1), M)
            head = min(max(head, 0), mem - 1)
            cnt = min(max(cnt, 0), mem)
            nx = (head + 1) % mem
            sy, yy, ss = sums[4 * nx + 2], sums[4 * nx + 3], sums[NSUMS - 4]
            if sy > 1e-12 * np.sqrt(ss * yy):
                head, cnt = nx, min(cnt + 1, mem)
                for i in range(cnt):
                    sl = (nx - i) % mem
                    SY[sl, nx] = sums[4 * sl + 2]
                    YY[sl, nx] = YY[nx, sl] = sums[4 * sl + 3]
                gamma = sy / yy
            else:
                cnt, resets, gamma = 0, resets + 1, 2.0 * gamma
            gamma = float(np.fmin(np.fmax(gamma, 1e-7), 1e2))
        slots = [(head - (cnt - 1) + i) % mem for i in range(cnt)]           # age order, oldest first
        ff = sums[NSUMS - 3]
        fd = gamma * ff
        if cnt:
            ix = np.ix_(slots, slots)
            Rm = np.triu(SY[ix])
            ps, py = -sums[[4 * s for s in slots]], -sums[[4 * s + 1 for s in slots]]         # S'g, Y'g with g = -F
            u = np.linalg.solve(Rm, ps)
            top = np.linalg.solve(Rm.T, (np.diag(np.diag(Rm)) + gamma * YY[ix]) @ u - gamma * py)
            fd = fd + top @ ps - gamma * (u @ py)
        coef, mask = np.zeros(1 + 2 * M), 0
        if fd > 0:
            for i, s in enumerate(slots):
                coef[1 + s], coef[1 + M + s] = -top[i], gamma * u[i]
                mask |= 1 << s
        else:
            cnt, resets = 0, resets + 1
    coef[0] = gamma
    return (cnt, head, mem, resets), np.concatenate([[gamma], SY.reshape(-1), YY.reshape(-1)]), coef, mask, (head + 1) % mem, float(fd)


# ---------------------------------------------------------------------------------------------
# the rows of a move as a table: one row of c3d_debug_lbfgs_move_rows, in float64
# ---------------------------------------------------------------------------------------------
MOVE_ROW_IN, MOVE_ROW_OUT = 6 + 6 * MAX_PAIRS, 10
# name -> what the mutated restatement does differently (tests/test_lbfgs_ref.py: each moves some row of the table by >= 100 of its bounds)
MOVE_MUTATIONS = {
    "ab_swapped": "a_j and b_j swapped",
    "sy_swapped": "s_j and y_j swapped",
    "slot_plus_one": "ring slot j read as j + 1",
    "mask_ignored": "every slot enters the direction whatever the mask",
    "gamma_dropped": "the direction starts from 0 instead of gamma F",
    "cap_no_sqrt": "the cap scales by max_step / d.d",
    "no_cap": "no per-bead cap",
    "s_uncapped": "s is stored before the cap",
    "mm_uncapped": "move.move is formed from the uncapped direction",
    "x_uncapped": "the bead moves by the uncapped direction",
}


def move_row_ref(coef, mask, slot, row, max_step, mut=None):
    """One row of c3d_debug_lbfgs_move_rows (section 3 of k_lbfgs_move / k64_lbfgs_move) in float64 on the values as given: coef [17] =
    (gamma, a_j, b_j by slot), row [54] = x[3], F[3], s_j[3] x 8, y_j[3] x 8.  d = gamma F + sum over the mask's slots of (b_j y_j, then
    a_j s_j), capped at max_step per bead; x' = x + move; ring slot `slot` = the move; move.move.  Returns (out [10] = x'[3], the ring's
    s[3], ring slot (slot + 1) % 8 as it was [3], move.move; scale [3] = gamma |F_c| + sum |a_j s_jc| + sum |b_j y_jc| of the direction;
    capped).  A slot outside the mask is not read.  mut: one name of MOVE_MUTATIONS."""
    assert mut is None or mut in MOVE_MUTATIONS, mut
    M = MAX_PAIRS
    coef, row = np.asarray(coef, dtype=np.float64), np.asarray(row, dtype=np.float64)
    x, F = row[0:3], row[3:6]
    s, y = row[6:6 + 3 * M].reshape(M, 3), row[6 + 3 * M:].reshape(M, 3)
    with np.errstate(all="ignore"):
        d = np.zeros(3) if mut == "gamma_dropped" else coef[0] * F
        scale = np.abs(coef[0] * F)
        for j in range(M):
            if not (mask >> j) & 1 and mut != "mask_ignored":
                continue
            a, b = (coef[1 + M + j], coef[1 + j]) if mut == "ab_swapped" else (coef[1 + j], coef[1 + M + j])
            k = (j + 1) % M if mut == "slot_plus_one" else j
            sj, yj = (y[k], s[k]) if mut == "sy_swapped" else (s[k], y[k])
            d = (d + b * yj) + a * sj
            scale = scale + np.abs(b * yj) + np.abs(a * sj)
        l2 = d[0] * d[0] + (d[1] * d[1] + d[2] * d[2])
        capped = bool(l2 > max_step * max_step) and mut != "no_cap"
        move = d * (max_step / (l2 if mut == "cap_no_sqrt" else np.sqrt(l2))) if capped else d
        xn = x + (d if mut == "x_uncapped" else move)
        st = d if mut == "s_uncapped" else move
        mv = d if mut == "mm_uncapped" else move
        mm = mv[0] * mv[0] + (mv[1] * mv[1] + mv[2] * mv[2])
    return np.concatenate([xn, st, s[(slot + 1) % M], [mm]]), scale, capped


def move_row_bounds(prec, mask, row, out, scale, capped):
    """The absolute bounds [10] of one row, fixed before any run from the count of roundings (T = float for prec 32, double for 64):
      direction, uncapped   (2 pairs + 2) ulps of the scale: one fma a term (2 a pair), gamma F, and the narrowing of a double coefficient
      capped                the terms of one sign, so the scale is |d_c|: the same count in ulps of the move, + 8 for the cap — the cap of
                            the fp32 and of the fp64 row tables (d.d carries twice the direction's error, the reciprocal root halves it)
      x'                    + 1 ulp of x' where x is not 0 (the sum x + move)
      move.move             twice the move's relative bound, + 2 ulps (three roundings of the fma order)
    and 0 for the neighbouring ring slot, which no statement writes."""
    T = np.float32 if prec == 32 else np.float64
    ulp = lambda v: float(np.spacing(T(min(abs(float(v)), float(np.finfo(T).max) / 2)))) if np.isfinite(v) else float("inf")
    pairs = bin(mask).count("1")
    n = 2 * pairs + 2
    with np.errstate(all="ignore"):
        mv = [n * ulp(scale[c]) if not capped else (n + 8) * ulp(out[3 + c]) for c in range(3)]
        xb = [mv[c] + (ulp(out[c]) if row[c] != 0.0 else 0.0) for c in range(3)]
        rel = max((mv[c] / abs(out[3 + c]) if out[3 + c] != 0 else 0.0) for c in range(3)) if capped else \
            max((mv[c] / scale[c] if scale[c] != 0 else 0.0) for c in range(3))
        mm = 2.0 * rel * (float(np.sum(scale * scale)) if not capped else out[9]) + 2 * ulp(out[9])
    return xb + mv + [0.0, 0.0, 0.0] + [mm]


_MU = np.array([0.6, -0.64, 0.48])
_MSG = np.array([1.0, -1.0, 1.0])
_MX0 = np.array([1.5, -2.5, 3.5])
MOVE_CALLS = [(0, 0)] + [(1 << j, j if j % 2 == 0 else (j + 1) % 8) for j in range(8)] + [(0xFF, 3), (0x55, 1), (0xAA, 1)]      # (mask, slot of s)


def move_coef(prec, mask):
    """coef [17] of a call: gamma, a_j, b_j all positive and distinct (a capped row's terms then have one sign when its vectors have), every
    slot's non-zero whether or not the mask holds it; exact in the precision's type"""
    T = np.float32 if prec == 32 else np.float64
    c = np.array([0.013] + [0.8 + 0.11 * j for j in range(MAX_PAIRS)] + [0.021 + 0.004 * j for j in range(MAX_PAIRS)]) * (1.0 + 0.001 * mask)
    return c.astype(T).astype(np.float64)


def move_rows(prec, mask, slot, max_step):
    """[(row54, tag)] of one call (mask, slot) for c3d_debug_lbfgs_move_rows in precision prec, every value exact in its type.  Every slot
    outside the mask holds NaN in s_j and y_j.  tag: "plain" | "capped" | "edge" (the two adjacent values of one component between which
    d.d crosses max_step^2) | "seed" (d.d at the end of the range of the cap's seed: near FLT_MAX in fp32; 2^127, 2^128, 1e40, 1e150, 1e300
    in fp64) | "beyond" (fp32: d finite, d.d beyond FLT_MAX) | "nan" (a NaN in F)."""
    T, I = (np.float32, np.int32) if prec == 32 else (np.float64, np.int64)
    q = lambda a: np.asarray(a, dtype=np.float64).astype(T).astype(np.float64)
    M = MAX_PAIRS
    coef = move_coef(prec, mask)
    ms2 = max_step * max_step
    inmask = [j for j in range(M) if (mask >> j) & 1]
    rng = np.random.default_rng(3300 + mask)
    # one-sign ring vectors, every slot's distinct and not parallel to another's
    S1 = np.array([_MSG * (0.3 + 0.1 * j, 0.5 - 0.05 * j, 0.2 + 0.07 * j) for j in range(M)])
    Y1 = np.array([_MSG * (0.25 + 0.03 * j, 0.15 + 0.11 * j, 0.4 - 0.02 * j) for j in range(M)])
    rows = []

    def row(x, F, S, Y):
        S, Y = np.array(S, dtype=np.float64), np.array(Y, dtype=np.float64)
        for j in range(M):
            if j not in inmask:
                S[j] = Y[j] = np.nan
        return q(np.concatenate([np.asarray(x, dtype=np.float64), np.asarray(F, dtype=np.float64), S.reshape(-1), Y.reshape(-1)]))

    def l2_of(r):
        o, _, _ = move_row_ref(coef, mask, slot, r, np.inf)
        return float(o[3] * o[3] + (o[4] * o[4] + o[5] * o[5]))

    def sized(target, x):
        """a one-sign row whose d.d is about target: F along _MU, the ring's vectors along their own directions"""
        r = row(x, _MU / coef[0] * 0.5, S1 * 0.1, Y1)
        k = np.sqrt(target / l2_of(r))
        return row(x, _MU / coef[0] * 0.5 * k, S1 * 0.1 * k, Y1 * k)

    tiny = float(T(1e-42)) if prec == 32 else 1e-310
    for x in (_MX0, np.zeros(3)):
        # the cap's edge: F's third component over the lattice of T
        r = sized(0.9 * ms2, x)
        lo, hi = int(T(r[5]).view(I)), int(T(4.0 * r[5]).view(I))

        def with_f(bits, r=r):
            r2 = r.copy()
            r2[5] = float(np.array(bits, dtype=I).view(T))
            return r2
        assert l2_of(with_f(lo)) <= ms2 < l2_of(with_f(hi))
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if l2_of(with_f(mid)) > ms2:
                hi = mid
            else:
                lo = mid
        rows += [(with_f(lo), "edge"), (with_f(hi), "edge")]
        rows += [(sized(4.0 * ms2, x), "capped"), (sized(1e16 * ms2, x), "capped"), (sized(0.25 * ms2, x), "plain")]
        rows.append((row(x, np.zeros(3), S1 * 0.0, Y1 * 0.0), "plain"))                                   # d = 0
        rows.append((row(x, _MU * tiny / coef[0], S1 * 0.0, Y1 * 0.0), "plain"))                          # a denormal move
        rows.append((row(x, (1.5, -0.0, 2.5), S1 * 0.01, Y1 * 0.01), "plain"))
        rows.append((row(x, (1.5, np.nan, 2.5), S1 * 0.01, Y1 * 0.01), "nan"))
        if prec == 32:
            fmax = float(np.finfo(np.float32).max)
            rows.append((sized(fmax * (1.0 - 2.0 ** -16), x), "seed"))          # (further below FLT_MAX than the 2 pairs + 5 roundings of d.d carry it)
            rows += [(sized(t, x), "beyond") for t in (2.0 ** 130, 1e40, 1e60)]
        else:
            rows += [(sized(t, x), "seed") for t in (2.0 ** 127, 2.0 ** 128, 1e40, 1e150, 1e300)]
    # vectors of any sign (the terms of a component cancel in part: the bound is in ulps of the scale), small and uncapped
    for k in range(5):
        x = _MX0 * rng.uniform(0.5, 2.0, 3) if k % 3 else np.zeros(3)
        rows.append((row(x, rng.uniform(-1, 1, 3) * 2.0, rng.uniform(-1, 1, (M, 3)) * 0.05, rng.uniform(-1, 1, (M, 3)) * 0.5), "plain"))
    out = []
    for r, tag in rows:
        capped = move_row_ref(coef, mask, slot, r, max_step)[2]
        assert capped == (tag in ("capped", "seed", "beyond")) or tag in ("edge", "nan"), (tag, capped)
        out.append((r, tag))
    return out


def move_row_check(prec, coef, mask, slot, row, tag, got, max_step):
    """The table's assertion on one row: got [10] of c3d_debug_lbfgs_move_rows against move_row_ref under move_row_bounds.  Returns the
    largest |difference| / bound of the row; raises AssertionError with the figures.  Whatever the tag: the neighbouring ring slot comes
    back bit for bit; no NaN in an output unless F holds one (then exactly where the restatement has one); at x = 0 the ring's s is x'
    bit for bit; move.move is the fma order of the STORED s within 2 ulps."""
    T = np.float32 if prec == 32 else np.float64
    got = np.asarray(got, dtype=np.float64)
    want, scale, capped = move_row_ref(coef, mask, slot, row, max_step)
    where = (prec, mask, slot, tag)
    assert np.array_equal(got[6:9], want[6:9], equal_nan=True), where + ("the neighbouring slot changed", got[6:9], want[6:9])
    bound = move_row_bounds(prec, mask, row, want, scale, capped)
    worst = 0.0
    for k in (0, 1, 2, 3, 4, 5, 9):
        if want[k] != want[k]:
            assert tag == "nan" and got[k] != got[k], where + (k, got[k], want[k])
            continue
        assert got[k] == got[k], where + ("a NaN reached an output", k, got)
        diff = abs(got[k] - want[k])
        assert diff <= bound[k], where + (k, got[k], want[k], diff, bound[k], list(row[:6]))
        worst = max(worst, diff / bound[k] if bound[k] > 0 else 0.0)
    if not row[0:3].any():
        assert np.array_equal(got[3:6], got[0:3], equal_nan=True), where + ("s is not x' - x at x = 0", got[:6])
    if got[9] == got[9]:
        s = got[3:6]
        mm = s[0] * s[0] + (s[1] * s[1] + s[2] * s[2])
        assert abs(got[9] - mm) <= 2.0 * float(np.spacing(T(min(mm, float(np.finfo(T).max) / 2)))), where + ("move.move is not the stored s's", got[9], mm)
    return worst
