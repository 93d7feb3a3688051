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
