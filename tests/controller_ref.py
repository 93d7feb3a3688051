"""A Python twin of the oracle's schedule runner (c3o_run_schedule with c3o_md_step, c3o_fire_step, c3o_bb_step: oracle/c3d_oracle.c) that
says, step by step, which branch of the step controller it took — and a table of named cases built so that every branch is taken, with a
margin, on a trajectory float32 can follow.  The forces are the oracle's own (O.energy_force), the Maxwell start its own
(O.init_velocities); the statements around them are restated here one for one, so that each can be MUTATED: a case is only worth running
on the GPU if a subtly wrong controller would end far from it (MUTATIONS, tests/test_controller_ref.py).

The last two sections restate the controller as TABLES (one row of sums and state in, the step's scalars out; one bead in, its update
out): step_scalars_ref for the fp32 and fp64 controllers, row_finish_ref for the fp64 row update, with the rows the GPU tests run.

branch names   fire: reset | hold | grow | cap        (power test failed | npos <= n_min | dt grows | dt held at dt_max)
               md:   plain | floor | clamp0           (T floored at 1e-2 | Berendsen lambda^2 clamped at 0; both: floor+clamp0)
               bb:   first | bb | negcurv, + "+lo" / "+hi" where the length was bounded by 1e-7 / 1e2
"""
import functools

import numpy as np

from oracle import oracle as O
from tests.util import oracle_fire_from, oracle_model_from, synthetic_if

KBOLTZ, ACCEL = 0.0019872, 418.4
SEED = 82364

# name -> what the mutated twin does differently (the list the GPU test's sensitivity rests on)
MUTATIONS = {
    "nmin_ge": "the n_min gate reads npos >= n_min",
    "no_dt_max": "dt grows without the dt_max cap",
    "reset_keeps_dt": "an uphill reset leaves dt as it was",
    "reset_keeps_alpha": "an uphill reset leaves alpha as it was",
    "reset_keeps_v": "an uphill reset leaves the velocities as they were",
    "alpha_not_decayed": "alpha is not multiplied by f_alpha",
    "no_max_step_fire": "FIRE moves without the per-bead max_step cap",
    "floor_1e3": "the temperature floor is 1e-3",
    "sqrt_abs_clamp": "lambda = sqrt(|lambda^2|) instead of the clamp at 0",
    "bb_parity_swapped": "the two two-point lengths on each other's parity",
    "bb_first_no_mass": "the first two-point length without / mass",
    "fbeta_10": "fbeta is a literal 10",
    "mass_100": "the mass is a literal 100",
    "s_noe_10": "s_noe is a literal 10",
}


def _copy_model(m, **kw):
    c = O.Model.from_buffer_copy(m)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


class Step:
    """stage, step of the stage, kind that ran (0 / 1 / 2 / 5), branch, beads the max_step cap acted on, margin of the step's discontinuous
    decision (None: it has none), steps since the controller's state was fresh (stage start or hand-over), RMS force of the evaluation"""
    __slots__ = ("stage", "it", "kind", "branch", "ncap", "margin", "since", "rms")

    def __init__(self, stage, it, kind, branch, ncap=0, margin=None, since=0, rms=None):
        self.stage, self.it, self.kind, self.branch, self.ncap, self.margin, self.since, self.rms = stage, it, kind, branch, ncap, margin, since, rms


def _capped(dr, max_step):
    d2 = (dr * dr).sum(1)
    over = d2 > max_step * max_step
    sc = np.where(over, max_step / np.sqrt(np.where(over, d2, 1.0)), 1.0)
    return sc[:, None] * dr, int(over.sum())


def run_twin(om, d10, stages, fire, replica, x0, tp=1000, checkpoints=(), round32=False, mut=None, seed=SEED):
    """c3o_run_schedule restated.  om / fire: oracle Model / FireParams; stages: rows (kind, nsteps, dt, w_all, w_vdw, repel_s, t_bath);
    tp: final_minimiser_steps.  Returns (x centred, v, log [Step per step], {k: (x centred, v) after k steps for k in checkpoints}).
    round32: coordinates and velocities rounded to float32 after every step (the conditioning probe).  mut: one name of MUTATIONS."""
    n = om.n
    mass = 100.0 if mut == "mass_100" else om.mass
    fbeta = 10.0 if mut == "fbeta_10" else om.fbeta
    fm = _copy_model(om, s_noe=10.0) if mut == "s_noe_10" else om
    x = np.array(x0, dtype=np.float64)
    v = np.zeros_like(x)
    log, cps, done, prev_kind = [], {}, 0, -1
    tp = max(int(tp), 2)

    def after_step():
        nonlocal x, v, done
        if round32:
            x, v = x.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)
        done += 1
        if done in checkpoints:
            cps[done] = (x - x.mean(0), v.copy())

    for s, (kind, nsteps, dt, w_all, w_vdw, repel_s, t_bath) in enumerate(stages):
        force = lambda: O.energy_force(fm, d10, x, w_all, w_vdw, repel_s)[0]
        if kind in (2, 5):
            fdt, alpha, npos = fire.dt_start, fire.alpha_start, 0
            L = [0.0, 0.0, 0.0, 0.0]
            nbb = min(nsteps, tp) if kind == 5 else 0
            v[:] = 0.0
            for it in range(nsteps):
                if it == nbb and nbb > 0:
                    fdt, alpha, npos, L = fire.dt_start, fire.alpha_start, 0, [0.0, 0.0, 0.0, 0.0]
                    v[:] = 0.0
                F = force()
                if it >= nbb:                                   # c3o_fire_step
                    vf, ff, vv = float((v * F).sum()), float((F * F).sum()), float((v * v).sum())
                    margin = L[0] / np.sqrt(L[1] * L[2]) if L[1] * L[2] > 0 else 0.0
                    if L[0] > 0:
                        mix = alpha * np.sqrt(L[2] / (L[1] if L[1] > 1e-30 else 1e-30))
                        v = (1.0 - alpha) * v + mix * F
                        branch = "hold"
                        if (npos >= fire.n_min) if mut == "nmin_ge" else (npos > fire.n_min):
                            grown = fdt * fire.f_inc
                            branch = "grow" if grown < fire.dt_max else "cap"
                            fdt = grown if (grown < fire.dt_max or mut == "no_dt_max") else fire.dt_max
                            if mut != "alpha_not_decayed":
                                alpha *= fire.f_alpha
                        npos += 1
                    else:
                        branch = "reset"
                        if mut != "reset_keeps_v":
                            v[:] = 0.0
                        if mut != "reset_keeps_alpha":
                            alpha = fire.alpha_start
                        if mut != "reset_keeps_dt":
                            fdt *= fire.f_dec
                        npos = 0
                    v = v + (fdt * ACCEL / mass) * F
                    dr = fdt * v
                    if mut == "no_max_step_fire":
                        ncap = 0
                    else:
                        dr, ncap = _capped(dr, fire.max_step)
                    x = x + dr
                    L = [vf, ff, vv, 0.0]
                    log.append(Step(s, it, 2, branch, ncap, margin, it - nbb, np.sqrt(ff / (3.0 * n))))
                else:                                           # c3o_bb_step
                    k, a_prev = npos, fdt
                    a, branch, margin = a_prev, "first", None
                    if k == 0:
                        a = fire.dt_start * fire.dt_start * ACCEL / (1.0 if mut == "bb_first_no_mass" else mass)
                    elif k >= 2:
                        sy = L[0]
                        margin = sy / np.sqrt(L[3] * L[2]) if L[3] * L[2] > 0 else 0.0
                        if sy > 0:
                            even = (k % 2 == 0) != (mut == "bb_parity_swapped")
                            a, branch = (L[3] / sy if even else sy / L[2]), "bb"
                        else:
                            a, branch = 2.0 * a_prev, "negcurv"
                        if not (a >= 1e-7):
                            a, branch = 1e-7, branch + "+lo"
                        if a > 1e2:
                            a, branch = 1e2, branch + "+hi"
                    q = [0.0, float((F * F).sum()), 0.0, 0.0]
                    if k > 0:
                        sv, _ = _capped(a_prev * v, fire.max_step)
                        y = v - F
                        q[0], q[2], q[3] = float((sv * y).sum()), float((y * y).sum()), float((sv * sv).sum())
                    dr, ncap = _capped(a * F, fire.max_step)
                    x = x + dr
                    v = F.copy()
                    fdt, npos, L = a, k + 1, q
                    log.append(Step(s, it, 5, branch, ncap, margin, it, np.sqrt(q[1] / (3.0 * n))))
                after_step()
        else:                                                   # c3o_md_step
            if prev_kind in (2, 5, -1):
                v = O.init_velocities(_copy_model(om, mass=mass), seed, replica, 0.5)
            ndf = max(3 * n - 3, 1)
            for it in range(nsteps):
                F = force()
                tprev = mass * float((v * v).sum()) / ACCEL / (ndf * KBOLTZ)
                floor = 1e-3 if mut == "floor_1e3" else 1e-2
                branch = "plain"
                if tprev < floor:
                    tprev, branch = floor, "floor"
                if kind == 0:
                    l2 = 1.0 + dt * fbeta * (t_bath / tprev - 1.0)
                    if l2 < 0:
                        l2 = abs(l2) if mut == "sqrt_abs_clamp" else 0.0
                        branch = "clamp0" if branch == "plain" else "floor+clamp0"
                    lam = np.sqrt(l2)
                else:
                    lam = np.sqrt(t_bath / tprev)
                v = lam * (v - v.mean(0)) + (dt * ACCEL / mass) * F
                x = x + dt * v
                log.append(Step(s, it, kind, branch, since=it))
                after_step()
        prev_kind = kind
    return x - x.mean(0), v, log, cps


# ---------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------
# the off-default scalars (every one of them enters a number the host derives: acc, t_fac, w_noe2n, w_rep4, rep_r2, kq, k_bond2, ...)
OFF = dict(mass=37.0, s_noe=6.0, k_bond=220.0, b0=3.6, k_ang=30.0, a0=5.1, k_rep=2.5, r0_rep=4.4, fbeta=400.0)
FIRE_A = dict(f_inc=1.3, dt_max=0.02, n_min=2, f_dec=0.4, alpha_start=0.2, f_alpha=0.95, max_step=2.0, dt_start=0.008)
FIRE_B = dict(f_inc=1.6, dt_max=0.025, n_min=0, f_dec=0.25, alpha_start=0.3, f_alpha=0.85, max_step=0.05, dt_start=0.012)
COLD = [(1, 2, 0.005, 1e-4, 1e-4, 0.85, 0.0), (0, 3, 0.003, 1e-4, 1e-4, 0.85, 3.0), (0, 4, 0.003, 1.0, 1.0, 0.85, 300.0),
        (0, 6, 0.003, 0.4, 0.003, 0.9, 0.02), (1, 4, 0.005, 1.0, 0.05, 1.0, 1500.0)]


class Case:
    """model / fire: fields off the library's defaults; start: "relaxed" (the oracle's result after 200 default FIRE steps from the coil
    under the case's model, rounded to float) or "coil"; ids: {beads: the two coils the starts are made from} (default 0 and 1 — a start
    is data, passed in through set_coords: which coil it came from is chosen per size for conditioning); first: the first replica number on
    the device (it keys the Maxwell velocities of an MD stage); checkpoints: step counts at which run_steps is split and everything is
    compared; vrel: checkpoints whose velocities are compared relative to the oracle's own max |v|; pot / gen: device potential and
    general tail, for the kernel names (a general tail has no multi-step form); two_point: kind-5 steps are in the range (5e-3 A)."""

    def __init__(self, model, fire, stages, checkpoints, start="relaxed", tp=1000, vrel=(), pot=4, gen=False, two_point=False, ids=None,
                 first=0):
        # (a stage's dt, weights and bath temperature as the C ABI holds them: floats)
        stages = [tuple(s[:2]) + tuple(float(np.float32(a)) for a in s[2:]) for s in stages]
        self.model, self.fire, self.stages, self.checkpoints, self.start, self.tp = model, fire, stages, tuple(checkpoints), start, tp
        self.vrel, self.pot, self.gen, self.two_point, self.ids, self.first = tuple(vrel), pot, gen, two_point, ids or {}, first
        self.nsteps = sum(s[1] for s in stages)
        assert self.checkpoints[-1] == self.nsteps

    def tol(self, precision=32):
        """the suite's coordinate tolerance for the case (Angstrom)"""
        return 2e-5 if precision == 64 else (5e-3 if self.two_point else 2e-3)

    def key(self):
        return tuple(sorted(self.model.items()))


_MIN = (0.0, 1.0, 1.0, 0.85, 0.0)          # a minimiser stage at the final stage's weights
_HOT = (0, 8, 0.003, 0.4, 0.003, 0.9, 2000.0)
_BIG = {1100: (4, 5)}                      # the coils whose relaxed starts are quiet at 1100 beads (coils 0 and 1 are not: SIZES below)
CASES = {
    # 7 mid-run resets, the dt_max cap, n_min 2, every bead below max_step; split directly after a mid-run reset (17: slot 0 at 250 beads);
    # then an MD stage without repel weight (w_vdw = 0: kq = 0)
    "fire_resets": Case({}, FIRE_A, [(2, 48) + _MIN, (0, 8, 0.003, 0.4, 0.0, 0.9, 2000.0)], [17, 48, 56], ids=_BIG),
    # n_min 0, a max_step that cuts some beads on some steps and none on others, every scalar off default
    "fire_partial_cap": Case(OFF, FIRE_B, [(2, 40) + _MIN], [40], ids={250: (0, 5)}),
    # the same over its first 14 steps, for 1100 beads (see SIZES)
    "fire_partial_cap_short": Case(OFF, FIRE_B, [(2, 14) + _MIN], [14], ids=_BIG),
    # floor (kinds 1 and 0), lambda^2 < 0, plain before and after; w_all = 1e-4 (kq large); a checkpoint right after the floor steps
    "md_cold": Case(OFF, {}, COLD, [4, 9, 19], vrel=(4,), ids=_BIG),
    # two-point steps, the hand-over to FIRE inside the window (step 13), split inside the two-point part (7) and in the FIRE part (17: the
    # range 8 .. 17 is five two-point ops and five FIRE ops, each segment long enough for a multi-step launch)
    "two_point": Case(OFF, dict(dt_start=0.006, max_step=2.0, n_min=3), [(5, 30) + _MIN], [7, 17, 30], tp=12, two_point=True, ids=_BIG),
    # every scalar off default on the shipped fast form, FIRE_A, then hot MD from the Maxwell velocities of replicas 5 and 6 (the mass)
    "off_default": Case(OFF, FIRE_A, [(2, 40) + _MIN, _HOT], [40, 48], ids=_BIG, first=5),
    "pot3_rs1_off": Case(dict(OFF, noe_pot=3, rswitch=1.0, mrswitch=11.0, masym=22.0, msoexp=1), FIRE_A, [(2, 30) + _MIN, _HOT], [30, 38],
                         pot=3, ids={250: (5, 7), 1100: (4, 5)}),
    "gen1_off": Case(dict(OFF, noe_pot=1, asym=1.0, rswitch=0.5), FIRE_A, [(2, 30) + _MIN, _HOT], [30, 38], pot=1, gen=True, ids=_BIG),
    # default FIRE values from the coil, then hot MD with full repel weight
    "rep_sep1": Case(dict(rep_sep=1), {}, [(2, 12) + _MIN, (0, 10, 0.003, 0.4, 1.0, 0.9, 2000.0)], [22], start="coil"),
    "rep_sep3": Case(dict(rep_sep=3), {}, [(2, 12) + _MIN, (0, 10, 0.003, 0.4, 1.0, 0.9, 2000.0)], [22], start="coil"),
}
# The sizes a case runs at.  At 1100 beads 200 relaxation steps leave more of the chain unsettled: under FIRE_B (max_step 0.05, dt up to
# 0.025) every start tried (coils 0 .. 5) either caps every bead for 30 steps or, within 40 steps, magnifies float32 rounding beyond a
# quarter of the tolerance in the velocities after a reset (0.25 .. 35 tolerances).  Its first 14 steps from coils 4 and 5 are quiet
# (0.04 / 0.07) and still cut some beads on 8 steps and hold dt at dt_max on 4: that window is the case at 1100 beads.
SIZES = {name: (250, 1100) for name in CASES}
SIZES["fire_partial_cap"] = (250,)
SIZES["fire_partial_cap_short"] = (1100,)


@functools.lru_cache(maxsize=None)
def problem(n):
    """(IF, dist10) of the synthetic matrix of n beads the GPU suite uses at that size"""
    IF = synthetic_if(n, seed=n)[0]
    return IF, O.if_to_dist10(IF)


def models(case, n):
    """(c3d_model, c3d_fire_params, oracle Model, oracle FireParams) of a case: the oracle's hold the float32 values of the library's"""
    from chromosome3d_amd import default_fire, default_model
    m, f = default_model(**case.model), default_fire(**case.fire)
    return m, f, oracle_model_from(m, n), oracle_fire_from(f)


@functools.lru_cache(maxsize=None)
def _start(model_key, kind, n, coil):
    from chromosome3d_amd import default_model
    om = oracle_model_from(default_model(**dict(model_key)), n)
    x = O.init_coords(om, SEED, coil)
    if kind != "coil":                     # "relaxed": 200 default FIRE steps; "fire30": 30 (forces still large)
        x = O.run_schedule(om, problem(n)[1], O.make_stages([(2, 200 if kind == "relaxed" else 30) + _MIN]), O.default_fire(), SEED, coil, x0=x)[0]
    return x.astype(np.float32)


def start_of(case, n, slot):
    return _start(case.key(), case.start, n, case.ids.get(n, (0, 1))[slot])


def start(name, n, slot):
    """float32 start coordinates of slot 0 / 1 of a case at n beads (cases of one model share their starts)"""
    return start_of(CASES[name], n, slot)


@functools.lru_cache(maxsize=None)
def reference(name, n, slot, round32=False, mut=None):
    """run_twin of a case's slot: (x, v, log, checkpoints)"""
    case = CASES[name]
    _, _, om, of = models(case, n)
    return run_twin(om, problem(n)[1], case.stages, of, case.first + slot, start(name, n, slot).astype(np.float64), tp=case.tp,
                    checkpoints=case.checkpoints, round32=round32, mut=mut)


def gap(a, b, case, precision=32):
    """how far two runs of a case are apart at their checkpoints, in units of the GPU tolerance there: coordinates against case.tol(),
    velocities against tol_v * max(1, max|v|) — at a checkpoint of case.vrel against tol_v * max|v| itself"""
    worst = 0.0
    tol_x = case.tol(precision)
    tol_v = 2e-5 if precision == 64 else 2e-3
    for k in case.checkpoints:
        (xa, va), (xb, vb) = a[3][k], b[3][k]
        vmax = np.abs(va).max()
        worst = max(worst, np.abs(xa - xb).max() / tol_x, np.abs(va - vb).max() / (tol_v * (vmax if k in case.vrel else max(1.0, vmax))))
    return float(worst)


# ---------------------------------------------------------------------------------------------
# the gradient exit and the L-BFGS case
# ---------------------------------------------------------------------------------------------
GTOL_CHECK_EVERY = 7
GTOL_STAGE = (2, 84) + _MIN


def gtol_stage():
    return tuple(GTOL_STAGE[:2]) + tuple(float(np.float32(a)) for a in GTOL_STAGE[2:])


@functools.lru_cache(maxsize=None)
def gradient_exit(name, n):
    """(gtol, steps): a final FIRE stage GTOL_STAGE of case `name`'s model, FIRE values and starts, its exit test looked at every
    GTOL_CHECK_EVERY steps.  gtol = the geometric mean of the largest-over-replicas RMS forces at the first two consecutive checks that
    differ by at least 10 % (the second lower, every earlier check above gtol); steps = where c3o_run_schedule then stops: the second."""
    case = CASES[name]
    _, _, om, of = models(case, n)
    logs = [run_twin(om, problem(n)[1], [gtol_stage()], of, slot, start(name, n, slot).astype(np.float64))[2] for slot in (0, 1)]
    checks = range(GTOL_CHECK_EVERY, GTOL_STAGE[1] + 1, GTOL_CHECK_EVERY)
    worst = [max(log[k - 1].rms for log in logs) for k in checks]
    for j in range(len(worst) - 1):
        gtol = float(np.sqrt(worst[j] * worst[j + 1]))
        if worst[j + 1] <= 0.9 * worst[j] and min(worst[:j + 1]) > gtol:
            return gtol, checks[j + 1]
    raise AssertionError(f"no two consecutive checks 10 % apart: {worst}")


# dt_start, max_step, mass and lbfgs_memory off default; 20 L-BFGS steps from 30 FIRE steps off the coil (tests/test_gpu_lbfgs.py's kind of start)
LBFGS_CASE = Case(dict(mass=37.0), dict(dt_start=0.004, max_step=0.2), [(8, 20) + _MIN], [20], start="fire30")
LBFGS_MEMORY = 3


# ---------------------------------------------------------------------------------------------
# the controller as a table: the statements of run_twin's three step kinds on one row of sums and state, in float64
# ---------------------------------------------------------------------------------------------
F32 = np.float32


def step_scalars_ref(kind, dt, t_bath, psum, state, npos, consts, fire, precision=32, mut=None, hits=None):
    """One row of c3d_debug_step_scalars (precision 32) or c3d_debug_step_scalars_f64 (64).  psum (4), state (dt, alpha), npos: the row;
    consts = (t_fac, inv_n, acc, fbeta) as the host holds them (precision 32: floats, widened, table_consts; 64: doubles formed as
    model64 / step64 form them, table_consts64); fire = c3d_fire_params (floats, widened).  The oracle's constants 1e-2, 1e-30, 1e-7, 1e2
    are the floats the fp32 device holds, or the doubles themselves.  Returns ((lambda, cmx, cmy, cmz, keep, mix), (dt, alpha), npos) in
    float64 — the statements of c3o_md_step, c3o_fire_step and c3o_bb_step that decide a step, one correctly rounded operation per oracle
    operation, with their comparisons as the oracle writes them (a NaN fails every one).  mut: one name of TABLE_MUTATIONS; hits: a
    Counter that receives the name of every branch the row takes."""
    t_fac, inv_n, acc, fbeta = (float(a) for a in consts[:4])
    c = (lambda v: float(F32(v))) if precision == 32 else float
    p = [float(a) for a in psum]
    sdt, alpha = float(state[0]), float(state[1])
    lam, cm, keep, mix = 1.0, [0.0, 0.0, 0.0], 0.0, 0.0

    def hit(name):
        if hits is not None:
            hits[name] += 1

    with np.errstate(all="ignore"):
        if kind in (0, 1):
            tprev = t_fac * p[0]
            hit("T_at_floor" if tprev == c(1e-2) else ("T_below_floor" if tprev < c(1e-2) else "T_above_floor"))
            if tprev < c(1e-2):
                tprev = c(1e-2)
            if kind == 0:
                dtfb = float(F32(dt) * F32(fbeta)) if precision == 32 else dt * fbeta
                l2 = 1.0 + dtfb * (float(np.float64(t_bath) / tprev) - 1.0)
                hit("l2_at_0" if l2 == 0 else ("l2_below_0" if l2 < 0 else "l2_above_0"))
                if mut == "sqrt_abs_clamp":
                    l2 = abs(l2)
                lam = float(np.sqrt(np.float64(l2 if l2 >= 0 else 0.0)))
            else:
                lam = float(np.sqrt(np.float64(t_bath) / tprev))
            cm = [p[1] * inv_n, p[2] * inv_n, p[3] * inv_n]
        elif kind in (5, 6):
            k = 0 if kind == 6 else npos
            a_prev = sdt
            a = a_prev
            if k == 0:
                a = float(fire.dt_start) ** 2 * acc
                hit("bb_first")
            elif k >= 2:
                sy = p[0]
                hit("bb_sy_nan" if sy != sy else ("bb_sy_zero" if sy == 0 else ("bb_sy_pos" if sy > 0 else "bb_sy_neg")))
                if sy > 0:
                    even = (k % 2 == 0) != (mut == "bb_parity_swapped")
                    hit("bb_even" if k % 2 == 0 else "bb_odd")
                    a = float(np.float64(p[3]) / sy) if even else float(np.float64(sy) / np.float64(p[2]))
                else:
                    a = 2.0 * a_prev
                    hit("bb_negcurv")
                if (a < c(1e-7)) if mut == "lo_lt" else (not (a >= c(1e-7))):
                    hit("bb_lo_nan" if a != a else "bb_lo")
                    a = c(1e-7)
                if a > 1e2:
                    a = 1e2
                    hit("bb_hi")
            else:
                hit("bb_second")
            lam, mix, sdt, npos = a_prev, a, a, k + 1
        else:
            hit("fire_vf_nan" if p[0] != p[0] else ("fire_vf_zero" if p[0] == 0 else ("fire_vf_pos" if p[0] > 0 else "fire_vf_neg")))
            if p[0] > 0:
                keep = 1.0 - alpha
                hit("fire_ff_floor" if not (p[1] > c(1e-30)) else "fire_ff")
                if p[1] == c(1e-30):
                    hit("fire_ff_at_floor")
                mix = alpha * float(np.sqrt(np.float64(p[2]) / (p[1] if p[1] > c(1e-30) else c(1e-30))))
                hit("npos_at_nmin" if npos == fire.n_min else ("npos_below_nmin" if npos < fire.n_min else "npos_above_nmin"))
                if (npos >= fire.n_min) if mut == "nmin_ge" else (npos > fire.n_min):
                    grown = sdt * float(fire.f_inc)
                    hit("dt_at_max" if grown == float(fire.dt_max) else ("dt_grow" if grown < float(fire.dt_max) else "dt_cap"))
                    sdt = grown if (grown < float(fire.dt_max) or mut == "no_dt_max") else float(fire.dt_max)
                    alpha *= float(fire.f_alpha)
                npos += 1
            else:
                hit("fire_reset")
                if mut != "reset_keeps_alpha":
                    alpha = float(fire.alpha_start)
                if mut != "reset_keeps_dt":
                    sdt = sdt * float(fire.f_dec)
                npos = 0
    return (lam, cm[0], cm[1], cm[2], keep, mix), (sdt, alpha), npos


# The table's model and FIRE values: products that float holds exactly, so that "at" is at (dt fbeta = 1/2, 1, 3/2; dt f_inc = dt_max)
TABLE_MODEL = dict(mass=37.0, fbeta=256.0)
TABLE_FIRE = dict(dt_start=0.006, dt_max=0.046875, f_inc=1.5, f_dec=0.25, alpha_start=0.3, f_alpha=0.875, n_min=3)
TABLE_N = 37


def table_consts(m, n):
    """(t_fac, inv_n, acc, fbeta) in the host's float arithmetic (dev_model)"""
    ndf = max(3 * n - 3, 1)
    mass = F32(m.mass)
    return (mass / F32(418.4) / (F32(ndf) * F32(0.0019872)), F32(1.0) / F32(n), F32(418.4) / mass, F32(m.fbeta))


def table_rows(kind, t_fac):
    """[(dt, t_bath, psum, state, npos)] of a kind: the grid of the issue"""
    nan, rows = float("nan"), []
    if kind in (0, 1):
        x_floor = float(F32(1e-2)) / float(t_fac)                      # sum v^2 at which T is the floor
        xs = [0.0, 0.5 * x_floor, float(np.nextafter(F32(x_floor), F32(0))), float(F32(x_floor)), float(np.nextafter(F32(x_floor), F32(1e9))),
              2.0 * x_floor, 300.0 / float(t_fac), 3.0e4 * x_floor]
        for dt in (2.0 ** -9, 2.0 ** -8, 3 * 2.0 ** -9):                # dt fbeta = 1/2, 1, 3/2: lambda^2 at t_bath 0 = 1/2, 0, -1/2
            for t_bath in ((0.0, 300.0, 2000.0) if kind == 0 else (0.0, 0.02, 300.0)):
                for x in xs:
                    if kind == 0 and 0.0 < t_bath < float(t_fac) * x * 1.001:      # cooling towards lambda^2 = 0 cancels: not a 4-ulp row
                        continue
                    rows.append((dt, t_bath, (x, 0.37 * (1 + len(rows) % 5), -1.25, 0.0), (0.01, 0.1), 4))
    elif kind in (2, 3):
        for vf in (3.0, 1e-30, 0.0, -0.0, -2.5, nan):
            for npos in (2, 3, 4):                                       # n_min - 1, n_min, n_min + 1
                for sdt in (0.03, 0.03125, 0.04):                        # dt f_inc below, at, above dt_max
                    for ff, vv in ((7.0, 0.3), (0.0, 0.3), (1e-35, 1e-20), (7.0, 0.0)):
                        rows.append((0.0, 0.0, (vf, ff, vv, 0.0), (sdt, 0.3 * 0.875 ** (npos % 3)), npos))
        rows.append((0.0, 0.0, (3.0, nan, 0.3, 0.0), (0.03, 0.3), 4))
        rows.append((0.0, 0.0, (3.0, 7.0, nan, 0.0), (0.03, 0.3), 4))
    else:
        for npos in (0, 1, 2, 3, 7, 8):
            for a_prev in (1e-5, 3e-8, 80.0):                            # the doubling leaves [1e-7, 1e2] on both sides
                for sy, yy, ss in ((2.0, 5.0, 3.0), (2.0, 5e9, 3e-9), (2.0, 1e-3, 9e2), (0.0, 5.0, 3.0), (-0.0, 5.0, 3.0), (-1.5, 5.0, 3.0),
                                   (nan, 5.0, 3.0), (2.0, nan, nan), (2.0, 0.0, 3.0), (1e-30, 5.0, 3.0)):
                    rows.append((0.0, 0.0, (sy, 11.0, yy, ss), (a_prev, 0.2), npos))
    return rows


# ---------------------------------------------------------------------------------------------
# the fp64 controller and the fp64 row update as tables (c3d_debug_step_scalars_f64, c3d_debug_row_finish_f64)
# ---------------------------------------------------------------------------------------------
# name -> what the mutated restatement does differently (tests/test_controller_ref.py: each moves some row by >= 1000 double ulps or an integer)
TABLE_MUTATIONS = {
    "nmin_ge": "the n_min gate reads npos >= n_min",
    "no_dt_max": "dt grows without the dt_max cap",
    "reset_keeps_dt": "an uphill reset leaves dt as it was",
    "reset_keeps_alpha": "an uphill reset leaves alpha as it was",
    "bb_parity_swapped": "the two two-point lengths on each other's parity",
    "lo_lt": "the lower bound reads a < 1e-7 (a NaN length passes)",
    "cap_ge": "the per-bead cap reads d2 >= max_step^2",
    "cap_no_sqrt": "the cap scales by max_step / d2",
    "sqrt_abs_clamp": "lambda = sqrt(|lambda^2|) instead of the clamp at 0",
    "no_cm": "the centre-of-mass velocity is not subtracted",
}
SCALAR_KINDS, ROW_KINDS = (0, 1, 2, 3, 5, 6), (0, 1, 2, 3, 4, 5, 6)
NAN = float("nan")


def table_consts64(m, n):
    """(t_fac, inv_n, kacc, fbeta, mass) as model64 / step64 form them: doubles from the model's floats"""
    ndf = 3 * n - 3
    mass = float(m.mass)
    return (mass / 418.4 / ((ndf if ndf > 0 else 1) * 0.0019872), 1.0 / n, 418.4 / mass, float(m.fbeta), mass)


def ulps(got, want):
    """|got - want| in units of the spacing of doubles at want (inf where one of them is not finite and they differ)"""
    if got == want:
        return 0.0
    if not (np.isfinite(got) and np.isfinite(want)):
        return float("inf")
    return abs(got - want) / float(np.spacing(np.float64(abs(want))))


def _next(x, up=True):
    return float(np.nextafter(np.float64(x), np.float64(np.inf if up else -np.inf)))


def _floor_edge(t_fac):
    """sum v^2 one double below, at, and one double above the place where t_fac * x is the double 1e-2"""
    x = 1e-2 / t_fac
    while t_fac * x > 1e-2:
        x = _next(x, False)
    while t_fac * x < 1e-2:
        x = _next(x)
    assert t_fac * x == 1e-2
    lo = x
    while t_fac * lo == 1e-2:
        lo = _next(lo, False)
    hi = x
    while t_fac * hi == 1e-2:
        hi = _next(hi)
    return lo, x, hi


def table_rows64(kind, t_fac):
    """[(dt, t_bath, psum, state, npos)] of a kind for the fp64 controller: table_rows' grid with every "one float either side" one double
    either side, and the rows on which a reciprocal or square root seeded in float can go wrong (sums and ratios outside float's range)."""
    rows = []
    if kind in (0, 1):
        lo, at, hi = _floor_edge(t_fac)
        xs = [0.0, 0.5 * at, lo, at, hi, 2.0 * at, 300.0 / t_fac, 3.0e4 * at, 1e30 / t_fac, 1e37 / t_fac]
        for dt in (2.0 ** -9, 2.0 ** -8, 3 * 2.0 ** -9):                # dt fbeta = 1/2, 1, 3/2: lambda^2 at t_bath 0 = 1/2, 0, -1/2
            for t_bath in ((0.0, 300.0, 2000.0) if kind == 0 else (0.0, 0.02, 300.0)):
                for x in xs:
                    if kind == 0 and 0.0 < t_bath < t_fac * x * 1.001:   # cooling towards lambda^2 = 0 cancels: no ulp bound holds
                        continue
                    rows.append((dt, t_bath, (x, 0.37 * (1 + len(rows) % 5), -1.25, 0.0), (0.01, 0.1), 4))
    elif kind in (2, 3):
        at = 0.03125                                                     # dt f_inc = dt_max
        for vf in (3.0, 1e-30, 5e-324, 0.0, -0.0, -2.5, NAN):
            for npos in (2, 3, 4):                                       # n_min - 1, n_min, n_min + 1
                for sdt in (0.03, _next(at, False), at, _next(at), 0.04):
                    for ff, vv in ((7.0, 0.3), (0.0, 0.3), (1e-35, 1e-20), (7.0, 0.0)):
                        rows.append((0.0, 0.0, (vf, ff, vv, 0.0), (sdt, 0.3 * 0.875 ** (npos % 3)), npos))
        rows.append((0.0, 0.0, (3.0, NAN, 0.3, 0.0), (0.03, 0.3), 4))
        rows.append((0.0, 0.0, (3.0, 7.0, NAN, 0.0), (0.03, 0.3), 4))
        # v.v / F.F outside float's range, by a sum that is itself outside it and by two that are inside
        for ratio in (1e-36, 1e-40, 1e-300, 1e36, 1e40):
            r2 = float(np.sqrt(ratio))
            for ff, vv in ((1.0, ratio), (1.0 / r2, r2), (3e-29, 3e-29 * ratio)):
                rows.append((0.0, 0.0, (3.0, ff, vv, 0.0), (0.03, 0.3), 4))
        for ff in (_next(1e-30, False), 1e-30, _next(1e-30)):            # F.F at the floor
            rows.append((0.0, 0.0, (3.0, ff, 0.3, 0.0), (0.03, 0.3), 4))
    else:
        for npos in (0, 1, 2, 3, 7, 8):
            for a_prev in (1e-5, 3e-8, 80.0):                            # the doubling leaves [1e-7, 1e2] on both sides
                for sy, yy, ss in ((2.0, 5.0, 3.0), (2.0, 5e9, 3e-9), (2.0, 1e-3, 9e2), (0.0, 5.0, 3.0), (-0.0, 5.0, 3.0), (-1.5, 5.0, 3.0),
                                   (NAN, 5.0, 3.0), (2.0, NAN, NAN), (2.0, 0.0, 3.0), (1e-30, 5.0, 3.0)):
                    rows.append((0.0, 0.0, (sy, 11.0, yy, ss), (a_prev, 0.2), npos))
        for npos in (2, 3):
            for sy in (1e-30, 1e-37, 1e-40, 1e-300, 5e-324):             # s.y below float's range: s.s / s.y is the upper bound's side
                rows.append((0.0, 0.0, (sy, 11.0, 5.0, 3.0), (1e-5, 0.2), npos))
            for yy in (1e-40, 1e-300):
                rows.append((0.0, 0.0, (2.0, 11.0, yy, 3.0), (1e-5, 0.2), npos))
            # lengths at both bounds and one double either side: s.y / y.y with y.y = 1, s.s / s.y with s.y = 1
            for a in (_next(1e-7, False), 1e-7, _next(1e-7), _next(1e2, False), 1e2, _next(1e2)):
                rows.append((0.0, 0.0, (a, 11.0, 1.0, a * a), (1e-5, 0.2), npos) if npos % 2 else (0.0, 0.0, (1.0, 11.0, 1.0, a), (1e-5, 0.2), npos))
    return rows


def row_finish_ref(kind, dt, row, consts, fire, mut=None, hits=None, precision=64, probe=None):
    """One row of c3d_debug_row_finish_f64 (precision 64) or c3d_debug_row_finish (32): the per-bead statements of c3o_md_step, c3o_fire_step
    and c3o_bb_step (oracle/c3d_oracle.c) and the bead's terms of the four sums the next step reads, in float64, one correctly rounded
    operation per oracle operation.  row (16) = x[3], v[3], F[3], lambda, cm[3], keep, mix, state dt.  precision 64: consts = table_consts64
    (acc = dt 418.4 / mass and dt_state (418.4 / mass) as step64 and the kernel form them).  precision 32: consts = table_consts, whose
    third entry is the host's float F32(418.4) / F32(mass); dt is the float the step holds, and dt acc, dt_state acc are the real products of
    those floats (the row's values are floats already).  Returns [x'[3], v'[3], q[4]].  mut: one name of TABLE_MUTATIONS; hits: a Counter of
    the branches taken; probe: a dict that receives the squared length each cap tested ("move_d2", "s_d2")."""
    kacc = float(consts[2])
    if precision == 32:
        dt = float(F32(dt))
        md_acc = dt * kacc
    else:
        md_acc = dt * 418.4 / float(consts[4])
    r = [float(a) for a in row]
    x, v, F = r[0:3], r[3:6], r[6:9]
    lam, cm, keep, mix, sdt = r[9], r[10:13], r[13], r[14], r[15]
    ms = float(fire.max_step)
    ms2 = ms * ms

    def hit(name):
        if hits is not None:
            hits[name] += 1

    def cap(d, which):
        d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if probe is not None:
            probe[which + "_d2"] = d2
        over = (d2 >= ms2) if mut == "cap_ge" else (d2 > ms2)
        hit(which + ("_at_cap" if d2 == ms2 else ("_capped" if d2 > ms2 else "_uncapped")))
        if not over:
            return 1.0
        hit(which + "_acted")                       # (an integer of the row: the only place ">=" for ">" at the cap shows — the scale there is 1)
        return float(np.float64(ms) / (np.float64(d2) if mut == "cap_no_sqrt" else np.sqrt(np.float64(d2))))

    with np.errstate(all="ignore"):
        if kind == 4:
            hit("md_begin")
            vn, xn = list(v), list(x)
            q = [vn[0] * vn[0] + vn[1] * vn[1] + vn[2] * vn[2], vn[0], vn[1], vn[2]]
        elif kind in (0, 1):
            hit("md")
            acc = md_acc
            vn = [lam * ((v[k] - cm[k]) if mut != "no_cm" else v[k]) + acc * F[k] for k in range(3)]
            xn = [x[k] + dt * vn[k] for k in range(3)]
            q = [vn[0] * vn[0] + vn[1] * vn[1] + vn[2] * vn[2], vn[0], vn[1], vn[2]]
        elif kind in (5, 6):
            q = [0.0, F[0] * F[0] + F[1] * F[1] + F[2] * F[2], 0.0, 0.0]
            if kind == 5:
                s = [lam * v[k] for k in range(3)]
                sc = cap(s, "s")
                s = [a * sc for a in s]
                y = [v[k] - F[k] for k in range(3)]
                q[0] = s[0] * y[0] + s[1] * y[1] + s[2] * y[2]
                q[2] = y[0] * y[0] + y[1] * y[1] + y[2] * y[2]
                q[3] = s[0] * s[0] + s[1] * s[1] + s[2] * s[2]
            dr = [mix * F[k] for k in range(3)]
            sc = cap(dr, "move")
            xn = [x[k] + sc * dr[k] for k in range(3)]
            vn = list(F)
        else:
            q = [v[0] * F[0] + v[1] * F[1] + v[2] * F[2], F[0] * F[0] + F[1] * F[1] + F[2] * F[2], v[0] * v[0] + v[1] * v[1] + v[2] * v[2], 0.0]
            acc = sdt * kacc
            vn = [keep * v[k] + mix * F[k] for k in range(3)]
            vn = [vn[k] + acc * F[k] for k in range(3)]
            dr = [sdt * vn[k] for k in range(3)]
            sc = cap(dr, "move")
            xn = [x[k] + sc * dr[k] for k in range(3)]
    return xn + vn + q


SEED_EDGE_D2 = (2.0 ** 127, 2.0 ** 128, 1e40, 1e150, 1e300)
_U = (0.6, -0.64, 0.48)                     # the direction of the tuned rows: every component in play, |u| = 1 to a rounding
_X0 = (1.5, -2.5, 3.5)                      # coordinates on the displacement's side of 0: x + (capped move) does not cancel


def _bisect(fn, lo, hi, target):
    """the double z in [lo, hi] (positive, fn non-decreasing there) with fn(z) == target"""
    a, b = int(np.float64(lo).view(np.int64)), int(np.float64(hi).view(np.int64))
    assert fn(lo) < target <= fn(hi), (fn(lo), target, fn(hi))
    while b - a > 1:
        mid = (a + b) // 2
        if fn(float(np.int64(mid).view(np.float64))) >= target:
            b = mid
        else:
            a = mid
    z = float(np.int64(b).view(np.float64))
    assert fn(z) == target, (fn(z), target)
    return z


def _d2(d):
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def row_finish_rows(kind, dt, consts, fire):
    """[(row16, tag)] of a kind for c3d_debug_row_finish_f64.  tag: "plain" (no cap acted: products and sums) or "capped".
    The capped quantity of a kind (FIRE: dt v'; two-point: mix F, and lambda v of the previous move) is put at max_step^2 and one double
    either side by a search on one component, and at 0, 1e-300, 4 and 1e16 max_step^2; F = 0, F with a -0, F with a NaN; lambda in {0, 1},
    keep / mix in {0, 0.7}; kind 5: both caps on either side independently; kinds 0, 1, 4 have no cap: the same moves uncapped."""
    kacc = float(consts[2])
    ms = float(fire.max_step)
    ms2 = ms * ms
    sdt = 0.03125
    rows = []

    def row(x, v, F, lam=1.0, cm=(0.0, 0.0, 0.0), keep=0.0, mix=0.0, st=sdt):
        return list(x) + list(v) + list(F) + [lam] + list(cm) + [keep, mix, st]

    def tag_of(r):
        from collections import Counter
        h = Counter()
        row_finish_ref(kind, dt, r, consts, fire, hits=h)
        return "capped" if (h["move_capped"] or h["s_capped"]) else "plain"

    def add(r):
        rows.append((r, tag_of(r)))

    if kind in (2, 3):
        # dr = st (keep v + mix F + st kacc F): v, F along _U; F's third component tuned
        for keep, mix in ((0.0, 0.0), (0.7, 0.7), (0.7, 0.0), (0.0, 0.7)):
            gain = mix + sdt * kacc

            def move_d2(fz, S, keep=keep, mix=mix):
                r = row(_X0, [0.5 * S * u for u in _U], [S * _U[0], S * _U[1], fz], keep=keep, mix=mix)
                acc = sdt * kacc
                vn = [keep * r[3 + k] + mix * r[6 + k] for k in range(3)]
                vn = [vn[k] + acc * r[6 + k] for k in range(3)]
                return _d2([sdt * a for a in vn]), r

            for target in (_next(ms2, False), ms2, _next(ms2)):
                S = 0.98 * ms / (sdt * (0.5 * keep + gain))
                fz = _bisect(lambda z: move_d2(z, S)[0], 0.5 * S * _U[2], 4.0 * S * _U[2], target)
                d2, r = move_d2(fz, S)
                assert d2 == target
                add(r)
            for f2 in (1e-300, 4.0, 1e16):
                S = float(np.sqrt(f2)) * ms / (sdt * (0.5 * keep + gain))
                add(row(_X0, [0.5 * S * u for u in _U], [S * u for u in _U], keep=keep, mix=mix))
            add(row(_X0, (0.3, -0.2, 0.1), (0.0, 0.0, 0.0), keep=keep, mix=mix))
            add(row(_X0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), keep=keep, mix=mix))                       # d2 = 0
            add(row(_X0, (0.3, -0.2, 0.1), (1.5, -0.0, 2.5), keep=keep, mix=mix))
            add(row(_X0, (0.3, -0.2, 0.1), (1.5, NAN, 2.5), keep=keep, mix=mix))
    elif kind in (5, 6):
        # move = mix F; kind 5: s = lambda v.  Each on either side of, and at, the cap, independently
        sides = [("edge", t) for t in (_next(ms2, False), ms2, _next(ms2))] + [("free", f2) for f2 in (1e-300, 0.25, 4.0, 1e16)]

        def tuned(length, what):
            """a vector w along _U with |length w|^2 == what[1] exactly ("edge") or about what[1] max_step^2 ("free")"""
            if what[0] == "free":
                S = float(np.sqrt(what[1])) * ms / length
                return [S * u for u in _U]
            S = 0.98 * ms / length
            fn = lambda z: _d2([length * S * _U[0], length * S * _U[1], length * z])
            z = _bisect(fn, 0.5 * S * _U[2], 4.0 * S * _U[2], what[1])
            return [S * _U[0], S * _U[1], z]

        for a_prev, a in ((1e-5, 3e-5), (0.7, 0.7), (1.0, 1e2), (0.0, 1e-7)):
            for mv in sides:
                F = [-c for c in tuned(a, mv)]                            # the move is along -_U, x0 on that side of 0
                x0 = [-c for c in _X0]
                if kind == 6:
                    add(row(x0, (0.0, 0.0, 0.0), F, lam=a_prev, mix=a))
                    continue
                for sv in (sides if a_prev > 0 else [("free", 4.0)]):
                    v = tuned(a_prev, sv) if a_prev > 0 else [3.0 * u for u in _U]
                    add(row(x0, v, F, lam=a_prev, mix=a))
        for a_prev, a in ((1e-5, 3e-5), (0.7, 0.7)):
            v = (0.0, 0.0, 0.0) if kind == 6 else (0.3, -0.2, 0.1)
            add(row(_X0, v, (0.0, 0.0, 0.0), lam=a_prev, mix=a))
            add(row(_X0, v, (1.5, -0.0, 2.5), lam=a_prev, mix=a))
            add(row(_X0, v, (1.5, NAN, 2.5), lam=a_prev, mix=a))
    else:
        # MD: v' = lambda (v - cm) + acc F, x' = x + dt v' (kind 4: v' = v, x' = x); no cap whatever the move
        step = dt if kind != 4 else sdt
        for lam in (0.0, 1.0, 0.93):
            for cm in ((0.0, 0.0, 0.0), (0.01, -0.02, 0.03)):
                for f2 in (0.0, 1e-300, 1.0, 4.0, 1e16):
                    S = float(np.sqrt(f2)) * ms / step
                    add(row(_X0, [S * u for u in _U], [0.5 * S * u for u in _U], lam=lam, cm=cm))
                add(row(_X0, (0.3, -0.2, 0.1), (0.0, 0.0, 0.0), lam=lam, cm=cm))
                add(row(_X0, (0.3, -0.2, 0.1), (1.5, -0.0, 2.5), lam=lam, cm=cm))
                add(row(_X0, (0.3, -0.2, 0.1), (1.5, NAN, 2.5), lam=lam, cm=cm))
    # vectors that are not parallel (a swapped component shows), in one sign pattern so that no sum of a capped row cancels: plain and capped
    rng = np.random.default_rng(3100 + kind)
    sg = np.array([1.0, -1.0, 1.0])
    for big in (False, True):
        for _ in range(8):
            v = sg * rng.uniform(0.2, 1.0, 3) * (40.0 * ms / sdt if big else 0.01)
            F = -sg * rng.uniform(0.2, 1.0, 3) * (40.0 * ms / sdt if big else 0.01)
            if kind in (2, 3):
                v = -v                                                    # v' = keep v + (mix + acc) F: one sign
            add(row(-sg * rng.uniform(1.0, 4.0, 3), v if kind not in (3, 6) else 0.0 * v, F, lam=0.9 if kind < 5 else 0.02, cm=(0.01, -0.02, 0.03) if kind < 2 else (0.0, 0.0, 0.0),
                    keep=0.7, mix=0.02 if kind >= 5 else 0.1))
    # the capped quantity either side of the range of the cap's float seed (v_rsq_f32 of (float)d.d is 0 from 2^128 on): d.d in A^2
    if kind in (2, 3, 5, 6):
        for d2 in SEED_EDGE_D2:
            mag = float(np.sqrt(d2))
            for x0 in (_X0, (0.0, 0.0, 0.0)):
                if kind in (2, 3):
                    for keep, mix in ((0.7, 0.7), (0.0, 0.0)):
                        S = mag / (sdt * (0.5 * keep + mix + sdt * kacc))
                        add(row(x0, [0.5 * S * u for u in _U], [S * u for u in _U], keep=keep, mix=mix))
                else:
                    for a_prev, a in ((0.7, 0.7), (1.0, 1e2)):
                        F = [-mag / a * u for u in _U]
                        add(row([-c for c in x0], (0.0, 0.0, 0.0) if kind == 6 else (0.3, -0.2, 0.1), F, lam=a_prev, mix=a))
                        if kind == 5:
                            add(row([-c for c in x0], [mag / a_prev * u for u in _U], F, lam=a_prev, mix=a))
                            add(row([-c for c in x0], [mag / a_prev * u for u in _U], [-0.1 * u for u in _U], lam=a_prev, mix=a))
    return rows


# ---------------------------------------------------------------------------------------------
# the fp32 row update as a table (c3d_debug_row_finish): finish_row, c3d_step_core.h
# ---------------------------------------------------------------------------------------------
FLT_MAX, FLT_MIN, FLT_DENORMAL = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny), float(F32(1e-42))
_TWO128 = 2.0 ** 128                        # what stands for a float's infinity when a gap is measured: the float after FLT_MAX


def f32(x):
    return float(F32(x))


def _next32(x, up=True):
    return float(np.nextafter(F32(x), F32(np.inf if up else -np.inf)))


def ulps32(got, want):
    """|got - want| in units of the spacing of floats at want.  want is a float64 value of the restatement: one below the denormals counts in
    units of the smallest denormal, one beyond FLT_MAX is the float's infinity, and an infinity counts as the float after FLT_MAX."""
    got, want = float(got), float(want)
    if got == want:
        return 0.0
    if got != got or want != want:
        return float("inf")
    g, w = max(min(got, _TWO128), -_TWO128), max(min(want, _TWO128), -_TWO128)
    return abs(g - w) / float(np.spacing(F32(min(abs(w), _next32(FLT_MAX, False)))))


def _cross32(fn, lo, hi, target):
    """the adjacent floats (z0, z1) in [lo, hi] (positive, fn non-decreasing there) with fn(z0) <= target < fn(z1)"""
    a, b = int(F32(lo).view(np.int32)), int(F32(hi).view(np.int32))
    assert fn(f32(lo)) <= target < fn(f32(hi)), (fn(f32(lo)), target, fn(f32(hi)))
    while b - a > 1:
        mid = (a + b) // 2
        if fn(float(np.int32(mid).view(np.float32))) > target:
            b = mid
        else:
            a = mid
    z0, z1 = float(np.int32(a).view(np.float32)), float(np.int32(b).view(np.float32))
    assert fn(z0) <= target < fn(z1) and _next32(z0) == z1
    return z0, z1


ROW_TAGS32 = ("plain", "capped", "overflow", "beyond", "beyond_s", "infinite")
_K7 = f32(0.7)


def row_finish_rows32(kind, dt, consts, fire):
    """[(row16, tag)] of a kind for c3d_debug_row_finish: row_finish_rows' structure with every input exactly a float32.  consts =
    table_consts.  tag: "plain" (no cap acted), "capped", and beyond what a float carries
      "overflow"  the capped quantity d finite and d.d at most one float below FLT_MAX (held as a capped row),
      "beyond"    d finite and d.d beyond FLT_MAX (the move), "beyond_s" the same for kind 5's previous move, "infinite" mix F itself infinite.
    The capped quantity of a kind (FIRE: dt v'; two-point: mix F, and lambda v of the previous move) sits on the two adjacent floats of one
    component between which the restatement's d.d crosses max_step^2, at 0, the smallest normal float, a denormal, and 2 and 1e8 max_step
    (d.d = 4 and 1e16 max_step^2); F = 0, F with a -0, F with a NaN; lambda in {0, 1, 0.93}, keep / mix in {0, 0.7}; kind 5: both caps on
    either side independently.  Every tuned row stands twice: beside _X0 and at x = 0, where the displacement itself is the output."""
    from collections import Counter
    acc = float(consts[2])
    ms = float(fire.max_step)
    ms2 = ms * ms
    sdt = 0.03125
    rows = []
    mags = (0.0, FLT_MIN, FLT_DENORMAL, 0.5 * ms, 2.0 * ms, 1e8 * ms)          # |d| of the rows that are not at the edge

    def row(x, v, F, lam=1.0, cm=(0.0, 0.0, 0.0), keep=0.0, mix=0.0, st=sdt):
        return [f32(a) for a in list(x) + list(v) + list(F) + [lam] + list(cm) + [keep, mix, st]]

    def add(r, tag=None):
        if tag is None:
            h = Counter()
            row_finish_ref(kind, dt, r, consts, fire, hits=h, precision=32)
            tag = "capped" if (h["move_capped"] or h["s_capped"]) else "plain"
        rows.append((r, tag))

    def add2(sign, v, F, **kw):
        """a tuned row beside _X0 (on the move's side of 0: sign) and at x = 0"""
        add(row([sign * c for c in _X0], v, F, **kw))
        add(row((0.0, 0.0, 0.0), v, F, **kw))

    def probe_d2(r, which):
        p = {}
        row_finish_ref(kind, dt, r, consts, fire, precision=32, probe=p)
        return p[which]

    if kind in (2, 3):
        for keep, mix in ((0.0, 0.0), (_K7, _K7), (_K7, 0.0), (0.0, _K7)):
            gain = mix + sdt * acc
            S = 0.98 * ms / (sdt * (0.5 * keep + gain))
            mk = lambda z, S=S, keep=keep, mix=mix: row(_X0, [0.5 * S * u for u in _U], [S * _U[0], S * _U[1], z], keep=keep, mix=mix)
            for z in _cross32(lambda z: probe_d2(mk(z), "move_d2"), 0.5 * S * _U[2], 4.0 * S * _U[2], ms2):
                r = mk(z)
                add2(1.0, r[3:6], r[6:9], keep=keep, mix=mix)
            for mag in mags:
                S = mag / (sdt * (0.5 * keep + gain))
                add2(1.0, [0.5 * S * u for u in _U], [S * u for u in _U], keep=keep, mix=mix)
            add(row(_X0, (0.3, -0.2, 0.1), (0.0, 0.0, 0.0), keep=keep, mix=mix))
            add(row(_X0, (0.3, -0.2, 0.1), (1.5, -0.0, 2.5), keep=keep, mix=mix))
            add(row(_X0, (0.3, -0.2, 0.1), (1.5, NAN, 2.5), keep=keep, mix=mix))
    elif kind in (5, 6):
        sides = [("edge", 0), ("edge", 1)] + [("free", mag) for mag in mags]

        def tuned(length, what):
            """a float vector w along _U with |length w| = what[1] ("free"), or on the lower / upper float of the crossing of max_step^2 ("edge")"""
            length = f32(length)
            if what[0] == "free":
                return [f32(what[1] / length * u) for u in _U]
            S = 0.98 * ms / length
            c0, c1 = f32(S * _U[0]), f32(S * _U[1])
            z = _cross32(lambda z: _d2([length * c0, length * c1, length * z]), 0.5 * S * _U[2], 4.0 * S * _U[2], ms2)[what[1]]
            return [c0, c1, z]

        for a_prev, a in ((1e-5, 3e-5), (0.7, 0.7), (1.0, 1e2), (0.0, 1e-7)):
            for mv in sides:
                F = [-c for c in tuned(a, mv)]                            # the move is along -_U, x0 on that side of 0
                if kind == 6:
                    add2(-1.0, (0.0, 0.0, 0.0), F, lam=a_prev, mix=a)
                    continue
                for sv in (sides if a_prev > 0 else [("free", 2.0 * ms)]):
                    # (a previous move at the foot of float's range is a denormal float: its error is 2^-150 whatever its size, and s.y carries
                    #  that times |y|, so no bound in ulps of s.y holds unless y = F_old - F is as small: such an s meets such moves only)
                    if sv[0] == "free" and 0.0 < sv[1] <= FLT_MIN and not (mv[0] == "free" and mv[1] <= FLT_MIN):
                        continue
                    v = tuned(a_prev, sv) if a_prev > 0 else [3.0 * u for u in _U]
                    add2(-1.0, v, F, lam=a_prev, mix=a)
        for a_prev, a in ((1e-5, 3e-5), (0.7, 0.7)):
            v = (0.0, 0.0, 0.0) if kind == 6 else (0.3, -0.2, 0.1)
            add(row(_X0, v, (0.0, 0.0, 0.0), lam=a_prev, mix=a))
            add(row(_X0, v, (1.5, -0.0, 2.5), lam=a_prev, mix=a))
            add(row(_X0, v, (1.5, NAN, 2.5), lam=a_prev, mix=a))
    else:
        step = float(F32(dt)) if kind != 4 else sdt
        for lam in (0.0, 1.0, 0.93):
            for cm in ((0.0, 0.0, 0.0), (0.01, -0.02, 0.03)):
                for mag in mags:
                    S = mag / step
                    add2(1.0, [S * u for u in _U], [0.5 * S * u for u in _U], lam=lam, cm=cm)
                add(row(_X0, (0.3, -0.2, 0.1), (0.0, 0.0, 0.0), lam=lam, cm=cm))
                add(row(_X0, (0.3, -0.2, 0.1), (1.5, -0.0, 2.5), lam=lam, cm=cm))
                add(row(_X0, (0.3, -0.2, 0.1), (1.5, NAN, 2.5), lam=lam, cm=cm))
    # vectors that are not parallel (a swapped component shows), in one sign pattern so that no sum of a capped row cancels: plain and capped
    rng = np.random.default_rng(3200 + kind)
    sg = np.array([1.0, -1.0, 1.0])
    for big in (False, True):
        for _ in range(8):
            v = sg * rng.uniform(0.2, 1.0, 3) * (40.0 * ms / sdt if big else 0.01)
            F = -sg * rng.uniform(0.2, 1.0, 3) * (40.0 * ms / sdt if big else 0.01)
            if kind in (2, 3):
                v = -v                                                    # v' = keep v + (mix + acc) F: one sign
            add(row(-sg * rng.uniform(1.0, 4.0, 3), v if kind not in (3, 6) else 0.0 * v, F, lam=0.9 if kind < 5 else 0.02, cm=(0.01, -0.02, 0.03) if kind < 2 else (0.0, 0.0, 0.0),
                    keep=_K7, mix=0.02 if kind >= 5 else 0.1))
    if kind not in (2, 3, 5, 6):
        return rows
    # Beyond what a float carries.  The vectors lie along one axis and meet only the factor 1 (FIRE: keep 1, no force, state dt 1; two-point:
    # length 1), so that the device's d is the row's own float and its d.d that float's square rounded once: finite below the edge
    # whatever the rounding.  zmax = the float whose square, rounded to float, is the float below FLT_MAX (the next float's is beyond it).
    zmax = f32(np.sqrt(np.float64(FLT_MAX)))
    while f32(zmax * zmax) >= FLT_MAX:
        zmax = _next32(zmax, False)
    assert f32(zmax * zmax) == _next32(FLT_MAX, False) and _next32(zmax) ** 2 > FLT_MAX
    zero = (0.0, 0.0, 0.0)

    def axis(k, z):
        return [z * sg[k] if j == k else 0.0 for j in range(3)]

    for k in range(3):
        for z, tag in ((zmax, "overflow"), (2.0 ** 64, "beyond"), (1e30, "beyond")):
            for x0 in (_X0, zero):
                if kind in (2, 3):
                    add(row(x0, axis(k, z), zero, keep=1.0, mix=0.0, st=1.0), tag)
                else:
                    add(row([-c for c in x0], zero, axis(k, -z), lam=1.0, mix=1.0), tag)
                    if kind == 5:
                        add(row(x0, axis(k, z), zero, lam=1.0, mix=1.0), "overflow" if tag == "overflow" else "beyond_s")
        if kind in (5, 6):
            for x0 in (_X0, zero):
                add(row([-c for c in x0], zero, axis(k, -1e37), lam=1.0, mix=1e2), "infinite")
    # (all three components in play: 2^-18 below FLT_MAX, further than the device's three roundings of d.d can carry it)
    S = float(np.sqrt(FLT_MAX * (1.0 - 2.0 ** -18)))
    for x0 in (_X0, zero):
        if kind in (2, 3):
            add(row(x0, [S * u for u in _U], zero, keep=1.0, mix=0.0, st=1.0), "overflow")
        else:
            add(row([-c for c in x0], zero, [-S * u for u in _U], lam=1.0, mix=1.0), "overflow")
    return rows


def finish_row_emulated32(kind, dt, row, consts, fire, rsq_shift=0):
    """finish_row (c3d_step_core.h) statement by statement in float32 — every fmaf an exact product plus sum rounded once, every other
    operation rounded once, v_rsq_f32 as the rounded 1 / sqrt moved by rsq_shift floats (its documented accuracy is 1 ulp).  Not the
    expected values: what tests/test_controller_ref.py runs against row_finish_ref to admit the table's bounds without a device."""
    f = F32
    fma = lambda a, b, c: f(np.float64(a) * np.float64(b) + np.float64(c))
    mul = lambda a, b: f(np.float64(a) * np.float64(b))
    sub = lambda a, b: f(np.float64(a) - np.float64(b))

    def rsq(x):
        y = f(1.0 / np.sqrt(np.float64(x)))
        for _ in range(abs(rsq_shift)):
            y = np.nextafter(y, f(np.inf if rsq_shift > 0 else 0.0))
        return y

    r = [f(a) for a in row]
    x, v, F = r[0:3], r[3:6], r[6:9]
    lam, cm, keep, mix, sdt = r[9], r[10:13], r[13], r[14], r[15]
    acc, ms, dt = f(consts[2]), f(fire.max_step), f(dt)
    dot = lambda a, b: fma(a[0], b[0], fma(a[1], b[1], mul(a[2], b[2])))
    with np.errstate(all="ignore"):
        if kind == 4:
            vn, xn = list(v), list(x)
            q = [dot(vn, vn), vn[0], vn[1], vn[2]]
        elif kind in (0, 1):
            a = mul(dt, acc)
            vn = [fma(a, F[k], mul(lam, sub(v[k], cm[k]))) for k in range(3)]
            xn = [fma(dt, vn[k], x[k]) for k in range(3)]
            q = [dot(vn, vn), vn[0], vn[1], vn[2]]
        elif kind in (5, 6):
            ms2 = mul(ms, ms)
            q = [f(0.0), dot(F, F), f(0.0), f(0.0)]
            if kind == 5:
                s = [mul(lam, v[k]) for k in range(3)]
                s2 = dot(s, s)
                scp = mul(ms, rsq(s2)) if s2 > ms2 else f(1.0)
                s = [mul(a, scp) for a in s]
                y = [sub(v[k], F[k]) for k in range(3)]
                q = [dot(s, y), q[1], dot(y, y), dot(s, s)]
            d = [mul(mix, F[k]) for k in range(3)]
            d2 = dot(d, d)
            scl = mul(ms, rsq(d2)) if d2 > ms2 else f(1.0)
            xn = [fma(scl, d[k], x[k]) for k in range(3)]
            vn = list(F)
        else:
            q = [dot(v, F), dot(F, F), dot(v, v), f(0.0)]
            a = mul(sdt, acc)
            vn = [fma(a, F[k], fma(keep, v[k], mul(mix, F[k]))) for k in range(3)]
            d = [mul(sdt, vn[k]) for k in range(3)]
            d2 = dot(d, d)
            scl = mul(ms, rsq(d2)) if d2 > mul(ms, ms) else f(1.0)
            xn = [fma(scl, d[k], x[k]) for k in range(3)]
    return [float(a) for a in xn + vn + q]


def row_gap32(got, want, tag, row):
    """The table's assertion on one row, shared by the CPU admission and the device test: got (10 floats) against row_finish_ref's want
    under the row's tag.  Returns the row's largest gap in float ulps (over what a bound holds); raises AssertionError with the figures.
      plain 4, capped and overflow 8 float ulps of the expected value; NaN where the restatement has NaN; a zero with the restatement's sign
      beyond / beyond_s / infinite: v' and the sums as the restatement within 8 — except what the dead cap itself feeds: the coordinates
      (beyond: x' = x exactly, the bead stays; infinite: NaN in the component whose move is infinite, x elsewhere) and, for beyond_s, the
      two sums made of the previous move (s.y and s.s are 0: the rebuilt move is scaled by 1 / sqrt(inf) = 0)."""
    cap = ROW_CAPS32[tag]
    worst = 0.0
    for j, (g, w) in enumerate(zip(got, want)):
        g = float(g)
        if tag in ("beyond", "infinite") and j < 3:
            moves_inf = tag == "infinite" and abs(float(row[14]) * float(row[6 + j])) > FLT_MAX
            assert (g != g) if moves_inf else (g == row[j]), (tag, j, g, row)
            continue
        if tag == "beyond_s" and j in (6, 9):
            assert g == 0.0, (tag, j, g, row)
            continue
        if w != w:
            assert g != g, (tag, j, g, w, row)
            continue
        if w == 0.0:
            assert g == 0.0 and np.signbit(g) == np.signbit(w), (tag, j, g, w, row)
            continue
        u = ulps32(g, w)
        assert u <= cap, (tag, j, g, w, u, cap, row)
        worst = max(worst, u)
    return worst


ROW_CAPS32 = {"plain": 4.0, "capped": 8.0, "overflow": 8.0, "beyond": 8.0, "beyond_s": 8.0, "infinite": 8.0}
