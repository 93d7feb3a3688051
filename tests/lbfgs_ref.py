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


def lbfgs_run(force, x0, nsteps, m=5, g0=1.67e-5, max_step=0.5, gtol=0.0, clamp=True):
    """nsteps steps from x0 (n x 3); force(x) -> F (n x 3).  Returns (x, info): info["evals"] = force evaluations made, info["resets"] =
    memory drops, info["rms"] = RMS force of every evaluation.  gtol > 0: stop after the evaluation whose RMS force is below it (that
    evaluation's move is not made: tools/minimiser_study.py's convention; the device and the oracle check after whole steps and chunks)."""
    x = np.array(x0, dtype=np.float64).reshape(-1)
    S, Y = [], []
    gamma = g0
    F_prev = s_prev = None
    resets, rmss = 0, []
    for k in range(nsteps):
        F = np.asarray(force(x.reshape(-1, 3)), dtype=np.float64).reshape(-1)
        rmss.append(rms(F))
        if gtol > 0 and rmss[-1] < gtol:
            break
        if k > 0:
            y = F_prev - F
            sy, yy, ss = s_prev @ y, y @ y, s_prev @ s_prev
            if sy > 1e-12 * np.sqrt(ss * yy):
                S.append(s_prev); Y.append(y)
                if len(S) > m:
                    S.pop(0); Y.pop(0)
                gamma = sy / yy
            else:
                S, Y = [], []
                resets += 1
                gamma *= 2.0
            if clamp:
                gamma = min(max(gamma, 1e-7), 1e2)
        d = compact_direction(F, S, Y, gamma)
        if not (F @ d > 0):
            S, Y = [], []
            resets += 1
            d = gamma * F
        step = d.reshape(-1, 3)
        ln = np.sqrt((step ** 2).sum(axis=1))
        step = step * np.where(ln > max_step, max_step / np.maximum(ln, 1e-300), 1.0)[:, None]
        xn = x + step.reshape(-1)
        F_prev, s_prev = F, xn - x
        x = xn
    return x.reshape(-1, 3), {"evals": len(rmss), "resets": resets, "rms": rmss}


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
