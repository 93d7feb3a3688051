"""The case table of the L-BFGS stage's controller (stage kind 8: the serial section of k_lbfgs_move / k64_lbfgs_move): short trajectories
built so that the restatement (tests/lbfgs_ref.py lbfgs_run, which logs the branch of every step) takes the pair test's reject branch —
at the start, twice in a row, and in mid-run with a full ring —, both clamps of gamma with unclamped steps between, the per-bead cap on
no, some and every bead, the ring's wrap-around at memory 1, 2, 5 and 8 and the hand-over to FIRE.  tests/test_lbfgs_cases.py admits
them on the CPU (branches, conditioning in float32, margins, sensitivity to MUTATIONS); tests/test_gpu_lbfgs_controller.py runs them on
the device.  A start is data: float32 coordinates that go in through c3d_set_coords, the restatement starts from the same values.

How the cases were found (all on the synthetic maps synthetic_if(n, seed=n)):
  relaxed start (200 default FIRE steps from the coil under the default model and the final stage's weights)
      no pair rejected, gamma 2e-4 .. 2e-3, few beads capped: the wrap-around cases, and at 250 beads the cap on some beads of a step
  the same start with k_bond = 2e6          s.y / y.y falls to 0.8e-7 .. 3e-7: the lower clamp on some steps, not on others
  the same start with w_all = 1e-5, w_vdw = 0 and dt_start = 2
                                            s.y / y.y is 40 .. 200: the upper clamp on some steps.  With the default dt_start the first
                                            move (gamma_0 F = 1.7e-5 x 1e-4 A) is below a float's grain at 30 A, the first pair is noise
                                            in float32 and the twin ends 0.2 .. 2 A away: dt_start = 2 makes the first move 1e-3 A
  the coil scaled by 0.05, max_step = 8     pairs rejected on steps 1 (and 2) with no bead capped: gamma's doubling moves every bead
  the coil scaled by 0.05, default max_step the same rejections at 250 beads with every bead capped on every later step
  coil 2 scaled by 0.08, 96 beads           step 1 rejected, six pairs kept, step 8 rejected (no bead capped on it) with the head at slot 5
                                            of 8: the ring refills from cnt = 0 in mid-run.  Memory 6 and 8 reach it, 2 .. 4 do not.
At 1100 beads (the wide and chunked forms) the relaxed starts of coils 4 and 5 are the quiet ones (controller_ref._BIG); the scaled coils
(0.01 .. 0.05, coils 0 .. 3) reject no pair there: the reject branch is held at 96 and 250 beads, where every evaluation form but the
wide one runs it — the branch itself is in k_lbfgs_move, which has one form.
Nothing reaches F.d <= 0 (with every kept pair s.y > 0 the compact form is positive definite)."""
import functools

import numpy as np

from oracle import oracle as O
from tests import controller_ref as R
from tests import lbfgs_ref as L
from tests.util import oracle_fire_from, oracle_model_from

SEED = R.SEED
FINAL = (1.0, 1.0, 0.85)                   # the final stage's weights: w_all, w_vdw, repel_s
CAP32 = 1e-2                               # A: the suite's bound for fp32 L-BFGS trajectories (tests/test_gpu_lbfgs.py)
CAP64 = 1e-8                               # A: fp64, read through c3d_get_coords_f64


class Case:
    """model / fire: fields off the library's defaults; weights: the stage's (w_all, w_vdw, repel_s); mem: lbfgs_memory; nsteps: length
    of the kind-8 stage; nl: final_minimiser_steps (L-BFGS for min(nsteps, nl) steps, then FIRE from a fresh state); checkpoints: step
    counts at which run_steps is split and everything is compared (the last is nsteps; all others lie in the L-BFGS part); start:
    "relaxed" or ("coil", scale); ids: {beads: the two coils the starts of slots 0 and 1 are made from} — its keys are the sizes."""

    def __init__(self, model, fire, weights, mem, nsteps, checkpoints, ids, start="relaxed", nl=1000):
        self.model, self.fire, self.mem, self.nsteps, self.nl, self.start, self.ids = model, fire, mem, nsteps, nl, start, ids
        self.weights = tuple(float(np.float32(a)) for a in weights)       # as the C ABI holds them: floats
        self.checkpoints = tuple(checkpoints)
        self.nlb = min(nsteps, nl)
        assert self.checkpoints[-1] == nsteps <= 40 and all(k <= self.nlb for k in self.checkpoints[:-1])

    @property
    def stage(self):
        return (8, self.nsteps, 0.0) + self.weights + (0.0,)


CASES = {
    # wrap-around; few or no beads capped, so the coefficients' scale is in the coordinates
    "wrap_m1": Case({}, {}, FINAL, 1, 12, [3, 12], {250: (0, 3)}),
    "wrap_m2_then_fire": Case({}, {}, FINAL, 2, 20, [5, 12, 20], {250: (2, 3)}, nl=12),
    "wrap_m5": Case({}, {}, FINAL, 5, 24, [4, 24], {96: (0, 2)}),
    "wrap_m8": Case({}, {}, FINAL, 8, 30, [6, 30], {250: (0, 1), 1100: (4, 5)}),
    "lower_clamp": Case(dict(k_bond=2e6), {}, FINAL, 5, 26, [8, 26], {96: (0, 1), 250: (0, 1)}),
    # s.y / y.y = 2e-8 .. 3e-8 on every step: what the mixed case cannot show (there gamma is within 25 % of the bound where it is clamped,
    # and a missing clamp moves a bead by 0.04 A at the most), this one does: without the clamp it ends 0.5 A away
    "lower_clamp_deep": Case(dict(k_bond=1e7), {}, FINAL, 5, 20, [6, 20], {96: (0, 1), 1100: (4, 5)}),
    "upper_clamp": Case({}, dict(dt_start=2.0), (1e-5, 0.0, 0.85), 5, 20, [4, 20], {96: (0, 1)}),
    # the same for the upper bound: s.y / y.y five times beyond it on every step
    "upper_clamp_deep": Case({}, dict(dt_start=2.0), (2e-6, 0.0, 0.85), 5, 20, [4, 20], {96: (0, 1), 1100: (4, 5)}),
    # rejected pairs at the start: the split at 2 is directly after the first rejection of both slots, at 3 after slot 0's second
    "reject_start": Case({}, dict(max_step=8.0), FINAL, 3, 16, [2, 3, 16], {96: (1, 0)}, start=("coil", 0.05)),
    "reject_all_capped": Case({}, {}, FINAL, 5, 16, [2, 16], {250: (0, 2)}, start=("coil", 0.05)),
    # a rejection in mid-run (slot 0, step 8; slot 1 has none): split directly after it
    "reject_midrun": Case({}, {}, FINAL, 8, 20, [9, 20], {96: (2, 0)}, start=("coil", 0.08)),
}
CASE_SIZES = [(name, n) for name, c in CASES.items() for n in c.ids]


def models(case, n):
    """(c3d_model, c3d_fire_params, oracle Model, oracle FireParams) of a case"""
    return R.models(case, n)


@functools.lru_cache(maxsize=None)
def start(name, n, slot):
    """float32 start coordinates of a slot"""
    case = CASES[name]
    coil = case.ids[n][slot]
    if case.start == "relaxed":
        return R._start((), "relaxed", n, coil)
    from chromosome3d_amd import default_model
    return (O.init_coords(oracle_model_from(default_model(), n), SEED, coil) * case.start[1]).astype(np.float32)


def first_length(case, n, precision=32):
    """gamma of the first step as the device forms it: in float arithmetic (fp32 kernels), in doubles (precision 64)"""
    m, fire, om, of = models(case, n)
    return L.gamma0(om, of) if precision == 32 else float(fire.dt_start) ** 2 * 418.4 / float(m.mass)


@functools.lru_cache(maxsize=None)
def reference(name, n, slot, round32=False, mut=None, precision=32):
    """The restatement of a case's slot: ({k: x centred after k steps for k in checkpoints}, log of the L-BFGS part, resets)."""
    case = CASES[name]
    _, _, om, of = models(case, n)
    d10 = R.problem(n)[1]
    force = lambda u: O.energy_force(om, d10, u, *case.weights)[0]
    x, info = L.lbfgs_run(force, start(name, n, slot).astype(np.float64), case.nlb, m=case.mem, g0=first_length(case, n, precision),
                          max_step=float(of.max_step), mutate=mut, round32=round32, checkpoints=case.checkpoints, mass=float(om.mass))
    cps = {k: v - v.mean(0) for k, v in info["checkpoints"].items()}
    if case.nsteps > case.nlb:                 # FIRE from a fresh state: the oracle's own, or its float32 twin
        tail = [(2, case.nsteps - case.nlb, 0.0) + case.weights + (0.0,)]
        if round32:
            xt = R.run_twin(om, d10, tail, of, slot, x, round32=True)[0]
        else:
            xt = O.run_schedule(om, d10, O.make_stages(tail), of, SEED, slot, x0=x)[0]
        cps[case.nsteps] = xt - xt.mean(0)
    return cps, info["log"], info["resets"]


def gap(a, b, case):
    """the largest coordinate distance (A) of two references over the case's checkpoints"""
    return max(float(np.abs(a[0][k] - b[0][k]).max()) for k in case.checkpoints)


def branches(log):
    return [s.branch + ("+" + s.clamp if s.clamp else "") for s in log]
