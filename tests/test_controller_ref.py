"""The controller cases of tests/controller_ref.py, admitted on the CPU: the twin is the oracle (1e-10), the cases jointly take every branch
of the step controller the list below names, each is a trajectory float32 can follow (same branches, a quarter of the GPU tolerance) with
every discontinuous decision away from its edge (1e-3), and every mutation of MUTATIONS ends at least ten GPU tolerances from some case.
tests/test_gpu_controllers.py runs the same table on the device: what is proved here is what makes a pass there mean something."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import controller_ref as R
from tests import lbfgs_ref as L

CASE_SIZES = [(name, n) for name in R.CASES for n in R.SIZES[name]]
ALL250 = [name for name in R.CASES if 250 in R.SIZES[name]]


def _runs(names=ALL250, n=250):
    return [(name, slot, R.reference(name, n, slot)[2]) for name in names for slot in (0, 1)]


@pytest.mark.parametrize("name,n", CASE_SIZES)
def test_twin_is_the_oracle(built, name, n):
    """run_twin against O.run_schedule on every case and size: coordinates to 1e-10 A, velocities to 1e-10 relative"""
    case = R.CASES[name]
    _, _, om, of = R.models(case, n)
    O.set_two_point_steps(case.tp)
    try:
        for slot in (0, 1):
            x, v, log, _ = R.reference(name, n, slot)
            xo, vo, ev = O.run_schedule(om, R.problem(n)[1], O.make_stages(case.stages), of, R.SEED, case.first + slot,
                                        x0=R.start(name, n, slot).astype(np.float64))
            assert ev == case.nsteps == len(log)
            assert np.abs(x - xo).max() < 1e-10, (slot, np.abs(x - xo).max())
            assert np.abs(v - vo).max() < 1e-10 * max(1.0, np.abs(vo).max()), (slot, np.abs(v - vo).max())
    finally:
        O.set_two_point_steps(1000)


def _mid_run_resets(log, n_min):
    """resets after step 2 of a minimiser run that at least n_min + 2 downhill steps follow"""
    out = []
    for k, s in enumerate(log):
        if s.kind == 2 and s.branch == "reset" and s.since >= 2 and log[k - 1].branch != "reset":      # (a double reset is one event)
            tail = log[k + 1:k + 1 + n_min + 3]
            # (the step after an uphill reset tests the sums of the reset step itself and may reset once more: skipped)
            run = [t for t in tail if t.kind == 2 and t.stage == s.stage]
            down = 0
            for t in run[1:] if run and run[0].branch == "reset" else run:
                if t.branch == "reset":
                    break
                down += 1
            if down >= n_min + 2:
                out.append(k)
    return out


def test_cases_take_every_branch(built):
    """The table's coverage, with counts (at 250 beads, both slots)."""
    from chromosome3d_amd import default_fire
    runs = _runs()
    n = 250
    # FIRE
    best_resets = 0
    for name, slot, log in runs:
        nm = default_fire(**R.CASES[name].fire).n_min
        res = _mid_run_resets(log, nm)
        for k in res:                              # hold (where n_min > 0) and grow are seen again after EVERY such reset, before the next one
            nxt = next((j for j in range(k + 2, len(log)) if log[j].branch == "reset"), len(log))
            after = [s.branch for s in log[k + 1:nxt]]
            assert ("hold" in after or nm == 0) and "grow" in after, (name, slot, k, after)
        best_resets = max(best_resets, len(res))
    assert best_resets >= 2, best_resets
    assert max(sum(1 for s in log if s.branch == "cap") for _, _, log in runs) >= 2      # twice within one run
    n_mins = {default_fire(**R.CASES[name].fire).n_min for name, _, log in runs if any(s.kind == 2 for s in log)}
    assert 0 in n_mins and n_mins - {0, 5}, n_mins
    assert any(sum(1 for s in log if s.kind == 2 and 0 < s.ncap < n) >= 5 and sum(1 for s in log if s.kind == 2 and s.ncap == 0) >= 5
               for _, _, log in runs)
    assert {R.CASES[name].start for name, _, log in runs if any(s.kind == 2 for s in log)} == {"relaxed", "coil"}
    # MD: in one run clamp0 >= 3, floor >= 2 of kind 0 and >= 1 of kind 1, plain before and after both
    ok = False
    for _, _, log in runs:
        md = [s for s in log if s.kind in (0, 1)]
        seq = [s.branch for s in md]
        if (seq.count("clamp0") >= 3 and sum(1 for s in md if s.branch == "floor" and s.kind == 0) >= 2
                and sum(1 for s in md if s.branch == "floor" and s.kind == 1) >= 1):
            f0, f1 = seq.index("floor"), len(seq) - 1 - seq[::-1].index("floor")
            c0, c1 = seq.index("clamp0"), len(seq) - 1 - seq[::-1].index("clamp0")
            ok = ok or ("plain" in seq[:min(f0, c0)] and "plain" in seq[max(f1, c1) + 1:] and "plain" in seq[min(f1, c1) + 1:max(f0, c0)])
    assert ok
    # two-point: the hand-over inside the window, a split inside the two-point part, a split directly after a mid-run FIRE reset
    tp = [c for c in (R.CASES[name] for name in ALL250) if c.stages[0][0] == 5]
    assert any(c.tp < c.stages[0][1] and any(k < c.tp for k in c.checkpoints[:-1]) for c in tp)
    for c in tp:
        assert c.two_point
    assert any(k < len(log) and log[k - 1].kind == 2 and log[k - 1].branch == "reset" and log[k - 1].since >= 2
               for name, _, log in runs for k in R.CASES[name].checkpoints)
    # model scalars
    scal = ("mass", "fbeta", "s_noe", "k_bond", "b0", "k_ang", "a0", "k_rep", "r0_rep")
    full = [c for c in R.CASES.values() if all(k in c.model for k in scal)]
    assert any(c.pot == 4 and not c.gen for c in full) and any(c.pot == 3 and c.model.get("rswitch") == 1.0 for c in full)
    assert any(c.gen and c.pot == 1 for c in full)
    assert {c.model.get("rep_sep") for c in R.CASES.values()} >= {1, 3}
    # stage weights
    st = [s for c in R.CASES.values() for s in c.stages]
    assert any(s[4] == 0.0 for s in st) and any(0.0 < s[3] <= 1e-4 for s in st)
    # the shorter window that stands in at 1100 beads cuts some beads and holds dt at dt_max
    for slot in (0, 1):
        log = R.reference("fire_partial_cap_short", 1100, slot)[2]
        assert sum(1 for s in log if 0 < s.ncap < 1100) >= 5 and sum(1 for s in log if s.branch == "cap") >= 2, slot


@pytest.mark.parametrize("name,n", CASE_SIZES)
def test_case_is_one_float32_can_follow(built, name, n):
    """Conditioning and margins: the twin with coordinates and velocities rounded to float32 after every step takes the same branches and
    ends within a quarter of the GPU tolerance at every checkpoint; every FIRE power test after a run's first two steps has
    |cos| >= 1e-3, every two-point test a margin >= 1e-3."""
    case = R.CASES[name]
    for slot in (0, 1):
        ref, r32 = R.reference(name, n, slot), R.reference(name, n, slot, True)
        assert [(s.branch, s.ncap > 0) for s in ref[2]] == [(s.branch, s.ncap > 0) for s in r32[2]], slot
        g = R.gap(ref, r32, case)
        assert g <= 0.25, (slot, g)
        for s in ref[2]:
            if s.kind == 2 and s.since >= 2:
                assert abs(s.margin) >= 1e-3, (slot, s.it, s.margin)
            if s.kind == 5 and s.margin is not None:
                assert abs(s.margin) >= 1e-3, (slot, s.it, s.margin)
        print(f"{name} n={n} slot {slot}: float32 probe {g:.3f} of the tolerance")


@pytest.mark.parametrize("mut", sorted(R.MUTATIONS))
def test_every_mutation_is_caught(built, mut):
    """Sensitivity: some case ends at least 10 GPU tolerances from its mutated twin, in the coordinates or velocities of a checkpoint."""
    worst = {}
    for name in ALL250:
        case = R.CASES[name]
        worst[name] = max(R.gap(R.reference(name, 250, slot), R.reference(name, 250, slot, False, mut), case) for slot in (0, 1))
    best = max(worst, key=worst.get)
    print(f"{mut} ({R.MUTATIONS[mut]}): {best} ends {worst[best]:.0f} tolerances away")
    assert worst[best] >= 10.0, worst


def test_gradient_exit_has_a_predictable_step(built):
    """The exit test of a final FIRE stage (RMS force below gtol, looked at every check_every steps): the case has two consecutive checks
    whose largest-over-replicas RMS forces differ by at least 10 %, the first of them above every earlier one's geometric mean."""
    gtol, stop = R.gradient_exit("fire_resets", 250)
    assert 0 < stop < R.GTOL_STAGE[1] and stop % R.GTOL_CHECK_EVERY == 0 and gtol > 0


def test_lbfgs_first_length_without_mass_is_caught(built):
    """The L-BFGS case of the GPU test (dt_start, max_step, mass off default): the restatement with a first length without / mass ends
    more than ten of its tolerances (1e-2 A after 20 steps at 250 beads, tests/test_gpu_lbfgs.py) away."""
    n = 250
    case = R.LBFGS_CASE
    _, fire, om, of = R.models(case, n)
    d10 = R.problem(n)[1]
    x0 = R.start_of(case, n, 0).astype(np.float64)
    force = lambda u: O.energy_force(om, d10, u, 1.0, 1.0, 0.85)[0]
    xa, _ = L.lbfgs_run(force, x0, case.nsteps, m=R.LBFGS_MEMORY, g0=L.gamma0(om, of), max_step=float(of.max_step))
    xb, _ = L.lbfgs_run(force, x0, case.nsteps, m=R.LBFGS_MEMORY, g0=L.gamma0(om, of) * float(om.mass), max_step=float(of.max_step))
    assert np.abs(xa - xb).max() > 10 * 1e-2, np.abs(xa - xb).max()
