"""The step controller (thermostat, FIRE, two-point step length, per-bead step cap) and the scalars the host derives from c3d_model and
c3d_fire_params, held to the oracle in every branch: the cases of tests/controller_ref.py — admitted on the CPU by
tests/test_controller_ref.py: each takes the branches it is for, float32 can follow it, its decisions have margins, and a subtly wrong
controller ends ten tolerances away — through every launch form, against the twin (which is the oracle, to 1e-10) at every checkpoint.

Forms: at 250 beads the multi-step kernels (k_cluster / k_cluster_tp), k_step at rows_per_wave 1, 2 and 4, the symmetric tiles and
k64_step; at 1100 beads the wide form with pair targets, column_chunk 256 and k64_step_chunked (f64_column_chunk 256).  A general tail has
no multi-step and no symmetric form.  Tolerances are the suite's: fp32 2e-3 A (5e-3 A once two-point steps are in the range), velocities
2e-3 max(1, max|v|), fp64 2e-5 A / 2e-5 max(1, max|v|); at a checkpoint of Case.vrel the velocities are held to 2e-3 max|v| itself.
Measured gaps: profiles/r25_controller_branches.md (every case leaves at least a factor 4)."""
import numpy as np
import pytest

from tests import controller_ref as R
from tests import lbfgs_ref as L
from tests.util import load_if, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

# form -> (options, precision); every option is put back to DEFAULTS afterwards
FORMS = {
    250: {"multi": dict(resident=1), "step1": dict(resident=0, rows_per_wave=1), "step2": dict(resident=0, rows_per_wave=2),
          "step4": dict(resident=0, rows_per_wave=4), "sym": dict(resident=0, symmetric=1), "f64": dict(precision=64)},
    1100: {"wide": {}, "chunk256": dict(column_chunk=256), "f64chunk": dict(precision=64, f64_column_chunk=256)},
}
DEFAULTS = dict(precision=32, resident=-1, rows_per_wave=2, symmetric=0, column_chunk=0, f64_column_chunk=0, final_minimiser_steps=1000,
                replica_groups=2, use_graph=1)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _tf(b):
    return "true" if b else "false"


def _forms(case, n):
    return [f for f in FORMS[n] if not (case.gen and f in ("multi", "sym"))]


def _kernel(case, m, n, form):
    """the kernel name after the case's last range in the form (every case ends on a stage with restraint weight)"""
    pot, gen = case.pot, case.gen
    if form == "multi":
        return f"c3d::k_cluster<{pot}, "
    if form.startswith("step"):
        return f"c3d::k_step<{pot}, {_tf(gen)}, {form[-1]}, false, 8, false>"
    if form == "sym":
        return f"c3d::k_pairs_sym<{pot}, {_tf(float(m.rswitch) == 1.0)}, false>"
    if form == "wide":
        return "c3d::k_step<4, false, 4, false, 16, true>" if pot == 4 else f"c3d::k_step<{pot}, {_tf(gen)}, 2, false, 8, false>"
    if form == "chunk256":
        return "c3d::k_step_chunked<4, false, 4, 16, true, 256>" if pot == 4 else f"c3d::k_step_chunked<{pot}, {_tf(gen)}, 2, 8, false, 256>"
    tail = f"{pot}, {_tf(gen)}, {_tf(pot == 4 and not gen)}"
    return f"c3d::k64_step<{tail}>" if form == "f64" else f"c3d::k64_step_chunked<{tail}, 256>"


def _run(solver, case, n, form, stages=None, gtol=0.0, check_every=250):
    """the case in the form: [(steps, coords, velocities, kernel name, cluster launches, step launches)] per checkpoint"""
    from chromosome3d_amd import make_stages
    m, fire, _, _ = R.models(case, n)
    opts = dict(FORMS[n][form], final_minimiser_steps=case.tp)
    try:
        for k, v in opts.items():
            solver.set_option(k, v)
        solver.set_model(m)
        solver.set_if_matrix(R.problem(n)[0])
        solver.set_schedule(make_stages(stages or case.stages), fire, gtol, check_every)
        solver.init_replicas(2, R.SEED, case.first)
        solver.set_coords(np.stack([R.start_of(case, n, slot) for slot in (0, 1)]))
        if gtol > 0.0:
            return solver
        out, done = [], 0
        for k in case.checkpoints:
            c0, s0 = solver.stat("cluster_launches"), solver.stat("step_launches")
            assert solver.run_steps(k - done) == k - done
            done = k
            out.append((k, solver.coords(), solver.velocities(), solver.step_kernel_name, solver.stat("cluster_launches") - c0,
                        solver.stat("step_launches") - s0))
        return out
    finally:
        if gtol == 0.0:
            _restore(solver)


def _restore(solver):
    for k, v in DEFAULTS.items():
        solver.set_option(k, v)


def _gaps(case, n, out, precision):
    """(coordinate gap, velocity gap) in units of the tolerance, worst checkpoint and slot, against the twin"""
    gx = gv = 0.0
    tol_v = 2e-5 if precision == 64 else 2e-3
    for k, x, v, *_ in out:
        for slot in (0, 1):
            xo, vo = R.reference(case_name(case), n, slot)[3][k]
            xc = x[slot].astype(np.float64)
            vmax = np.abs(vo).max()
            gx = max(gx, np.abs(xc - xc.mean(0) - xo).max() / case.tol(precision))
            gv = max(gv, np.abs(v[slot] - vo).max() / (tol_v * (vmax if k in case.vrel else max(1.0, vmax))))
    return float(gx), float(gv)


def case_name(case):
    return next(k for k, c in R.CASES.items() if c is case)


@pytest.mark.parametrize("name,n", [(name, n) for name in R.CASES for n in R.SIZES[name]])
def test_controller_case_follows_the_oracle_in_every_form(solver, O, name, n):
    """One case of the table at one size through every form that takes it: the form is asserted by kernel name and launch counters, every
    checkpoint is held to the twin in coordinates and velocities, and the fp32 forms that share a summation order (all but the symmetric
    tiles) end every checkpoint in the same bits.  Measured worst over all cases and forms: coordinates 0.19 of the tolerance (the fp64
    forms at 1100 beads: the float read-back's half ulp at 32-64 A; fp32 0.05), velocities 0.14 (off_default, 250 beads)."""
    case = R.CASES[name]
    m = R.models(case, n)[0]
    runs = {}
    for form in _forms(case, n):
        out = runs[form] = _run(solver, case, n, form)
        f64 = form.startswith("f64")
        kname, cl = out[-1][3], sum(o[4] for o in out)
        want = _kernel(case, m, n, form)
        assert kname.startswith(want) if form == "multi" else kname == want, (form, kname, want)
        if form == "multi":                        # every op of every range in a multi-step launch: none fell back to k_step
            assert all(o[4] >= 1 and o[5] == 0 for o in out), (form, [(o[4], o[5]) for o in out])
            if case.two_point:                     # the first range holds two-point steps alone
                assert out[0][3].startswith(f"c3d::k_cluster_tp<{case.pot}, "), out[0][3]
        else:
            assert cl == 0 and sum(o[5] for o in out) >= case.nsteps, (form, cl)
        gx, gv = _gaps(case, n, out, 64 if f64 else 32)
        print(f"GAP {name} {n} {form} {kname}: x {gx:.3f} v {gv:.3f} of the tolerance")
        assert gx < 1.0 and gv < 1.0, (form, gx, gv)
    same = [f for f in runs if f != "sym" and not f.startswith("f64")]
    for f in same[1:]:
        for a, b in zip(runs[same[0]], runs[f]):
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (same[0], f, a[0])


@pytest.mark.parametrize("form", ["multi", "step2"])
def test_gradient_exit_stops_where_the_oracle_stops(solver, O, form):
    """c3d_run with check_every 7 and gtol between the largest RMS forces of two consecutive checks (10 % apart or more) stops after exactly
    the step count c3o_run_schedule stops at, on the multi-step and on the per-step path: 14 steps, an even count of odd chunks."""
    from chromosome3d_amd import make_stages
    n, name = 250, "fire_resets"
    case = R.CASES[name]
    gtol, stop = R.gradient_exit(name, n)
    _, _, om, of = R.models(case, n)
    evs = []
    for slot in (0, 1):        # the oracle itself, not only its twin
        _, _, ev = O.run_schedule(om, R.problem(n)[1], O.make_stages([R.gtol_stage()]), of, R.SEED, slot,
                                  x0=R.start_of(case, n, slot).astype(np.float64), gtol=gtol, check_every=R.GTOL_CHECK_EVERY)
        evs.append(ev)
    assert max(evs) == stop, (evs, stop)           # (a replica alone stops at its own first check below gtol)
    try:
        s = _run(solver, case, n, form, stages=[R.gtol_stage()], gtol=gtol, check_every=R.GTOL_CHECK_EVERY)
        c0 = s.stat("cluster_launches")
        s.run()
        assert s.steps_done == stop, (s.steps_done, stop, gtol)
        assert (s.stat("cluster_launches") > c0) == (form == "multi"), form
    finally:
        solver.set_schedule(make_stages(case.stages), None, 0.0, 250)      # (gtol and check_every back to the context's defaults)
        _restore(solver)


@pytest.mark.parametrize("precision", [32, 64])
def test_lbfgs_off_default_follows_the_restatement(solver, O, precision):
    """Kind 8 with dt_start, max_step, mass and lbfgs_memory off default (the first length is dt_start^2 kAccel / mass), 20 steps at 250
    beads: fp32 within 1e-2 A of tests/lbfgs_ref.py (test_gpu_lbfgs.py's bound for 20 steps at this size), fp64 (f64_lbfgs) within the
    read-back's grain, max(2e-5, 1.2e-7 max|x|) (test_gpu_f64_lbfgs.py)."""
    from chromosome3d_amd import make_stages
    n, case = 250, R.LBFGS_CASE
    m, fire, om, of = R.models(case, n)
    d10 = R.problem(n)[1]
    x0 = np.stack([R.start_of(case, n, slot) for slot in (0, 1)])
    try:
        if precision == 64:
            solver.set_option("f64_lbfgs", 1)
            solver.set_option("precision", 64)
        solver.set_option("lbfgs_memory", R.LBFGS_MEMORY)
        solver.set_model(m)
        solver.set_if_matrix(R.problem(n)[0])
        solver.set_schedule(make_stages(case.stages), fire)
        solver.init_replicas(2, R.SEED, 0)
        solver.set_coords(x0)
        before = solver.stat("lbfgs_steps")
        assert solver.run_steps(case.nsteps) == case.nsteps and solver.stat("lbfgs_steps") - before == case.nsteps
        name = solver.step_kernel_name
        assert name.startswith("c3d::k_lbfgs_eval<4, false, 2, ") if precision == 32 else name == "c3d::k64_lbfgs_eval<4, false, true>", name
        x = solver.coords().astype(np.float64)
        _, _, _, w_all, w_vdw, repel_s, _ = case.stages[0]
        force = lambda u: O.energy_force(om, d10, u, w_all, w_vdw, repel_s)[0]
        g0 = L.gamma0(om, of) if precision == 32 else float(fire.dt_start) ** 2 * 418.4 / float(m.mass)
        for slot in (0, 1):
            xo, _ = L.lbfgs_run(force, x0[slot].astype(np.float64), case.nsteps, m=R.LBFGS_MEMORY, g0=g0, max_step=float(of.max_step))
            xo -= xo.mean(0)
            gap = float(np.abs(x[slot] - x[slot].mean(0) - xo).max())
            tol = 1e-2 if precision == 32 else max(2e-5, 1.2e-7 * float(np.abs(xo).max()))
            print(f"GAP lbfgs {n} precision {precision} slot {slot} {name}: {gap:.2e} A (tolerance {tol:.1e})")
            assert gap < tol, (slot, gap, tol)
    finally:
        solver.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]))
        solver.set_option("precision", 32)
        solver.set_option("f64_lbfgs", 0)
        solver.set_option("lbfgs_memory", 5)


# w_all, w_vdw, repel_s: the final stage's, w_vdw = 0, repel_s = 0 (rep_r2 = 0: the guard of inv_rep_r2), a hot stage's
EVAL_WEIGHTS = [(1.0, 1.0, 0.85), (1.0, 0.0, 0.85), (1.0, 1.0, 0.0), (0.4, 0.003, 0.9)]


@pytest.mark.parametrize("variant", ["off_default", "pot3_rs1_off", "gen1_off"])
def test_forces_and_energies_of_the_off_default_model(solver, O, variant):
    """c3d_eval (both of its forms) and c3d_eval_f64 with every model scalar off default, against O.energy_force at the bounds of
    test_force_energy_parity (|dF| <= 1e-5 |F| + 1e-6 max|F|, energies 1e-7 relative) and of test_gpu_f64_boundary.py (forces 8.0e-12
    (|F| + 0.1 max|F|), energies 2.5e-13 relative); coils at full size, x 0.4 and x 0.15 (pairs on both sides of every switch)."""
    from tests.test_gpu_f64_boundary import E_BOUND, F_BOUND, F32, rel_energy_gap, rel_force_gap
    n, case = 250, R.CASES[variant]
    m, _, om, _ = R.models(case, n)
    d10 = R.problem(n)[1]
    x = np.stack([random_coil(n, 100 + r) * s for r, s in enumerate((1.0, 0.4, 0.15))])
    try:
        for precision in (32, 64):
            solver.set_option("precision", precision)
            solver.set_model(m)
            solver.set_if_matrix(R.problem(n)[0])
            solver.init_replicas(3, 1234, 5)
            solver.set_coords(x)
            for w in EVAL_WEIGHTS:
                wf = F32(*w)
                ref = [O.energy_force(om, d10, x[r].astype(np.float64), *wf) for r in range(3)]
                if precision == 64:
                    F, e = solver.eval64(*wf)
                    for r, (Fo, eo) in enumerate(ref):
                        gf, ge = rel_force_gap(F[r], Fo), rel_energy_gap(e[r][np.array(eo) != 0], np.array(eo)[np.array(eo) != 0])
                        assert gf <= F_BOUND and ge <= E_BOUND, (variant, w, r, gf, ge)
                        assert np.all(e[r][np.array(eo) == 0] == 0)
                    continue
                for form in (4, 2):
                    solver.set_option("eval_rows_per_wave", form)
                    F, e = solver.eval(*w)
                    for r, (Fo, eo) in enumerate(ref):
                        assert (np.abs(F[r] - Fo) <= 1e-5 * np.abs(Fo) + 1e-6 * np.abs(Fo).max()).all(), (variant, w, form, r, np.abs(F[r] - Fo).max())
                        assert np.allclose(e[r], eo, rtol=1e-7, atol=1e-6), (variant, w, form, r, e[r], eo)
    finally:
        solver.set_option("eval_rows_per_wave", 4)
        solver.set_option("precision", 32)


@pytest.mark.parametrize("cid", ["chr21_1mb", "syn300"])
@pytest.mark.parametrize("min_sep", [3, 9])
def test_min_sep_off_default(built, O, cid, min_sep):
    """min_sep 3 and 9, set before the matrix: K1's tenths and the restraint count equal O.if_to_dist10 / O.dist_to_rr(d10, min_sep), and
    c3d_score_replicas' satisfied / sum of deviations equal c3d_assess on those rows (chr21_1mb: 37 beads; 300: more than one column block)."""
    from chromosome3d_amd import default_model, make_stages, pipeline
    from chromosome3d_amd import Solver
    IF = load_if(cid) if cid.startswith("chr") else synthetic_if(int(cid[3:]), seed=int(cid[3:]))[0]
    solver = Solver(0)         # its own context: min_sep cannot be changed on one that holds targets (c3d_set_model)
    try:
        solver.set_model(default_model(min_sep=min_sep))
        d10 = pipeline.IF2dist_new(solver, IF)
        assert np.array_equal(d10, O.if_to_dist10(IF))
        ri, rj, rt = O.dist_to_rr(d10, min_sep)
        assert solver.num_restraints == len(ri) and len(ri) != len(O.dist_to_rr(d10, 5)[0])
        rows = pipeline.restraints_from_dist10(d10, min_sep)
        assert sorted(zip(rows[0], rows[1], rows[2])) == sorted(zip(ri, rj, rt))
        solver.set_schedule(make_stages([(2, 12, 0.0, 1.0, 1.0, 0.85, 0.0)]))
        solver.init_replicas(2, R.SEED, 0)
        for phase in ("coil", "moved"):
            if phase == "moved":
                assert solver.run_steps(12) == 12
            x = solver.coords()
            sat, dev, _ = solver.score()
            for r in range(2):
                hs, hd = pipeline.assess(x[r], (ri, rj, rt))
                assert sat[r] == hs and abs(dev[r] - hd) <= 1e-10 * max(1.0, abs(hd)), (phase, r, sat[r], hs, dev[r], hd)
                assert (hs, hd) != pipeline.assess(x[r], O.dist_to_rr(d10, 5)), (phase, r)
    finally:
        solver.close()


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 5, 6])
def test_step_scalars_table_equals_the_oracles_statements(solver, kind):
    """c3d_debug_step_scalars (step_scalars<true>, the function k_step, k_cluster[_tp] and k_update_sym share) on the grid of
    controller_ref.table_rows against the oracle's statements in float64: every output within 4 float ulps (rcp, rsq and sqrt are 1 ulp each,
    at most three are chained), integer state exact, NaN where the oracle has NaN.  The grid: both signs and both zeros of the deciding
    sum, npos at n_min - 1, n_min, n_min + 1, dt f_inc below, at and above dt_max, T below, at (and one float either side of) and above
    1e-2, lambda^2 below, at and above 0, two-point steps 0 .. 3 and beyond with lengths below 1e-7 and above 1e2 and the doubling out of
    both bounds, NaN sums where the oracle's comparisons define the branch (FIRE, two-point; in MD the oracle's temperature stays NaN).
    Left out: Berendsen rows that cool towards lambda^2 = 0, where 1 + dt fbeta (T0 / T - 1) cancels and no ulp bound holds."""
    from chromosome3d_amd import default_fire, default_model, make_stages
    m, fire = default_model(**R.TABLE_MODEL), default_fire(**R.TABLE_FIRE)
    solver.set_model(m)
    solver.set_if_matrix(load_if("chr21_1mb"))
    assert solver.n == R.TABLE_N
    solver.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]), fire)
    consts = R.table_consts(m, solver.n)
    rows = R.table_rows(kind, consts[0])
    by_step = {}
    for r in rows:
        by_step.setdefault(r[:2], []).append(r)
    checked = 0
    for (dt, t_bath), group in by_step.items():
        psum = np.array([g[2] for g in group], dtype=np.float32)
        state = np.array([g[3] for g in group], dtype=np.float32)
        npos = np.array([g[4] for g in group], dtype=np.int32)
        sc, so, no = solver.debug_step_scalars(kind, dt, t_bath, psum, state, npos)
        for i in range(len(group)):
            want_sc, want_st, want_n = R.step_scalars_ref(kind, dt, t_bath, psum[i], state[i], int(npos[i]), consts, fire)
            assert no[i] == want_n, (kind, group[i], no[i], want_n)
            for got, want in zip(list(sc[i]) + list(so[i]), list(want_sc) + list(want_st)):
                if np.isnan(want):
                    assert np.isnan(got), (kind, group[i], got, want)
                else:
                    tol = 4.0 * float(np.spacing(np.float32(abs(want)))) if want != 0.0 and np.isfinite(want) else 0.0
                    assert abs(float(got) - want) <= tol, (kind, group[i], float(got), want, tol)
            checked += 1
    assert checked == len(rows) >= 24
