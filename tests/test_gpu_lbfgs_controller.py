"""The L-BFGS stage's controller on the device, branch by branch: every case of tests/lbfgs_cases.py (admitted on the CPU by
tests/test_lbfgs_cases.py: rejected pairs at the start, twice in a row and in mid-run, both clamps of gamma, the cap on no, some and all
beads, wrap-around at memory 1, 2, 5 and 8, the hand-over to FIRE) through every form that takes it, against the fp64 restatement
(tests/lbfgs_ref.py) started from the very values the device holds, at every checkpoint: coordinates, the stat lbfgs_steps, the stat
lbfgs_resets (exactly the restatement's count over both replicas), and the fp32 forms in the same bits.

Forms: at 96 and 250 beads k_lbfgs_eval at rows_per_wave 1, 2 and 4 and k64_lbfgs_eval; at 1100 beads the wide form, column_chunk 256
and k64_lbfgs_eval_chunked (f64_column_chunk 256).  fp32 starts go in through c3d_set_coords, fp64 starts through c3d_set_coords_f64 and
are read back through c3d_get_coords_f64.

Bounds: 8 x the gap measured on an MI355X at that checkpoint (MEASURED, from profiles/r27_lbfgs_controller.md; the margin the fp64-boundary
tests use for re-ordered sums), never more than 1e-2 A (fp32: the suite's bound for 20 L-BFGS steps) or 1e-8 A (fp64)."""
import numpy as np
import pytest

from tests import lbfgs_cases as T

pytestmark = pytest.mark.gpu

FORMS = {
    96: {"step1": dict(resident=0, rows_per_wave=1), "step2": dict(resident=0, rows_per_wave=2), "step4": dict(resident=0, rows_per_wave=4),
         "f64": dict(precision=64, f64_lbfgs=1)},
    1100: {"wide": {}, "chunk256": dict(column_chunk=256), "f64chunk": dict(precision=64, f64_lbfgs=1, f64_column_chunk=256)},
}
FORMS[250] = FORMS[96]
DEFAULTS = dict(precision=32, f64_lbfgs=0, resident=-1, rows_per_wave=2, column_chunk=0, f64_column_chunk=0, final_minimiser_steps=1000, lbfgs_memory=5)

# (case, beads, "fp32" | "fp64") -> {checkpoint: worst gap over both replicas to the fp64 restatement, A}, measured on an MI355X
MEASURED = {
    ("wrap_m1", 250, "fp32"): {3: 1.685e-05, 12: 3.424e-04},
    ("wrap_m1", 250, "fp64"): {3: 2.558e-13, 12: 1.107e-11},
    ("wrap_m2_then_fire", 250, "fp32"): {5: 6.267e-05, 12: 1.519e-04, 20: 1.518e-04},
    ("wrap_m2_then_fire", 250, "fp64"): {5: 8.882e-13, 12: 4.579e-12, 20: 4.505e-12},
    ("wrap_m5", 96, "fp32"): {4: 7.999e-05, 24: 8.980e-04},
    ("wrap_m5", 96, "fp64"): {4: 2.540e-12, 24: 4.347e-11},
    ("wrap_m8", 250, "fp32"): {6: 7.473e-05, 30: 3.005e-04},
    ("wrap_m8", 250, "fp64"): {6: 8.615e-13, 30: 7.020e-12},
    ("wrap_m8", 1100, "fp32"): {6: 4.048e-05, 30: 3.023e-03},
    ("wrap_m8", 1100, "fp64"): {6: 5.702e-13, 30: 1.251e-11},
    ("lower_clamp", 96, "fp32"): {8: 2.881e-06, 26: 4.125e-03},
    ("lower_clamp", 96, "fp64"): {8: 3.553e-14, 26: 9.109e-11},
    ("lower_clamp", 250, "fp32"): {8: 3.341e-06, 26: 5.009e-03},
    ("lower_clamp", 250, "fp64"): {8: 1.688e-13, 26: 3.506e-11},
    ("lower_clamp_deep", 96, "fp32"): {6: 2.083e-05, 20: 7.444e-05},
    ("lower_clamp_deep", 96, "fp64"): {6: 2.345e-13, 20: 1.177e-12},
    ("lower_clamp_deep", 1100, "fp32"): {6: 2.793e-05, 20: 4.968e-04},
    ("lower_clamp_deep", 1100, "fp64"): {6: 1.672e-12, 20: 2.767e-11},
    ("upper_clamp", 96, "fp32"): {4: 1.326e-05, 20: 1.008e-05},
    ("upper_clamp", 96, "fp64"): {4: 4.192e-13, 20: 4.707e-13},
    ("upper_clamp_deep", 96, "fp32"): {4: 7.860e-06, 20: 3.821e-06},
    ("upper_clamp_deep", 96, "fp64"): {4: 2.238e-13, 20: 1.243e-13},
    ("upper_clamp_deep", 1100, "fp32"): {4: 7.011e-06, 20: 9.768e-05},
    ("upper_clamp_deep", 1100, "fp64"): {4: 1.847e-13, 20: 1.224e-12},
    ("reject_start", 96, "fp32"): {2: 4.141e-07, 3: 1.689e-06, 16: 3.965e-05},
    ("reject_start", 96, "fp64"): {2: 2.220e-15, 3: 1.243e-14, 16: 4.565e-13},
    ("reject_all_capped", 250, "fp32"): {2: 2.052e-07, 16: 4.335e-05},
    ("reject_all_capped", 250, "fp64"): {2: 1.416e-15, 16: 2.980e-13},
    ("reject_midrun", 96, "fp32"): {9: 1.325e-04, 20: 3.689e-03},
    ("reject_midrun", 96, "fp64"): {9: 7.851e-13, 20: 1.581e-11},
}


def _kernel(form, lbfgs):
    """the kernel name after a range that ended in the L-BFGS part (lbfgs) or in the FIRE part of the stage"""
    if form.startswith("step"):
        return f"c3d::k_lbfgs_eval<4, false, {form[-1]}, " if lbfgs else f"c3d::k_step<4, false, {form[-1]}, "
    if form == "wide":
        return "c3d::k_lbfgs_eval<4, false, 4, false, 16, true>"
    if form == "chunk256":
        return "c3d::k_lbfgs_eval_chunked<4, false, 4, 16, true, 256>"
    if form == "f64":
        return "c3d::k64_lbfgs_eval<4, false, true>" if lbfgs else "c3d::k64_step<4, false, true>"
    return "c3d::k64_lbfgs_eval_chunked<4, false, true, 256>"


def _run(solver, name, n, form):
    """[(steps, coordinates (float64, as read), lbfgs_steps of the range, lbfgs_resets, kernel name)] per checkpoint"""
    from chromosome3d_amd import default_model, make_stages
    case = T.CASES[name]
    m, fire, _, _ = T.models(case, n)
    opts = dict(FORMS[n][form], final_minimiser_steps=case.nl, lbfgs_memory=case.mem)
    f64 = opts.get("precision") == 64
    x0 = np.stack([T.start(name, n, slot) for slot in (0, 1)])
    try:
        for k in ("f64_lbfgs", "precision"):                   # (the option before the precision that needs it)
            if k in opts:
                solver.set_option(k, opts[k])
        for k, v in opts.items():
            solver.set_option(k, v)
        solver.set_model(m)
        solver.set_if_matrix(T.R.problem(n)[0])
        solver.set_schedule(make_stages([case.stage]), fire)
        solver.init_replicas(2, T.SEED, 0)
        if f64:
            solver.set_coords64(x0.astype(np.float64))
        else:
            solver.set_coords(x0)
        out, done = [], 0
        for k in case.checkpoints:
            before = solver.stat("lbfgs_steps")
            assert solver.run_steps(k - done) == k - done
            x = solver.coords64() if f64 else solver.coords().astype(np.float64)
            out.append((k, x, solver.stat("lbfgs_steps") - before, solver.stat("lbfgs_resets"), solver.step_kernel_name))
            done = k
        return out
    finally:
        solver.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]))
        for k in ("precision", "f64_lbfgs"):
            solver.set_option(k, DEFAULTS[k])
        for k, v in DEFAULTS.items():
            solver.set_option(k, v)
        solver.set_model(default_model())


@pytest.mark.parametrize("name,n", T.CASE_SIZES)
def test_lbfgs_case_follows_the_restatement_in_every_form(solver, name, n):
    """One case at one size through every form; see the module's docstring for what is asserted."""
    case = T.CASES[name]
    runs = {}
    for form in FORMS[n]:
        out = runs[form] = _run(solver, name, n, form)
        prec = 64 if form.startswith("f64") else 32
        refs = [T.reference(name, n, slot, precision=prec) for slot in (0, 1)]
        cap = T.CAP64 if prec == 64 else T.CAP32
        measured = MEASURED.get((name, n, f"fp{prec}"), {})
        done = 0
        for k, x, nlb, resets, kname in out:
            lb = min(k, case.nlb) - min(done, case.nlb)          # L-BFGS steps of this range
            want = _kernel(form, k <= case.nlb)
            assert nlb == lb, (form, k, nlb, lb)
            assert kname.startswith(want), (form, k, kname, want)
            want_resets = sum(sum(s.branch.count("rejected") + s.branch.count("dropped") for s in r[1][:k]) for r in refs)
            gaps = []
            for slot in (0, 1):
                xc = x[slot] - x[slot].mean(0)
                gaps.append(float(np.abs(xc - refs[slot][0][k]).max()))
            bound = min(cap, 8.0 * measured[k]) if k in measured else cap
            print(f"GAP {name} {n} {form} fp{prec} after {k}: {max(gaps):.3e} A (bound {bound:.1e}) resets {resets:.0f} / {want_resets} {kname}")
            assert resets == want_resets, (form, k, resets, want_resets)
            assert max(gaps) <= bound, (form, k, gaps, bound)
            done = k
    same = [f for f in runs if not f.startswith("f64")]
    for f in same[1:]:
        for a, b in zip(runs[same[0]], runs[f]):
            assert np.array_equal(a[1], b[1]), (same[0], f, a[0])
    assert all((name, n, p) in MEASURED for p in ("fp32", "fp64")), "no measured gap for this case: profiles/r27_lbfgs_controller.md"
