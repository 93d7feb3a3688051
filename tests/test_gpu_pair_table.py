"""The pair term, pair by pair: the tables of tests/pair_cases.py (admitted on the CPU by tests/test_pair_cases.py) through every form that
evaluates a pair term, each held to the oracle on the coordinates rounded to the type under test, component by component, within a bound
formed from the row's own term scales BEFORE anything ran (tests/pair_ref.py; profiles/r34_pair_table.md has the count of roundings):

    fp32   |F_c - Fo_c| <= 32 x 2^-24 x sum_terms scale |x_ic - x_jc|  +  the guard's share, scale x min(1, 1e-12 / (2 r^2))
    fp64   |F_c - Fo_c| <= 1e-11 x the same sum (the suite's fp64 force cap, on the row's own scale instead of the replica's max|F|)

The guard's share is a property of the fp32 form, not an error: the pair loop adds 1e-12 to r^2 inside its fma chain where the oracle
clamps r^2 at 1e-12, so a pair 1e-4 A apart is evaluated at a distance 5e-5 (relative) longer.  Rows that must feel nothing — pairs without
a target under a zero repel weight, the "no restraint = a target of 1e30 / 1e300" convention — are asserted == 0; no output may be NaN or
inf.  Forms:
  fp32  the forces hook at eval_rows_per_wave 4, 2 and -2 (2 against -2 in the same bits; energies against the oracle's at rtol 1e-7 of
        the sum of |terms|); k_step at 1, 2 and 4 rows a wave through the velocity slot of a kind-6 step; k_lbfgs_eval (kind 9);
        k_cluster_tp (kind 6, resident 1, resident_min_ops 1) where the planner has a geometry (not for a general tail; potentials 0-2
        at 250 only); the symmetric tiles (clamp forms); at 1100 the shipped potential's wide form (pair_targets 1), k_step streaming the
        targets (pair_targets 0) and column_chunk 256, the other potentials k_step at two rows a wave.  The launch forms among themselves
        in the same bits (the symmetric tiles sum in another order: bounds only).
  fp64  c3d_eval_f64 (energies at the 1e-11 cap), k64_step (kind 6) and k64_lbfgs_eval (kind 9) through c3d_get_velocities_f64, both held
        to the bound, k64_lbfgs_eval also asserted in the hook's bits (the relation the project documents; k64_step's is not documented
        and not asserted); at 1100 staged and with f64_column_chunk 256.
Exact zeros: under the stage's w_vdw = 0 in every form; with k_rep = 0 in the MODEL through hook form 4 and c3d_eval_f64 only.
k_cluster: one kind-3 step, see the last test.
Every run asserts the kernel's name.  Measured worst fractions of the bounds: profiles/r34_pair_table.md."""
import functools

import numpy as np
import pytest

from tests import pair_cases as C
from tests import pair_ref as R
from tests.util import oracle_model_from

pytestmark = pytest.mark.gpu

E_RTOL32, E_CAP64 = 1e-7, 1e-11
DEFAULTS32 = dict(resident=-1, rows_per_wave=2, symmetric=0, column_chunk=0, pair_targets=1, resident_min_ops=4, eval_rows_per_wave=4)
CASES = [("a", v, n) for n in C.SIZES for v in C.A_VARIANTS] + [("b", v, n) for n in C.SIZES for v in C.B_VARIANTS]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ctx64():
    from chromosome3d_amd import Solver
    s = Solver(0)
    for key, val in (("f64_lbfgs", 1), ("precision", 64)):
        s.set_option(key, val)
    yield s
    s.close()


def f32(*v):
    return tuple(float(np.float32(a)) for a in v)


def tf(b):
    return "true" if b else "false"


def _model(kind, variant, **more):
    if kind == "a":
        return C.model_a(variant, **more)
    return C.model_b(variant), 4, False


@functools.lru_cache(maxsize=4)
def _expected(kind, variant, n, precision):
    """per weight set: [(oracle force, oracle energies, bound [n, 3], sums of |energy terms|)] per replica; the table; the rows that feel nothing
    under a zero repel weight (table A's pairs without a target)"""
    from oracle import oracle as O
    m, _, _ = _model(kind, variant)
    T = C.table_for(kind, n, m, precision)
    P, om = R.params_from(m), oracle_model_from(m, n)
    out = {}
    for w in C.WEIGHTS:
        rows = []
        for r in range(T["x"].shape[0]):
            x = T["x"][r].astype(np.float64)
            Fo, eo = O.energy_force(om, T["t10"], x, *f32(*w))
            ref = R.energy_force(P, T["t10"], x, *f32(*w), guard=R.GUARD32 if precision == 32 else R.GUARD64)
            rows.append((Fo, np.array(eo), R.force_bound(ref, precision), np.array(ref["abs_e"]), ref["guard_part"]))
        out[w] = rows
    none = np.array(T["none"] + [p + n // 2 for p in T["none"]]) if kind == "a" else np.zeros(0, dtype=int)
    return out, T, none


class Book:
    """collects every form's worst fraction of its bound and every miss, so that one run shows the whole table"""

    def __init__(self, label):
        self.label, self.misses, self.worst = label, [], {}

    def forces(self, form, w, F, rows, none):
        F = np.asarray(F, dtype=np.float64)
        if not np.isfinite(F).all():
            self.misses.append((form, w, "non-finite force", int((~np.isfinite(F)).sum())))
            return
        frac = rounding = 0.0
        for r, (Fo, _, bound, _, guard) in enumerate(rows):
            diff = np.abs(F[r] - Fo)
            bad = diff > bound
            if bad.any():
                i, c = np.argwhere(bad)[0]
                self.misses.append((form, w, "replica %d: %d components outside the bound, first bead %d component %d: %.9g against %.9g, bound %.3g"
                                    % (r, int(bad.sum()), i, c, F[r][i, c], Fo[i, c], bound[i, c])))
            with np.errstate(divide="ignore", invalid="ignore"):
                frac = max(frac, float(np.nanmax(np.where(diff > 0, diff / bound, 0.0))))
                # where the guard's share is under 1 % of the bound the fraction is rounding alone (elsewhere the guard's systematic
                # shift, which the bound states outright, fills most of it)
                rounding = max(rounding, float(np.nanmax(np.where((diff > 0) & (guard <= 0.01 * bound), diff / bound, 0.0))))
            if w[1] == 0.0 and len(none) and (F[r][none] != 0).any():
                self.misses.append((form, w, "replica %d: a pair without a target feels %.3g under a zero repel weight" % (r, float(np.abs(F[r][none]).max()))))
        self.worst[(form, w[0])] = frac
        self.worst[(form + " rounding", w[0])] = rounding

    def energies(self, form, w, e, rows, rtol):
        frac = 0.0
        for r, (_, eo, _, scale, _) in enumerate(rows):
            if not np.isfinite(e[r]).all():
                self.misses.append((form, w, "replica %d: non-finite energy" % r))
                continue
            tol = rtol * scale
            if (np.abs(e[r] - eo) > tol).any():
                self.misses.append((form, w, "replica %d: energies %s against %s (sums of |terms| %s)" % (r, e[r], eo, scale)))
            frac = max(frac, float(np.max(np.where(scale > 0, np.abs(e[r] - eo) / np.maximum(tol, 1e-300), 0.0))))
        self.worst[(form + " energy", w[0])] = frac

    def same_bits(self, what, a, b):
        if not np.array_equal(np.asarray(a), np.asarray(b)):
            self.misses.append((what, "not the same bits: %d values differ" % int((np.asarray(a) != np.asarray(b)).sum())))

    def close(self):
        for key, frac in sorted(self.worst.items()):
            print("FRAC %s %s w_all %.1f: %.3f of the bound" % (self.label, key[0], key[1], frac))
        assert not self.misses, "%s: %d misses:\n" % (self.label, len(self.misses)) + "\n".join(str(m) for m in self.misses[:40])


def _step_force(s, T, m, kind_of_stage, w, opts, precision=32):
    """the force a step kernel evaluates, read from the velocity slot after the FIRST step of a two-point (5) or L-BFGS (8) stage with
    the float weights w; (force, kernel name, cluster launches of that step)"""
    from chromosome3d_amd import make_stages
    for k, v in opts.items():
        s.set_option(k, v)
    s.set_schedule(make_stages([(kind_of_stage, 4, 0.0) + tuple(w) + (0.0,)]))
    s.init_replicas(T["x"].shape[0], 82364, 0)
    (s.set_coords64 if precision == 64 else s.set_coords)(T["x"])
    c0 = s.stat("cluster_launches")
    assert s.run_steps(1) == 1
    v = s.velocities64() if precision == 64 else s.velocities()
    return v, s.step_kernel_name, s.stat("cluster_launches") - c0


@pytest.mark.parametrize("kind,variant,n", CASES)
def test_fp32_forms_hold_every_pair_term_to_the_oracle(solver, kind, variant, n):
    from chromosome3d_amd import default_model, make_stages
    s = solver
    m, pot, gen = _model(kind, variant)
    want, T, none = _expected(kind, variant, n, 32)
    book = Book(f"{kind} {variant} {n} fp32")
    nc = tf(n == 328)
    try:
        s.set_model(m)
        s.set_restraints(n, T["ri"], T["rj"], T["rt10"])
        if kind == "b":       # table C: the listed pairs closer than min_sep are not counted, and (below) not felt by any form
            assert s.num_restraints == len(T["ri"]) - len(T["listed_close"]) > 0
        else:
            assert s.num_restraints == len(T["ri"])
        s.set_schedule(make_stages([(5, 4, 0.0) + C.STAGE + (0.0,)]))
        s.init_replicas(T["x"].shape[0], 82364, 0)
        s.set_coords(T["x"])
        # the forces hook
        hook = {}
        for form in (4, 2, -2):
            s.set_option("eval_rows_per_wave", form)
            for w in C.WEIGHTS:
                F, e = s.eval(*w)
                hook[(form, w)] = F
                book.forces(f"hook {form}", w, F, want[w], none)
                book.energies(f"hook {form}", w, e, want[w], E_RTOL32)
        for w in C.WEIGHTS:
            book.same_bits(f"hook 2 against -2, w_all {w[0]}", hook[(2, w)], hook[(-2, w)])
        s.set_option("eval_rows_per_wave", 4)
        if kind == "a":       # the exact zeros once more with the repel term off in the model (k_rep = 0)
            m0, _, _ = _model(kind, variant, k_rep=0.0)
            s.set_model(m0)
            F, _ = s.eval(*C.STAGE)
            if not (np.isfinite(F).all() and (F[:, none] == 0).all()):
                book.misses.append(("hook 4, k_rep 0", "a pair without a target feels a force", float(np.abs(F[:, none]).max())))
            s.set_model(m)
        # the launch forms: (name, stage kind, options, kernel name or its beginning, multi-step launch?)
        forms = []
        if n <= 328:
            for rpw in (1, 2, 4):
                forms.append((f"k_step {rpw}", 5, dict(resident=0, rows_per_wave=rpw), f"c3d::k_step<{pot}, {tf(gen)}, {rpw}, {nc}, 8, false>", False))
            forms.append(("k_lbfgs_eval", 8, dict(resident=0, rows_per_wave=2), f"c3d::k_lbfgs_eval<{pot}, {tf(gen)}, 2, {nc}, 8, false>", False))
            if not gen and (n == 250 or pot >= 3):
                forms.append(("k_cluster_tp", 5, dict(resident=1, resident_min_ops=1), f"c3d::k_cluster_tp<{pot}, ", True))
        elif pot == 4 and not gen:
            forms.append(("wide", 5, dict(resident=0), "c3d::k_step<4, false, 4, false, 16, true>", False))
            # (the wide form reads the pre-scaled pair targets: without them the step is k_step at two rows a wave, streaming the targets)
            forms.append(("pair_targets 0", 5, dict(resident=0, pair_targets=0), "c3d::k_step<4, false, 2, false, 8, false>", False))
            forms.append(("column_chunk 256", 5, dict(resident=0, column_chunk=256), "c3d::k_step_chunked<4, false, 4, 16, true, 256>", False))
            forms.append(("k_lbfgs_eval wide", 8, dict(resident=0), "c3d::k_lbfgs_eval<4, false, 4, false, 16, true>", False))
        else:
            forms.append(("k_step 2", 5, dict(resident=0, rows_per_wave=2), f"c3d::k_step<{pot}, {tf(gen)}, 2, ", False))
            forms.append(("k_lbfgs_eval", 8, dict(resident=0, rows_per_wave=2), f"c3d::k_lbfgs_eval<{pot}, {tf(gen)}, 2, ", False))
        if not gen:
            forms.append(("symmetric tiles", 5, dict(resident=0, symmetric=1), f"c3d::k_pairs_sym<{pot}, {tf(m.rswitch == 1.0)}, false>", False))
        first = {}
        for name, stage_kind, opts, kernel, multi in forms:
            for w in C.WEIGHTS:
                F, ran, launches = _step_force(s, T, m, stage_kind, w, opts)
                for k in opts:
                    s.set_option(k, DEFAULTS32[k])
                if not ran.startswith(kernel) or (launches > 0) != multi:
                    book.misses.append((name, w, "ran %s (%d multi-step launches), expected %s" % (ran, launches, kernel)))
                    continue
                book.forces(name, w, F, want[w], none)
                if name != "symmetric tiles":       # the launch forms of one step kind among themselves
                    if (stage_kind, w) in first:
                        book.same_bits(f"{name} against {first[(stage_kind, w)][0]}, w_all {w[0]}", F, first[(stage_kind, w)][1])
                    else:
                        first[(stage_kind, w)] = (name, F)
        book.close()
    finally:
        for k, v in DEFAULTS32.items():
            s.set_option(k, v)
        s.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]))
        s.set_model(default_model())


def _newton_figures(label, T, m, F, rows, w_all):
    """Prints what the rows that isolate them say about pair64's d and 1 / D (profiles/r34_pair_table.md).  `zero` regime: d = t to a
    step, the force is -2 w S (1 - t / d) dx and an error of d shows as 2 w S (dd / d) dx.  `small` regime of the fast soft lower side
    (d << t, D = t - d beyond mrswitch): the force is w S mrs^4 / (D^3 d) dx, D carries none of d's error, and the force's relative
    error is three times 1 / D's plus that of 1 / d."""
    h = T["half"]
    partner = np.concatenate([np.arange(h) + h, np.arange(h)])
    idx = np.arange(2 * h)
    t = 0.1 * T["t10"][idx, partner]
    for r, name in ((0, "zero"), (3, "small")):
        x = T["x"][r]
        dv = np.abs(x - x[partner])
        d = np.sqrt((dv * dv).sum(1))
        pick = (t > 0) & (d > 1.0) if name == "zero" else (t - d > m.mrswitch) & (d > 0) & (m.noe_pot == 3) & (m.msoexp == 2) & (m.masym == 0)
        if not np.any(pick):
            continue
        err = np.abs(F[r] - rows[r][0])
        with np.errstate(divide="ignore", invalid="ignore"):
            if name == "zero":
                rel = np.where(dv > 0, err / (2.0 * w_all * m.s_noe * dv), 0.0)[pick]
            else:
                rel = np.where(np.abs(rows[r][0]) > 0, err / np.abs(rows[r][0]), 0.0)[pick]
        print("NEWTON %s %s: relative error of %s at most %.3e (%d rows)" % (label, name, "d" if name == "zero" else "the force (3 x that of 1/D + that of 1/d)", float(rel.max()), int(np.sum(pick))))


@pytest.mark.parametrize("kind,variant,n", CASES)
def test_fp64_forms_hold_every_pair_term_to_the_oracle(ctx64, kind, variant, n):
    from chromosome3d_amd import make_stages
    s = ctx64
    m, pot, gen = _model(kind, variant)
    want, T, none = _expected(kind, variant, n, 64)
    book = Book(f"{kind} {variant} {n} fp64")
    try:
        s.set_model(m)
        s.set_restraints(n, T["ri"], T["rj"], T["rt10"])
        for chunk in ((0, 256) if n == 1100 else (0,)):
            s.set_option("f64_column_chunk", chunk)
            label = f"chunk {chunk}"
            s.set_schedule(make_stages([(5, 4, 0.0) + C.STAGE + (0.0,)]))
            s.init_replicas(T["x"].shape[0], 82364, 0)
            s.set_coords64(T["x"])
            hook = {}
            for w in C.WEIGHTS:
                F, e = s.eval64(*f32(*w))
                hook[w] = F
                book.forces(f"c3d_eval_f64, {label}", w, F, want[w], none)
                book.energies(f"c3d_eval_f64, {label}", w, e, want[w], E_CAP64)
                if kind == "a" and w == C.WEIGHTS[1] and chunk == 0:      # (repel weight 0: the NOE term alone)
                    _newton_figures(book.label, T, m, F, want[w], float(np.float32(w[0])))
            if kind == "a" and chunk == 0:
                m0, _, _ = _model(kind, variant, k_rep=0.0)
                s.set_model(m0)
                F, _ = s.eval64(*f32(*C.STAGE))
                if not (np.isfinite(F).all() and (F[:, none] == 0).all()):
                    book.misses.append(("c3d_eval_f64, k_rep 0", "a pair without a target feels a force", float(np.abs(F[:, none]).max())))
                s.set_model(m)
            tail = f"_chunked<{pot}, {tf(gen)}, %s, {chunk}>" if chunk else f"<{pot}, {tf(gen)}, %s>"
            for name, stage_kind, kernel in (("k64_step", 5, "c3d::k64_step"), ("k64_lbfgs_eval", 8, "c3d::k64_lbfgs_eval")):
                for w in C.WEIGHTS:
                    F, ran, _ = _step_force(s, T, m, stage_kind, w, {}, precision=64)
                    if ran != kernel + tail % tf(pot == 4 and not gen):
                        book.misses.append((name, label, w, "ran " + ran))
                        continue
                    book.forces(f"{name}, {label}", w, F, want[w], none)
                    if stage_kind == 8:                # (documented: the hook's force has the bits of the force a kind-9 step leaves)
                        book.same_bits(f"{name} against c3d_eval_f64, {label}, w_all {w[0]}", F, hook[w])
        book.close()
    finally:
        s.set_option("f64_column_chunk", 0)
        s.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]))


# every case for which the planner gives k_cluster a geometry: the clamp forms of A at 250, potentials 3 / 4 of A at 328 (a narrow last
# block: potentials 0-2 have none there), B (the shipped potential; k_cluster's own chain pass, take-back, rep_sep edges, listed pairs) at
# 250 and 328; none at 1100
KIND3_CASES = ([("a", v, 250) for v in C.A_VARIANTS if not v.startswith("gen")] + [("a", v, 328) for v in ("shipped", "pot3_clamp", "pot3_rs1")]
               + [("b", v, n) for n in (250, 328) for v in C.B_VARIANTS])


@pytest.mark.parametrize("kind,variant,n", KIND3_CASES)
def test_k_cluster_takes_one_fire_step_in_k_steps_bits_on_the_oracles_force(solver, O, kind, variant, n):
    """k_cluster leaves no force behind, so it is held through ONE kind-3 step (the first step of a FIRE stage, resident 1, resident_min_ops
    1): coordinates and velocities in the bits of k_step's step, and k_step's held to the oracle's step.  The oracle's first FIRE step
    halves dt (no power yet), leaves v = f Fo with f = dt 418.4 / mass, dt = dt_start f_dec, and moves a bead by dt v, capped at max_step
    (asserted here against O.run_schedule, which centres its result: equal up to one shift).  Bounds, from the force's:
      v    f bound_F + 4 roundings of v
      x    not capped: dt times v's bound; capped (the move is max_step v / |v|): max_step (dv_c + |v_c| |dv| / |v|) / |v|, plus 8
           roundings of max_step for the scale; either way plus 2 roundings of x' and 4 of the move (rows within 1e-4 of the cap's edge
           take the larger of the two)."""
    from chromosome3d_amd import default_fire, default_model, make_stages
    from tests.util import oracle_fire_from
    s = solver
    m, pot, gen = _model(kind, variant)
    want, T, none = _expected(kind, variant, n, 32)
    fire = default_fire()
    stage = (2, 4, 0.0) + C.STAGE + (0.0,)
    nc = tf(n == 328)
    out = {}
    try:
        s.set_model(m)
        s.set_restraints(n, T["ri"], T["rj"], T["rt10"])
        for name, opts in (("k_step", dict(resident=0)), ("k_cluster", dict(resident=1, resident_min_ops=1))):
            for k, v in opts.items():
                s.set_option(k, v)
            s.set_schedule(make_stages([stage]), fire)
            s.init_replicas(T["x"].shape[0], 82364, 0)
            s.set_coords(T["x"])
            c0 = s.stat("cluster_launches")
            assert s.run_steps(1) == 1
            out[name] = (s.coords(), s.velocities(), s.step_kernel_name, s.stat("cluster_launches") - c0)
        assert out["k_step"][2] == f"c3d::k_step<{pot}, false, 2, {nc}, 8, false>" and out["k_step"][3] == 0, out["k_step"][2:]
        assert out["k_cluster"][2].startswith(f"c3d::k_cluster<{pot}, ") and out["k_cluster"][3] >= 1, out["k_cluster"][2:]
        assert np.array_equal(out["k_step"][0], out["k_cluster"][0]) and np.array_equal(out["k_step"][1], out["k_cluster"][1])
        dt, ms = float(fire.dt_start) * float(fire.f_dec), float(fire.max_step)
        f = dt * 418.4 / float(m.mass)
        om, of = oracle_model_from(m, n), oracle_fire_from(fire)
        x, v = out["k_step"][0].astype(np.float64), out["k_step"][1].astype(np.float64)
        assert np.isfinite(v).all() and np.isfinite(x).all()
        worst_v = worst_x = 0.0
        for r, (Fo, _, bound, _, _) in enumerate(want[C.STAGE]):
            x0 = T["x"][r].astype(np.float64)
            xo, vo, evals = O.run_schedule(om, T["t10"], O.make_stages([(2, 1, 0.0) + f32(*C.STAGE) + (0.0,)]), of, 82364, r, x0=x0)
            assert evals == 1 and np.abs(vo - f * Fo).max() <= 1e-9 * np.abs(vo).max()
            # the one-step restatement on the oracle's velocity, tied to the oracle's own step
            move = dt * vo
            length = np.sqrt((move * move).sum(1, keepdims=True))
            capped = length > ms
            xe = x0 + np.where(capped, ms / np.maximum(length, 1e-300), 1.0) * move
            shift = xo - xe
            assert np.abs(shift - shift.mean(0)).max() <= 1e-9 * max(1.0, np.abs(x0).max()), (kind, variant, n, r)
            tol_v = f * bound + 4.0 * R.EPS32 * np.abs(vo)
            vn = np.maximum(np.sqrt((vo * vo).sum(1, keepdims=True)), 1e-300)
            plain = dt * tol_v
            at_cap = ms * (tol_v + np.abs(vo) * np.sqrt((tol_v * tol_v).sum(1, keepdims=True)) / vn) / vn + 8.0 * R.EPS32 * ms
            near = np.abs(length / ms - 1.0) < 1e-4
            tol_x = np.where(near, np.maximum(plain, at_cap), np.where(capped, at_cap, plain)) + R.EPS32 * (2.0 * np.abs(xe) + 4.0 * np.abs(xe - x0))
            assert (np.abs(v[r] - vo) <= tol_v).all(), (kind, variant, n, r, "v", float((np.abs(v[r] - vo) / np.maximum(tol_v, 1e-300)).max()))
            assert (np.abs(x[r] - xe) <= tol_x).all(), (kind, variant, n, r, "x", float((np.abs(x[r] - xe) / np.maximum(tol_x, 1e-300)).max()))
            with np.errstate(divide="ignore", invalid="ignore"):
                worst_v = max(worst_v, float(np.nanmax(np.where(vo != v[r], np.abs(v[r] - vo) / tol_v, 0.0))))
                worst_x = max(worst_x, float(np.nanmax(np.where(xe != x[r], np.abs(x[r] - xe) / tol_x, 0.0))))
        print("FRAC %s %s %d fp32 kind-3 step w_all 1.0: v %.3f, x %.3f of the bound (%d beads capped in the last replica)" % (kind, variant, n, worst_v, worst_x, int(capped.sum())))
    finally:
        for k, val in DEFAULTS32.items():
            s.set_option(k, val)
        s.set_schedule(make_stages([(2, 1, 0.0, 1.0, 1.0, 0.85, 0.0)]))
        s.set_model(default_model())
