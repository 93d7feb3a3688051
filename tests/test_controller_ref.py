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


# ---------------------------------------------------------------------------------------------
# the fp64 tables (tests/test_gpu_f64_controller_table.py runs them on the device): admitted here, without one
# ---------------------------------------------------------------------------------------------
ROW_DT = 2.0 ** -9          # the MD step of the row-finish table (kinds 0, 1)


def _table64():
    from chromosome3d_amd import default_fire, default_model
    m, fire = default_model(**R.TABLE_MODEL), default_fire(**R.TABLE_FIRE)
    return R.table_consts64(m, R.TABLE_N), fire


def _scalar_hits(kind):
    from collections import Counter
    consts, fire = _table64()
    h = Counter()
    for dt, t_bath, psum, state, npos in R.table_rows64(kind, consts[0]):
        R.step_scalars_ref(kind, dt, t_bath, psum, state, npos, consts, fire, precision=64, hits=h)
    return h


def _row_hits(kind):
    from collections import Counter
    consts, fire = _table64()
    h = Counter()
    rows = R.row_finish_rows(kind, ROW_DT, consts, fire)
    for r, _ in rows:
        R.row_finish_ref(kind, ROW_DT, r, consts, fire, hits=h)
    return h, rows


def test_fp64_table_takes_every_branch(built):
    """every branch and edge the fp64 tables are there for is taken by at least one row, counted by the restatement itself"""
    for kind in (0, 1):
        h = _scalar_hits(kind)
        for name in ("T_below_floor", "T_at_floor", "T_above_floor"):
            assert h[name] >= 1, (kind, name, dict(h))
    h = _scalar_hits(0)
    for name in ("l2_below_0", "l2_at_0", "l2_above_0"):
        assert h[name] >= 1, (name, dict(h))
    for kind in (2, 3):
        h = _scalar_hits(kind)
        for name in ("fire_vf_pos", "fire_vf_zero", "fire_vf_neg", "fire_vf_nan", "fire_reset", "fire_ff", "fire_ff_floor", "fire_ff_at_floor",
                     "npos_below_nmin", "npos_at_nmin", "npos_above_nmin", "dt_grow", "dt_at_max", "dt_cap"):
            assert h[name] >= 1, (kind, name, dict(h))
    h = _scalar_hits(5)
    for name in ("bb_first", "bb_second", "bb_even", "bb_odd", "bb_negcurv", "bb_lo", "bb_lo_nan", "bb_hi", "bb_sy_pos", "bb_sy_zero", "bb_sy_neg",
                 "bb_sy_nan"):
        assert h[name] >= 1, (name, dict(h))
    assert _scalar_hits(6)["bb_first"] == len(R.table_rows64(6, _table64()[0][0]))
    for kind in (2, 3, 6):
        h, rows = _row_hits(kind)
        for name in ("move_uncapped", "move_at_cap", "move_capped"):
            assert h[name] >= 1, (kind, name, dict(h))
    h, rows = _row_hits(5)
    for name in ("move_uncapped", "move_at_cap", "move_capped", "s_uncapped", "s_at_cap", "s_capped"):
        assert h[name] >= 1, (name, dict(h))
    # kind 5: the two caps independently — each of the four combinations on some row
    from collections import Counter
    consts, fire = _table64()
    combos = set()
    for r, _ in rows:
        c = Counter()
        R.row_finish_ref(5, ROW_DT, r, consts, fire, hits=c)
        combos.add((bool(c["s_capped"]), bool(c["move_capped"])))
    assert combos == {(False, False), (False, True), (True, False), (True, True)}
    for kind in (0, 1):
        assert _row_hits(kind)[0]["md"] >= 1
    h, rows = _row_hits(4)
    assert h["md_begin"] == len(rows)
    for r, _ in rows:                                          # kind 4: v = vinit, x unchanged
        out = R.row_finish_ref(4, ROW_DT, r, consts, fire)
        assert all(a == b or (a != a and b != b) for a, b in zip(out[:6], r[:6]))


def test_fp64_table_edges_are_at_the_edge(built):
    """exact equality in float64 where a row is meant to sit at an edge, and one double either side where it is meant to sit beside it"""
    consts, fire = _table64()
    t_fac = consts[0]
    lo, at, hi = R._floor_edge(t_fac)
    assert t_fac * at == 1e-2 and t_fac * lo < 1e-2 < t_fac * hi
    assert t_fac * lo == float(np.nextafter(1e-2, 0.0)) and t_fac * hi == float(np.nextafter(1e-2, 1.0))
    xs = {r[2][0] for r in R.table_rows64(0, t_fac)}
    assert {lo, at, hi} <= xs
    # lambda^2 = 0 exactly: dt fbeta = 1 at t_bath 0; and the products of the FIRE values that are "at"
    assert 2.0 ** -8 * consts[3] == 1.0 and 1.0 + 2.0 ** -8 * consts[3] * (0.0 / 1e-2 - 1.0) == 0.0
    assert 0.03125 * float(fire.f_inc) == float(fire.dt_max)
    assert float(np.nextafter(0.03125, 0.0)) * float(fire.f_inc) < float(fire.dt_max) < float(np.nextafter(0.03125, 1.0)) * float(fire.f_inc)
    sdts = {r[3][0] for r in R.table_rows64(2, t_fac)}
    assert {float(np.nextafter(0.03125, 0.0)), 0.03125, float(np.nextafter(0.03125, 1.0))} <= sdts
    assert fire.n_min == 3 and {r[4] for r in R.table_rows64(2, t_fac)} >= {2, 3, 4}
    ffs = {r[2][1] for r in R.table_rows64(2, t_fac)}
    assert {float(np.nextafter(1e-30, 0.0)), 1e-30, float(np.nextafter(1e-30, 1.0))} <= ffs
    # two-point lengths at both bounds and one double either side
    got = set()
    for dt, t_bath, psum, state, npos in R.table_rows64(5, t_fac):
        if npos in (2, 3) and psum[0] > 0 and psum[2] == 1.0:
            a = psum[0] / psum[2] if npos % 2 else psum[3] / psum[0]
            got.add((npos % 2, a))
    for par in (0, 1):
        for b in (1e-7, 1e2):
            assert {(par, float(np.nextafter(b, 0.0))), (par, b), (par, float(np.nextafter(b, 1e3)))} <= got, (par, b)
    # the capped quantity at max_step^2 and one double either side, per kind and per cap
    ms = float(fire.max_step)
    ms2 = ms * ms
    want = {float(np.nextafter(ms2, 0.0)), ms2, float(np.nextafter(ms2, 1.0))}
    for kind in (2, 3, 5, 6):
        seen_move, seen_s = set(), set()
        for r, _ in R.row_finish_rows(kind, ROW_DT, consts, fire):
            x, v, F, lam, keep, mix, sdt = r[0:3], r[3:6], r[6:9], r[9], r[13], r[14], r[15]
            if kind in (2, 3):
                acc = sdt * consts[2]
                vn = [keep * v[k] + mix * F[k] for k in range(3)]
                vn = [vn[k] + acc * F[k] for k in range(3)]
                seen_move.add(R._d2([sdt * a for a in vn]))
            else:
                seen_move.add(R._d2([mix * a for a in F]))
                seen_s.add(R._d2([lam * a for a in v]))
        assert want <= seen_move, kind
        if kind == 5:
            assert want <= seen_s


def _rows_differ(a, b):
    """largest difference of two result rows in double ulps (inf: NaN against a number, or an integer that differs)"""
    worst = 0.0
    for g, w in zip(a, b):
        if isinstance(w, int) or isinstance(g, int):
            if g != w:
                return float("inf")
        elif (g != g) != (w != w):
            return float("inf")
        elif w == w:
            worst = max(worst, R.ulps(g, w))
    return worst


@pytest.mark.parametrize("mut", sorted(R.TABLE_MUTATIONS))
def test_fp64_table_catches_every_mutation(built, mut):
    """each mutation of the restatement moves some row of the fp64 tables by at least 1000 double ulps, or changes an integer"""
    consts, fire = _table64()
    worst = 0.0
    for kind in R.SCALAR_KINDS:
        for dt, t_bath, psum, state, npos in R.table_rows64(kind, consts[0]):
            a = R.step_scalars_ref(kind, dt, t_bath, psum, state, npos, consts, fire, precision=64)
            b = R.step_scalars_ref(kind, dt, t_bath, psum, state, npos, consts, fire, precision=64, mut=mut)
            worst = max(worst, _rows_differ(list(b[0]) + list(b[1]) + [b[2]], list(a[0]) + list(a[1]) + [a[2]]))
    from collections import Counter
    for kind in R.ROW_KINDS:
        for r, _ in R.row_finish_rows(kind, ROW_DT, consts, fire):
            ha, hb = Counter(), Counter()
            a, b = R.row_finish_ref(kind, ROW_DT, r, consts, fire, hits=ha), R.row_finish_ref(kind, ROW_DT, r, consts, fire, mut=mut, hits=hb)
            # (the row's integers: whether each cap acted.  ">=" for ">" in the cap test changes nothing else — at d2 = max_step^2 the scale
            #  max_step / sqrt(d2) is 1 to a rounding — so no table of outputs, on the CPU or on the device, can tell the two apart)
            acted = [ha["move_acted"], ha["s_acted"]], [hb["move_acted"], hb["s_acted"]]
            worst = max(worst, _rows_differ(b + acted[1], a + acted[0]))
    print(f"{mut} ({R.TABLE_MUTATIONS[mut]}): {worst:.3g} double ulps")
    assert worst >= 1000.0, worst


def test_fp64_row_restatement_is_the_oracles_step(built):
    """row_finish_ref against the oracle's own step functions through O.run_schedule: one bead cannot be run alone, so a short FIRE and a short
    two-point stage of the 37-bead model are followed bead by bead with the restatement (forces from O.energy_force) to 1e-12 A"""
    from chromosome3d_amd import default_fire, default_model
    from tests.util import load_if, oracle_fire_from, oracle_model_from
    m, fire = default_model(**R.TABLE_MODEL), default_fire(**R.TABLE_FIRE, max_step=0.01)
    IF = load_if("chr21_1mb")
    n = IF.shape[0]
    om, of, d10 = oracle_model_from(m, n), oracle_fire_from(fire), O.if_to_dist10(IF)
    consts = R.table_consts64(m, n)
    x0 = O.init_coords(om, R.SEED, 0)
    for stage_kind, nsteps in ((2, 9), (5, 9)):
        stage = (stage_kind, nsteps) + tuple(float(np.float32(a)) for a in (0.0, 1.0, 1.0, 0.85, 0.0))
        xo = O.run_schedule(om, d10, O.make_stages([stage]), of, R.SEED, 0, x0=x0)[0]
        x, v = np.array(x0, dtype=np.float64), np.zeros((n, 3))
        sums, state, npos = (0.0, 0.0, 0.0, 0.0), (float(of.dt_start), float(of.alpha_start)), 0
        capped = 0
        for it in range(nsteps):
            F = O.energy_force(om, d10, x, *stage[3:6])[0]
            kind = stage_kind if it else stage_kind + 1
            sc, state, npos = R.step_scalars_ref(kind, 0.0, 0.0, sums, state, npos, consts, fire, precision=64)
            from collections import Counter
            h = Counter()
            out = np.array([R.row_finish_ref(kind, 0.0, list(x[i]) + list(v[i]) + list(F[i]) + list(sc) + [state[0]], consts, fire, hits=h) for i in range(n)])
            capped += h["move_capped"]
            x, v = out[:, 0:3], out[:, 3:6]
            sums = tuple(out[:, 6 + k].sum() for k in range(4))
        assert capped > 0, stage_kind
        x = x - x.mean(0)
        assert np.abs(x - xo).max() < 1e-12, (stage_kind, np.abs(x - xo).max())
    # MD: the Maxwell start (kind 4: no move, the sums of its velocities), then Berendsen / rescaling steps
    for stage_kind in (0, 1):
        stage = (stage_kind, 6) + tuple(float(np.float32(a)) for a in (0.003, 0.4, 0.003, 0.9, 300.0))
        dt, t_bath = stage[2], stage[6]
        xo, vo, _ = O.run_schedule(om, d10, O.make_stages([stage]), of, R.SEED, 0, x0=x0)
        x, v = np.array(x0, dtype=np.float64), O.init_velocities(om, R.SEED, 0, 0.5)
        sc = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
        for kind in (4,) + (stage_kind,) * 6:
            F = O.energy_force(om, d10, x, *stage[3:6])[0]
            if kind != 4:
                sc = R.step_scalars_ref(kind, dt, t_bath, sums, (0.0, 0.0), 0, consts, fire, precision=64)[0]
            out = np.array([R.row_finish_ref(kind, dt, list(x[i]) + list(v[i]) + list(F[i]) + list(sc) + [0.0], consts, fire) for i in range(n)])
            x, v = out[:, 0:3], out[:, 3:6]
            sums = tuple(out[:, 6 + k].sum() for k in range(4))
        assert np.abs(x - x.mean(0) - xo).max() < 1e-12 and np.abs(v - vo).max() < 1e-12 * np.abs(vo).max(), stage_kind


# ---------------------------------------------------------------------------------------------
# the fp32 row table (tests/test_gpu_row_finish_table.py runs it on the device): admitted here, without one
# ---------------------------------------------------------------------------------------------
def _table32():
    from chromosome3d_amd import default_fire, default_model
    m, fire = default_model(**R.TABLE_MODEL), default_fire(**R.TABLE_FIRE)
    return R.table_consts(m, R.TABLE_N), fire


def _probe32(kind, r, consts, fire):
    from collections import Counter
    h, p = Counter(), {}
    out = R.row_finish_ref(kind, ROW_DT, r, consts, fire, precision=32, hits=h, probe=p)
    return out, h, p


def test_fp32_row_table_is_made_of_floats_and_takes_every_branch(built):
    """every input is a float32; every tuned row stands beside _X0 and at x = 0; each cap on either side (kind 5: the four combinations);
    at least 50 rows and, where there is a cap, 20 capped rows a kind; every tag the device test treats apart occurs"""
    from collections import Counter
    consts, fire = _table32()
    assert float(fire.max_step) ** 2 == float(np.float32(fire.max_step) * np.float32(fire.max_step))      # F32(max_step)^2 is the device's float too
    for kind in R.ROW_KINDS:
        rows = R.row_finish_rows32(kind, ROW_DT, consts, fire)
        assert 50 <= len(rows) <= 2048, (kind, len(rows))
        tags, hits, combos, at_zero = Counter(t for _, t in rows), Counter(), set(), 0
        for r, tag in rows:
            assert tag in R.ROW_TAGS32 and all(a != a or float(np.float32(a)) == a for a in r), (kind, r)
            _, h, _ = _probe32(kind, r, consts, fire)
            hits.update(h)
            combos.add((bool(h["s_capped"]), bool(h["move_capped"])))
            at_zero += r[0:3] == [0.0, 0.0, 0.0]
        assert at_zero >= 20, (kind, at_zero)
        if kind in (2, 3, 5, 6):
            assert tags["capped"] >= 20 and tags["overflow"] >= 6 and tags["beyond"] >= 6 and hits["move_uncapped"] and hits["move_capped"], (kind, tags)
            assert (tags["infinite"] >= 6) == (kind in (5, 6)) and (tags["beyond_s"] >= 6) == (kind == 5)
        else:
            assert set(tags) == {"plain"} and hits["md" if kind != 4 else "md_begin"] == len(rows)
        if kind == 5:
            assert combos == {(False, False), (False, True), (True, False), (True, True)}
        # F = 0, a -0 and a NaN among the forces; lambda and keep / mix at the issue's values
        Fs = [r[6:9] for r, _ in rows]
        assert any(F == [0.0, 0.0, 0.0] for F in Fs) and any(np.signbit(F[1]) and F[1] == 0.0 for F in Fs) and any(F[1] != F[1] for F in Fs)
        if kind < 2:
            assert {r[9] for r, _ in rows} >= {0.0, 1.0, R.f32(0.93)}
        if kind in (2, 3):
            assert {(r[13], r[14]) for r, _ in rows} >= {(0.0, 0.0), (R._K7, R._K7), (R._K7, 0.0), (0.0, R._K7)}


def test_fp32_row_table_edges_are_at_the_edge(built):
    """each capped quantity on two ADJACENT floats of one component between which the restatement's d.d crosses F32(max_step)^2, beside
    _X0 and at 0; at 0, the smallest normal float, a denormal, 2 and 1e8 max_step; and at the float's own edge: d.d at most one float below
    FLT_MAX with d finite, d.d beyond it with d finite, d itself infinite"""
    consts, fire = _table32()
    ms = float(fire.max_step)
    ms2 = ms * ms
    for kind in (2, 3, 5, 6):
        rows = R.row_finish_rows32(kind, ROW_DT, consts, fire)
        for which in (("move_d2",) if kind != 5 else ("move_d2", "s_d2")):
            comp = 8 if which == "move_d2" else 5                                       # the tuned component: F's or v's third
            below, above, sizes = {}, {}, set()
            for r, tag in rows:
                if tag not in ("plain", "capped"):
                    continue
                d2 = _probe32(kind, r, consts, fire)[2][which]
                sizes.add(d2)
                key = tuple(a for j, a in enumerate(r) if j != comp and a == a)
                if 0.9 * ms2 < d2 <= ms2:
                    below.setdefault(key, set()).add(abs(r[comp]))
                if ms2 < d2 < 1.1 * ms2:
                    above.setdefault(key, set()).add(abs(r[comp]))
            pairs = [(lo, hi) for key in below if key in above for lo in below[key] for hi in above[key] if R._next32(lo) == hi]
            assert len(pairs) >= (4 if kind != 5 else 8), (kind, which, len(pairs))      # every (keep, mix) / length pair, at both x0
            assert 0.0 in sizes and any(0.0 < s <= 1.01 * R.FLT_MIN ** 2 for s in sizes) and any(0.0 < s < 1e-83 for s in sizes), (kind, which)
            assert any(abs(s / ms2 - 4.0) < 1e-5 for s in sizes) and any(abs(s / ms2 - 1e16) < 1e10 for s in sizes), (kind, which)
        edge = float(np.nextafter(np.float32(R.FLT_MAX), np.float32(0)))
        seen = {"overflow": 0, "beyond": 0, "beyond_s": 0, "infinite": 0}
        for r, tag in rows:
            if tag in ("plain", "capped"):
                continue
            p = _probe32(kind, r, consts, fire)[2]
            d2 = p["s_d2"] if (tag == "beyond_s" or (kind == 5 and tag == "overflow" and p["s_d2"] > 1.0)) else p["move_d2"]
            if tag == "overflow":
                assert 0.999 * R.FLT_MAX < d2 and R.f32(d2) <= edge, (kind, r, d2)
                seen[tag] += R.f32(d2) == edge                                                  # one float below FLT_MAX: the axis rows
            elif tag in ("beyond", "beyond_s"):
                assert d2 > R.FLT_MAX and all(np.isfinite(np.float32(a)) for a in r), (kind, r, d2)
                seen[tag] += 1
            else:
                assert max(abs(r[14] * a) for a in r[6:9]) > R.FLT_MAX and all(np.isfinite(np.float32(a)) for a in r), (kind, r)
                seen[tag] += 1
        assert seen["overflow"] >= 6 and seen["beyond"] >= 6, (kind, seen)


@pytest.mark.parametrize("mut", ["cap_no_sqrt", "no_cm"])
def test_fp32_row_table_catches_the_row_mutations(built, mut):
    """the mutations of TABLE_MUTATIONS that change a row's outputs move some row of the fp32 table by at least 1000 float ulps — 125 times the
    widest bound (">=" for ">" at the cap changes no output, as test_fp64_table_catches_every_mutation says, and the fp32 rows lie beside the
    cap, not on it)"""
    consts, fire = _table32()
    worst = 0.0
    for kind in R.ROW_KINDS:
        for r, tag in R.row_finish_rows32(kind, ROW_DT, consts, fire):
            if tag not in ("plain", "capped", "overflow"):
                continue
            a = R.row_finish_ref(kind, ROW_DT, r, consts, fire, precision=32)
            b = R.row_finish_ref(kind, ROW_DT, r, consts, fire, precision=32, mut=mut)
            worst = max([worst] + [R.ulps32(g, w) for g, w in zip(b, a) if w == w and g == g])
    print(f"{mut} ({R.TABLE_MUTATIONS[mut]}): {worst:.3g} float ulps")
    assert worst >= 1000.0, worst


def test_fp32_row_bounds_hold_for_a_float_emulation_of_finish_row(built):
    """finish_row restated in float32 (exact-product fma, one rounding an operation, v_rsq_f32 as the rounded 1 / sqrt moved -1, 0 and +1
    float) against the float64 restatement under the table's own assertion: the arithmetic of the reference and of a correct device text
    lies inside the bounds (plain 4, capped 8) with room to spare, and behaves beyond the domain as the device test asserts"""
    consts, fire = _table32()
    worst = {}
    for kind in R.ROW_KINDS:
        for r, tag in R.row_finish_rows32(kind, ROW_DT, consts, fire):
            want = R.row_finish_ref(kind, ROW_DT, r, consts, fire, precision=32)
            for shift in (-1, 0, 1):
                worst[tag] = max(worst.get(tag, 0.0), R.row_gap32(R.finish_row_emulated32(kind, ROW_DT, r, consts, fire, shift), want, tag, r))
    print({t: round(w, 2) for t, w in worst.items()})
    assert worst["plain"] <= 3.5 and worst["capped"] <= 4.0 and worst["overflow"] <= 4.0, worst
    # and a wrong text leaves them: the cap applied to the uncapped side, a swapped component
    r, tag = next((r, t) for r, t in R.row_finish_rows32(2, ROW_DT, consts, fire) if t == "capped")
    got = R.finish_row_emulated32(2, ROW_DT, r, consts, fire)
    with pytest.raises(AssertionError):
        R.row_gap32(got[:1] + [got[2], got[1]] + got[3:], R.row_finish_ref(2, ROW_DT, r, consts, fire, precision=32), tag, r)


def test_row_restatement_precision_switch_leaves_the_fp64_table_alone(built):
    """precision=32 changes only how dt acc is formed: on the fp64 table's constants the two agree wherever the products agree, and the default
    is the fp64 form"""
    consts, fire = _table64()
    for kind in R.ROW_KINDS:
        for r, _ in R.row_finish_rows(kind, ROW_DT, consts, fire)[:40]:
            a, b = R.row_finish_ref(kind, ROW_DT, r, consts, fire), R.row_finish_ref(kind, ROW_DT, r, consts, fire, precision=64)
            assert all(x == y or (x != x and y != y) for x, y in zip(a, b))


def test_fp64_row_table_reaches_beyond_the_caps_float_seed(built):
    """kinds 2, 3, 5, 6: the capped quantity (and kind 5's previous move) with d.d at 2^127, 2^128, 1e40, 1e150 and 1e300 A^2 — either side
    of where v_rsq_f32 of (float)d.d turns 0 — beside _X0 and at x = 0, every such row a capped row whose restatement moves by max_step"""
    consts, fire = _table64()
    ms = float(fire.max_step)
    assert R.SEED_EDGE_D2[0] < float(np.finfo(np.float32).max) < R.SEED_EDGE_D2[1]
    for kind in (2, 3, 5, 6):
        seen = {w: set() for w in ("move_d2", "s_d2")}
        for r, tag in R.row_finish_rows(kind, ROW_DT, consts, fire):
            p = {}
            out = R.row_finish_ref(kind, ROW_DT, r, consts, fire, probe=p)
            for w, d2 in p.items():
                for t in R.SEED_EDGE_D2:
                    if abs(d2 / t - 1.0) < 1e-9:
                        assert tag == "capped", (kind, r)
                        seen[w].add((t, any(r[0:3])))
                        if w == "move_d2":
                            assert abs(np.linalg.norm(np.array(out[0:3]) - np.array(r[0:3])) - ms) < 1e-12, (kind, r, out[:3])
        want = {(t, at) for t in R.SEED_EDGE_D2 for at in (True, False)}
        assert seen["move_d2"] == want and (kind != 5 or seen["s_d2"] == want), (kind, seen)
