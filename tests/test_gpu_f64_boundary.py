"""A precision-64 context's boundary in doubles: c3d_set_coords_f64 / c3d_get_coords_f64 / c3d_get_velocities_f64 move the fp64 state bit
for bit, c3d_eval_f64 evaluates forces (k64_eval_forces[_chunked]) and energies (k64_energy) with the fp64 kernels at the fp64 coordinates.
With that boundary the fp64 kernels are held to the oracle at their own grain, the step kernels that existed before it included.

Sizes, for the branches of c3d_f64_step_body.inc (main = the two-column main loop, 64 = the 64-column block, joint / split = the last pass):
37 split only; 96 64 + joint 32; 113 64 + split 49, odd last row; 128 main only; 455 main + 64 + joint 7; 300 at f64_column_chunk 256 one full
chunk and a split 44 in the next; 640 at 256 three chunks with n % 64 == 0; 2561 the default chunked form (512), one replica.

Bounds.  Every bound is 8 x the largest gap tools/f64_boundary.py measured on an MI355X (profiles/r16_f64_boundary.md: the sums run in
another order than the oracle's, pair64 refines its reciprocals by Newton steps, the trajectories are chaotic), under a cap that no pass
through fp32 could meet.  The trajectories are bounded schedule by schedule, each by 8 x its own largest gap:
  forces        |F - Fo| <= B_F (|Fo| + 0.1 max|Fo|), cap B_F <= 1e-10 (that is 1e-10 |F| + 1e-11 max|F|; the fp32 hook's bound is 1e-5 / 1e-6)
                measured 9.98e-13 (n = 37, potential 0 at w_all 0.4; at most 6.3e-13 elsewhere): B_F = 8.0e-12
  energies      |e - eo| <= B_E |eo|, cap 1e-11; measured 3.10e-14 (n = 2561, potential 2): B_E = 2.5e-13
  trajectories  max|x - xo| <= B_X Angstrom and max|v - vo| <= B_V max(1, max|vo|), cap 1e-8 each; measured, x / v:
                anneal 1.92e-10 / 3.35e-12 (n = 2561), two-point 1.51e-12 / 7.56e-13, L-BFGS 1.46e-10 / 3.46e-11 (n = 113)
On the CPU, the restatement against itself with the force's pair sums reversed (tools/f64_boundary.py --cpu-check) ends these schedules
at most 7.3e-12 A and 6.7e-13 apart (the L-BFGS stage at 455 beads; the anneal and the two-point stage stay below 4e-14 A): the step
counts leave three orders under the cap for re-ordered sums alone."""
import functools

import numpy as np
import pytest

from tests import lbfgs_ref as L
from tests.util import oracle_fire_from, oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

# ---- bounds: 8 x the measured gap (profiles/r16_f64_boundary.md: the "largest" lines of the MI355X section), each under its cap ----
F_MEASURED, E_MEASURED = 9.98e-13, 3.10e-14
XV_MEASURED = {"anneal": (1.92e-10, 3.35e-12), "two-point": (1.51e-12, 7.56e-13), "lbfgs": (1.46e-10, 3.46e-11)}     # schedule: (x in A, v)
F_CAP, E_CAP, XV_CAP = 1e-10, 1e-11, 1e-8
F_BOUND, E_BOUND = 8 * F_MEASURED, 8 * E_MEASURED
XV_BOUND = {k: (8 * x, 8 * v) for k, (x, v) in XV_MEASURED.items()}
assert F_BOUND <= F_CAP and E_BOUND <= E_CAP and all(x <= XV_CAP and v <= XV_CAP for x, v in XV_BOUND.values())

# n -> the f64_column_chunk settings that run it (the first one is the form the table names)
FORMS = {37: (0,), 96: (0,), 113: (0,), 128: (0,), 455: (0, 256), 300: (256, 0), 640: (256, 0, 512), 2561: (0, 256, 1024)}
# model -> (c3d_model fields, <pot, gen> of the kernel): every noe_pot in the clamp form and with a general tail, and the shipped model
MODELS = {"shipped": ({}, (4, False)),
          "pot0": (dict(noe_pot=0), (0, False)), "pot1": (dict(noe_pot=1), (1, False)), "pot2": (dict(noe_pot=2), (2, False)),
          "pot3": (dict(noe_pot=3, mrswitch=4.0, masym=8.0, msoexp=1), (3, False)),
          "gen0": (dict(noe_pot=0, asym=3.0, rswitch=2.0), (0, True)), "gen1": (dict(noe_pot=1, asym=1.0, rswitch=0.5), (1, True)),
          "gen2": (dict(noe_pot=2, asym=1.5, rswitch=1.0), (2, True)), "gen3": (dict(noe_pot=3, mrswitch=4.0, masym=3.0, msoexp=1), (3, True))}
WEIGHTS = ((1.0, 1.0, 0.85), (0.4, 0.003, 0.9))          # w_all 1 and != 1 (FOLD multiplies by it)
F32 = lambda *a: tuple(float(np.float32(v)) for v in a)  # a stage's weights as the C ABI holds them, widened


def _nrep(n):
    return 1 if n > 2000 else 2


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    for key, val in (("max_beads", 16384), ("f64_max_beads", 16384), ("f64_lbfgs", 1), ("precision", 64)):
        s.set_option(key, val)
    yield s
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=None)
def start64(n, nrep):
    """a random coil moved by amounts no float holds: a round trip through fp32 anywhere shows"""
    rng = np.random.default_rng(1000 + n)
    x = np.stack([random_coil(n, 7 * n + r).astype(np.float64) for r in range(nrep)])
    x += rng.normal(scale=1e-3, size=x.shape)
    assert not np.array_equal(x, x.astype(np.float32).astype(np.float64))
    return x


@functools.lru_cache(maxsize=None)
def matrix(n):
    return synthetic_if(n, seed=n)[0]


def problem(s, n, model_kw=None, chunk=0):
    """matrix (only when n changes), model and column form on the context; returns (c3d_model, integer tenths as the device holds them)"""
    from chromosome3d_amd import default_model
    m = default_model(**(model_kw or {}))
    s.set_option("f64_column_chunk", chunk)
    s.set_model(m)
    if getattr(s, "_boundary_n", None) != n:
        s.set_if_matrix(matrix(n))
        s._boundary_n, s._boundary_d10 = n, s.dist10()
    return m, s._boundary_d10


def begin(s, stages, nrep, x0, nl=1000):
    from chromosome3d_amd import default_fire, make_stages
    fire = default_fire()
    s.set_option("final_minimiser_steps", nl)
    s.set_schedule(make_stages(stages), fire)
    s.init_replicas(nrep, 82364, 0)
    s.set_coords64(x0)
    return fire


def rel_force_gap(F, Fo):
    return float((np.abs(F - Fo) / (np.abs(Fo) + 0.1 * np.abs(Fo).max())).max())


def rel_energy_gap(e, eo):
    e, eo = np.asarray(e, dtype=np.float64), np.asarray(eo, dtype=np.float64)
    return float((np.abs(e - eo) / np.maximum(np.abs(eo), 1e-300)).max())


# ---- 1-3: forces and energies against the oracle, every form, the same bits from every column form and from a second call -------------
def measure_forces_energies(s, O, n):
    """{(model, w_all): (force gap, energy gap)} at n, after asserting the bits: chunk settings against one another, a call against its repeat"""
    nrep = _nrep(n)
    x0 = start64(n, nrep)
    out = {}
    try:
        for name, (kw, (pot, gen)) in MODELS.items():
            results = {}
            for chunk in FORMS[n]:
                m, d10 = problem(s, n, kw, chunk)
                begin(s, [(2, 10, 0.0, 1.0, 1.0, 0.85, 0.0)], nrep, x0)
                for w in WEIGHTS:
                    before = s.stat("f64_evals")
                    F, e = s.eval64(*w)
                    F2, e2 = s.eval64(*w)
                    assert s.stat("f64_evals") == before + 2
                    assert np.array_equal(F, F2) and np.array_equal(e, e2), (n, name, chunk, w, "two calls differ")
                    assert np.isfinite(F).all() and np.isfinite(e).all()
                    results[(chunk, w)] = (F, e)
                # the model reaches the instantiation family MODELS names: one step of the stage (w_all 1) through the same form64
                assert s.run_steps(1) == 1
                tf = lambda b: "true" if b else "false"
                form = f"{pot}, {tf(gen)}, {tf(pot == 4 and not gen)}"
                option = FORMS[n][FORMS[n].index(chunk)]
                cols = option if option and n > option else (0 if n <= 2560 else 512)
                want = f"c3d::k64_step_chunked<{form}, {cols}>" if cols else f"c3d::k64_step<{form}>"
                assert s.step_kernel_name == want, (n, name, chunk, s.step_kernel_name, want)
            om = oracle_model_from(m, n)
            for w in WEIGHTS:
                F, e = results[(FORMS[n][0], w)]
                for chunk in FORMS[n][1:]:
                    assert np.array_equal(results[(chunk, w)][0], F), (n, name, chunk, w, "the column forms' forces differ")
                    assert np.array_equal(results[(chunk, w)][1], e), (n, name, chunk, w, "the column forms' energies differ")
                gf = ge = 0.0
                for r in range(nrep):
                    Fo, eo = O.energy_force(om, d10, x0[r], *w)
                    gf, ge = max(gf, rel_force_gap(F[r], Fo)), max(ge, rel_energy_gap(e[r], eo))
                out[(name, w[0])] = (gf, ge)
    finally:
        problem(s, n)
    return out


@pytest.mark.parametrize("n", sorted(FORMS))
def test_forces_and_energies_follow_the_oracle_in_every_form(ctx, O, n):
    gaps = measure_forces_energies(ctx, O, n)
    for key, (gf, ge) in gaps.items():
        print(n, key, f"force {gf:.2e} / {F_BOUND:.2e}  energy {ge:.2e} / {E_BOUND:.2e}")
    assert all(gf <= F_BOUND and ge <= E_BOUND for gf, ge in gaps.values()), {k: v for k, v in gaps.items() if v[0] > F_BOUND or v[1] > E_BOUND}


# ---- 4: the hook's force is the step's force --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk", [(113, 0), (455, 0), (455, 256), (300, 256)])
def test_the_eval_force_is_the_step_force(ctx, n, chunk):
    """A kind-8 stage's first step (kind 9) leaves F at the old coordinates in the velocity slot: eval64 at the start, with the stage's float
    weights widened, returns those bits.  The form is the stage's: k64_eval_forces beside k64_lbfgs_eval, both <4, false, true>."""
    s = ctx
    w = (1.0, 1.0, 0.85)
    try:
        problem(s, n, None, chunk)
        begin(s, [(8, 10, 0.0) + w + (0.0,)], 2, start64(n, 2))
        name0 = s.step_kernel_name
        F, _ = s.eval64(*F32(*w), energies=False)
        assert s.step_kernel_name == name0
        assert s.run_steps(1) == 1
        tail = f"_chunked<4, false, true, {chunk}>" if chunk else "<4, false, true>"
        assert s.step_kernel_name == "c3d::k64_lbfgs_eval" + tail, s.step_kernel_name
        v = s.velocities64()
        assert np.array_equal(v, F), float(np.abs(v - F).max())
    finally:
        problem(s, n)


# ---- 5: the hook changes nothing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chunk", [(113, 0), (300, 256)])
@pytest.mark.parametrize("what", ["hot MD", "L-BFGS"])
def test_eval_changes_no_state(ctx, what, n, chunk):
    """7 steps, eval64 (forces and energies, other weights than the stage's), 7 more: coordinates and velocity slot of an uninterrupted run of
    14, bit for bit.  7 is odd (the hook runs on parity 1); inside the L-BFGS part the ring is in use and the kernel name is the stage's."""
    s = ctx
    stages = [(0, 30, 0.003, 0.4, 0.003, 0.9, 2000.0)] if what == "hot MD" else [(8, 30, 0.0, 1.0, 1.0, 0.85, 0.0)]
    try:
        problem(s, n, None, chunk)
        x0 = start64(n, 2)
        l0 = s.stat("lbfgs_steps")
        begin(s, stages, 2, x0)
        assert s.run_steps(14) == 14
        ref = (s.coords64(), s.velocities64(), s.coords(), s.stat("lbfgs_steps") - l0)
        assert ref[3] == (14 if what == "L-BFGS" else 0)
        l0 = s.stat("lbfgs_steps")
        begin(s, stages, 2, x0)
        assert s.run_steps(7) == 7
        name, steps, resets = s.step_kernel_name, s.steps_done, s.stat("lbfgs_resets")
        mid = (s.coords64(), s.velocities64())
        s.eval64(0.7, 2.0, 1.1)
        assert (s.step_kernel_name, s.steps_done, s.stat("lbfgs_resets")) == (name, steps, resets)
        assert np.array_equal(s.coords64(), mid[0]) and np.array_equal(s.velocities64(), mid[1])
        assert s.run_steps(7) == 7
        assert np.array_equal(s.coords64(), ref[0]) and np.array_equal(s.velocities64(), ref[1]) and np.array_equal(s.coords(), ref[2])
        assert s.stat("lbfgs_steps") - l0 == ref[3]
        assert np.isfinite(ref[0]).all() and not np.array_equal(ref[0], mid[0])
    finally:
        problem(s, n)


# ---- 6: round trip -----------------------------------------------------------------------------------------------------------------
def test_round_trip(ctx):
    from chromosome3d_amd import C3DError
    s = ctx
    n = 113
    problem(s, n)
    x = start64(n, 2)
    begin(s, [(2, 10, 0.0, 1.0, 1.0, 0.85, 0.0)], 2, x)
    assert np.array_equal(s.coords64(), x)
    assert np.array_equal(s.coords(), x.astype(np.float32))
    assert np.array_equal(s.velocities64(), np.zeros_like(x))
    # the float mirror holds the new structure: the restraint energy of the rounded coordinates (the bond term of a coil with exact
    # 3.8 A steps moved by 1e-3 A is all perturbation: a float's rounding shows in its third digit)
    assert np.allclose(s.eval(forces=False)[1][:, 0], s.eval64(forces=False)[1][:, 0], rtol=1e-4)
    for bad in (np.nan, np.inf):
        y = x + 1.0
        y[1, n - 1, 2] = bad
        with pytest.raises(C3DError, match="non-finite"):
            s.set_coords64(y)
        assert np.array_equal(s.coords64(), x) and np.array_equal(s.coords(), x.astype(np.float32))
    # one fp64 context to another, nothing rounded on the way
    assert s.run_steps(5) == 5
    xa = s.coords64()
    s.set_coords64(xa)
    assert np.array_equal(s.coords64(), xa) and not np.array_equal(xa, xa.astype(np.float32))


# ---- 7: the step kernels that were there before, at fp64 grain ------------------------------------------------------------------------
ANNEAL = [(2, 4, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 20, 0.003, 0.4, 0.003, 0.9, 2000.0), (0, 12, 0.003, 0.4, 0.003, 0.9, 1000.0)]
TWO_POINT = [(5, 30, 0.0, 1.0, 1.0, 0.85, 0.0)]
LBFGS = [(8, 30, 0.0, 1.0, 1.0, 0.85, 0.0)]
SCHEDULES = {"anneal": ANNEAL, "two-point": TWO_POINT, "lbfgs": LBFGS}


def restatement(O, m, fire, d10, x0, which, replica):
    """(x, v) of the fp64 restatement from x0: O.run_schedule (centred at its end), or tests/lbfgs_ref.py for the kind-8 stage; the stages'
    numbers are the floats the C ABI holds, widened"""
    n = x0.shape[0]
    om, of = oracle_model_from(m, n), oracle_fire_from(fire)
    stages = [(k, c) + F32(*rest) for (k, c, *rest) in SCHEDULES[which]]
    if which != "lbfgs":
        O.set_two_point_steps(1000)
        x, v, ev = O.run_schedule(om, d10, O.make_stages(stages), of, 82364, replica, x0=x0)
        assert ev == sum(st[1] for st in stages)
        return x, v
    _, k, _, w_all, w_vdw, repel_s, _ = stages[0]
    force = lambda u: O.energy_force(om, d10, u, w_all, w_vdw, repel_s)[0]
    dt = float(fire.dt_start)
    g0 = (dt * dt) * (418.4 / float(m.mass))
    x_last, _ = L.lbfgs_run(force, x0, k - 1, m=5, g0=g0, max_step=float(fire.max_step))
    x, _ = L.lbfgs_run(force, x0, k, m=5, g0=g0, max_step=float(fire.max_step))
    return x, force(x_last)                      # the slot holds the last evaluation's force


def measure_trajectory(s, O, n, which):
    """(x gap in Angstrom, v gap relative to max(1, max|v|)) of SCHEDULES[which] from a set_coords64 start, worst replica; where n runs in
    more than one column form, the forms end in the same bits"""
    nrep = _nrep(n)
    x0 = start64(n, nrep)
    nsteps = sum(st[1] for st in SCHEDULES[which])
    out = []
    try:
        for chunk in FORMS[n][:2]:
            m, d10 = problem(s, n, None, chunk)
            fire = begin(s, SCHEDULES[which], nrep, x0)
            assert s.run_steps(10 ** 6) == nsteps
            out.append((s.coords64(), s.velocities64()))
            assert np.isfinite(out[-1][0]).all() and np.isfinite(out[-1][1]).all()
            assert s.stat("last_path") == 3
    finally:
        problem(s, n)
    for x, v in out[1:]:
        assert np.array_equal(x, out[0][0]) and np.array_equal(v, out[0][1]), (n, which, "the column forms differ")
    x, v = out[0]
    gx = gv = 0.0
    for r in range(nrep):
        xo, vo = restatement(O, m, fire, d10, x0[r], which, r)
        xc = x[r] - x[r].mean(0) if which != "lbfgs" else x[r]
        gx = max(gx, float(np.abs(xc - xo).max()))
        gv = max(gv, float(np.abs(v[r] - vo).max() / max(1.0, np.abs(vo).max())))
    return gx, gv


@pytest.mark.parametrize("which", sorted(SCHEDULES))
@pytest.mark.parametrize("n", [113, 455, 300, 2561])
def test_step_kernels_follow_the_restatement_at_fp64_grain(ctx, O, n, which):
    """k64_step / k64_step_chunked (4 FIRE + 20 hot MD + 12 cooling steps; 30 two-point steps) and k64_lbfgs_eval + k64_lbfgs_move (30 steps)
    against the restatement in doubles, coordinates and velocity slot: a thousand times below a float's half ulp at these coordinates."""
    gx, gv = measure_trajectory(ctx, O, n, which)
    bx, bv = XV_BOUND[which]
    print(n, which, f"x {gx:.2e} / {bx:.2e} A   v {gv:.2e} / {bv:.2e}")
    assert gx <= bx and gv <= bv, (gx, gv)


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    from chromosome3d_amd import C3DError, Solver, default_fire, default_model, make_stages
    IF = synthetic_if(37, seed=37)[0]
    x = start64(37, 2)
    f = Solver(0)
    try:
        f.set_model(default_model())
        f.set_if_matrix(IF)
        f.set_schedule(make_stages([(2, 10, 0.0, 1.0, 1.0, 0.85, 0.0)]), default_fire())
        f.nrep = 2
        calls = (("c3d_get_coords_f64", f.coords64), ("c3d_get_velocities_f64", f.velocities64),
                 ("c3d_set_coords_f64", lambda: f.set_coords64(x)), ("c3d_eval_f64", f.eval64))
        f.set_option("precision", 64)
        for name, call in calls:                       # precision 64, no replicas yet
            with pytest.raises(C3DError, match=name + ".*c3d_init_replicas"):
                call()
        f.set_option("precision", 32)
        f.init_replicas(2, 82364, 0)
        for name, call in calls:                       # replicas, precision 32
            with pytest.raises(C3DError, match=name + ".*precision"):
                call()
        assert np.isfinite(f.coords()).all() and f.stat("f64_evals") == 0
    finally:
        f.close()
    s = ctx
    problem(s, 37)
    begin(s, [(2, 10, 0.0, 1.0, 1.0, 0.85, 0.0)], 2, x)
    before = s.stat("f64_evals")
    with pytest.raises(C3DError, match="c3d_eval_f64.*both NULL"):
        s.eval64(forces=False, energies=False)
    assert s.stat("f64_evals") == before
    s.eval64(energies=False)
    s.eval64(forces=False)
    assert s.stat("f64_evals") == before + 2
