"""Every launchable form of the multi-step cluster kernel, once: k_cluster / k_cluster_tp <potential, rpw, nb, wl, late> under each of the
planner's ten geometries {compute waves x rows per wave}, with and without left-over columns, as one workgroup per replica and as
several — the 538 keys of tests/cluster_forms.py, each at the smallest bead count that realises it, plus the left-over extremes and 17
replicas (three on the fullest XCD).  The geometry is forced (option cluster_geometry), so a form runs whether or not the planner's cost
model would choose it for the problem; the library confirms every key through its plan statistics and the kernel's name.

Per case: the multi-step kernel (resident 1) and the per-step kernel (resident 0) from the same start, bit for bit at four checkpoints
(c3d.h: the two paths "end in the same bits"), and the per-step run — so both — against the fp64 oracle at the tolerances of
test_gpu_step_kernels.py: coordinates 2e-3 A after steps 22 and 30, 5e-3 A after 38 and 50 (two-point steps), velocities
2e-3 x max(1, |v|max) after 30.  Potential 2 on two or three column blocks is compared with the oracle after step 22 alone: without a
switch its force grows with the violation, and where (nearly) every pair is restrained the later stages magnify fp32 rounding about a
hundredfold in every fp32 form (test_gpu_step_kernels.py, section F); its bit comparison with the per-step path is complete.

The per-step run and the oracle depend on (variant, beads, replicas) alone: computed once, shared by the geometries, never modified.
Measured worst over all cases: 3.3e-5 A after step 30, 5.7e-4 A after step 50 (potential 3, 9 beads x 17 replicas; 4.4e-5 A otherwise);
the module takes 27 s, its slowest test 3.1 s (profiles/r24_cluster_forms.md).
"""
import functools

import numpy as np
import pytest

from tests import cluster_forms as cf
from tests.test_gpu_step_kernels import VARIANTS, _oracle, _worst
from tests.util import synthetic_if

pytestmark = pytest.mark.gpu

# FIRE from the coil, MD at 2000 K (kind 4 begins it, then kind 0), kind 1, kind 5 with the hand-over to FIRE after 8 of its steps.  No
# stage without restraint weight: at every checkpoint the last kernel is the cluster kernel's own.
STAGES = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 12, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 8, 0.005, 1.0, 0.05, 1.0, 1500.0),
          (5, 20, 0.0, 1.0, 1.0, 0.85, 0.0)]
TP = 8
CHECKPOINTS = (22, 30, 38, 50)
TOL = {22: 2e-3, 30: 2e-3, 38: 5e-3, 50: 5e-3}
FIVE = ("pot0", "pot1", "pot2", "pot3_clamp", "shipped")
WORST = {}                                        # device potential -> {checkpoint: worst deviation from the oracle}, for the printed summary


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@functools.lru_cache(maxsize=None)
def _if(n):
    IF = synthetic_if(n, seed=n)[0]
    IF.setflags(write=False)
    return IF


@functools.lru_cache(maxsize=None)
def _d10(n):
    from oracle import oracle
    return oracle.if_to_dist10(_if(n))


def _restore(solver):
    solver.set_option("cluster_geometry", 0)
    solver.set_option("cluster_late_tiles", 1)
    solver.set_option("resident", -1)
    solver.set_option("replica_groups", 2)
    solver.set_option("final_minimiser_steps", 1000)


def _start(solver, variant, n, nrep, resident, geometry, late_tiles):
    from chromosome3d_amd import default_fire, default_model, make_stages
    solver.set_option("resident", resident)
    solver.set_option("replica_groups", 1)
    solver.set_option("final_minimiser_steps", TP)
    solver.set_option("cluster_geometry", geometry)
    solver.set_option("cluster_late_tiles", late_tiles)
    solver.set_model(default_model(**VARIANTS[variant][0]))
    solver.set_if_matrix(_if(n))
    solver.set_schedule(make_stages(STAGES), default_fire())
    solver.init_replicas(nrep, 82364, 0)


def _segments(solver):
    """the schedule checkpoint by checkpoint: [(step, coordinates, velocities, kernel name, cluster launches, step launches)]"""
    out, done = [], 0
    for k in CHECKPOINTS:
        c0, s0 = solver.stat("cluster_launches"), solver.stat("step_launches")
        assert solver.run_steps(k - done) == k - done
        done = k
        out.append((k, solver.coords(), solver.velocities(), solver.step_kernel_name, solver.stat("cluster_launches") - c0,
                    solver.stat("step_launches") - s0))
    return out


_PER_STEP = {}


def _per_step(solver, O, variant, n, nrep):
    """(start, per-step run, oracle, worst deviation per checkpoint) of a (variant, bead count, replica count): run once, held to the
    oracle once"""
    key = (variant, n, nrep)
    if key in _PER_STEP:
        return _PER_STEP[key]
    from chromosome3d_amd import default_fire, default_model
    kw, pot, gen = VARIANTS[variant]
    _start(solver, variant, n, nrep, 0, 0, 1)
    x0 = solver.coords()
    out = _segments(solver)
    for k, x, v, name, cl, sl in out:
        assert name.startswith(f"c3d::k_step<{pot}, false, ") and cl == 0 and sl > 0, (key, k, name, cl, sl)
        x.setflags(write=False)
        v.setflags(write=False)
    m = default_model(**kw)
    only22 = variant == "pot2" and n > 256         # (module docstring)
    worst = {}
    for k, x, v, *_ in out:
        if only22 and k != 22:
            continue
        ref = _oracle(O, m, default_fire(), _d10(n), STAGES, x0, TP, k)
        worst[k] = _worst(x, ref)
        if k == 30:
            for r in range(nrep):
                vo = ref[r][1]
                assert np.abs(v[r] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max()), (key, r)
    print(f"{variant} n={n} x{nrep} per-step path against the oracle: " + " ".join(f"{k}: {w:.2e}" for k, w in worst.items()))
    for k, w in worst.items():
        assert w < TOL[k], (key, k, w)
        WORST.setdefault(pot, {})[k] = max(WORST.setdefault(pot, {}).get(k, 0.0), w)
    _PER_STEP[key] = (x0, out)
    return _PER_STEP[key]


def _run_case(solver, O, variant, case):
    k, pot = case.key, VARIANTS[variant][1]
    assert pot == k.pot
    x0, ref = _per_step(solver, O, variant, case.n, case.nrep)
    # run A: the forced geometry
    _start(solver, variant, case.n, case.nrep, 1, cf.geometry_option(k.cw, k.rpw), case.late_tiles)
    plan = {s: solver.stat(s) for s in ("cluster_ok", "cluster_compute_waves", "cluster_rows_per_wave", "cluster_helper_waves",
                                        "cluster_late_tiles", "cluster_parts")}
    assert (plan["cluster_ok"], plan["cluster_compute_waves"], plan["cluster_rows_per_wave"], plan["cluster_helper_waves"],
            plan["cluster_late_tiles"], plan["cluster_parts"] > 1) == (1, k.cw, k.rpw, cf.HELPERS, int(k.late), k.multi), (case, plan)
    assert plan["cluster_parts"] == cf.parts(k.cw, k.rpw, case.n), (case, plan)
    assert np.array_equal(solver.coords(), x0), case
    quiet = ("resident_fallbacks", "cluster_incomplete", "cluster_placement_mismatches")
    before = [solver.stat(s) for s in quiet]
    out = _segments(solver)
    assert [solver.stat(s) for s in quiet] == before, (case, before)
    form = f"<{pot}, {k.rpw}, {k.nb}, {k.wl}, {'true' if k.late else 'false'}>"
    for (step, x, v, name, cl, sl), (_, xr, vr, *_) in zip(out, ref):
        assert name == ("c3d::k_cluster_tp" if step == 38 else "c3d::k_cluster") + form, (case, step, name)
        assert cl >= 1 and (sl == 0 or step == 50), (case, step, cl, sl)      # (50: the hand-over's own ops run per step)
        assert np.array_equal(x, xr) and np.array_equal(v, vr), (case, step, np.abs(x - xr).max(), np.abs(v - vr).max())
    return form


def _rs1_case(cs):
    """the key of a geometry that pot3_rs1 runs too: the one with the most of the body in it (parts, late tiles, left-over columns, blocks)"""
    return max((c for c in cs if c.why == "key"), key=lambda c: (c.key.multi, c.key.late, c.key.left, c.key.nb, c.key.wl))


# (geometry, column blocks, widths of the last block): 12 x 2 alone reaches three column blocks, and those cases — 513 to 713 beads, each
# bead count with an oracle run of its own — are two tests of their own
ALL = (1, 2, 3, 4)
SLICES = ([(g, ALL, ALL) for g in cf.GEOMETRIES if g != (12, 2)]
          + [((12, 2), (1, 2), ALL), ((12, 2), (3,), (1, 2)), ((12, 2), (3,), (3, 4))])


SLICE_IDS = [f"{g[0]}x{g[1]}" + ("" if (b, w) == (ALL, ALL) else "-nb" + "".join(map(str, b)) + ("" if w == ALL else "-wl" + "".join(map(str, w))))
             for g, b, w in SLICES]


def _slice_cases(variant, geometry, blocks, widths):
    return [(variant, c) for c in cf.cases(VARIANTS[variant][1], *geometry) if c.key.nb in blocks and c.key.wl in widths]


# (potentials 0-2 have the full last block only: no cases in the slice of widths 1 and 2)
TESTS = [(v,) + sl for v in FIVE for sl in SLICES if _slice_cases(v, *sl)]


@pytest.mark.parametrize("variant,geometry,blocks,widths", TESTS, ids=[f"{t[0]}-{SLICE_IDS[SLICES.index(t[1:])]}" for t in TESTS])
def test_every_launchable_form_ends_in_the_per_step_bits_and_follows_the_oracle(solver, O, variant, geometry, blocks, widths):
    """Every case of tests/cluster_forms.py for the variant's device potential under the geometry (module docstring), nb in `blocks` and
    wl in `widths`; potential 3 under pot3_rs1 (rswitch 1: the upper bound is 1/d itself) at one more case per slice."""
    cs = _slice_cases(variant, geometry, blocks, widths)
    if variant == "pot3_clamp":
        cs.append(("pot3_rs1", _rs1_case([c for _, c in cs])))
    forms = set()
    try:
        for v, c in cs:
            forms.add(_run_case(solver, O, v, c))
    finally:
        _restore(solver)
    print(f"{variant} {geometry[0]}x{geometry[1]}: {len(cs)} cases, {len(forms)} template forms of k_cluster and of k_cluster_tp; "
          f"worst of potential {VARIANTS[variant][1]} so far: {WORST.get(VARIANTS[variant][1])}")


def test_refused_geometries_plan_nothing(solver):
    """What the table says cluster_plan refuses, it refuses — a case of every rule that can refuse (cluster_forms.REFUSED): no plan, a
    resident 1 run on the per-step kernel; with cluster_geometry back at 0 the planner's own choice returns: the geometry that
    cluster_forms.planner_choice names, or none where the table accepts none."""
    try:
        for variant, geom, n, nrep, rule in cf.REFUSED:
            pot = VARIANTS[variant][1]
            _start(solver, variant, n, nrep, 1, geom, 1)
            assert solver.stat("cluster_ok") == 0 and solver.stat("cluster_parts") == 0, (variant, geom, n, nrep, rule)
            c0 = solver.stat("cluster_launches")
            assert solver.run_steps(12) == 12
            assert solver.stat("last_path") == 0 and solver.stat("cluster_launches") == c0, (variant, geom, n, nrep, rule)
            assert solver.step_kernel_name.startswith(f"c3d::k_step<{pot}, "), solver.step_kernel_name
            solver.set_option("cluster_geometry", 0)
            solver.init_replicas(nrep, 82364, 0)
            accepted = [g for g in cf.GEOMETRIES if cf.refusal(pot, *g, n, nrep, 1) is None]
            assert solver.stat("cluster_ok") == (1 if accepted else 0), (variant, n, nrep, accepted)
            if accepted:
                chosen = (int(solver.stat("cluster_compute_waves")), int(solver.stat("cluster_rows_per_wave")))
                assert chosen in accepted and solver.stat("cluster_helper_waves") == cf.HELPERS, (variant, n, nrep, chosen)
                assert chosen == cf.planner_choice(pot, n, nrep), (variant, n, nrep, chosen)      # the cost model as restated
                assert solver.stat("cluster_parts") == cf.parts(*chosen, n)
                assert solver.run_steps(10) == 10 and solver.stat("last_path") == 2, (variant, n, nrep, chosen)
    finally:
        _restore(solver)
