"""Stage kind 8: L-BFGS on the per-step path (k_lbfgs_eval + k_lbfgs_move, csrc/c3d_lbfgs.h), then FIRE.  Held to the fp64 restatement
(tests/lbfgs_ref.py) replica by replica, through every potential and the wide form beyond 1024 beads; the same bits across replica groups,
graphs, chunking, first_replica and the resident knob; the schedule and API rules; convergence against kind 5; the CLI.  Every test asserts,
by kernel name and the stat lbfgs_steps, that the L-BFGS kernels ran."""
import os
import subprocess

import numpy as np
import pytest

from tests import lbfgs_ref as L
from tests.util import GOLD, load_if, oracle_fire_from, oracle_model_from, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = os.path.join(GOLD, "inputs", "chr21_1mb_matrix.txt")
LB = (1.0, 1.0, 0.85)                    # the final stage's weights: w_all, w_vdw, repel_s


def _stage(kind, n):
    return (kind, n, 0.0, LB[0], LB[1], LB[2], 0.0)


def _prepare(solver, IF, nrep, pre_fire, model_kw=None):
    """Targets and model, then `pre_fire` FIRE steps from the coil: the start coordinates of the tests (float32, not centred)."""
    from chromosome3d_amd import default_fire, default_model, make_stages, pipeline
    m = default_model(**(model_kw or {}))
    solver.set_model(m)
    d10 = pipeline.IF2dist_new(solver, IF)
    fire = default_fire()
    solver.set_schedule(make_stages([(2, pre_fire, 0.0, 1.0, 20.0, 0.5, 0.0)]), fire)
    solver.init_replicas(nrep, 82364, 0)
    solver.run_steps(pre_fire)
    return d10, m, fire, solver.coords()


def _run_lbfgs(solver, stages, x0, nrep, first=0, gtol=0.0, check_every=250, steps=None):
    from chromosome3d_amd import default_fire, make_stages
    solver.set_schedule(make_stages(stages), default_fire(), gtol, check_every)
    solver.init_replicas(nrep, 82364, first)
    solver.set_coords(x0)
    before = solver.stat("lbfgs_steps")
    if steps is None:
        solver.run_steps(10 ** 6)
    else:
        for k in steps:
            solver.run_steps(k)
    return solver.coords(), solver.stat("lbfgs_steps") - before


def _worst_vs_ref(x, x0, d10, m, fire, stage, n_lbfgs, mem=5):
    om, of = oracle_model_from(m, x0.shape[1]), oracle_fire_from(fire)
    worst = 0.0
    for r in range(x.shape[0]):
        xo, _ = L.lbfgs_stage(om, d10, x0[r].astype(np.float64), stage, of, n_lbfgs, m=mem, replica=r)
        xc = x[r].astype(np.float64)
        worst = max(worst, float(np.abs(xc - xc.mean(0) - xo).max()))
    return worst


@pytest.fixture
def lbfgs_steps40(solver):
    solver.set_option("final_minimiser_steps", 40)
    yield solver
    solver.set_option("final_minimiser_steps", 1000)
    solver.set_option("lbfgs_memory", 5)


@pytest.mark.parametrize("cid,nrep", [("chr21_1mb", 20), ("chr13_1mb", 20), ("chr1_500kb", 20)])
def test_lbfgs_stage_follows_the_restatement(lbfgs_steps40, cid, nrep):
    """A kind-8 stage of 60 steps from coordinates set with c3d_set_coords (40 FIRE steps from the coil: RMS force ~450), L-BFGS for 40 of
    them (fresh start, ring wrap-around at m = 5 from step 7), then FIRE from a fresh state: every replica against the restatement after 3,
    12 and 60 steps.  The gap is fp32 rounding, then its growth: 1e-6 A after the first step (a move along the force), 2-5e-5 after the
    second (y = F_prev - F of fp32 forces), x1.3-1.5 a step after that (measured on the first four replicas: <= 4.7e-5 A at step 3, <= 7.1e-4
    at step 12; over all 20 at step 60: 0.049 chr21_1mb, 0.010 chr13_1mb, 0.038 chr1_500kb)."""
    solver = lbfgs_steps40
    IF = load_if(cid)
    d10, m, fire, x0 = _prepare(solver, IF, nrep, 40)
    stage = _stage(8, 60)
    bounds = {3: 2e-4, 12: 1e-2, 60: 0.1}
    x, nlb = _run_lbfgs(solver, [stage], x0, nrep, steps=[3])
    assert nlb == 3 and solver.step_kernel_name.startswith("c3d::k_lbfgs_eval<4, false, 2, "), solver.step_kernel_name
    worst = {3: _worst_vs_ref(x, x0, d10, m, fire, _stage(8, 3), 40)}
    b0 = solver.stat("lbfgs_steps")
    solver.run_steps(9)
    worst[12] = _worst_vs_ref(solver.coords(), x0, d10, m, fire, _stage(8, 12), 40)
    solver.run_steps(10 ** 6)
    assert solver.stat("lbfgs_steps") - b0 == 37
    worst[60] = _worst_vs_ref(solver.coords(), x0, d10, m, fire, stage, 40)
    print(f"{cid}: worst {worst} A")
    assert all(worst[k] < bounds[k] for k in bounds), worst


@pytest.mark.parametrize("variant", ["pot0", "pot1", "pot2", "pot3_clamp", "shipped", "gen1"])
def test_lbfgs_every_potential(lbfgs_steps40, variant):
    """Potentials 0-3, the shipped potential (device potential 4) and a general tail at N = 250 (last column block four columns a lane)."""
    from tests.test_gpu_step_kernels import VARIANTS
    kw, pot, gen = VARIANTS[variant]
    solver = lbfgs_steps40
    solver.set_option("final_minimiser_steps", 20)
    IF = synthetic_if(250, seed=250)[0]
    d10, m, fire, x0 = _prepare(solver, IF, 4, 30, kw)
    x, nlb = _run_lbfgs(solver, [_stage(8, 20)], x0, 4)
    assert nlb == 20
    name = solver.step_kernel_name
    assert name.startswith(f"c3d::k_lbfgs_eval<{pot}, {'true' if gen else 'false'}, "), name
    worst = _worst_vs_ref(x, x0, d10, m, fire, _stage(8, 20), 20)
    print(f"{variant}: worst {worst:.3g} A")
    assert worst < 1e-2, worst


@pytest.mark.parametrize("n", [1025, 2500, 5120])
def test_lbfgs_large_n(lbfgs_steps40, n):
    """Beyond the multi-step kernel's reach: the wide form (16 rows a workgroup) and the tile tails, 20 L-BFGS steps x 2 replicas."""
    solver = lbfgs_steps40
    IF = synthetic_if(n)[0]
    d10, m, fire, x0 = _prepare(solver, IF, 2, 10)
    x, nlb = _run_lbfgs(solver, [_stage(8, 20)], x0, 2)
    assert nlb == 20
    assert solver.step_kernel_name == "c3d::k_lbfgs_eval<4, false, 4, false, 16, true>", solver.step_kernel_name
    worst = _worst_vs_ref(x, x0, d10, m, fire, _stage(8, 20), 40)
    print(f"n = {n}: worst {worst:.3g} A")
    assert worst < 1e-2, worst


def test_lbfgs_same_bits_everywhere(lbfgs_steps40):
    """MD, then kind 8 (L-BFGS 40 steps, FIRE 20): the same bits for replica_groups 1 / 2 / 4, use_graph 0 / 1, one c3d_run_steps against
    chunks of 1, 7, 13 and the rest, replicas 3-5 of six against a context of three with first_replica 3, resident -1 against 0.  A kind-8
    stage run in many chunks captures its graphs once."""
    from chromosome3d_amd import Solver
    solver = lbfgs_steps40
    IF = load_if("chr13_1mb")
    _, _, _, x0 = _prepare(solver, IF, 6, 30)
    stages = [(0, 20, 0.003, 0.4, 0.003, 0.9, 2000.0), _stage(8, 60)]
    ref, nlb = _run_lbfgs(solver, stages, x0, 6)
    assert nlb == 40 and np.isfinite(ref).all()
    out = {}
    for key, val in (("replica_groups", 1), ("replica_groups", 4), ("use_graph", 0), ("resident", 0)):
        solver.set_option(key, val)
        try:
            out[f"{key}={val}"] = _run_lbfgs(solver, stages, x0, 6)[0]
        finally:
            solver.set_option(key, {"replica_groups": 2, "use_graph": 1, "resident": -1}[key])
    out["chunks"] = _run_lbfgs(solver, stages, x0, 6, steps=[1, 7, 13, 10 ** 6])[0]
    out["md+lbfgs in one"] = _run_lbfgs(solver, stages, x0, 6, steps=[40, 10 ** 6])[0]
    for k, v in out.items():
        assert np.array_equal(v, ref), k
    s2 = Solver(0)
    try:
        _prepare(s2, IF, 3, 30)
        s2.set_option("final_minimiser_steps", 40)
        x3, _ = _run_lbfgs(s2, stages, x0[3:], 3, first=3)
        assert np.array_equal(x3, ref[3:])
    finally:
        s2.close()
    # graphs: one capture per (parity, group) for a stage's chunks, however many chunks
    solver.set_option("final_minimiser_steps", 1000)
    from chromosome3d_amd import default_fire, make_stages
    solver.set_schedule(make_stages([_stage(8, 400)]), default_fire())
    solver.init_replicas(6, 82364, 0)
    solver.set_coords(x0)
    solver.run_steps(1)
    solver.run_steps(20)
    c0 = solver.stat("graph_captures")
    for _ in range(6):
        solver.run_steps(20)
    assert solver.stat("graph_captures") == c0
    assert solver.step_kernel_name.startswith("c3d::k_lbfgs_eval<"), solver.step_kernel_name


def test_lbfgs_schedules_and_api(lbfgs_steps40):
    from chromosome3d_amd import C3DError, default_fire, make_stages
    solver = lbfgs_steps40
    IF = load_if("chr21_1mb")
    _, _, _, x0 = _prepare(solver, IF, 4, 60)
    # MD after kind 8, FIRE after kind 8
    for stages in ([_stage(8, 50), (0, 20, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 10, 0.005, 1.0, 1.0, 1.0, 300.0)], [_stage(8, 30), _stage(2, 30)]):
        x, nlb = _run_lbfgs(solver, stages, x0, 4)
        assert nlb == min(stages[0][1], 40) and np.isfinite(x).all()
    # the gtol exit of c3d_run
    solver.set_option("final_minimiser_steps", 3000)
    solver.set_schedule(make_stages([_stage(8, 3000)]), default_fire(), 1e-2, 10)
    solver.init_replicas(4, 82364, 0)
    solver.set_coords(x0)
    solver.run()
    assert solver.last_timing()[1] < 3000 and solver.stat("rms_force") < 1e-2
    assert solver.step_kernel_name.startswith("c3d::k_lbfgs_eval<"), solver.step_kernel_name
    assert solver.stat("lbfgs_resets") >= 0
    # 3000 steps of L-BFGS with no exit test stay finite (gamma's clamp: a converged replica does not double it to inf)
    solver.set_schedule(make_stages([_stage(8, 3000)]), default_fire(), 0.0, 250)
    solver.init_replicas(4, 82364, 0)
    solver.set_coords(x0)
    before = solver.stat("lbfgs_steps")
    solver.run()                                            # raises on C3D_ERR_DIVERGED
    assert solver.stat("lbfgs_steps") - before == 3000 and np.isfinite(solver.coords()).all()
    solver.set_option("final_minimiser_steps", 40)
    # lbfgs_memory: 1..8; m = 3 and m = 5 end in different bits
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(C3DError):
            solver.set_option("lbfgs_memory", bad)
    x5, _ = _run_lbfgs(solver, [_stage(8, 40)], x0, 4)
    solver.set_option("lbfgs_memory", 3)
    x3, _ = _run_lbfgs(solver, [_stage(8, 40)], x0, 4)
    solver.set_option("lbfgs_memory", 5)
    assert not np.array_equal(x3, x5)
    # precision 64 with a kind-8 stage: refused in either order, nothing changes
    before = solver.coords()
    with pytest.raises(C3DError):
        solver.set_option("precision", 64)
    assert np.array_equal(solver.coords(), before)
    solver.set_schedule(make_stages([_stage(2, 10)]), default_fire())
    solver.set_option("precision", 64)
    try:
        with pytest.raises(C3DError):
            solver.set_schedule(make_stages([_stage(8, 10)]), default_fire())
    finally:
        solver.set_option("precision", 32)


@pytest.mark.parametrize("cid", ["chr13_1mb", "chr4_1mb"])
def test_lbfgs_final_stage_converges_faster(solver, cid):
    """The default schedule x 6 with its final stage as kind 8 against kind 5 (exit test every 10 steps): the final stage needs <= 0.7 x the
    steps, and the best-energy replica's Spearman(IF, d) is within 5e-3 of kind 5's."""
    from chromosome3d_amd import default_fire, default_model, default_schedule, pipeline
    IF = load_if(cid)
    res = {}
    for kind in (5, 8):
        solver.set_model(default_model())
        pipeline.IF2dist_new(solver, IF)
        sched = default_schedule(3000, final_kind=kind)
        fixed = sum(s.nsteps for s in sched[:-1])
        solver.set_schedule(sched, default_fire(), 1e-2, 10)
        solver.init_replicas(6, 82364, 0)
        before = solver.stat("lbfgs_steps")
        solver.run()
        final = solver.last_timing()[1] - fixed
        e = solver.energies().sum(axis=1)
        rho = solver.score(IF)[2]
        res[kind] = (final, float(np.asarray(rho)[int(np.argmin(e))]), solver.stat("lbfgs_steps") - before, solver.step_kernel_name)
    print(cid, res)
    assert res[8][2] > 0 and res[8][3].startswith("c3d::k_lbfgs_eval<"), res[8]
    assert res[8][0] <= 0.7 * res[5][0], res
    assert abs(res[8][1] - res[5][1]) <= 5e-3, res


def test_c3d_solve_lbfgs(built, tmp_path):
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--if",
                          MATRIX, "--out", str(tmp_path), "-m", "4", "--lbfgs"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    pdbs = sorted(tmp_path.glob("chr21_1mb_matrix_*.pdb"))
    assert len(pdbs) == 4
    assert all(sum(1 for l in open(p) if l.startswith("ATOM")) == 37 for p in pdbs)
