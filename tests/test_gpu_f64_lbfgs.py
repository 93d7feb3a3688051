"""Stage kind 8 on a precision-64 context (option f64_lbfgs): k64_lbfgs_eval[_chunked] + k64_lbfgs_move (csrc/c3d_f64.hip), then FIRE.
Held to the fp64 restatement (tests/lbfgs_ref.py lbfgs_run, gamma_0 = dt_start^2 * 418.4 / mass formed in fp64, the oracle's force; the FIRE
tail from oracle.run_schedule from a fresh state) replica by replica within the project's fp64 tolerance, max(2e-5, 1.2e-7 max|x|) A after
centring: the fp32 read-back's grain.  Every form of the evaluation, the chunked form against the staged one bit for bit, past the staged
limit, the 16384-bead ceiling, the same bits across replica groups / graphs / chunking / first_replica, the option's rules, convergence
against kind 5, the CLI.  Every test asserts, by kernel name and the stat lbfgs_steps, that the fp64 L-BFGS kernels ran.

Every test here runs on a context of its own (module fixture), never the session's: precision 64, f64_lbfgs and both limits stay raised."""
import os
import subprocess

import numpy as np
import pytest

from tests import lbfgs_ref as L
from tests.util import GOLD, load_if, oracle_fire_from, oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = os.path.join(GOLD, "inputs", "chr21_1mb_matrix.txt")
LB = (1.0, 1.0, 0.85)                    # the final stage's weights: w_all, w_vdw, repel_s
MD = (0, 0, 0.003, 0.4, 0.003, 0.9, 2000.0)


def _stage(kind, n, w=LB):
    return (kind, n, 0.0, w[0], w[1], w[2], 0.0)


def _md(n):
    return (MD[0], n) + MD[2:]


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    s.set_option("max_beads", 16384)
    s.set_option("f64_max_beads", 16384)
    s.set_option("f64_lbfgs", 1)
    s.set_option("precision", 64)
    yield s
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _prepare(s, IF, nrep, pre_fire, model_kw=None):
    """model and targets, then `pre_fire` FIRE steps from the coil: the start coordinates of the tests (float32, as c3d_set_coords takes them)"""
    from chromosome3d_amd import default_fire, default_model, make_stages
    m = default_model(**(model_kw or {}))
    s.set_model(m)
    s.set_if_matrix(IF)
    fire = default_fire()
    s.set_schedule(make_stages([(2, pre_fire, 0.0, 1.0, 20.0, 0.5, 0.0)]), fire)
    s.init_replicas(nrep, 82364, 0)
    s.run_steps(pre_fire)
    return m, fire, s.coords()


def _begin(s, stages, x0, nrep, nl, first=0, gtol=0.0, check_every=250):
    from chromosome3d_amd import default_fire, make_stages
    s.set_option("final_minimiser_steps", nl)
    s.set_schedule(make_stages(stages), default_fire(), gtol, check_every)
    s.init_replicas(nrep, 82364, first)
    s.set_coords(x0)


def _run(s, stages, x0, nrep, nl, steps=(10 ** 6,), first=0):
    """`stages` from x0 in the given run_steps calls: coordinates, the velocity slot, L-BFGS steps run, kernel name after the last call"""
    _begin(s, stages, x0, nrep, nl, first)
    before = s.stat("lbfgs_steps")
    for k in steps:
        s.run_steps(k)
    return s.coords(), s.velocities(), s.stat("lbfgs_steps") - before, s.step_kernel_name


def _restatement(O, m, fire, d10, x0, stage, nl, mem=5, replica=0):
    """lbfgs_run for min(nsteps, nl) steps with gamma_0 in fp64, then the oracle's FIRE from a fresh state; centred"""
    om, of = oracle_model_from(m, x0.shape[0]), oracle_fire_from(fire)
    _, nsteps, _, w_all, w_vdw, repel_s, _ = stage
    # the values the C ABI receives (its stage weights are floats: 0.85 -> 0.8500000238); with repel_s left a double the restatement ends
    # 7.0e-5 A away after 40 steps (chr21_1mb replica 3: 3.5e-6 after 12), two restatements apart and the device on the float's side
    w_all, w_vdw, repel_s = (float(np.float32(a)) for a in (w_all, w_vdw, repel_s))
    force = lambda u: O.energy_force(om, d10, u, w_all, w_vdw, repel_s)[0]
    g0 = float(fire.dt_start) ** 2 * 418.4 / float(m.mass)
    k = min(nsteps, nl)
    x, info = L.lbfgs_run(force, x0.astype(np.float64), k, m=mem, g0=g0, max_step=float(fire.max_step))
    if nsteps > k:
        x, _, ev = O.run_schedule(om, d10, O.make_stages([(2, nsteps - k, 0.0, w_all, w_vdw, repel_s, 0.0)]), of, 82364, replica, x0=x)
        assert ev == nsteps - k
    return x - x.mean(0)


def _gaps(O, m, fire, d10, x0, x, stage, nl, mem=5):
    """(gap, tolerance) of every replica against the restatement"""
    out = []
    for r in range(x.shape[0]):
        xo = _restatement(O, m, fire, d10, x0[r], stage, nl, mem, r)
        xc = x[r].astype(np.float64)
        xc -= xc.mean(0)
        out.append((float(np.abs(xc - xo).max()), max(2e-5, 1.2e-7 * float(np.abs(xo).max()))))
    return out


def _assert_within(gaps, label):
    print(label, " ".join(f"{e:.2e}/{t:.2e}" for e, t in gaps))
    assert all(np.isfinite(e) and e < t for e, t in gaps), (label, gaps)


def _tail(pot, gen, fold):
    return f"{pot}, {'true' if gen else 'false'}, {'true' if fold else 'false'}"


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,nrep", [("chr21_1mb", 4), ("syn96", 2), ("syn250", 2), ("chr1_500kb", 4)])
def test_follows_the_restatement(ctx, O, case, nrep):
    """A kind-8 stage of 50 steps, L-BFGS for 40 of them (ring wrap-around at m = 5), then FIRE from a fresh state, from coordinates set
    with c3d_set_coords after 40 FIRE steps from the coil; every replica after 3, 12 and 50 steps.  chr21_1mb: n = 37, left-over columns
    only, one row per pass; 96: a 64-column block and 32 left-over columns in the two-rows pass; 250: main loop + block + 58; chr1_500kb: 455.
    Measured: chr21_1mb <= 8.5e-7 A after 3 steps, 9.6e-7 after 12, 1.1e-6 after 50; 96 and 250 beads <= 9.9e-7 throughout; chr1_500kb
    <= 1.9e-6 after 12 and 50 — the fp32 read-back's half ulp at every checkpoint, no growth to see (n = 2561 after 12 steps and n = 16384
    after 2: 3.8e-6)."""
    s = ctx
    IF = load_if(case) if case.startswith("chr") else synthetic_if(int(case[3:]), seed=int(case[3:]))[0]
    m, fire, x0 = _prepare(s, IF, nrep, 40)
    d10 = O.if_to_dist10(IF)
    for upto, nlb in ((3, 3), (12, 12), (50, 40)):
        x, _, n_l, name = _run(s, [_stage(8, 50)], x0, nrep, 40, steps=(upto,))
        assert n_l == nlb, (upto, n_l)
        if upto <= 40:
            assert name == f"c3d::k64_lbfgs_eval<{_tail(4, False, True)}>", name
        else:
            assert name == f"c3d::k64_step<{_tail(4, False, True)}>", name
        _assert_within(_gaps(O, m, fire, d10, x0, x, _stage(8, upto), 40), f"{case} after {upto}:")


CLAMP = {"pot0": (dict(noe_pot=0), 0), "pot1": (dict(noe_pot=1), 1), "pot2": (dict(noe_pot=2), 2),
         "pot3_clamp": (dict(noe_pot=3, mrswitch=4.0, masym=8.0, msoexp=1), 3)}


@pytest.mark.parametrize("variant", ["shipped", "pot0", "pot1", "pot2", "pot3_clamp", "gen0", "gen1", "gen2", "gen3", "w_all=0"])
def test_every_form(ctx, O, variant):
    """n = 250 x 2, 20 L-BFGS steps: the shipped potential (<4, false, true>: FOLD), the clamp forms of potentials 0-3, the four general
    tails of test_gpu_f64_large.GENERAL, and the shipped potential in a kind-8 stage without restraint weight (w_all = 0: form64 drops
    FOLD, <4, false, false>; repel and nothing else acts)."""
    from tests.test_gpu_f64_large import GENERAL
    s = ctx
    w = LB
    if variant == "shipped":
        kw, form = {}, (4, False, True)
    elif variant == "w_all=0":
        kw, form, w = {}, (4, False, False), (0.0, 4.0, 1.2)
    elif variant in CLAMP:
        kw, form = CLAMP[variant][0], (CLAMP[variant][1], False, False)
    else:
        kw, form = GENERAL[variant][0], (GENERAL[variant][1], True, False)
    IF = synthetic_if(250, seed=250)[0]
    try:
        m, fire, x0 = _prepare(s, IF, 2, 30, kw)
        d10 = O.if_to_dist10(IF)
        x, _, n_l, name = _run(s, [_stage(8, 20, w)], x0, 2, 20)
        assert n_l == 20 and name == f"c3d::k64_lbfgs_eval<{_tail(*form)}>", (n_l, name)
        _assert_within(_gaps(O, m, fire, d10, x0, x, _stage(8, 20, w), 20), f"{variant}:")
    finally:
        from chromosome3d_amd import default_model
        s.set_model(default_model())


@pytest.mark.parametrize("n,chunks", [(257, (256,)), (383, (256,)), (545, (256,)), (1025, (256, 1024))])
def test_chunked_form_has_the_bits_of_the_staged_form(ctx, n, chunks):
    """MD 10 steps, then kind 8 of 30 steps (20 L-BFGS + 10 FIRE), 2 replicas: k64_lbfgs_eval_chunked at f64_column_chunk 256 (and 1024 at
    n = 1025) ends in k64_lbfgs_eval's bits, coordinates and velocity slot (the force, inside the L-BFGS part), both compared after the
    L-BFGS part and at the end of the stage."""
    s = ctx
    IF = synthetic_if(n, seed=n)[0]
    _, _, x0 = _prepare(s, IF, 2, 10)
    stages = [_md(10), _stage(8, 30)]
    out = {}
    for chunk in (0,) + chunks:
        s.set_option("f64_column_chunk", chunk)
        try:
            xa, va, n_l, name = _run(s, stages, x0, 2, 20, steps=(30,))
            want = f"c3d::k64_lbfgs_eval_chunked<{_tail(4, False, True)}, {chunk}>" if chunk else f"c3d::k64_lbfgs_eval<{_tail(4, False, True)}>"
            assert n_l == 20 and name == want, (n_l, name)
            s.run_steps(10 ** 6)
            out[chunk] = (xa, va, s.coords(), s.velocities())
        finally:
            s.set_option("f64_column_chunk", 0)
    assert all(np.isfinite(a).all() for a in out[0])
    for chunk in chunks:
        for a, b, what in zip(out[chunk], out[0], ("x after L-BFGS", "force slot", "x at the end", "v at the end")):
            assert np.array_equal(a, b), (chunk, what, float(np.abs(a - b).max()))


def test_past_the_staged_limit(ctx, O):
    """n = 2561 x 1 with the default chunk: k64_lbfgs_eval_chunked<4, false, true, 512>, 12 L-BFGS steps against the restatement."""
    s = ctx
    n = 2561
    IF = synthetic_if(n, seed=n)[0]
    m, fire, x0 = _prepare(s, IF, 1, 10)
    d10 = O.if_to_dist10(IF)
    x, _, n_l, name = _run(s, [_stage(8, 12)], x0, 1, 40)
    assert n_l == 12 and name == f"c3d::k64_lbfgs_eval_chunked<{_tail(4, False, True)}, 512>", (n_l, name)
    _assert_within(_gaps(O, m, fire, d10, x0, x, _stage(8, 12), 40), "n = 2561:")


def test_the_ceiling_16384(ctx, O):
    """n = 16384, one replica, test_gpu_f64_large.test_the_ceiling_16384's sparse restraint set through c3d_set_restraints: two steps (kind
    9, then one kind 8: y, the ring slot and the partials of 2048 tiles), finite, and against the restatement on the dense tenths."""
    from chromosome3d_amd import default_fire, default_model
    s = ctx
    n = 16384
    rng = np.random.default_rng(16384)
    truth = random_coil(n, 7) * 0.25
    ri = np.concatenate([np.arange(n - k) for k in range(5, 65)])          # banded part: |i - j| = 5 .. 64 (min_sep 5)
    rj = np.concatenate([np.arange(k, n) for k in range(5, 65)])
    li = rng.integers(0, n, 120000)
    lj = rng.integers(0, n, 120000)
    keep = np.abs(li - lj) > 64
    li, lj = np.minimum(li, lj)[keep][:100000], np.maximum(li, lj)[keep][:100000]
    ri, rj = np.concatenate([ri, li]), np.concatenate([rj, lj])
    d = np.linalg.norm(truth[ri] - truth[rj], axis=1)
    t10 = np.maximum(np.round(d * 10.0), 10).astype(np.int32)
    m = default_model()
    s.set_model(m)
    s.set_restraints(n, (ri + 1).astype(np.int32), (rj + 1).astype(np.int32), t10)
    x0 = (truth * 1.1).astype(np.float32)[None]
    x, f, n_l, name = _run(s, [_stage(8, 2)], x0, 1, 40)
    assert n_l == 2 and name == f"c3d::k64_lbfgs_eval_chunked<{_tail(4, False, True)}, 512>", (n_l, name)
    assert np.isfinite(x).all() and np.isfinite(f).all()
    d10 = np.zeros((n, n), dtype=np.int32)
    d10[ri, rj] = t10
    d10[rj, ri] = t10
    del ri, rj, li, lj
    _assert_within(_gaps(O, m, default_fire(), d10, x0, x, _stage(8, 2), 40), "n = 16384:")


def test_same_bits_everywhere(ctx):
    """chr13_1mb x 6, MD 20 steps + kind 8 of 60 steps (L-BFGS 40, FIRE 20): the same bits for replica_groups 1 / 2 / 4, use_graph 0 / 1, one
    c3d_run_steps against chunks of 1, 7, 13 and the rest, replicas 3-5 of six against a second context of three with first_replica 3.  A
    long kind-8 stage run in many chunks captures its graphs once."""
    from chromosome3d_amd import Solver
    s = ctx
    IF = load_if("chr13_1mb")
    _, _, x0 = _prepare(s, IF, 6, 30)
    stages = [_md(20), _stage(8, 60)]
    ref, vref, n_l, _ = _run(s, stages, x0, 6, 40)
    assert n_l == 40 and np.isfinite(ref).all()
    out = {}
    for key, val in (("replica_groups", 1), ("replica_groups", 4), ("use_graph", 0)):
        s.set_option(key, val)
        try:
            out[f"{key}={val}"] = _run(s, stages, x0, 6, 40)[:2]
        finally:
            s.set_option(key, {"replica_groups": 2, "use_graph": 1}[key])
    out["chunks"] = _run(s, stages, x0, 6, 40, steps=(1, 7, 13, 10 ** 6))[:2]
    x_mid = _run(s, stages, x0, 6, 40, steps=(60,))
    assert x_mid[2] == 40 and x_mid[3] == f"c3d::k64_lbfgs_eval<{_tail(4, False, True)}>", x_mid[2:]
    s.run_steps(10 ** 6)
    out["md+lbfgs in one"] = (s.coords(), s.velocities())
    for k, (x, v) in out.items():
        assert np.array_equal(x, ref) and np.array_equal(v, vref), k
    s2 = Solver(0)
    try:
        s2.set_option("f64_lbfgs", 1)
        s2.set_option("precision", 64)
        _prepare(s2, IF, 3, 30)
        x3, v3, n3, _ = _run(s2, stages, x0[3:], 3, 40, first=3)
        assert n3 == 40 and np.array_equal(x3, ref[3:]) and np.array_equal(v3, vref[3:])
    finally:
        s2.close()
    # graphs: one capture per (parity, group) for a stage's chunks, however many chunks
    _begin(s, [_stage(8, 400)], x0, 6, 1000)
    s.run_steps(1)
    s.run_steps(20)
    c0 = s.stat("graph_captures")
    for _ in range(6):
        s.run_steps(20)
    assert s.stat("graph_captures") == c0
    assert s.step_kernel_name == f"c3d::k64_lbfgs_eval<{_tail(4, False, True)}>", s.step_kernel_name


def test_option_and_api_rules(ctx):
    from chromosome3d_amd import C3DError, Solver, default_fire, default_model, make_stages
    lb, fire_only = make_stages([_stage(8, 10)]), make_stages([_stage(2, 10)])
    f = Solver(0)
    try:
        f.set_model(default_model())
        for bad in (2, -1, 0.5):
            with pytest.raises(C3DError):
                f.set_option("f64_lbfgs", bad)
        # f64_lbfgs 0 (the default, and set explicitly): both refusals, today's messages
        f.set_option("f64_lbfgs", 0)
        f.set_schedule(lb, default_fire())
        with pytest.raises(C3DError, match="no fp64 form"):
            f.set_option("precision", 64)
        f.set_schedule(fire_only, default_fire())
        f.set_option("precision", 64)
        with pytest.raises(C3DError, match="no fp64 form; set precision 32 first"):
            f.set_schedule(lb, default_fire())
        # f64_lbfgs 1: both orders accepted
        f.set_option("f64_lbfgs", 1)
        f.set_schedule(lb, default_fire())
        f.set_option("precision", 32)
        f.set_option("precision", 64)
        # back to 0: refused while precision is 64 and the schedule holds a kind-8 stage
        with pytest.raises(C3DError, match="f64_lbfgs"):
            f.set_option("f64_lbfgs", 0)
        f.set_schedule(fire_only, default_fire())
        f.set_option("f64_lbfgs", 0)
        f.set_option("f64_lbfgs", 1)
        f.set_schedule(lb, default_fire())
        f.set_option("precision", 32)
        f.set_option("f64_lbfgs", 0)
    finally:
        f.close()
    s = ctx
    IF = load_if("chr21_1mb")
    _, _, x0 = _prepare(s, IF, 4, 60)
    name = f"c3d::k64_lbfgs_eval<{_tail(4, False, True)}>"
    # lbfgs_memory 3 and 5 end in different bits
    try:
        x5, _, n5, name5 = _run(s, [_stage(8, 40)], x0, 4, 40)
        s.set_option("lbfgs_memory", 3)
        x3, _, n3, name3 = _run(s, [_stage(8, 40)], x0, 4, 40)
    finally:
        s.set_option("lbfgs_memory", 5)
    assert n5 == 40 and n3 == 40 and name5 == name and name3 == name
    assert np.isfinite(x3).all() and np.isfinite(x5).all() and not np.array_equal(x3, x5)
    # the gtol exit of c3d_run
    _begin(s, [_stage(8, 3000)], x0, 4, 3000, gtol=1e-2, check_every=10)
    before = s.stat("lbfgs_steps")
    s.run()
    assert s.last_timing()[1] < 3000 and s.stat("rms_force") < 1e-2, (s.last_timing(), s.stat("rms_force"))
    assert s.stat("lbfgs_steps") - before == s.last_timing()[1] and s.step_kernel_name == name
    assert s.stat("lbfgs_resets") >= 0
    # 3000 steps without an exit test stay finite
    _begin(s, [_stage(8, 3000)], x0, 4, 3000)
    before = s.stat("lbfgs_steps")
    s.run()                                                 # raises on C3D_ERR_DIVERGED
    assert s.stat("lbfgs_steps") - before == 3000 and s.step_kernel_name == name
    assert np.isfinite(s.coords()).all() and np.isfinite(s.velocities()).all()


def test_final_stage_converges_faster(ctx):
    """chr13_1mb x 6, the default schedule in fp64 with its final stage as kind 8 against kind 5 (exit test every 10 steps): the final stage
    needs <= 0.7 x the steps, the best-energy replica's Spearman(IF, d) is within 5e-3 of kind 5's (the fp32 test's two numbers)."""
    from chromosome3d_amd import default_fire, default_model, default_schedule
    s = ctx
    IF = load_if("chr13_1mb")
    s.set_option("final_minimiser_steps", 1000)
    res = {}
    for kind in (5, 8):
        s.set_model(default_model())
        s.set_if_matrix(IF)
        sched = default_schedule(3000, final_kind=kind)
        fixed = sum(st.nsteps for st in sched[:-1])
        s.set_schedule(sched, default_fire(), 1e-2, 10)
        s.init_replicas(6, 82364, 0)
        before = s.stat("lbfgs_steps")
        s.run()
        final = s.last_timing()[1] - fixed
        e = s.energies().sum(axis=1)
        rho = s.score(IF)[2]
        res[kind] = (final, float(np.asarray(rho)[int(np.argmin(e))]), s.stat("lbfgs_steps") - before, s.step_kernel_name)
    print(res)
    assert res[8][2] > 0 and res[5][2] == 0, res
    assert res[8][3] in (f"c3d::k64_lbfgs_eval<{_tail(4, False, True)}>", f"c3d::k64_step<{_tail(4, False, True)}>"), res[8]
    assert res[8][0] <= 0.7 * res[5][0], res
    assert abs(res[8][1] - res[5][1]) <= 5e-3, res


def test_c3d_solve_precision_64_lbfgs(tmp_path):
    out = subprocess.run([os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve"), "--if", MATRIX, "--out", str(tmp_path), "-m", "4",
                          "--precision", "64", "--lbfgs"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    pdbs = sorted(tmp_path.glob("chr21_1mb_matrix_*.pdb"))
    assert len(pdbs) == 4
    assert all(sum(1 for l in open(p) if l.startswith("ATOM")) == 37 for p in pdbs)
