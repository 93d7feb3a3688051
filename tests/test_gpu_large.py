"""BASELINE.json configs[4]: synthetic N = 2500 (R ~ 3.1 M restraints), beyond anything the reference
can run (N <= 663, chromosome3D.pl:93-94).  Size-independent properties + oracle parity of one
force evaluation at full size."""
import numpy as np
import pytest

from tests.util import oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    return synthetic_if(2500)


def test_k1_and_forces_at_n2500(solver, big):
    from chromosome3d_amd import default_model, pipeline
    from oracle import oracle as O
    IF, truth = big
    n = IF.shape[0]
    m = default_model()
    solver.set_model(m)
    d10 = pipeline.IF2dist_new(solver, IF)
    assert np.array_equal(d10, O.if_to_dist10(IF))
    assert solver.num_restraints == (n - 5) * (n - 4) // 2          # every pair restrained: R = 3 113 760
    solver.init_replicas(2, 82364, 0)
    x = np.stack([truth.astype(np.float32) * 1.1, random_coil(n, 3) * 0.3])
    solver.set_coords(x)
    F, e = solver.eval(1.0, 1.0, 0.85)
    om = oracle_model_from(m, n)
    for r in range(2):
        Fo, eo = O.energy_force(om, d10, x[r].astype(np.float64), 1.0, 1.0, 0.85)
        scale = np.abs(Fo).max()
        assert (np.abs(F[r] - Fo) <= 2e-5 * np.abs(Fo) + 2e-6 * scale).all()
        assert np.allclose(e[r], eo, rtol=1e-6)
    assert (np.abs(F.sum(1)).max(1) < 5e-5 * np.abs(F).sum(1).max(1)).all()     # Newton's third law


def test_two_point_stage_on_the_wide_per_step_kernel_follows_the_oracle_at_n2500(solver, big):
    """Config 5's kernel — the per-step kernel's wide form, k_step<4, false, 4, false, 16, true> — through the final stage's kinds
    (chromosome3D.pl:1790-1803; kinds 6 / 5, the hand-over, 3 / 2) against the CPU restatement at N = 2500 x 2: 8 FIRE steps from the coil,
    then a kind-5 stage of 15 steps with the hand-over after 9 (round 5 held this form to a property test only for kind 5)."""
    from chromosome3d_amd import default_fire, default_model, make_stages, pipeline
    from oracle import oracle as O
    from tests.util import oracle_fire_from
    IF, _ = big
    n = IF.shape[0]
    stages = [(2, 8, 0.0, 1.0, 1.0, 0.85, 0.0), (5, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]
    m, fire = default_model(), default_fire()
    solver.set_option("final_minimiser_steps", 9)
    O.set_two_point_steps(9)
    try:
        solver.set_model(m)
        d10 = pipeline.IF2dist_new(solver, IF)
        solver.set_schedule(make_stages(stages), fire)
        solver.init_replicas(2, 82364, 0)
        x0 = solver.coords()
        assert solver.run_steps(10 ** 6) == 23
        assert "k_step<4, false, 4, false, 16, true>" in solver.step_kernel_name, solver.step_kernel_name
        x = solver.coords()
        om, of = oracle_model_from(m, n), oracle_fire_from(fire)
        for r in range(2):
            xo, _, ev = O.run_schedule(om, d10, O.make_stages(stages), of, 82364, r, x0=x0[r].astype(np.float64))
            xc = x[r].astype(np.float64)
            xc -= xc.mean(0)
            assert ev == 23
            assert np.abs(xc - xo).max() < 4e-3, np.abs(xc - xo).max()
    finally:
        solver.set_option("final_minimiser_steps", 1000)
        O.set_two_point_steps(1000)


def test_md_kinds_on_the_wide_per_step_kernel_follow_the_oracle_at_n2500(solver, big):
    """The wide per-step kernel, k_step<4, false, 4, false, 16, true>, through the MD kinds at N = 2500 x 2 (the test above holds it to the
    oracle for the minimiser kinds only): 8 FIRE steps from the coil, 12 MD steps at 2000 K (kind 4 begins the stage, then kind 0), 8 steps
    of kind 1.  Measured worst: 8.1e-5 A (coordinates)."""
    from chromosome3d_amd import default_fire, default_model, make_stages, pipeline
    from oracle import oracle as O
    from tests.util import oracle_fire_from
    IF, _ = big
    n = IF.shape[0]
    stages = [(2, 8, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 12, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 8, 0.005, 1.0, 0.05, 1.0, 1500.0)]
    m, fire = default_model(), default_fire()
    solver.set_model(m)
    d10 = pipeline.IF2dist_new(solver, IF)
    solver.set_schedule(make_stages(stages), fire)
    solver.init_replicas(2, 82364, 0)
    x0 = solver.coords()
    assert solver.run_steps(10 ** 6) == 28
    assert solver.step_kernel_name == "c3d::k_step<4, false, 4, false, 16, true>", solver.step_kernel_name
    x, v = solver.coords(), solver.velocities()
    om, of = oracle_model_from(m, n), oracle_fire_from(fire)
    worst = 0.0
    for r in range(2):
        xo, vo, ev = O.run_schedule(om, d10, O.make_stages(stages), of, 82364, r, x0=x0[r].astype(np.float64))
        xc = x[r].astype(np.float64)
        xc -= xc.mean(0)
        assert ev == 28
        worst = max(worst, float(np.abs(xc - xo).max()))
        assert np.abs(v[r] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max())
    assert worst < 2e-3, worst
    print(f"N=2500 MD kinds on the wide kernel: worst {worst:.2e} A")


@pytest.mark.parametrize("n", [5120, 4097])
def test_fp32_path_at_its_bead_limit_follows_the_oracle(solver, n):
    """The fp32 path at the largest size it accepts (5120 beads: 3 npad floats of a replica in LDS, step_lds_bytes 61 744 of 65 536 B) and
    at 4097 (odd: the last wide workgroup owns a tile of one bead): K1 bit-exact; forces and energies of two coordinate sets (stretched,
    collapsed) against the oracle; Newton's third law; ten FIRE and ten MD steps through the wide per-step kernel against the oracle.
    Measured worst after the 20 steps: 4.0e-5 A (5120), 5.0e-5 A (4097)."""
    from chromosome3d_amd import default_fire, default_model, make_stages, pipeline
    from oracle import oracle as O
    from tests.util import oracle_fire_from
    IF, truth = synthetic_if(n, seed=n)
    m, fire = default_model(), default_fire()
    solver.set_model(m)
    d10 = pipeline.IF2dist_new(solver, IF)
    assert np.array_equal(d10, O.if_to_dist10(IF))
    del IF
    om = oracle_model_from(m, n)
    solver.init_replicas(1, 82364, 0)
    for x in (truth.astype(np.float32) * 1.1, random_coil(n, 3) * 0.3):
        solver.set_coords(x[None])
        F, e = solver.eval(1.0, 1.0, 0.85)
        Fo, eo = O.energy_force(om, d10, x.astype(np.float64), 1.0, 1.0, float(np.float32(0.85)))
        assert (np.abs(F[0] - Fo) <= 1e-5 * np.abs(Fo) + 1e-6 * np.abs(Fo).max()).all(), np.abs(F[0] - Fo).max()
        assert np.allclose(e[0], eo, rtol=1e-7, atol=1e-6), (e[0], eo)
        assert np.abs(F[0].sum(0)).max() < 5e-5 * np.abs(F[0]).sum(0).max()          # Newton's third law
    stages = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 10, 0.003, 0.4, 0.003, 0.9, 2000.0)]
    solver.set_schedule(make_stages(stages), fire)
    solver.init_replicas(1, 82364, 0)
    x0 = solver.coords()
    assert solver.run_steps(10 ** 6) == 20
    assert solver.step_kernel_name == "c3d::k_step<4, false, 4, false, 16, true>", solver.step_kernel_name
    xo, vo, ev = O.run_schedule(om, d10, O.make_stages(stages), oracle_fire_from(fire), 82364, 0, x0=x0[0].astype(np.float64))
    xc = solver.coords()[0].astype(np.float64)
    xc -= xc.mean(0)
    assert ev == 20
    worst = float(np.abs(xc - xo).max())
    assert worst < 2e-3, worst
    assert np.abs(solver.velocities()[0] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max())
    print(f"N={n}: worst {worst:.2e} A after 20 steps")


def test_anneal_recovers_synthetic_structure(solver, big):
    """Ground truth is known: after the schedule the model's pair distances correlate with the
    generating structure's (Spearman > 0.9) and Spearman(IF, d) is strongly negative."""
    from chromosome3d_amd import default_model, default_schedule, pipeline
    from scipy.stats import spearmanr
    IF, truth = big
    n = IF.shape[0]
    solver.set_model(default_model())
    pipeline.IF2dist_new(solver, IF)
    solver.set_schedule(default_schedule(1500), None, 0.0, 250)
    solver.init_replicas(8, 82364, 0)            # BASELINE configs[4]: 8 replicas
    solver.run()
    ms, steps, launches = solver.last_timing()
    x = solver.coords()
    e = solver.energies()
    assert np.isfinite(x).all() and np.isfinite(e).all()
    rng = np.random.default_rng(0)
    i = rng.integers(0, n, 200000)
    j = rng.integers(0, n, 200000)
    keep = np.abs(i - j) >= 3
    dt = np.linalg.norm(truth[i[keep]] - truth[j[keep]], axis=1)
    for r in range(8):
        dm = np.linalg.norm(x[r, i[keep]] - x[r, j[keep]], axis=1)
        assert spearmanr(dt, dm)[0] > 0.9
        assert spearmanr(IF[i[keep], j[keep]], dm)[0] < -0.85
    # the replicas are independent draws (different random coils), not copies
    assert len({round(float(v), 1) for v in e[:, 0]}) == 8
    # replica composition does not change a replica: replicas 2..3 alone reproduce columns 2..3 of the batch of eight
    solver.init_replicas(2, 82364, 2)
    solver.run()
    assert np.array_equal(solver.coords(), x[2:4])
    print(f"N=2500 x 8 replicas: {steps} SA steps in {ms:.1f} ms = {1e3 * ms / launches:.1f} us/step")


@pytest.mark.gpu
@pytest.mark.parametrize("n,nrep", [(256, 3), (257, 3), (600, 2), (760, 2), (9, 5), (64, 11), (65, 11)])
def test_cluster_kernel_every_column_block_count(solver, n, nrep):
    """Cluster kernel instantiations for 1..3 column blocks (targets held in registers), the block boundary
    N = 256 / 257, the largest N whose replica fits one XCD's 32 CUs, one-workgroup replicas (N <= 64, no hand-off)
    and the first size with two workgroups: same bits as the per-step path after MD and FIRE steps."""
    from chromosome3d_amd import default_model, make_stages
    from tests.util import synthetic_if
    IF, _ = synthetic_if(n, seed=7)
    out = []
    for resident in (0, 1):
        solver.set_model(default_model())
        solver.set_if_matrix(IF)
        solver.set_schedule(make_stages([(2, 12, 0.0, 1.0, 1.0, 0.85, 0.0), (0, 20, 0.003, 1.0, 0.5, 0.9, 2000.0),
                                         (1, 20, 0.005, 1.0, 0.01, 0.9, 500.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]))
        solver.set_option("resident", resident)
        solver.init_replicas(nrep, 3, 0)
        solver.run_steps(10 ** 6)
        out.append((solver.coords(), solver.velocities(), solver.last_timing()[2]))
    solver.set_option("resident", -1)
    assert solver.stat("cluster_parts") >= 1
    assert out[1][2] == 1 and out[0][2] > 60
    assert np.isfinite(out[0][0]).all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1100, 1030])
def test_symmetric_tile_step_matches_oracle_and_per_step_kernel(solver, n):
    """Large-N step kernels (c3d_sym.hip: every pair once, row- and column-side partial forces summed in a fixed order):
    short MD + FIRE trajectories against the fp64 oracle, and against the per-step kernel that walks full rows (the two
    differ in the order of a row's sum, so within rounding, not bitwise).  n = 1030: a last row group of 6 rows and a
    column block that is almost all padding."""
    from chromosome3d_amd import default_fire, default_model, make_stages, pipeline
    from oracle import oracle as O
    from tests.util import oracle_fire_from, synthetic_if
    IF, _ = synthetic_if(n, seed=5)
    stages = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 12, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 8, 0.005, 1.0, 0.05, 1.0, 1500.0),
              (2, 10, 0.0, 1.0, 1.0, 0.85, 0.0)]
    m, fire = default_model(), default_fire()
    out = {}
    for sym in (1, 0):
        solver.set_option("symmetric", sym)
        solver.set_model(m)
        d10 = pipeline.IF2dist_new(solver, IF)
        solver.set_schedule(make_stages(stages), fire)
        solver.init_replicas(2, 82364, 0)
        x0 = solver.coords()
        assert solver.run_steps(10 ** 6) == 40
        out[sym] = (solver.coords(), solver.velocities(), solver.step_kernel_name)
    solver.set_option("symmetric", 0)
    assert "k_pairs_sym" in out[1][2] and "k_step<4, false, 4, false, 16, true>" in out[0][2]
    assert np.abs(out[1][0] - out[0][0]).max() < 5e-4 and np.abs(out[1][1] - out[0][1]).max() < 5e-3
    om, of = oracle_model_from(m, n), oracle_fire_from(fire)
    for r in range(2):
        xo, vo, ev = O.run_schedule(om, d10, O.make_stages(stages), of, 82364, r, x0=x0[r].astype(np.float64))
        assert ev == 40
        for form in (1, 0):      # symmetric tiles; the per-step kernel (its wide form beyond n = 1024: 16 rows a workgroup, four a wave)
            xc = out[form][0][r].astype(np.float64)
            xc -= xc.mean(0)
            assert np.abs(xc - xo).max() < 2e-3, (form, np.abs(xc - xo).max())
            assert np.abs(out[form][1][r] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max())


@pytest.mark.parametrize("n", [1101, 1041, 1025, 2049])
def test_resident_pair_targets_change_no_bit_and_wide_tiles_agree(solver, n):
    """Beyond the cluster kernel's reach (n > 1024) the per-step kernel of the shipped potential reads pre-scaled targets of row pairs
    (DevModel::tgs2: t / mrs, "no restraint" as 1e30) instead of forming the pair constants from the target matrix in every step: same
    operations per restrained pair, an exact zero either way for the others — the trajectories must agree bit for bit (option
    pair_targets 0 = the constants formed per step; option wide_tiles 0 = the narrow form of the kernel, eight rows a workgroup and one
    packed row pair a wave).  The wide form — 16 rows a workgroup, two packed row pairs a wave, resident targets only: the default —
    against the narrow one: another order of a row's sum, so within rounding after 50 chaotic steps, not bitwise.  Odd bead counts: the last row pair's second row is a repeat of the last bead; n = 1041: an odd number of 8-row
    tiles, the last workgroup of the wide form owns one; n = 1025 and 2049: that tile holds a single bead."""
    from chromosome3d_amd import default_fire, default_model, make_stages, pipeline
    IF, _ = synthetic_if(n, seed=11)
    stages = make_stages([(2, 12, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 25, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 13, 0.005, 1.0, 0.5, 0.9, 1000.0)])
    out = {}
    try:
        for wide, on in ((1, 1), (0, 1), (0, 0), (1, 0)):
            solver.set_option("wide_tiles", wide)
            solver.set_option("pair_targets", on)
            solver.set_model(default_model())
            pipeline.IF2dist_new(solver, IF)
            solver.set_schedule(stages, default_fire(), 0.0, 250)
            solver.init_replicas(3, 82364, 0)
            assert solver.run_steps(10 ** 6) == 50
            # (the wide form reads the resident pair targets only: without them the launcher takes the narrow form)
            assert ("k_step<4, false, 4, false, 16, true>" if wide and on else "k_step<4, false, 2, false, 8, false>") in solver.step_kernel_name
            out[wide, on] = (solver.coords().copy(), solver.velocities().copy())
    finally:
        solver.set_option("pair_targets", 1)
        solver.set_option("wide_tiles", 1)
    assert np.isfinite(out[1, 1][0]).all() and np.isfinite(out[0, 1][0]).all()
    for a, b in (((0, 1), (0, 0)), ((0, 0), (1, 0))):
        assert np.array_equal(out[a][0], out[b][0]) and np.array_equal(out[a][1], out[b][1])
    assert np.abs(out[1, 1][0] - out[0, 1][0]).max() < 2e-3 and np.abs(out[1, 1][1] - out[0, 1][1]).max() < 2e-2
