"""Every step kernel against the fp64 oracle, beyond what the benchmark runs: each NOE potential (and its general-tail form) through
the three launch forms — k_cluster / k_cluster_tp (many steps per launch), k_step (one launch per step), k64_step (fp64) — the fp64
kernel's column layouts up to its 2560-bead limit, a model switched on a live context, device scoring past the rank-prefetch limit, and
the fourth form, the opt-in symmetric tiles (k_pairs_sym + k_update_sym, option symmetric 1): potentials, tile layouts, replica indexing.

Every test asserts through the kernel name and the launch counters that the kernel it claims to test ran.  Tolerances are those of
test_gpu_parity.py: fp32 coordinates 2e-3 A (5e-3 A once two-point steps are involved), fp64 2e-5 A (the grain of the fp32 read-back).
"""
import functools
import time

import numpy as np
import pytest

from tests.util import load_if, oracle_fire_from, oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# Model variants: (c3d_model fields, device potential, general-tail form).  Device potential 4 is the shipped lower side's fast form.
VARIANTS = {
    "shipped": ({}, 4, False),
    "pot0": (dict(noe_pot=0), 0, False),
    "pot1": (dict(noe_pot=1), 1, False),
    "pot2": (dict(noe_pot=2), 2, False),
    "pot3_clamp": (dict(noe_pot=3, mrswitch=4.0, masym=8.0, msoexp=1), 3, False),
    "pot3_rs1": (dict(noe_pot=3, rswitch=1.0, mrswitch=11.0, masym=22.0), 3, False),
    "gen0": (dict(noe_pot=0, asym=3.0, rswitch=2.0), 0, True),
    "gen1": (dict(noe_pot=1, asym=1.0, rswitch=0.5), 1, True),
    "gen2": (dict(noe_pot=2, asym=1.5, rswitch=1.0), 2, True),
    "gen3": (dict(noe_pot=3, mrswitch=4.0, masym=3.0, msoexp=1), 3, True),
    "ang0": (dict(ang_mode=0, k_ang=200.0, a0=6.0), 4, False),
    "kang0": (dict(k_ang=0.0), 4, False),
}

# FIRE from the coil, MD at 2000 K (kind 4 begins it, then kind 0), kind 1, an MD stage without restraint weight (fp32: the general
# per-step kernel; fp64: k64_step<4, false, false>), then kind 5 with the hand-over to FIRE after TP steps.
def _stages(a, b, c, d, e):
    return [(2, a, 0.0, 1.0, 20.0, 0.5, 0.0), (0, b, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, c, 0.005, 1.0, 0.05, 1.0, 1500.0),
            (0, d, 0.003, 0.0, 1.0, 0.9, 2000.0), (5, e, 0.0, 1.0, 1.0, 0.85, 0.0)]


S32, TP32 = _stages(10, 12, 8, 4, 20), 8          # 54 steps: MD 24, minimisation 30
S64, TP64 = _stages(60, 80, 40, 20, 40), 15       # 240 steps


def _problem(size):
    if size == "syn250":                           # last column block four columns a lane, nothing left over: every potential's k_cluster
        return synthetic_if(250, seed=250)[0]
    return load_if(size)                           # chr4_1mb: a narrow last block (k_step<..., true>; k_cluster for potentials 3 / 4 only)


def _centred(x):
    x = x.astype(np.float64)
    return x - x.mean(0)


def _oracle(O, m, fire, d10, stages, x0, tp, upto):
    """oracle coordinates and velocities of every replica after the first `upto` steps of `stages`, from x0"""
    head, left = [], upto
    for st in stages:
        if left <= 0:
            break
        head.append(st[:1] + (min(st[1], left),) + st[2:])
        left -= st[1]
    O.set_two_point_steps(tp)
    try:
        om, of = oracle_model_from(m, d10.shape[0]), oracle_fire_from(fire)
        out = []
        for r in range(x0.shape[0]):
            xo, vo, ev = O.run_schedule(om, d10, O.make_stages(head), of, 82364, r, x0=x0[r].astype(np.float64))
            assert ev == upto
            out.append((xo, vo))
        return out
    finally:
        O.set_two_point_steps(1000)


def _run_form(solver, m, IF, stages, tp, precision, resident, rpw, checkpoints, nrep=2, groups=2, symmetric=0, use_graph=1, first=0):
    """Runs `stages` in the given form, stopping at each checkpoint: [(steps, coords, velocities, kernel name, cluster launches, step
    launches)], plus the start coordinates.  Replicas first .. first + nrep - 1."""
    from chromosome3d_amd import default_fire, make_stages
    solver.set_option("precision", precision)
    solver.set_option("resident", resident)
    solver.set_option("rows_per_wave", rpw)
    solver.set_option("replica_groups", groups)
    solver.set_option("final_minimiser_steps", tp)
    solver.set_option("symmetric", symmetric)
    solver.set_option("use_graph", use_graph)
    try:
        solver.set_model(m)
        solver.set_if_matrix(IF)
        solver.set_schedule(make_stages(stages), default_fire())
        solver.init_replicas(nrep, 82364, first)
        x0 = solver.coords()
        out, done = [], 0
        for k in checkpoints:
            c0, s0 = solver.stat("cluster_launches"), solver.stat("step_launches")
            assert solver.run_steps(k - done) == k - done
            done = k
            out.append((k, solver.coords(), solver.velocities(), solver.step_kernel_name, solver.stat("cluster_launches") - c0,
                        solver.stat("step_launches") - s0))
        return x0, out
    finally:
        solver.set_option("precision", 32)
        solver.set_option("resident", -1)
        solver.set_option("rows_per_wave", 2)
        solver.set_option("replica_groups", 2)
        solver.set_option("final_minimiser_steps", 1000)
        solver.set_option("symmetric", 0)
        solver.set_option("use_graph", 1)


def _worst(x, ref):
    return max(float(np.abs(_centred(x[r]) - ref[r][0]).max()) for r in range(len(ref)))


# ---------------------------------------------------------------------------------------------
# A. potential x launch form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["syn250", "chr4_1mb"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_potential_through_every_launch_form_follows_the_oracle(solver, O, variant, size):
    """One short schedule through every stage kind (FIRE; MD at 2000 K: kinds 4 then 0; kind 1; an MD stage with w_all = 0; kind 5 with the
    hand-over to FIRE after 8 of its steps) in every launch form a variant has at the size:
      multi-step (resident = 1): k_cluster<pot, ...> / k_cluster_tp<pot, ...> around the general per-step kernel of the w_all = 0 stage;
        at syn250 (N = 250: last column block four columns a lane, nothing left over) for every fast form, at chr4_1mb (a narrow last
        block) for potentials 3 and 4 only — cluster_plan refuses potentials 0-2 there; a general tail has no multi-step form;
      per-step (resident = 0): k_step<pot, gen, rpw, false|true, 8, false> — the left-over / narrow-block code at chr4_1mb; for the shipped
        potential and potential 1 at rows_per_wave 1, 2 and 4;
      fp64 (precision = 64, syn250): k64_step<pot, gen, fold> over 240 steps, <4, false, false> inside the w_all = 0 stage.
    Each against O.run_schedule replica by replica, after the zero-weight stage (34 steps) and at the end (54); wherever two fp32 forms
    ran they end in the same bits.  Measured worst over all cases: fp32 1.1e-4 A (after the zero-weight stage) / 8.8e-5 A (at the end), fp64 1.1e-5 A."""
    from chromosome3d_amd import default_fire, default_model
    kw, pot, gen = VARIANTS[variant]
    m = default_model(**kw)
    fire = default_fire()
    IF = _problem(size)
    forms = {}
    # fp32: checkpoints after the zero-weight stage, inside the two-point part of kind 5, at the end
    cps = [34, 40, 54]
    has_cluster = not gen and (size == "syn250" or pot >= 3)
    if has_cluster:
        forms["multi"] = _run_form(solver, m, IF, S32, TP32, 32, 1, 2, cps)
    for rpw in ((1, 2, 4) if variant in ("shipped", "pot1") else (2,)):
        forms[f"step{rpw}"] = _run_form(solver, m, IF, S32, TP32, 32, 0, rpw, cps)
    d10 = O.if_to_dist10(IF)
    x0 = next(iter(forms.values()))[0]
    ref = {k: _oracle(O, m, fire, d10, S32, x0, TP32, k) for k in (34, 54)}
    tail = "false" if size == "syn250" else "true"       # k_step's left-over / narrow-block code
    for name, (xs, out) in forms.items():
        assert np.array_equal(xs, x0), name
        (_, xa, va, ka, cla, sla), (_, xb, vb, kb, clb, slb), (_, xc, vc, kc, clc, slc) = out
        # which kernel ran
        if name == "multi":
            assert ka.startswith(f"c3d::k_step<{pot}, true, 2, ") and cla >= 1 and sla >= 4, (ka, cla, sla)
            assert kb.startswith(f"c3d::k_cluster_tp<{pot}, ") and clb >= 1 and slb == 0, (kb, clb, slb)
            assert kc.startswith(f"c3d::k_cluster<{pot}, ") and clc >= 1, (kc, clc)      # (the hand-over's own ops run per step)
        else:
            rpw = int(name[-1])
            for k, cl in ((ka, cla), (kb, clb), (kc, clc)):
                assert cl == 0, (name, k)
            assert ka == f"c3d::k_step<{pot}, true, {rpw}, {tail}, 8, false>", ka
            assert kc == f"c3d::k_step<{pot}, {'true' if gen else 'false'}, {rpw}, {tail}, 8, false>", kc
        # against the oracle
        wa, wc = _worst(xa, ref[34]), _worst(xc, ref[54])
        assert wa < 2e-3 and wc < 5e-3, (name, wa, wc)
        for r in range(2):
            vo = ref[34][r][1]
            assert np.abs(va[r] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max()), (name, r)
        print(f"{variant} {size} {name}: {ka} / {kb} / {kc}: worst {wa:.2e} {wc:.2e} A")
    # the fp32 forms end in the same bits
    names = list(forms)
    for name in names[1:]:
        for k in range(3):
            assert np.array_equal(forms[name][1][k][1], forms[names[0]][1][k][1]), (names[0], name, k)
            assert np.array_equal(forms[name][1][k][2], forms[names[0]][1][k][2]), (names[0], name, k)
    if size != "syn250":
        return
    # fp64: 240 steps; the zero-weight stage takes the non-FOLD form of the shipped potential's kernel
    x064, out = _run_form(solver, m, IF, S64, TP64, 64, -1, 2, [200, 240])
    (_, xa, va, ka, cla, _), (_, xc, vc, kc, clc, _) = out
    fold = "true" if pot == 4 else "false"
    assert ka == f"c3d::k64_step<{pot}, {'true' if gen else 'false'}, false>", ka
    assert kc == f"c3d::k64_step<{pot}, {'true' if gen else 'false'}, {fold}>", kc
    assert cla == 0 and clc == 0
    for k, x, v in ((200, xa, va), (240, xc, vc)):
        ref64 = _oracle(O, m, fire, d10, S64, x064, TP64, k)
        w = _worst(x, ref64)
        assert w < 2e-5, (k, w)
        for r in range(2):
            assert np.abs(v[r] - ref64[r][1]).max() < 2e-5 * max(1.0, np.abs(ref64[r][1]).max()), (k, r)
        print(f"{variant} fp64 {ka} / {kc} after {k}: worst {w:.2e} A")


@pytest.mark.parametrize("precision", [32, 64])
def test_model_switched_on_a_live_context_follows_the_oracle(solver, O, precision):
    """c3d_set_model alone between runs — the matrix set once — must leave nothing of the previous model behind: the pre-scaled pair
    targets (freed), the multi-step plan (re-planned: every switch comes AFTER c3d_init_replicas, which planned for the previous model) and
    the fp64 target matrix's "no restraint" value (re-encoded per potential).  The walk passes general -> shipped -> general and every
    device potential; each run is compared with the oracle.  Measured worst: fp32 3.0e-5 A, fp64 1.2e-5 A."""
    from chromosome3d_amd import default_fire, default_model, make_stages
    walk = ["gen1", "shipped", "gen3", "pot0", "shipped", "pot3_clamp", "pot2", "gen0", "shipped", "pot1", "ang0"]
    IF = _problem("syn250")
    stages = ([(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 12, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 8, 0.005, 1.0, 0.05, 1.0, 1500.0)]
              if precision == 32 else
              [(2, 40, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 100, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 40, 0.005, 1.0, 0.05, 1.0, 1500.0)])
    nsteps = sum(s[1] for s in stages)
    tol = 2e-3 if precision == 32 else 2e-5
    fire = default_fire()
    solver.set_option("precision", precision)
    solver.set_option("resident", -1)
    try:
        solver.set_model(default_model(**VARIANTS[walk[0]][0]))
        solver.set_if_matrix(IF)                  # once: the walk below changes the model alone
        d10 = solver.dist10()
        worst = 0.0
        for v in walk:
            kw, pot, gen = VARIANTS[v]
            m = default_model(**kw)
            solver.set_schedule(make_stages(stages), fire)
            solver.init_replicas(2, 82364, 0)
            solver.set_model(m)
            x0 = solver.coords()
            c0 = solver.stat("cluster_launches")
            assert solver.run_steps(10 ** 6) == nsteps
            name = solver.step_kernel_name
            if precision == 64:
                assert name == f"c3d::k64_step<{pot}, {'true' if gen else 'false'}, {'true' if pot == 4 else 'false'}>", (v, name)
            elif gen:
                assert name.startswith(f"c3d::k_step<{pot}, true, ") and solver.stat("cluster_launches") == c0, (v, name)
            else:
                assert name.startswith(f"c3d::k_cluster<{pot}, ") and solver.stat("cluster_launches") > c0, (v, name)
            ref = _oracle(O, m, fire, d10, stages, x0, 1000, nsteps)
            w = _worst(solver.coords(), ref)
            assert w < tol, (v, name, w)
            worst = max(worst, w)
        print(f"precision {precision}: worst {worst:.2e} A over {len(walk)} switches")
    finally:
        solver.set_option("precision", 32)


# ---------------------------------------------------------------------------------------------
# B. fp64 column layouts up to the 2560-bead limit
# ---------------------------------------------------------------------------------------------
B_CASES = ([(n, "shipped", 2, 2) for n in (9, 32, 33, 64, 65, 96, 127, 128, 129, 160, 161, 192, 193, 255, 257, 1025, 2049, 2559, 2560)]
           + [(129, "gen1", 2, 2), (161, "gen3", 2, 2), (2049, "gen0", 2, 2), (193, "shipped", 20, 2)])


@pytest.mark.parametrize("n,variant,nrep,groups", B_CASES)
def test_fp64_column_layouts_follow_the_oracle(solver, O, n, variant, nrep, groups):
    """k64_step's column loop (c3d_f64.hip) takes, for n columns: the two-column main loop over n & ~127 of them (n >= 128), then one
    64-column block if 64 or more are left, then the last `left` = 0..63 columns — both rows of a wave in one pass if left <= 32, one row
    after the other if 33 <= left <= 63.  The sizes:
      9, 32: two-rows pass alone                    33: one-row-at-a-time left-over alone
      64: one 64-column block                       65, 96: block + two-rows pass            127: block + left-over of 63
      128, 2560: main loop alone                    129, 160, 257, 1025, 2049: main + two-rows pass (1 / 32 / 1 columns)
      161: main + left-over of 33                   192: main + block    193: main + block + 1    255, 2559: main + block + 63
    Tile tails: n % 8 == 1 (9, 33, 65, 129, 161, 193, 257, 1025, 2049) leaves a last tile of ONE row, whose wave's second row is clamped
    to the last bead; 127, 255, 2559 a tile of 7 rows.  2560 is the limit (61 760 B of LDS).  Shipped potential (k64_step<4, false, true>)
    at every n, a general tail of each kind at 129, 161 and 2049, and 20 replicas in two replica groups at 193.  About 100 steps up to
    n = 257, 28 beyond (FIRE, MD at 2000 K, kind 1, FIRE), every replica against the oracle.  Measured worst: 1.8e-5 A (2049, potential 0's general tail), 7.6e-6 A for the shipped potential."""
    from chromosome3d_amd import default_fire, default_model
    kw, pot, gen = VARIANTS[variant]
    m = default_model(**kw)
    IF = synthetic_if(n, seed=n)[0]
    a, b, c, d = (20, 50, 20, 10) if n <= 455 else (6, 10, 6, 6)
    stages = [(2, a, 0.0, 1.0, 20.0, 0.5, 0.0), (0, b, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, c, 0.005, 1.0, 0.05, 1.0, 1500.0),
              (2, d, 0.0, 1.0, 1.0, 0.85, 0.0)]
    k = a + b + c + d
    x0, out = _run_form(solver, m, IF, stages, 1000, 64, -1, 2, [k], nrep=nrep, groups=groups)
    (_, x, v, name, cl, sl) = out[0]
    assert name == f"c3d::k64_step<{pot}, {'true' if gen else 'false'}, {'true' if pot == 4 else 'false'}>", name
    assert cl == 0 and sl >= k
    ref = _oracle(O, m, default_fire(), O.if_to_dist10(IF), stages, x0, 1000, k)
    worst = 0.0
    for r in range(nrep):
        xo, vo = ref[r]
        # the read-back is fp32: half an ulp of the largest coordinate, 2e-5 A up to |x| ~ 160
        tol = max(2e-5, 1.2e-7 * np.abs(xo).max())
        e = float(np.abs(_centred(x[r]) - xo).max())
        assert e < tol, (r, e, tol)
        assert np.abs(v[r] - vo).max() < 2e-5 * max(1.0, np.abs(vo).max()), r
        worst = max(worst, e)
    print(f"n={n} {variant} x{nrep}: {name}, worst {worst:.2e} A")


def test_fp64_refuses_one_bead_beyond_its_limit(solver):
    """n = 2561: the fp32 path takes it, precision 64 refuses it at c3d_init_replicas, on the host — no kernel is launched."""
    from chromosome3d_amd import C3DError, default_model
    solver.set_option("precision", 64)
    try:
        solver.set_model(default_model())
        solver.set_if_matrix(np.ones((2561, 2561)))
        with pytest.raises(C3DError, match="2560"):
            solver.init_replicas(2, 82364, 0)
    finally:
        solver.set_option("precision", 32)


# ---------------------------------------------------------------------------------------------
# E. device scoring past the rank-prefetch limit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2048, 2500])
def test_device_scoring_beyond_the_rank_prefetch_limit(solver, O, n):
    """c3d_score_replicas takes the IF ranks the helper thread of c3d_set_if_matrix prepared up to 2048 beads and ranks the matrix itself
    beyond (c3d_api.cpp kRankPrefetchBeads): at n = 2048 (prefetched) and 2500 (ranked in place), on the coil and after a short anneal,
    the Spearman coefficient equals the host's and the oracle's to 5e-12 (measured: 1.9e-12), and satisfied / sum of deviations equal the host's and the oracle's (the oracle
    reads the coordinates as a PDB file holds them, %8.3f).  The coil is a compact one: device scoring refuses pair distances beyond its
    histogram's 262 A, which a random coil of 2048 beads at full size exceeds."""
    from chromosome3d_amd import default_model, make_stages, pipeline
    IF = synthetic_if(n, seed=n)[0]
    solver.set_model(default_model())
    d10 = pipeline.IF2dist_new(solver, IF)
    rows = pipeline.restraints_from_dist10(d10)
    rr = O.dist_to_rr(d10)
    solver.set_schedule(make_stages([(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]))
    solver.init_replicas(2, 82364, 0)
    for phase in ("coil", "annealed"):
        if phase == "annealed":
            assert solver.run_steps(10 ** 6) == 45
        else:
            solver.set_coords(random_coil(n, 5)[None].repeat(2, 0) * np.float32([[[0.25]], [[0.35]]]))
        x = solver.coords()
        h0 = solver.stat("rank_prefetch_hits")
        sat, dev, rho = solver.score(IF, 3)
        host_rho = pipeline.spearman_IF_models(IF, x)
        assert solver.stat("rank_prefetch_hits") - h0 == (1 if n <= 2048 else 0), phase
        for r in range(2):
            xo = np.array([[float("%.3f" % c) for c in row] for row in x[r].astype(np.float64)])     # what a PDB holds: the oracle's input
            # the device sums the 4-6 M rank products in per-workgroup partial sums, the host and the oracle one after the other:
            # 1.9e-12 apart at both sizes and both phases (measured; 1e-12 holds up to N = 455, test_device_scoring_equals_host_scoring)
            assert abs(rho[r] - host_rho[r]) <= 5e-12, (phase, r, rho[r] - host_rho[r])
            assert abs(rho[r] - O.spearman_if_dist(IF, xo, 3)) <= 5e-12, (phase, r)
            hs, hd = pipeline.assess(x[r], rows)
            os_, od = O.assess(xo, rr)
            assert sat[r] == hs == os_, (phase, r, sat[r], hs, os_)
            assert abs(dev[r] - hd) <= 1e-10 * max(1.0, abs(hd)) and abs(dev[r] - od) <= 1e-10 * max(1.0, abs(od)), (phase, r, dev[r], hd, od)


# ---------------------------------------------------------------------------------------------
# F. the symmetric-tile form (c3d_sym.hip, option symmetric 1)
# ---------------------------------------------------------------------------------------------
# k_pairs_sym evaluates the clamp form itself (not pair_term): u = 1 - t/d, a clamp per potential, RS1 (rswitch 1: the upper bound is
# 1/d itself) as its own branch, and repel on every pair, the chain pass taking the |i - j| < rep_sep neighbours back out.  This section's
# own variants: rep_sep 1 (nothing taken back) and 3 (both chain neighbours; every other variant has the default, 2), RS1 for potentials
# 0 and 1 (pot3_rs1 has it for potential 3).
F_VARIANTS = dict(VARIANTS, rep1=(dict(rep_sep=1), 4, False), rep3=(dict(rep_sep=3), 4, False),
                  pot0_rs1=(dict(noe_pot=0, rswitch=1.0), 0, False), pot1_rs1=(dict(noe_pot=1, rswitch=1.0), 1, False))


def _sym_name(m, pot):
    return f"c3d::k_pairs_sym<{pot}, {'true' if m.rswitch == 1.0 else 'false'}, false>"


@functools.lru_cache(maxsize=2)
def _f_problem(size):
    if size == "syn1100":                          # beyond the cluster kernel's reach: 5 column blocks x 18 row groups
        return synthetic_if(1100, seed=1100)[0]
    return _problem(size)


# (potential 2 at syn1100 is held to the oracle by the layout test below instead: see the docstring)
F_CASES = [(v, size) for v in sorted(F_VARIANTS) for size in ("syn250", "chr4_1mb", "syn1100") if (v, size) != ("pot2", "syn1100")]


@pytest.mark.parametrize("variant,size", F_CASES)
def test_every_potential_through_the_symmetric_tiles_follows_the_oracle(solver, O, variant, size):
    """The schedule of section A (FIRE; MD at 2000 K: kinds 4 then 0; kind 1; an MD stage with w_all = 0; kind 5 with the hand-over to
    FIRE after 8 of its steps) with symmetric 1 and resident 0 (the multi-step kernel takes syn250 and chr4_1mb otherwise), against the
    oracle after the zero-weight stage (34 steps) and at the end (54), and against the per-step path (symmetric 0) of the same case.
    A clamp-form model runs k_pairs_sym<pot, rs1, false> at every checkpoint — the zero-weight stage and kinds 5 / 6 included, which
    k_update_sym steps itself; a general tail runs k_step<pot, true, ...>, in the bits of the symmetric 0 run.  The symmetric form sums a
    row in another order than k_step: the two agree within the oracle tolerances, not bit for bit.  Measured worst of k_pairs_sym over
    its 35 cases: 9.6e-5 A after the zero-weight stage (pot2, syn250) / 1.0e-4 A at the end (kang0, syn250); the general tails' k_step
    1.1e-3 / 5.7e-4 A (gen2, syn1100).  Left out: potential 2 at syn1100.  It has no switch, so its force grows with the violation,
    and syn1100 restrains every pair.  There the stages after step 22 magnify fp32 rounding about a hundredfold in every fp32 form.
    k_step has it too: 2e-5 A from the oracle after step 22, 2.4e-3 A after step 34.  The oracle cannot see a kernel error through that.  Its
    k_pairs_sym<2, ...> runs on several column blocks in the layout test below, at 2049 beads."""
    from chromosome3d_amd import default_fire, default_model
    kw, pot, gen = F_VARIANTS[variant]
    m = default_model(**kw)
    IF = _f_problem(size)
    cps = [34, 40, 54]
    forms = {"sym": _run_form(solver, m, IF, S32, TP32, 32, 0, 2, cps, symmetric=1),
             "step": _run_form(solver, m, IF, S32, TP32, 32, 0, 2, cps)}
    d10 = solver.dist10()
    x0 = forms["step"][0]
    ref = {k: _oracle(O, m, default_fire(), d10, S32, x0, TP32, k) for k in (34, 54)}
    worst = {}
    for name, (xs, out) in forms.items():
        assert np.array_equal(xs, x0), name
        done = 0
        for k, x, v, kn, cl, sl in out:
            assert cl == 0 and sl >= k - done, (name, k, cl, sl)
            done = k
            if name == "sym" and not gen:
                assert kn == _sym_name(m, pot), (name, k, kn)
            else:                                  # (the zero-weight stage ends at 34: k_step's general form)
                assert kn.startswith(f"c3d::k_step<{pot}, {'true' if gen or k == 34 else 'false'}, "), (name, k, kn)
        (_, xa, va, *_), _, (_, xc, vc, *_) = out
        wa, wc = _worst(xa, ref[34]), _worst(xc, ref[54])
        assert wa < 2e-3 and wc < 5e-3, (name, wa, wc)
        for r in range(2):
            vo = ref[34][r][1]
            assert np.abs(va[r] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max()), (name, r)
        worst[name] = (wa, wc)
    # the symmetric form against the per-step path
    for (_, xs, vs, *_), (k, xp, vp, *_) in zip(forms["sym"][1], forms["step"][1]):
        if gen:                                    # the same kernel ran: the same bits
            assert np.array_equal(xs, xp) and np.array_equal(vs, vp), k
        else:
            assert np.abs(xs - xp).max() < (2e-3 if k == 34 else 5e-3), (k, np.abs(xs - xp).max())
            assert np.abs(vs - vp).max() < 2e-3 * max(1.0, np.abs(vp).max()), k
    print(f"{variant} {size}: {forms['sym'][1][-1][3]}: worst {worst['sym'][0]:.2e} {worst['sym'][1]:.2e} A "
          f"(per-step path {worst['step'][0]:.2e} {worst['step'][1]:.2e})")


F_GEOMETRY = ([(n, "shipped") for n in (9, 64, 65, 128, 255, 256, 257, 320, 321, 1025, 2049, 5120)]
              + [(n, v) for v in ("pot3_rs1", "pot0") for n in (257, 2049)] + [(2049, "pot2")])


@pytest.mark.parametrize("n,variant", F_GEOMETRY)
def test_symmetric_tile_layouts_follow_the_oracle(solver, O, n, variant):
    """k_pairs_sym cuts the pair matrix into tiles of 64 rows (row group g, G = ceil(n / 64) of them) x 256 columns (column block q,
    Q = npad / 256) and visits a tile only on or above the diagonal: q >= g / 4.  The tile that crosses the diagonal (q = g / 4, G of
    them) keeps j > i alone (k_pairs_sym<..., true>); the others (od of them) are a launch of their own.  k_update_sym gathers a row's
    rows-side partials over q >= g / 4 and its column-side partials over the row groups 0 .. gmax = min(4 q + 3, G - 1).  The sizes:
      9: one diagonal tile, 247 padding columns       64: one full row group        65: a second row group of ONE row
      128: two row groups, half the block padding     255: four groups, the last of 63 rows, one padding column
      256: one column block, every tile diagonal (G = 4, od = 0), no padding
      257: the first off-diagonal tiles (Q = 2, G = 5, od = 4): row group 4 is one row, block 1 one live column, gmax clamped to G - 1
      320: block 1 of 64 live columns, row group 4 full   321: Q = 2, G = 6, the last group one row
      1025: Q = 5, G = 17, od = 40, a last group of one row    2049: Q = 9, G = 33, od = 144, a last group of one row
      5120: the limit (Q = 20, G = 80, od = 760, no padding)
    The shipped potential at every n, pot3_rs1 (RS1) and potential 0 at 257 and 2049, potential 2 at 2049.  FIRE, MD at 2000 K (kinds 4 then 0), FIRE — 32
    steps up to 1025, 20 beyond; resident 0 up to 768 (the multi-step kernel's reach), the library's choice beyond; 2 replicas, every one
    against the oracle.  Measured worst: 7.2e-5 A for the shipped potential (at 5120), 8.2e-5 A (potential 2, 2049).  The oracle takes
    3.5 s at 5120 (two replicas, 20 steps), the whole case 4.7 s."""
    from chromosome3d_amd import default_fire, default_model
    kw, pot, gen = VARIANTS[variant]
    m = default_model(**kw)
    IF = synthetic_if(n, seed=n)[0]
    a, b, d = (10, 12, 10) if n <= 1025 else (6, 8, 6)
    stages = [(2, a, 0.0, 1.0, 20.0, 0.5, 0.0), (0, b, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, d, 0.0, 1.0, 1.0, 0.85, 0.0)]
    k = a + b + d
    x0, out = _run_form(solver, m, IF, stages, 1000, 32, 0 if n <= 768 else -1, 2, [k], symmetric=1)
    (_, x, v, name, cl, sl) = out[0]
    assert name == _sym_name(m, pot) and cl == 0 and sl >= k, (name, cl, sl)
    d10 = solver.dist10()
    del IF
    t0 = time.perf_counter()
    ref = _oracle(O, m, default_fire(), d10, stages, x0, 1000, k)
    t_oracle = time.perf_counter() - t0
    worst = _worst(x, ref)
    assert worst < 2e-3, worst
    for r in range(2):
        assert np.abs(v[r] - ref[r][1]).max() < 2e-3 * max(1.0, np.abs(ref[r][1]).max()), r
    print(f"n={n} {variant}: {name}, worst {worst:.2e} A (oracle {t_oracle:.1f} s)")


def test_symmetric_tiles_index_replicas_by_their_global_number(solver):
    """The slabs of k_pairs_sym / k_update_sym and the FIRE state are indexed by the global replica, rep_base + blockIdx.y: 5 replicas at
    n = 1100 (S32: every stage kind) give the same bits in replica groups 1, 2, 3 and 4 (uneven groups, rep_base 0 .. 4), eagerly and
    through graphs, and replica r alone (first_replica r) gives the bits of replica r of the five."""
    from chromosome3d_amd import default_model
    m = default_model()
    IF = _f_problem("syn1100")
    name = _sym_name(m, 4)
    runs = {f"groups{g}": _run_form(solver, m, IF, S32, TP32, 32, -1, 2, [54], nrep=5, groups=g, symmetric=1) for g in (1, 2, 3, 4)}
    runs["eager"] = _run_form(solver, m, IF, S32, TP32, 32, -1, 2, [54], nrep=5, groups=3, symmetric=1, use_graph=0)
    x0, ((_, x, v, *_),) = runs["groups1"]
    assert np.isfinite(x).all() and not np.array_equal(x[0], x[1])
    for key, (xs, ((_, xr, vr, kn, cl, sl),)) in runs.items():
        assert kn == name and cl == 0 and sl >= 54, (key, kn, cl, sl)
        assert np.array_equal(xs, x0) and np.array_equal(xr, x) and np.array_equal(vr, v), key
    for r in range(5):
        xs, ((_, xr, vr, kn, cl, _),) = _run_form(solver, m, IF, S32, TP32, 32, -1, 2, [54], nrep=1, symmetric=1, first=r)
        assert kn == name and cl == 0, (r, kn)
        assert np.array_equal(xs[0], x0[r]) and np.array_equal(xr[0], x[r]) and np.array_equal(vr[0], v[r]), r


@pytest.mark.parametrize("start", ["clamp", "general"])
def test_model_switched_on_a_live_context_takes_the_symmetric_tiles_where_they_apply(solver, O, start):
    """The walk of test_model_switched_on_a_live_context_follows_the_oracle with symmetric 1 (resident 0, syn250): c3d_set_model alone
    between runs, after c3d_init_replicas, which ran under the PREVIOUS model.  The symmetric form evaluates the clamp form only: a clamp-form
    model must run k_pairs_sym<pot, rs1, false>, a general tail k_step<pot, true, ...> — decided per op from the model in force.  Two walks
    through every device potential, general <-> clamp both ways: one whose first c3d_init_replicas sees a clamp form, one whose first sees a
    general tail.  Each run against the oracle.  Measured worst: 7.0e-5 A.  Before the choice was made per op, the first walk ran
    k_pairs_sym on every general tail: gen1, gen3 and gen0 missed the oracle by 1.8, 5.1 and 6.0 A.  The second ran k_step on every
    clamp form: the symmetric option was silently off."""
    from chromosome3d_amd import default_fire, default_model, make_stages
    walk = {"clamp": ["shipped", "gen1", "pot0", "gen3", "pot3_rs1", "gen0", "pot1", "gen2", "pot2", "pot3_clamp", "gen1", "ang0"],
            "general": ["gen1", "shipped", "gen3", "pot0", "gen0", "pot3_clamp", "gen2", "pot1", "pot2", "pot3_rs1", "gen1", "shipped"]}[start]
    IF = _problem("syn250")
    stages = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 12, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 8, 0.005, 1.0, 0.05, 1.0, 1500.0)]
    nsteps = sum(s[1] for s in stages)
    fire = default_fire()
    solver.set_option("resident", 0)
    solver.set_option("symmetric", 1)
    try:
        solver.set_model(default_model(**VARIANTS[walk[0]][0]))
        solver.set_if_matrix(IF)                  # once: the walk below changes the model alone
        d10 = solver.dist10()
        seen = []
        for v in walk:
            kw, pot, gen = VARIANTS[v]
            m = default_model(**kw)
            solver.set_schedule(make_stages(stages), fire)
            solver.init_replicas(2, 82364, 0)
            solver.set_model(m)
            x0 = solver.coords()
            c0 = solver.stat("cluster_launches")
            assert solver.run_steps(10 ** 6) == nsteps
            name = solver.step_kernel_name
            ok = solver.stat("cluster_launches") == c0 and (name.startswith(f"c3d::k_step<{pot}, true, ") if gen else name == _sym_name(m, pot))
            ref = _oracle(O, m, fire, d10, stages, x0, 1000, nsteps)
            seen.append((v, name, ok, _worst(solver.coords(), ref)))
        # every run first, then the verdict: the message shows the whole walk
        assert all(ok and w < 2e-3 for _, _, ok, w in seen), "; ".join(f"{v}: {name}{'' if ok else ' (WRONG KERNEL)'} {w:.2e} A"
                                                                        for v, name, ok, w in seen)
        print(f"start {start}: worst {max(w for *_, w in seen):.2e} A over {len(walk)} switches")
    finally:
        solver.set_option("symmetric", 0)
        solver.set_option("resident", -1)
