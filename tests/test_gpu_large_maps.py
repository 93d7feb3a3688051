"""Chromosomes beyond 5120 beads on the fp32 per-step path: the options max_beads / column_chunk, the chunked form of the per-step kernels
(k_*_chunked: ColsChunked in csrc/c3d_step_core.h) against the staged form bit for bit where both run, and against the oracle past the old limit, up to 16384 beads.

Every test here runs on a context of its own (module fixture), never the session's: max_beads stays raised on it."""
import os
import subprocess

import numpy as np
import pytest

from tests import lbfgs_ref as L
from tests.util import oracle_fire_from, oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRE_MD = [(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 10, 0.003, 0.4, 0.003, 0.9, 2000.0)]
FINAL = (1.0, 1.0, 0.85)


def _stage(kind, n):
    return (kind, n, 0.0) + FINAL + (0.0,)


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    s.set_option("max_beads", 16384)
    yield s
    s.close()


_IF = {}


def _if(n):
    if n not in _IF:
        _IF.clear()
        _IF[n] = synthetic_if(n, seed=n)
    return _IF[n]


def _targets(s, n, model_kw=None):
    from chromosome3d_amd import default_model, pipeline
    m = default_model(**(model_kw or {}))
    s.set_model(m)
    d10 = pipeline.IF2dist_new(s, _if(n)[0])
    return d10, m


def _run(s, stages, nrep, x0=None, chunk=0, **opts):
    """the schedule from the same start under column_chunk `chunk`: coordinates, velocities, kernel name"""
    from chromosome3d_amd import default_fire, make_stages
    s.set_option("column_chunk", chunk)
    for k, v in opts.items():
        s.set_option(k, v)
    try:
        s.set_schedule(make_stages(stages), default_fire())
        s.init_replicas(nrep, 82364, 0)
        if x0 is not None:
            s.set_coords(x0)
        s.run_steps(10 ** 6)
        return s.coords(), s.velocities(), s.step_kernel_name
    finally:
        s.set_option("column_chunk", 0)
        for k in opts:
            s.set_option(k, {"final_minimiser_steps": 1000, "wide_tiles": 1, "pair_targets": 1, "eval_rows_per_wave": 4}[k])


# ---------------------------------------------------------------------------------------------------------------------------------
def test_options(ctx):
    from chromosome3d_amd import C3DError, Solver
    s = Solver(0)
    try:
        IF = np.ones((5121, 5121))
        with pytest.raises(C3DError, match="5120"):
            s.set_if_matrix(IF)
        for bad in (5119, 16385, 6000.5, -1):
            with pytest.raises(C3DError):
                s.set_option("max_beads", bad)
        for bad in (128, 512, 3072, 4096, 8192, 100.5, -256):
            with pytest.raises(C3DError):
                s.set_option("column_chunk", bad)
        for ok in (0, 256, 1024, 2048):
            s.set_option("column_chunk", ok)
        s.set_option("max_beads", 6000)
        IF = synthetic_if(5121, seed=5121)[0]
        s.set_if_matrix(IF)
        assert s.n == 5121
        with pytest.raises(C3DError, match="6000"):
            s.set_if_matrix(np.ones((6001, 6001)))
        # symmetric tiles stage a replica in LDS: refused beyond 5120 at c3d_init_replicas, with a message
        s.set_if_matrix(IF)
        s.set_option("symmetric", 1)
        with pytest.raises(C3DError, match="symmetric"):
            s.init_replicas(2, 82364, 0)
        s.set_option("symmetric", 0)
        s.init_replicas(2, 82364, 0)
        # precision 64 keeps its own limit
        s.set_option("precision", 64)
        with pytest.raises(C3DError, match="2560"):
            s.init_replicas(1, 82364, 0)
        s.set_option("precision", 32)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 2500, 4097, 5120])
def test_chunked_form_has_the_bits_of_the_staged_form(ctx, n):
    """Where both forms run, the chunked form (CHUNK 256 and 2048) ends in the same bits as the staged one: FIRE + MD, a kind-5 stage across
    its hand-over, a kind-8 stage, the forces hook in its three forms and four potentials; the wide, the two-row packed and the general
    forms.  Every chunked run is identified by its kernel name."""
    s = ctx
    nrep = 2
    _targets(s, n)
    x0 = None
    cases = [
        ("fire+md", FIRE_MD, {}, "k_step_chunked<4, false, 4, 16, true, {c}>"),
        ("fire+md two-row", FIRE_MD, {"wide_tiles": 0}, "k_step_chunked<4, false, 2, 8, false, {c}>"),
        ("fire+md streamed", FIRE_MD, {"pair_targets": 0}, "k_step_chunked<4, false, 2, 8, false, {c}>"),
        ("kind 5", [(2, 6, 0.0, 1.0, 20.0, 0.5, 0.0), _stage(5, 10)], {"final_minimiser_steps": 5}, "k_step_chunked<4, false, 4, 16, true, {c}>"),
        ("kind 8", [(2, 6, 0.0, 1.0, 20.0, 0.5, 0.0), _stage(8, 12)], {"final_minimiser_steps": 12}, "k_lbfgs_eval_chunked<4, false, 4, 16, true, {c}>"),
    ]
    for label, stages, opts, name in cases:
        ref = _run(s, stages, nrep, x0, 0, **opts)
        assert "_chunked" not in ref[2], (label, ref[2])
        for c in (256, 2048):
            got = _run(s, stages, nrep, x0, c, **opts)
            assert got[2] == "c3d::" + name.format(c=c), (label, got[2])
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (label, c)
    x = s.coords()
    # the general forms (noe_pot 0 / 1 / 2) through the step kernel, then the forces hook of all four potentials in all three forms
    for kw, pot in ((dict(noe_pot=0), 0), (dict(noe_pot=1), 1), (dict(noe_pot=2), 2), ({}, 4)):
        _targets(s, n, kw)
        if pot != 4 and n in (2500, 5120):
            ref = _run(s, FIRE_MD, nrep, x)
            for c in (256, 2048):
                got = _run(s, FIRE_MD, nrep, x, c)
                assert got[2].startswith(f"c3d::k_step_chunked<{pot}, ") and got[2].endswith(f", 2, 8, false, {c}>"), got[2]
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), (pot, c)
        s.init_replicas(nrep, 82364, 0)
        s.set_coords(x)
        for erpw in ((4, 2, -2) if pot == 4 else (4,)):
            s.set_option("eval_rows_per_wave", erpw)
            F0, e0 = s.eval(*FINAL)
            for c in (256, 2048):
                s.set_option("column_chunk", c)
                F, e = s.eval(*FINAL)
                s.set_option("column_chunk", 0)
                assert np.array_equal(F, F0) and np.array_equal(e, e0), (pot, erpw, c)
        s.set_option("eval_rows_per_wave", 4)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5121, 8192])
def test_past_the_old_limit_follows_the_oracle(ctx, n):
    """K1 bit-exact; forces and energies of two coordinate sets within the tolerances of test_fp32_path_at_its_bead_limit_follows_the_oracle
    and Newton's third law; ten FIRE and ten MD steps against the oracle.  At 5121 x 2 also a kind-5 stage across its hand-over and a
    kind-8 stage against the fp64 L-BFGS restatement, and the forces of the four potentials."""
    from chromosome3d_amd import default_fire, make_stages
    from oracle import oracle as O
    s = ctx
    IF, truth = _if(n)
    d10, m = _targets(s, n)
    assert np.array_equal(d10, O.if_to_dist10(IF))
    om = oracle_model_from(m, n)
    s.init_replicas(1, 82364, 0)
    for x in (truth.astype(np.float32) * 1.1, random_coil(n, 3) * 0.3):
        s.set_coords(x[None])
        F, e = s.eval(*FINAL)
        Fo, eo = O.energy_force(om, d10, x.astype(np.float64), 1.0, 1.0, float(np.float32(0.85)))
        assert (np.abs(F[0] - Fo) <= 1e-5 * np.abs(Fo) + 1e-6 * np.abs(Fo).max()).all(), np.abs(F[0] - Fo).max()
        assert np.allclose(e[0], eo, rtol=1e-7, atol=1e-6), (e[0], eo)
        assert np.abs(F[0].sum(0)).max() < 5e-5 * np.abs(F[0]).sum(0).max()
    fire = default_fire()
    s.set_schedule(make_stages(FIRE_MD), fire)
    s.init_replicas(1, 82364, 0)
    x0 = s.coords()
    assert s.run_steps(10 ** 6) == 20
    assert s.step_kernel_name == "c3d::k_step_chunked<4, false, 4, 16, true, 1024>", s.step_kernel_name
    xo, vo, ev = O.run_schedule(om, d10, O.make_stages(FIRE_MD), oracle_fire_from(fire), 82364, 0, x0=x0[0].astype(np.float64))
    xc = s.coords()[0].astype(np.float64)
    xc -= xc.mean(0)
    assert ev == 20
    worst = float(np.abs(xc - xo).max())
    assert worst < 2e-3, worst
    assert np.abs(s.velocities()[0] - vo).max() < 2e-3 * max(1.0, np.abs(vo).max())
    print(f"N={n}: worst {worst:.2e} A after 20 steps")
    if n != 5121:
        return
    # kind 5 across its hand-over, 2 replicas
    pre = [(2, 8, 0.0, 1.0, 1.0, 0.85, 0.0)]
    s.set_option("final_minimiser_steps", 9)
    O.set_two_point_steps(9)
    try:
        stages = pre + [_stage(5, 15)]
        s.set_schedule(make_stages(stages), fire)
        s.init_replicas(2, 82364, 0)
        x0 = s.coords()
        assert s.run_steps(10 ** 6) == 23
        assert s.step_kernel_name == "c3d::k_step_chunked<4, false, 4, 16, true, 1024>", s.step_kernel_name
        for r in range(2):
            xo, _, _ = O.run_schedule(om, d10, O.make_stages(stages), oracle_fire_from(fire), 82364, r, x0=x0[r].astype(np.float64))
            xc = s.coords()[r].astype(np.float64)
            assert np.abs(xc - xc.mean(0) - xo).max() < 2e-3
    finally:
        s.set_option("final_minimiser_steps", 1000)
        O.set_two_point_steps(1000)
    # kind 8 against the fp64 restatement: 20 L-BFGS steps
    s.set_option("final_minimiser_steps", 20)
    try:
        s.set_schedule(make_stages([(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0)]), fire)
        s.init_replicas(2, 82364, 0)
        s.run_steps(10)
        x0 = s.coords()
        s.set_schedule(make_stages([_stage(8, 20)]), fire)
        s.init_replicas(2, 82364, 0)
        s.set_coords(x0)
        before = s.stat("lbfgs_steps")
        s.run_steps(10 ** 6)
        assert s.stat("lbfgs_steps") - before == 20
        assert s.step_kernel_name == "c3d::k_lbfgs_eval_chunked<4, false, 4, 16, true, 1024>", s.step_kernel_name
        x = s.coords()
        of = oracle_fire_from(fire)
        for r in range(2):
            xo, _ = L.lbfgs_stage(om, d10, x0[r].astype(np.float64), _stage(8, 20), of, 20, m=5, replica=r)
            xc = x[r].astype(np.float64)
            assert np.abs(xc - xc.mean(0) - xo).max() < 1e-2
    finally:
        s.set_option("final_minimiser_steps", 1000)
    # the four potentials' forces
    xc = (truth.astype(np.float32) * 1.05)[None]
    for kw in (dict(noe_pot=0), dict(noe_pot=1), dict(noe_pot=2), dict(noe_pot=3, mrswitch=4.0, masym=8.0, msoexp=1)):
        d10, m = _targets(s, n, kw)
        s.init_replicas(1, 82364, 0)
        s.set_coords(xc)
        F, e = s.eval(*FINAL)
        Fo, eo = O.energy_force(oracle_model_from(m, n), d10, xc[0].astype(np.float64), 1.0, 1.0, float(np.float32(0.85)))
        assert (np.abs(F[0] - Fo) <= 1e-5 * np.abs(Fo) + 1e-6 * np.abs(Fo).max()).all(), (kw, np.abs(F[0] - Fo).max())
        assert np.allclose(e[0], eo, rtol=1e-7, atol=1e-6), (kw, e[0], eo)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_ceiling_16384(ctx):
    """n = 16384, one replica, from a sparse restraint set (|i - j| <= 64 and 10^5 random long-range pairs): forces and energies against
    the oracle on the dense target matrix, then three FIRE steps, finite."""
    from chromosome3d_amd import default_fire, default_model, make_stages
    from oracle import oracle as O
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
    s.init_replicas(1, 82364, 0)
    x = (truth * 1.1).astype(np.float32)
    s.set_coords(x[None])
    F, e = s.eval(*FINAL)
    d10 = np.zeros((n, n), dtype=np.int32)
    d10[ri, rj] = t10
    d10[rj, ri] = t10
    del ri, rj, li, lj
    Fo, eo = O.energy_force(oracle_model_from(m, n), d10, x.astype(np.float64), 1.0, 1.0, float(np.float32(0.85)))
    del d10
    assert (np.abs(F[0] - Fo) <= 1e-5 * np.abs(Fo) + 1e-6 * np.abs(Fo).max()).all(), np.abs(F[0] - Fo).max()
    assert np.allclose(e[0], eo, rtol=1e-7, atol=1e-6), (e[0], eo)
    s.set_schedule(make_stages([(2, 3, 0.0, 1.0, 20.0, 0.5, 0.0)]), default_fire())
    s.init_replicas(1, 82364, 0)
    assert s.run_steps(10 ** 6) == 3
    assert s.step_kernel_name == "c3d::k_step_chunked<4, false, 4, 16, true, 1024>", s.step_kernel_name
    assert np.isfinite(s.coords()).all()


# ---------------------------------------------------------------------------------------------------------------------------------
def test_whole_run_at_8192x4(ctx):
    """c3d_run of a short schedule at 8192 x 4 (FIRE, two short hot stages, a kind-5 final stage with gtol): finite, E_noe down; c3d_rank;
    the device's satisfied / sum_dev equal the host's c3d_assess on the same coordinates."""
    from chromosome3d_amd import default_fire, make_stages, pipeline
    s = ctx
    n = 8192
    d10, m = _targets(s, n)
    stages = [(2, 60, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 20, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, 20, 0.003, 1.0, 1.0, 1.0, 300.0),
              _stage(5, 200)]
    s.set_schedule(make_stages(stages), default_fire(), 1e-2, 50)
    s.init_replicas(4, 82364, 0)
    e0 = s.energies()
    s.run()
    x = s.coords()
    e1 = s.energies()
    assert np.isfinite(x).all() and np.isfinite(e1).all()
    assert (e1[:, 0] < e0[:, 0]).all(), (e0[:, 0], e1[:, 0])
    assert sorted(s.rank().tolist()) == [0, 1, 2, 3]
    sat, dev, _ = s.score()
    rows = pipeline.restraints_from_dist10(d10)
    for k in range(4):
        hs, hd = pipeline.assess(x[k], rows)
        assert int(sat[k]) == int(hs)
        assert np.isclose(dev[k], hd, rtol=1e-9, atol=1e-9), (dev[k], hd)


# ---------------------------------------------------------------------------------------------------------------------------------
def _write_banded(path, n, width=200):
    """a symmetric IF matrix that is zero for |i - j| > width (contact.tbl stays small)"""
    band = ["%.4g" % (1.0 / (1.0 + d)) for d in range(width + 1)]
    with open(path, "w") as f:
        for i in range(n):
            lo, hi = max(0, i - width), min(n, i + width + 1)
            f.write(" ".join(["0"] * lo + [band[abs(j - i)] for j in range(lo, hi)] + ["0"] * (n - hi)) + "\n")


def test_cli_past_the_old_limit(tmp_path):
    """c3d_solve on a banded 6000-bead matrix writes the models (it raises max_beads itself); on 16385 beads it fails naming the limit."""
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    m6000 = tmp_path / "big_matrix.txt"
    _write_banded(str(m6000), 6000)
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, "-i", str(m6000), "-o", str(out), "-m", "2", "--min-steps", "40"], capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    pdbs = sorted(f for f in os.listdir(out) if f.endswith(".pdb"))
    assert len(pdbs) == 2, os.listdir(out)
    ca = [l for l in open(out / pdbs[0]) if l.startswith("ATOM")]
    assert len(ca) == 6000
    m16385 = tmp_path / "huge_matrix.txt"
    _write_banded(str(m16385), 16385, width=2)
    p = subprocess.run([exe, "-i", str(m16385), "-o", str(out), "-m", "1", "--min-steps", "10"], capture_output=True, text=True, timeout=900)
    assert p.returncode != 0
    assert "16384" in p.stderr, p.stderr[-2000:]
