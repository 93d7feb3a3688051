"""The fp64 step beyond 2560 beads: the options f64_max_beads / f64_column_chunk, the chunked form of the fp64 step kernel
(k64_step_chunked, csrc/c3d_f64_step_body.inc) against the staged form bit for bit where both run, against the oracle past the old limit,
the 16384-bead ceiling from a restraint list, and c3d_solve --precision 64.

Every test here runs on a context of its own (module fixture), never the session's: precision 64 and both limits stay raised on it."""
import os
import subprocess

import numpy as np
import pytest

from tests.util import oracle_fire_from, oracle_model_from, random_coil, synthetic_if

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TP = 4                                             # two-point steps of the kind-5 stage before its hand-over to FIRE


def _stages(a, b, c, d, e=0):
    """test_fp64_column_layouts_follow_the_oracle's four stages (FIRE, MD at 2000 K, kind 1, FIRE), then e steps of kind 5"""
    st = [(2, a, 0.0, 1.0, 20.0, 0.5, 0.0), (0, b, 0.003, 0.4, 0.003, 0.9, 2000.0), (1, c, 0.005, 1.0, 0.05, 1.0, 1500.0),
          (2, d, 0.0, 1.0, 1.0, 0.85, 0.0)]
    return st + ([(5, e, 0.0, 1.0, 1.0, 0.85, 0.0)] if e else [])


SHORT = _stages(6, 10, 6, 6, 10)                  # 38 steps, the kind-5 stage across its hand-over (TP = 4 of its 10 steps)
GENERAL = {"gen0": (dict(noe_pot=0, asym=3.0, rswitch=2.0), 0), "gen1": (dict(noe_pot=1, asym=1.0, rswitch=0.5), 1),
           "gen2": (dict(noe_pot=2, asym=1.5, rswitch=1.0), 2), "gen3": (dict(noe_pot=3, mrswitch=4.0, masym=3.0, msoexp=1), 3)}


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    s.set_option("max_beads", 16384)
    s.set_option("f64_max_beads", 16384)
    s.set_option("precision", 64)
    s.set_option("final_minimiser_steps", TP)
    yield s
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.set_two_point_steps(TP)
    yield oracle
    oracle.set_two_point_steps(1000)


def _run(s, stages, nrep, chunk, x0=None, groups=2):
    """the schedule from the same start under f64_column_chunk `chunk`: start, coordinates, velocities, kernel name"""
    from chromosome3d_amd import default_fire, make_stages
    s.set_option("f64_column_chunk", chunk)
    s.set_option("replica_groups", groups)
    try:
        s.set_schedule(make_stages(stages), default_fire())
        s.init_replicas(nrep, 82364, 0)
        if x0 is not None:
            s.set_coords(x0)
        start = s.coords()
        k = sum(st[1] for st in stages)
        assert s.run_steps(10 ** 6) == k
        return start, s.coords(), s.velocities(), s.step_kernel_name
    finally:
        s.set_option("f64_column_chunk", 0)
        s.set_option("replica_groups", 2)


def _against_oracle(O, m, d10, stages, start, x, v):
    """every replica against O.run_schedule from the same start, within the fp32 read-back's grain (the existing fp64 test's tolerance)"""
    from chromosome3d_amd import default_fire
    n = start.shape[1]
    om, of = oracle_model_from(m, n), oracle_fire_from(default_fire())
    k = sum(st[1] for st in stages)
    worst = 0.0
    for r in range(start.shape[0]):
        xo, vo, ev = O.run_schedule(om, d10, O.make_stages(stages), of, 82364, r, x0=start[r].astype(np.float64))
        assert ev == k
        xc = x[r].astype(np.float64)
        xc -= xc.mean(0)
        tol = max(2e-5, 1.2e-7 * np.abs(xo).max())
        e = float(np.abs(xc - xo).max())
        ev_ = float(np.abs(v[r] - vo).max())
        print(f"n={n} replica {r}: |dx| {e:.2e} (tol {tol:.2e}), |dv| {ev_:.2e} (tol {2e-5 * max(1.0, np.abs(vo).max()):.2e})")
        assert e < tol, (r, e, tol)
        assert ev_ < 2e-5 * max(1.0, np.abs(vo).max()), (r, ev_)
        worst = max(worst, e)
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
def test_options():
    """Bad values of both options are refused; f64_max_beads = 3000 lets 2561 beads initialise and refuses 3001 naming 3000; a fresh
    context without the option still refuses 2561 naming 2560."""
    from chromosome3d_amd import C3DError, Solver, default_model
    s = Solver(0)
    try:
        for bad in (2559, 16385, 3000.5, -1, 0):
            with pytest.raises(C3DError):
                s.set_option("f64_max_beads", bad)
        for bad in (128, 384, 2048, 100.5, -256):
            with pytest.raises(C3DError):
                s.set_option("f64_column_chunk", bad)
        for ok in (256, 512, 1024, 0):
            s.set_option("f64_column_chunk", ok)
        s.set_model(default_model())
        s.set_option("precision", 64)
        s.set_if_matrix(np.ones((2561, 2561)))
        with pytest.raises(C3DError, match="2560"):
            s.init_replicas(1, 82364, 0)
        s.set_option("f64_max_beads", 3000)
        s.init_replicas(1, 82364, 0)
        assert s.n == 2561 and np.isfinite(s.coords()).all()
        s.set_if_matrix(np.ones((3001, 3001)))
        with pytest.raises(C3DError, match="3000"):
            s.init_replicas(1, 82364, 0)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 383, 384, 512, 545, 1025, 2049, 2559, 2560])
def test_chunked_form_has_the_bits_of_the_staged_form(ctx, n):
    """Where both forms run, k64_step_chunked (CHUNK 256 and, where n > 1024, 1024) ends in k64_step's bits: FIRE, MD at 2000 K, kind 1,
    FIRE and a kind-5 stage across its hand-over; coordinates and velocities array_equal, every run identified by its kernel name.  With
    CHUNK 256: 257 = the two-rows pass of one column alone in chunk 2; 383 = 64-column block + 63 left-over columns in chunk 2; 384 = a
    chunk of one main pass; 512 = whole chunks, no tail; 545 = a left-over of 33 alone in chunk 3; 1025 = a last tile of one row; 2049 at
    CHUNK 1024 = one column in chunk 3; 2559 = a tile of seven rows; 2560 = n = np (no padding bead).  The shipped potential at every n, one
    general tail of each kind at 545, 2 replicas, and 20 replicas in two groups at 545."""
    from chromosome3d_amd import default_model
    s = ctx
    IF = synthetic_if(n, seed=n)[0]
    cases = [("shipped", {}, 4, False, 2)]
    if n == 545:
        cases += [(k, kw, pot, True, 2) for k, (kw, pot) in GENERAL.items()] + [("shipped x20", {}, 4, False, 20)]
    for label, kw, pot, gen, nrep in cases:
        s.set_model(default_model(**kw))
        s.set_if_matrix(IF)
        tail = f"{pot}, {'true' if gen else 'false'}, {'true' if pot == 4 else 'false'}"
        _, x, v, name = _run(s, SHORT, nrep, 0)
        assert name == f"c3d::k64_step<{tail}>", (label, name)
        assert np.isfinite(x).all()
        for chunk in (256, 1024):
            if n <= chunk:
                continue
            _, xc, vc, namec = _run(s, SHORT, nrep, chunk)
            assert namec == f"c3d::k64_step_chunked<{tail}, {chunk}>", (label, namec)
            assert np.array_equal(xc, x) and np.array_equal(vc, v), (label, chunk, float(np.abs(xc - x).max()))
    s.set_model(default_model())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrep,chunks", [(2561, 2, (0,)), (3073, 1, (0,)), (5121, 1, (512, 1024))])
def test_past_the_old_limit_follows_the_oracle(ctx, O, n, nrep, chunks):
    """2561 x 2 and 3073 x 1 (= 3 x 1024 + 1) with the default chunk, 5121 x 1 at CHUNK 512 and 1024: the four stages in their short form
    (6 / 10 / 6 / 6 steps), every replica against O.run_schedule from the same start within max(2e-5, 1.2e-7 max|x|) A after centring and
    2e-5 max(1, max|v|) for the velocities: the fp32 read-back's grain, the tolerance of test_fp64_column_layouts_follow_the_oracle."""
    from chromosome3d_amd import default_model
    s = ctx
    m = default_model()
    s.set_model(m)
    IF = synthetic_if(n, seed=n)[0]
    s.set_if_matrix(IF)
    d10 = O.if_to_dist10(IF)
    stages = _stages(6, 10, 6, 6)
    ref = None
    for chunk in chunks:
        start, x, v, name = _run(s, stages, nrep, chunk)
        assert name == f"c3d::k64_step_chunked<4, false, true, {chunk or 512}>", name
        if ref is None:                            # the oracle once: every chunk starts from the same coordinates
            _against_oracle(O, m, d10, stages, start, x, v)
            ref = (start, x, v)
        else:                                      # and the chunked forms agree bit for bit
            assert np.array_equal(start, ref[0]) and np.array_equal(x, ref[1]) and np.array_equal(v, ref[2]), chunk


# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_ceiling_16384(ctx, O):
    """n = 16384, one replica, from test_the_ceiling_16384's sparse restraint set (|i - j| <= 64 and 10^5 random long-range pairs) through
    c3d_set_restraints: two FIRE steps with the default chunk, finite, and against the oracle's two steps on the dense tenths within the
    tolerance above."""
    from chromosome3d_amd import default_model
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
    stages = [(2, 2, 0.0, 1.0, 20.0, 0.5, 0.0)]
    start, x, v, name = _run(s, stages, 1, 0, x0=(truth * 1.1).astype(np.float32)[None])
    assert name == "c3d::k64_step_chunked<4, false, true, 512>", name
    assert np.isfinite(x).all() and np.isfinite(v).all()
    d10 = np.zeros((n, n), dtype=np.int32)
    d10[ri, rj] = t10
    d10[rj, ri] = t10
    del ri, rj, li, lj
    _against_oracle(O, m, d10, stages, start, x, v)


# ---------------------------------------------------------------------------------------------------------------------------------
def _write_banded(path, n, width=200):
    """a symmetric IF matrix that is zero for |i - j| > width (contact.tbl stays small) (tests/test_gpu_large_maps.py's)"""
    band = ["%.4g" % (1.0 / (1.0 + d)) for d in range(width + 1)]
    with open(path, "w") as f:
        for i in range(n):
            lo, hi = max(0, i - width), min(n, i + width + 1)
            f.write(" ".join(["0"] * lo + [band[abs(j - i)] for j in range(lo, hi)] + ["0"] * (n - hi)) + "\n")


def test_cli_precision_64(tmp_path):
    """c3d_solve --precision 64 on a banded 2600-bead matrix (it raises f64_max_beads itself) exits 0 and writes two models of 2600 beads."""
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    mat = tmp_path / "matrix.txt"
    _write_banded(str(mat), 2600)
    out = tmp_path / "out"
    out.mkdir()
    p = subprocess.run([exe, "-i", str(mat), "-o", str(out), "-m", "2", "--min-steps", "40", "--precision", "64"], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    pdbs = sorted(f for f in os.listdir(out) if f.endswith(".pdb"))
    assert len(pdbs) == 2, os.listdir(out)
    for f in pdbs:
        assert len([l for l in open(out / f) if l.startswith("ATOM")]) == 2600
