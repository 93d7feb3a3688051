"""Model geometry on the device (c3d_geometry_replicas, c3d_separation_profile; csrc/c3d_score_geometry.inc k_geo_*, k_sep_*) against the numpy
restatement tests/geometry_ref.py, which tests/test_geometry_ref.py holds to the reference's clash counts, to tests/util.chain_stats and
to tests/ensemble_ref.

Shapes, the smallest at which each part can still go wrong.  k_geo_pairs gives a workgroup 64 row beads and walks the columns in blocks of
64; k_sep_profile gives a workgroup 64 separations, walks i in chunks of 64 and stages the picked models in blocks of 8:
  n3, n63, n64, n65, n129   2 replicas each: the smallest chain, one tile short by a bead, one full tile, a second tile of one bead, three
  n257                      257 beads x 5 + 2 extra fp64 models that no float holds: five row blocks / separation blocks, K = 7
  k17                       64 beads x 17: three staged model blocks in the profile, the last of one model
  the seven bundled models  n = 35 .. 455: zero to seven tile edges, against the reference's own counts
  n6000                     6000 beads x 1 + 1 extra fp64 model on a context of its own with max_beads raised: 94 row blocks of which the last
                            has 48 beads, past the 5120 beads a context holds by default; coils at 0.5 and 0.6 of the usual step, so that
                            tens of thousands of pairs clash; cutoff 3.5 and sep 2 (one sep: the numpy side takes 2 s a model and sep), the
                            profile at cutoff 7.6 over all 6000 separations.  Printed on an MI355X: 45974 and 33006 clashes, counts,
                            nearest and extent equal, largest chain gap 4.4e-16 under a bound of 1.0e-9, largest profile gap 0.016 of
                            its bound (mean) and 0.002 (sd)

Bounds.  Distances have the host's bits, so counts, minima and maxima are compared with ==.  A sum of T same-sign fp64 terms taken in two
orders differs by at most 2 T 2^-53 relative; the tests assert 8 T 2^-53 x the largest magnitude entering the sum (the factor 4 covers
the division, the square root and the mean's own error entering the deviations), T = n for the chain fields and (n - s) Kp for the
profile.  The largest magnitude is the largest distance summed; for the radius of gyration it is the largest |x_i - centroid|, which
bounds the result."""
import os
import subprocess

import numpy as np
import pytest

from tests import ensemble_ref as E
from tests import geometry_ref as G
from tests.util import GOLD, SHORT, golden, load_pdb_xyz, random_coil, restrained, shared_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SIZES = {"n3": 3, "n63": 63, "n64": 64, "n65": 65, "n129": 129}
CASES = list(SIZES) + ["n257"]
PICK257 = [6, 4, 2, 2, 0]


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _context(s, n, nrep):
    """a context of n beads with nrep replicas (restrained() needs a few beads to draw its restraints from)"""
    if n >= 8:
        return restrained(s, n, nrep)
    from chromosome3d_amd import default_model, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
    s.init_replicas(nrep)


def _models(name):
    if name in SIZES:
        n = SIZES[name]
        return np.stack([random_coil(n, 20 * n + r) for r in range(2)]), None
    return shared_models(name)


def _load(s, name):
    """the context holding the case's replicas; returns (extra, all K models as doubles)"""
    x, extra = _models(name)
    _context(s, x.shape[1], x.shape[0])
    s.set_coords(x)
    return extra, [m.astype(np.float64) for m in x] + ([] if extra is None else list(extra))


_HOST = {}


def _host_geometry(name, models, cutoff, sep):
    key = ("geo", name, cutoff, sep)
    if key not in _HOST:
        _HOST[key] = [G.geometry(m, cutoff, sep) for m in models]
    return _HOST[key]


def _host_profile(name, models, pick, cutoff):
    key = ("sep", name, None if pick is None else tuple(pick), cutoff)
    if key not in _HOST:
        _HOST[key] = G.separation_profile(models, pick, cutoff)
    return _HOST[key]


def _check_geometry(got, host, models, what):
    n = len(models[0])
    for k, (h, x) in enumerate(zip(host, models)):
        assert got["clashes"][k] == h["clashes"], (what, k)
        assert np.array_equal(got["bead_clashes"][k], h["bead_clashes"]), (what, k)
        assert int(got["bead_clashes"][k].sum()) == 2 * int(got["clashes"][k])
        assert got["nearest"][k].tobytes() == h["nearest"].tobytes(), (what, k)              # bitwise
        assert got["chain"][k, 5].tobytes() == h["chain"][5].tobytes(), (what, k)
        dmax = h["chain"][5]
        u = x - x.mean(0)
        big = [dmax, dmax, dmax, dmax, np.sqrt((u * u).sum(1)).max()]
        gaps = [abs(got["chain"][k, f] - h["chain"][f]) for f in range(5)]
        tols = [8 * n * U * b for b in big]
        print(f"{what} model {k}: clashes {got['clashes'][k]}, chain gaps {['%.2e' % g for g in gaps]}, bounds {['%.2e' % t for t in tols]}")
        for f in range(5):
            assert gaps[f] <= tols[f], (what, k, f, gaps[f], tols[f])


def _check_profile(got, host, n, Kp, what):
    mean, sd, contact = got
    hmean, hsd, hcontact, hcount, largest = host
    T = (n - np.arange(n)) * Kp
    tol = 8 * T * U * largest
    print(f"{what}: n {n}, Kp {Kp}, max mean gap / bound {np.nanmax(np.abs(mean - hmean)[1:] / tol[1:]):.3f}, max sd gap / bound "
          f"{np.nanmax(np.abs(sd - hsd)[1:] / tol[1:]):.3f}")
    assert (np.abs(mean - hmean) <= tol).all(), what
    assert (np.abs(sd - hsd) <= tol).all(), what
    assert (mean[0], sd[0]) == (0.0, 0.0)
    if hcount is not None:
        assert np.array_equal(np.rint(contact * T).astype(np.int64), hcount), what           # exact counts
        assert np.array_equal(contact, hcontact) and contact[0] == 1.0                        # divided once


@pytest.mark.parametrize("cid", sorted(golden()))
def test_the_references_clash_counts_come_out_of_the_device(ctx, cid):
    """Each bundled model as an extra model beside one replica: clash_count(pdb, 3.5) of chromosome3D.pl:693-714."""
    g = golden()[cid]
    x = load_pdb_xyz(os.path.join(GOLD, "models", g["model"]))
    _context(ctx, g["n"], 1)
    got = ctx.geometry(x, 3.5, 1)
    print(f"{cid}: n {g['n']}, clashes {got['clashes'][1]} (reference {g['clash_3p5']}), closest pair {got['nearest'][1].min():.3f} A")
    assert got["clashes"][1] == g["clash_3p5"]
    assert int(got["bead_clashes"][1].sum()) == 2 * g["clash_3p5"]
    h = G.geometry(x, 3.5, 1)
    assert np.array_equal(got["bead_clashes"][1], h["bead_clashes"]) and got["nearest"][1].tobytes() == h["nearest"].tobytes()


@pytest.mark.parametrize("name", CASES)
def test_geometry_equals_the_restatement(ctx, name):
    extra, models = _load(ctx, name)
    n = len(models[0])
    for sep in sorted({s for s in (1, 2, 5) if s <= n - 1} | {n - 1}):
        got = ctx.geometry(extra, 3.5, sep)
        assert got["clashes"].shape == (len(models),) and got["bead_clashes"].shape == got["nearest"].shape == (len(models), n)
        _check_geometry(got, _host_geometry(name, models, 3.5, sep), models, f"{name} sep {sep}")
    ends = ctx.geometry(extra, 3.5, n - 1)["nearest"]
    assert np.isfinite(ends[:, [0, n - 1]]).all() and (n == 3 or np.isinf(ends[:, 1:n - 1]).all())   # only the end beads have a partner
    # a cutoff that a distance of model 0 equals exactly: `<=` counts that pair, `<` would not
    d = E.distances(models[0])
    a, b = 0, min(n - 1, 5)
    cut = float(d[a, b])
    got = ctx.geometry(extra, cut, 1)
    host = _host_geometry(name, models, cut, 1)
    _check_geometry(got, host, models, f"{name} cutoff d({a},{b})")
    strictly = int((d[np.triu_indices(n, 1)] < cut).sum())
    assert got["clashes"][0] > strictly and got["clashes"][0] == int((d[np.triu_indices(n, 1)] <= cut).sum())


@pytest.mark.parametrize("name", ["k17", "n257", "n65", "n3"])
def test_profile_equals_the_restatement_and_the_maps_diagonals(ctx, name):
    extra, models = _load(ctx, name)
    n, K = len(models[0]), len(models)
    picks = [None] + ({"k17": [[16, 3, 8, 0, 9, 1, 12, 5, 7], [2, 16, 2]], "n257": [[0, 2, 4, 6], PICK257]}.get(name, []))
    for pick in picks:
        Kp = K if pick is None else len(pick)
        got = ctx.separation_profile(extra, pick, 7.6)
        host = _host_profile(name, models, pick, 7.6)
        _check_profile(got, host, n, Kp, f"{name} pick {pick}")
        maps = ctx.ensemble_map(extra, pick, 7.6, sd=False)
        diag = np.array([np.diagonal(maps["mean"], s).mean() for s in range(n)])
        assert (np.abs(got[0] - diag) <= 8 * (n - np.arange(n)) * Kp * U * host[4]).all()
        count = np.array([np.rint(np.diagonal(maps["contact"], s) * Kp).sum() for s in range(n)]).astype(np.int64)
        assert np.array_equal(np.rint(got[2] * (n - np.arange(n)) * Kp).astype(np.int64), count)
    if name == "n257":
        assert np.abs(ctx.separation_profile(extra, PICK257)[0] - ctx.separation_profile(extra, [0, 2, 4, 6])[0]).max() > 1e-3   # the repeat counts
        assert 0.0 < got[2][3] < 1.0                                            # the cutoff separates something
    mean, sd, contact = ctx.separation_profile(extra)                           # no cutoff: no contact profile
    assert contact is None and mean.tobytes() == ctx.separation_profile(extra, None, 7.6)[0].tobytes()


@pytest.fixture(scope="module")
def ctx6000():
    """a context of 6000 beads (max_beads raised) holding the case n6000; yields (solver, extra, models)"""
    from chromosome3d_amd import Solver
    n = 6000
    x = (random_coil(n, 60000) * np.float32(0.5))[None]
    extra = (random_coil(n, 60001).astype(np.float64) * 0.6 + np.random.default_rng(6000).normal(scale=1e-3, size=(n, 3)))[None]
    assert not np.array_equal(extra, extra.astype(np.float32))
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        restrained(s, n, 1)
        s.set_coords(x)
        yield s, extra, [x[0].astype(np.float64), extra[0]]
    finally:
        s.close()


def test_geometry_of_6000_beads_equals_the_restatement(ctx6000):
    """c3d_geometry_replicas beyond the default bead limit: counts, nearest and extent equal, the chain fields within 8 n 2^-53."""
    s, extra, models = ctx6000
    got = s.geometry(extra, 3.5, 2)
    assert got["clashes"].shape == (2,) and got["bead_clashes"].shape == got["nearest"].shape == (2, 6000)
    _check_geometry(got, [G.geometry(m, 3.5, 2) for m in models], models, "n6000 sep 2")
    assert got["clashes"].min() > 10000                                         # the cutoff counts something in both models


def test_profile_of_6000_beads_equals_the_restatement(ctx6000):
    """c3d_separation_profile over all 6000 separations, both models, within 8 (n - s) Kp 2^-53 x the largest distance at s."""
    s, extra, models = ctx6000
    got = s.separation_profile(extra, None, 7.6)
    _check_profile(got, G.separation_profile(models, None, 7.6), 6000, 2, "n6000")
    assert 0.0 < got[2][5] < 1.0 and got[2][5999] == 0.0                        # the cutoff separates something


def test_f64_state_is_measured_in_doubles():
    """A precision-64 context: the results follow the fp64 state, not its float rounding."""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        restrained(s, 96, 3)
        rng = np.random.default_rng(96)
        x = np.stack([random_coil(96, 960 + r).astype(np.float64) for r in range(3)]) + rng.normal(scale=1e-3, size=(3, 96, 3))
        assert not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x)
        got = s.geometry(None, 3.5, 2)
        _check_geometry(got, [G.geometry(m, 3.5, 2) for m in x], list(x), "f64")
        rounded = [G.geometry(m, 3.5, 2) for m in x.astype(np.float32).astype(np.float64)]
        assert all(got["nearest"][k].tobytes() != rounded[k]["nearest"].tobytes() for k in range(3))
        prof = s.separation_profile(None, None, 7.6)
        _check_profile(prof, G.separation_profile(list(x), None, 7.6), 96, 3, "f64")
        # rounding coordinates of 10 A to float moves the distances by up to 5e-7 A; 1e-9 is a thousand times the bound on the device
        assert np.abs(prof[0] - G.separation_profile(list(x.astype(np.float32).astype(np.float64)))[0]).max() > 1e-9
    finally:
        s.close()


def test_two_calls_return_the_same_bytes_and_nothing_of_the_solve_changes(ctx):
    extra, models = _load(ctx, "n257")
    ctx.run_steps(20)                                                           # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    runs = ctx.stat("geometry_runs"), ctx.stat("separation_runs")
    g1, g2 = ctx.geometry(extra, 3.5, 2), ctx.geometry(extra, 3.5, 2)
    p1, p2 = ctx.separation_profile(extra, PICK257, 7.6), ctx.separation_profile(extra, PICK257, 7.6)
    for k in g1:
        assert g1[k].tobytes() == g2[k].tobytes(), k
    for a, b in zip(p1, p2):
        assert a.tobytes() == b.tobytes()
    alone = ctx.geometry(None, 3.5, 2)                                          # without the extra models: the replicas keep their bits
    for k in g1:
        assert alone[k].tobytes() == g1[k][:5].tobytes(), k
    assert ctx.separation_profile(None, [4, 0, 0], 7.6)[1].tobytes() == ctx.separation_profile(extra, [4, 0, 0], 7.6)[1].tobytes()
    assert (ctx.stat("geometry_runs"), ctx.stat("separation_runs")) == (runs[0] + 3, runs[1] + 4)
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    # one output alone: the same bits
    from chromosome3d_amd import lib
    only = np.empty((5, 6))
    assert ctx._L.c3d_geometry_replicas(ctx._h, None, 0, 0.0, 2, None, None, None, lib.dptr(only)) == 0       # the chain fields need no cutoff
    assert only.tobytes() == alone["chain"].tobytes()
    sd = np.empty(257)
    assert ctx._L.c3d_separation_profile(ctx._h, lib.dptr(extra), 2, lib.i32ptr(np.array(PICK257, np.int32)), 5, 0.0, None, lib.dptr(sd), None) == 0
    assert sd.tobytes() == p1[1].tobytes()
    assert ctx.run_steps(5) == 5                                                # and the solve goes on


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name; none counts as a run; the context works afterwards."""
    import ctypes as C
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    extra, models = _load(ctx, "n64")
    n, M = 64, 2
    L, h = ctx._L, ctx._h
    runs = ctx.stat("geometry_runs"), ctx.stat("separation_runs")
    state = ctx.coords().tobytes()
    cl, bead, near, chain = np.empty(300, np.int64), np.empty((300, n), np.int32), np.empty((300, n)), np.empty((300, 6))
    prof = np.empty((3, n))
    clp, bp, np_, cp = cl.ctypes.data_as(C.POINTER(C.c_int64)), lib.i32ptr(bead), lib.dptr(near), lib.dptr(chain)
    m, s, c = lib.dptr(prof[0]), lib.dptr(prof[1]), lib.dptr(prof[2])
    good = np.stack(models)
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows
    i32 = lambda v: lib.i32ptr(np.array(v, np.int32))

    def geo_refused(*a):
        assert L.c3d_geometry_replicas(h, *a) == -1 and b"c3d_geometry_replicas" in L.c3d_last_error(), a

    def sep_refused(*a):
        assert L.c3d_separation_profile(h, *a) == -1 and b"c3d_separation_profile" in L.c3d_last_error(), a

    geo_refused(None, 0, 3.5, 1, None, None, None, None)                        # every output NULL
    sep_refused(None, 0, None, 0, 7.6, None, None, None)
    for sep in (0, n, -1):                                                      # sep outside 1..n-1
        geo_refused(None, 0, 3.5, sep, clp, bp, np_, cp)
    for bad in (0.0, np.nan, -1.0, np.inf):                                     # a count without a usable cutoff
        geo_refused(None, 0, bad, 1, clp, None, None, None)
        geo_refused(None, 0, bad, 1, None, bp, None, None)
        sep_refused(None, 0, None, 0, bad, m, s, c)                             # contact without a cutoff
    sep_refused(None, 0, i32([0, M]), 2, 7.6, m, s, c)                          # a pick index = K
    sep_refused(None, 0, i32([0, -1]), 2, 7.6, m, s, c)
    sep_refused(None, 0, i32([0]), 0, 7.6, m, s, c)                             # a list without a length
    sep_refused(None, 0, None, 2, 7.6, m, s, c)                                 # a length without a list
    sep_refused(None, 0, i32([0] * 4097), 4097, 7.6, m, s, c)
    geo_refused(None, 1, 3.5, 1, clp, bp, np_, cp)                              # n_extra > 0 without coordinates
    sep_refused(None, 1, None, 0, 7.6, m, s, c)
    geo_refused(lib.dptr(good), -1, 3.5, 1, clp, bp, np_, cp)
    sep_refused(lib.dptr(good), -1, None, 0, 7.6, m, s, c)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        geo_refused(lib.dptr(e), M, 3.5, 1, clp, bp, np_, cp)
        sep_refused(lib.dptr(e), M, None, 0, 7.6, m, s, c)
    geo_refused(lib.dptr(big), len(big), 3.5, 1, clp, bp, np_, cp)              # K = 257
    sep_refused(lib.dptr(big), len(big), None, 0, 7.6, m, s, c)
    assert (ctx.stat("geometry_runs"), ctx.stat("separation_runs")) == runs
    assert ctx.coords().tobytes() == state
    # 256 models are accepted; nearest and the chain fields need no cutoff; the context works
    got = ctx.geometry(big[:-1] + good[0], 3.5, 1)
    h0 = G.geometry(models[0], 3.5, 1)
    assert got["clashes"][0] == got["clashes"][255] == h0["clashes"] and got["nearest"][255].tobytes() == h0["nearest"].tobytes()
    assert L.c3d_geometry_replicas(h, None, 0, np.nan, 1, None, None, np_, cp) == 0
    assert near[:M].tobytes() == got["nearest"][:M].tobytes()
    _check_geometry(ctx.geometry(None, 3.5, 5), _host_geometry("n64", models, 3.5, 5), models, "n64 after the refusals")
    _check_profile(ctx.separation_profile(None, None, 7.6), _host_profile("n64", models, None, 7.6), n, M, "n64 after the refusals")
    # no replicas; 2 beads: a profile, no geometry
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(2, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        for call in (s2.geometry, s2.separation_profile):
            with pytest.raises(C3DError, match="c3d_(geometry_replicas|separation_profile).*c3d_init_replicas"):
                call()
        s2.init_replicas(2)
        with pytest.raises(C3DError, match="c3d_geometry_replicas.*fewer than 3 beads"):
            s2.geometry()
        two = s2.separation_profile(cutoff=1e3)
        d = G.separation_profile([x.astype(np.float64) for x in s2.coords()], None, 1e3)
        assert np.array_equal(two[0], d[0]) and np.array_equal(two[2], np.ones(2))
        assert s2.stat("geometry_runs") == 0 and s2.stat("separation_runs") == 1
    finally:
        s2.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --geometry on the smallest bundled matrix: both files, rows in rank order, and a clash column that is Solver.geometry's of
    the written models."""
    cid, M = "chr21_1mb", 4
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "geo")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--geometry", prefix], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = [l.split() for l in open(prefix + "_geometry.txt") if not l.startswith("#")]
    assert len(rows) == M and [int(r[0]) for r in rows] == [1, 2, 3, 4] and sorted(int(r[1]) for r in rows) == [1, 2, 3, 4] and all(len(r) == 10 for r in rows)
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r + 1}.pdb") for r in range(M)])
    restrained(ctx, 37, M)
    ctx.set_coords(x)
    got = ctx.geometry(None, 3.5, 1)
    for r in rows:
        k = int(r[1]) - 1
        print(f"rank {r[0]} model {r[1]}: clashes {r[2]} (of the written model {got['clashes'][k]}), nearest {r[3]} ({got['nearest'][k].min():.3f})")
        assert int(r[2]) == got["clashes"][k]
        # written coordinates are rounded to 3 decimals (a distance moves by at most sqrt(3) 1e-3) and so are the printed numbers (5e-4)
        assert abs(float(r[3]) - got["nearest"][k].min()) <= 2.3e-3
        assert np.abs(np.array([float(v) for v in r[4:]]) - got["chain"][k]).max() <= 2.3e-3
    prof = np.array([[float(v) for v in l.split()] for l in open(prefix + "_separation.txt") if not l.startswith("#")])
    assert prof.shape == (37, 4) and np.array_equal(prof[:, 0], np.arange(37)) and tuple(prof[0, 1:]) == (0.0, 0.0, 1.0)
    mean, sd, contact = ctx.separation_profile(None, None, 2 * 3.8)
    assert np.abs(prof[:, 1] - mean).max() <= 2.3e-3 and np.abs(prof[:, 2] - sd).max() <= 2.3e-3
    top = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", str(M), "--quiet", "--geometry", str(tmp_path / "top"), "--ensemble-top", "2",
                          "--ensemble-cutoff", "0", "--clash-cutoff", "8", "--clash-sep", "3"], capture_output=True, text=True)
    assert top.returncode == 0, top.stderr
    assert "# s mean sd   (2 models)" in open(tmp_path / "top_separation.txt").read()
    assert "pairs |i-j| >= 3; clash: d <= 8 A" in open(tmp_path / "top_geometry.txt").read()
    # a cutoff that counts something: a written distance is within sqrt(3) 1e-3 of the one the run counted, so the file's count lies between
    # the written models' counts at 8 -+ 2e-3
    rows = [l.split() for l in open(tmp_path / "top_geometry.txt") if not l.startswith("#")]
    ctx.set_coords(np.stack([load_pdb_xyz(tmp_path / "b" / f"{cid}_matrix_{r + 1}.pdb") for r in range(M)]))
    lo, hi = ctx.geometry(None, 8.0 - 2e-3, 3)["clashes"], ctx.geometry(None, 8.0 + 2e-3, 3)["clashes"]
    for r in rows:
        k = int(r[1]) - 1
        print(f"cutoff 8, sep 3, model {r[1]}: clashes {r[2]}, of the written model {lo[k]} .. {hi[k]}")
        assert lo[k] <= int(r[2]) <= hi[k], (r, lo[k], hi[k])
    assert sum(int(r[2]) for r in rows) > 0
