"""Entanglement on the device (c3d_entanglement; csrc/c3d_score_entangle.inc k_ent_*) against the numpy restatement tests/entangle_ref.py, which
tests/test_entangle_ref.py holds to a quadrature of the Gauss integral, to the four-asin form, to shapes with known answers and to
itself in extended precision.

Shapes, the smallest at which each part can still go wrong.  k_ent_pairs gives a workgroup 64 row segments (the tile the issue names; it
was built as such) and walks the column segments in blocks of 64; a model of n beads has S = n - 1 segments:
  n4, n5                  3 and 4 segments: one counted pair from each side, then three
  n64, n65, n66           63, 64 and 65 segments: one short of a tile, a full tile, a second tile of one segment
  n130                    129 segments: three tiles, the last of one segment; the windows 3..10 (cuts inside a tile and skips whole blocks)
                          and S-1..S-1 (a single pair)
  n257                    257 beads x 5 + 2 extra fp64 models that no float holds: four full tiles, K = 7; the same windows; the domain
                          tables D = 1, D = 4 on the tile edges, D = 5 off them with a one-segment domain, D = 256 with every segment its own
  k17                     64 beads x 17 models
  n50                     the shapes with known answers as extra models: straight chain, planar spiral, helix and its mirror, two rings
  n6000                   6000 beads x 1 on a context of its own with max_beads raised: 94 tiles, the last of 47 segments; 96 sampled rows

Bounds.  A sum of terms g is held to 8 x 2^-53 x (the sum of kappa over its terms) plus one unit in the last place of the sum for the
device's one division by 2 pi; kappa(s, t) = max(1, |u||v||w| / |den|), the larger of the two triangles, is the conditioning of the atan2
whose numerator and denominator each carry a few roundings of size |u||v||w|.  The restatement itself stays under 0.3 % of that bound on
rows against 80-bit arithmetic (tests/test_entangle_ref.py).  Integers, refusals and bit identities are compared with ==.
Printed on an MI355X, the largest device-host gap as a fraction of its bound: 0.070 over the whole file (a single-pair entry of the D = 256
table), 0.021 over row sums and totals (n257, window 3..10), 0.0003 over the 96 sampled rows of n6000; the linked rings' block
-1.000000000000, the unlinked rings' 1.8e-18 (profiles/r34_entanglement.md)."""
import os
import subprocess

import numpy as np
import pytest

from tests import entangle_ref as E
from tests.util import GOLD, SHORT, load_pdb_xyz, random_coil, restrained, shared_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SIZES = {"n4": 4, "n5": 5, "n64": 64, "n65": 65, "n66": 66, "n130": 130}
WINDOWS = {"n130": [(3, 10), (128, 128)], "n257": [(3, 10), (255, 255), (2, 255)]}
BOUNDS257 = {"D1": [0, 256], "D4": [0, 64, 128, 192, 256], "D5": [0, 30, 31, 100, 193, 256], "D256": list(range(257))}


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


def _context(s, n, nrep):
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
        return np.stack([random_coil(n, 30 * n + r) for r in range(2)]), None
    return shared_models(name)


def _load(s, name):
    """the context holding the case's replicas; returns (extra, all K models as doubles)"""
    x, extra = _models(name)
    _context(s, x.shape[1], x.shape[0])
    s.set_coords(x)
    return extra, [m.astype(np.float64) for m in x] + ([] if extra is None else list(extra))


_HOST = {}


def _host(name, models, min_sep, max_sep, bounds=None):
    key = (name, min_sep, max_sep, None if bounds is None else tuple(bounds))
    if key not in _HOST:
        _HOST[key] = [E.entanglement(m, min_sep, max_sep, bounds) for m in models]
    return _HOST[key]


def _tol(kappa, ref):
    return 8 * U * np.asarray(kappa) + np.spacing(np.abs(np.asarray(ref, np.float64)))


def _check(got, host, what, table=False):
    worst = 0.0
    for k, h in enumerate(host):
        pairs = [(got["seg_writhe"][k], h["seg_writhe"], h["seg_kappa"]), (got["seg_acn"][k], h["seg_acn"], h["seg_kappa"]),
                 (got["writhe"][k], h["writhe"], h["kappa"]), (got["acn"][k], h["acn"], h["kappa"])]
        if table:
            pairs += [(got["link"][k], h["link"], h["link_kappa"]), (got["link_abs"][k], h["link_abs"], h["link_kappa"])]
        for q, (dev, ref, kappa) in enumerate(pairs):
            gap, tol = np.abs(np.asarray(dev) - np.asarray(ref)), _tol(kappa, ref)
            worst = max(worst, float(np.max(gap / tol)))
            assert (gap <= tol).all(), (what, k, q, float(np.max(gap / tol)))
        zero = np.asarray(h["seg_kappa"]) == 0                                   # a segment without a counted partner
        assert (got["seg_writhe"][k][zero] == 0).all() and (got["seg_acn"][k][zero] == 0).all()
        assert (got["seg_acn"][k] >= np.abs(got["seg_writhe"][k])).all() and got["acn"][k] >= abs(got["writhe"][k])
    print(f"{what}: K {len(host)}, writhe {['%.4f' % w for w in got['writhe'][:3]]}, acn {['%.4f' % a for a in got['acn'][:3]]}, largest gap / bound {worst:.4f}")
    return worst


@pytest.mark.parametrize("name", list(SIZES) + ["k17", "n257"])
def test_rows_and_totals_equal_the_restatement(ctx, name):
    extra, models = _load(ctx, name)
    S = len(models[0]) - 1
    for lo, hi in [(2, 0)] + WINDOWS.get(name, []):
        got = ctx.entanglement(extra, lo, hi)
        assert got["seg_writhe"].shape == (len(models), S) and got["writhe"].shape == (len(models),) and got["device_ms"] >= 0
        _check(got, _host(name, models, lo, hi), f"{name} sep {lo}..{hi}")
    if name in WINDOWS:
        lo, hi = WINDOWS[name][1]                                              # the single pair (0, S-1), from both sides
        got = ctx.entanglement(extra, lo, hi)
        assert (got["seg_writhe"][:, 1:-1] == 0).all() and (got["seg_writhe"][:, 0] != 0).all() and (got["seg_writhe"][:, -1] != 0).all()
    if name == "n257":                                                          # max_sep = S - 1 is what 0 stands for: the same bits
        assert ctx.entanglement(extra, 2, 255)["seg_writhe"].tobytes() == ctx.entanglement(extra, 2, 0)["seg_writhe"].tobytes()
    if name == "n4":                                                            # the one pair: segments 0 and 2
        got = ctx.entanglement(extra)
        assert (got["seg_writhe"][:, 1] == 0).all() and (got["writhe"] != 0).all()


@pytest.mark.parametrize("dom", list(BOUNDS257))
def test_domain_tables_equal_the_restatement(ctx, dom):
    extra, models = _load(ctx, "n257")
    b = BOUNDS257[dom]
    D = len(b) - 1
    for lo, hi in [(2, 0)] + ([(3, 10)] if dom == "D5" else []):
        got = ctx.entanglement(extra, lo, hi, b)
        host = _host("n257", models, lo, hi, b)
        assert got["link"].shape == got["link_abs"].shape == (7, D, D)
        _check(got, host, f"n257 {dom} sep {lo}..{hi}", table=True)
        for k in range(7):
            assert got["link"][k].tobytes() == got["link"][k].T.copy().tobytes() and got["link_abs"][k].tobytes() == got["link_abs"][k].T.copy().tobytes()
            gap = abs(got["link"][k].sum() - got["writhe"][k])
            assert gap <= _tol(host[k]["kappa"], got["writhe"][k]), (dom, k, gap)
            gap = abs(got["link_abs"][k].sum() - got["acn"][k])
            assert gap <= _tol(host[k]["kappa"], got["acn"][k]), (dom, k, gap)
        if dom == "D256":                                                       # every block one pair; a segment has no pair with itself or its neighbour
            assert (np.diagonal(got["link"], axis1=1, axis2=2) == 0).all() and (np.diagonal(got["link"], 1, axis1=1, axis2=2) == 0).all()
            # entry (p, q), p < q, is g(p, q) alone: row p of the table sums to what the row kernel gives within both sums' bounds
            for k in range(7):
                gap = np.abs(got["link"][k].sum(1) - got["seg_writhe"][k])
                assert (gap <= 2 * _tol(host[k]["seg_kappa"], got["seg_writhe"][k])).all()
        if dom == "D1":
            assert np.abs(got["link"][:, 0, 0] - got["writhe"]).max() <= _tol(max(h["kappa"] for h in host), got["writhe"]).max()
    # the table alone, and one table alone: the same bits
    from chromosome3d_amd import lib
    only = np.empty((7, D, D))
    bb = np.array(b, np.int32)
    assert ctx._L.c3d_entanglement(ctx._h, lib.dptr(extra), 2, 2, 0, lib.i32ptr(bb), D, None, None, None, None, None, lib.dptr(only), None) == 0
    assert only.tobytes() == ctx.entanglement(extra, 2, 0, b)["link_abs"].tobytes()


def test_identities_on_the_device(ctx):
    """Mirror, repeat, extra models, and the solve untouched."""
    extra, models = _load(ctx, "n257")
    ctx.run_steps(20)                                                           # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    b = BOUNDS257["D5"]
    mirrored = extra * np.array([1.0, -1.0, 1.0])
    both = np.concatenate([extra, mirrored])
    g1, g2 = ctx.entanglement(both, 2, 0, b), ctx.entanglement(both, 2, 0, b)
    for k in g1:
        if k != "device_ms":
            assert g1[k].tobytes() == g2[k].tobytes(), k
    for k in ("writhe", "seg_writhe", "link"):
        assert (g1[k][5:7] == -g1[k][7:9]).all() and (g1[k][5:7] != 0).any(), k
    for k in ("acn", "seg_acn", "link_abs"):
        assert g1[k][5:7].tobytes() == g1[k][7:9].tobytes(), k
    local = ctx.entanglement(both, 3, 10)
    assert (local["seg_writhe"][5:7] == -local["seg_writhe"][7:9]).all() and local["seg_acn"][5:7].tobytes() == local["seg_acn"][7:9].tobytes()
    alone = ctx.entanglement(None, 2, 0, b)                                     # without the extra models: the replicas keep their bits
    for k in alone:
        if k != "device_ms":
            assert alone[k].tobytes() == g1[k][:5].tobytes(), k
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for p, q in zip(before[:3], after[:3]):
        assert p.tobytes() == q.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    from chromosome3d_amd import lib
    only = np.empty(5)
    assert ctx._L.c3d_entanglement(ctx._h, None, 0, 2, 0, None, 0, None, lib.dptr(only), None, None, None, None, None) == 0     # one output alone
    assert only.tobytes() == alone["acn"].tobytes()
    assert ctx.run_steps(5) == 5                                                # and the solve goes on


def test_shapes_with_known_answers(ctx):
    n = 50
    restrained(ctx, n, 2)
    rings, b = E.two_rings(True)
    apart, _ = E.two_rings(False)
    helix = E.helix(n)
    shapes = np.stack([E.straight(n), E.spiral(n), helix, helix * np.array([-1.0, 1.0, 1.0]), rings, apart])
    got = ctx.entanglement(shapes, 2, 0, b)
    host = _host("n50", list(shapes), 2, 0, b)
    _check({k: v[2:] for k, v in got.items() if k != "device_ms"}, host, "n50 shapes", table=True)
    for k in (2, 3):                                                            # the straight chain and the planar spiral: exact zeros
        assert (got["seg_writhe"][k] == 0).all() and (got["seg_acn"][k] == 0).all() and got["writhe"][k] == 0 and got["acn"][k] == 0
        assert (got["link"][k] == 0).all() and (got["link_abs"][k] == 0).all()
    print(f"helix {got['writhe'][4]:.6f}, its mirror {got['writhe'][5]:.6f}; linked rings' block {got['link'][6, 0, 2]:.12f}, unlinked {got['link'][7, 0, 2]:.3e}")
    assert got["writhe"][4] > 1.0 and got["writhe"][5] == -got["writhe"][4] and got["acn"][5] == got["acn"][4]
    assert abs(abs(got["link"][6, 0, 2]) - 1.0) <= 1e-9 and abs(got["link"][7, 0, 2]) <= 1e-9
    assert (np.diagonal(got["link"][6])[[0, 2]] == 0).all()                     # a planar ring has no writhe


def test_the_report_lists_the_models_in_rank_order(ctx):
    from chromosome3d_amd import pipeline
    extra, models = _load(ctx, "k17")
    ctx.run_steps(10)                                                           # energies to rank by
    rep = pipeline.entanglement_report(ctx, None, 2, 0, [0, 20, 63])
    plain = ctx.entanglement(None, 2, 0, [0, 20, 63])
    for k in plain:
        if k != "device_ms":
            assert rep[k].tobytes() == plain[k].tobytes(), k
    assert list(rep["order"]) == [int(k) for k in ctx.rank()] and sorted(rep["order"]) == list(range(17))
    w = plain["writhe"]
    assert rep["writhe_mean"] == w.mean() and rep["writhe_sd"] == w.std() and np.array_equal(rep["acn_per_segment"], plain["acn"] / 63)
    assert rep["sign_agreement"] == np.mean(np.sign(w) == np.sign(w.mean())) and 0.0 < rep["sign_agreement"] <= 1.0
    rows = [l.split() for l in rep["text"].splitlines() if not l.startswith("#")]
    assert [int(r[0]) - 1 for r in rows] == list(rep["order"]) and all(abs(float(r[1]) - w[int(r[0]) - 1]) <= 5e-10 for r in rows)
    assert "17 models of 63 segments, separations 2..62" in rep["text"].splitlines()[0]


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
        got = s.entanglement()
        _check(got, [E.entanglement(m) for m in x], "f64")
        # rounding coordinates of 10 A to float moves them by up to 5e-7 A; 1e-9 is far above the bound on the device
        rounded = [E.entanglement(m) for m in x.astype(np.float32).astype(np.float64)]
        assert all(np.abs(got["seg_writhe"][k] - rounded[k]["seg_writhe"]).max() > 1e-9 for k in range(3))
    finally:
        s.close()


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    extra, models = _load(ctx, "n64")
    n, M, S = 64, 2, 63
    L, h = ctx._L, ctx._h
    state = ctx.coords().tobytes()
    w, a, sw, sa = np.full(300, 7.0), np.full(300, 7.0), np.full((300, S), 7.0), np.full((300, S), 7.0)
    lk, la = np.full((300, 4, 4), 7.0), np.full((300, 4, 4), 7.0)
    outs = (lib.dptr(w), lib.dptr(a), lib.dptr(sw), lib.dptr(sa))
    tabs = (lib.dptr(lk), lib.dptr(la))
    i32 = lambda v: lib.i32ptr(np.array(v, np.int32))
    good = np.stack(models)
    big = np.zeros((256 - M + 1, n, 3))                                         # one model more than C3D_COMPARE_MAX_MODELS allows
    ok = [0, 10, 20, 63]

    def refused(*args):
        assert L.c3d_entanglement(h, *args) == -1 and b"c3d_entanglement" in L.c3d_last_error(), args

    refused(None, 0, 2, 0, None, 0, None, None, None, None, None, None, None)   # every output NULL
    for lo, hi in ((1, 0), (0, 0), (-1, 0), (S, 0), (2, S), (2, -1), (5, 4), (S, S)):          # min_sep outside 2..S-1, max_sep outside min_sep..S-1
        refused(None, 0, lo, hi, None, 0, *outs, None, None, None)
    refused(None, 0, 2, 0, None, 3, *outs, *tabs, None)                         # a table without bounds
    refused(None, 0, 2, 0, None, 3, None, None, None, None, None, tabs[1], None)
    for D in (0, -1, 257):                                                      # n_domains outside 1..256
        refused(None, 0, 2, 0, i32(list(range(258))), D, *outs, *tabs, None)
    for bad in ([1, 10, 20, 63], [0, 10, 20, 62], [0, 10, 20, 64], [0, 20, 10, 63], [0, 10, 10, 63], [0, -1, 20, 63]):
        refused(None, 0, 2, 0, i32(bad), 3, *outs, *tabs, None)
    refused(None, 1, 2, 0, None, 0, *outs, None, None, None)                    # n_extra > 0 without coordinates
    refused(lib.dptr(good), -1, 2, 0, None, 0, *outs, None, None, None)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(lib.dptr(e), M, 2, 0, None, 0, *outs, None, None, None)
    refused(lib.dptr(big), len(big), 2, 0, None, 0, *outs, None, None, None)    # K = 257
    assert (w == 7.0).all() and (sw == 7.0).all() and (lk == 7.0).all() and ctx.coords().tobytes() == state
    # bounds are not looked at when no table is asked for; 256 models are accepted; the context works
    assert L.c3d_entanglement(h, None, 0, 2, 0, i32([5, 4]), 999, *outs, None, None, None) == 0
    got = ctx.entanglement(big[:-1] + good[0], 2, 0, ok)
    _check({k: v[[0, 255]] for k, v in got.items() if k != "device_ms"}, [_host("n64", models, 2, 0, ok)[0]] * 2, "n64 x 256 after the refusals", table=True)
    assert got["writhe"][0] == got["writhe"][255] and w[:M].tobytes() == got["writhe"][:M].tobytes()
    # no replicas; 3 beads
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(3, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_entanglement.*c3d_init_replicas"):
            s2.entanglement()
        s2.init_replicas(2)
        with pytest.raises(C3DError, match="c3d_entanglement.*fewer than 4 beads"):
            s2.entanglement()
    finally:
        s2.close()


def test_from_the_command_line(ctx, tmp_path):
    """c3d_solve --entanglement on the smallest bundled matrix: the three files, rows in rank order, and numbers that are Solver.entanglement's of
    the written models."""
    cid, M, n = "chr21_1mb", 4, 37
    exe = os.path.join(ROOT, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "ent")
    (tmp_path / "bounds.txt").write_text("0 12 13\n36\n")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", str(M), "--quiet", "--entanglement", prefix, "--entangle-bounds",
                          str(tmp_path / "bounds.txt")], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    rows = [l.split() for l in open(prefix + "_entanglement.txt") if not l.startswith("#")]
    assert len(rows) == M and [int(r[0]) for r in rows] == [1, 2, 3, 4] and sorted(int(r[1]) for r in rows) == [1, 2, 3, 4] and all(len(r) == 5 for r in rows)
    x = np.stack([load_pdb_xyz(tmp_path / "a" / f"{cid}_matrix_{r + 1}.pdb") for r in range(M)])
    restrained(ctx, n, M)
    ctx.set_coords(x)
    got = ctx.entanglement(None, 2, 0, [0, 12, 13, 36])
    # The files print 9 decimals of one call: their own sums agree at 1e-6.  The written coordinates are the run's rounded to 3 decimals: a bead
    # moves by up to sqrt(3) 5e-4 = 8.7e-4 A, a pair's four beads change g by at most about 4 x 8.7e-4 x L / (4 pi d^2) — 1.1e-5 for a
    # bond L = 4 A seen from d = 10 A — and 36 x 35 pairs of one sign would add up to 1.4e-2: the written models are held at 5e-2 (seen: 1.4e-4).
    seg = np.array([[float(v) for v in l.split()] for l in open(prefix + "_segments.txt") if not l.startswith("#")])
    link = np.array([[float(v) for v in l.split()] for l in open(prefix + "_link.txt") if not l.startswith("#")])
    assert seg.shape == (M * (n - 1), 4) and link.shape == (M * 6, 5)
    for r in rows:
        k = int(r[1])
        mine = seg[seg[:, 0] == k]
        assert np.array_equal(mine[:, 1], np.arange(1, n))
        assert abs(mine[:, 2].sum() - float(r[2])) <= 1e-6 and abs(mine[:, 3].sum() - float(r[3])) <= 1e-6 and abs(float(r[3]) / (n - 1) - float(r[4])) <= 1e-8
        t = link[link[:, 0] == k]
        assert abs(t[t[:, 1] == t[:, 2], 3].sum() + 2 * t[t[:, 1] != t[:, 2], 3].sum() - float(r[2])) <= 1e-6
        print(f"rank {r[0]} model {k}: writhe {r[2]} (of the written model {got['writhe'][k - 1]:.9f}), acn {r[3]} ({got['acn'][k - 1]:.9f})")
        assert abs(float(r[2]) - got["writhe"][k - 1]) <= 5e-2 and abs(float(r[3]) - got["acn"][k - 1]) <= 5e-2
    head = open(prefix + "_entanglement.txt").readline()
    assert "36 segments, separations 2..35" in head and "sign agreement" in head
    local = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "b"), "-m", str(M), "--quiet", "--entanglement", str(tmp_path / "loc"), "--entangle-sep", "3:10"],
                           capture_output=True, text=True)
    assert local.returncode == 0, local.stderr
    assert "separations 3..10" in open(tmp_path / "loc_entanglement.txt").readline() and not os.path.exists(tmp_path / "loc_link.txt")
    bad = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "c"), "-m", str(M), "--quiet", "--entanglement", str(tmp_path / "bad"), "--entangle-sep", "1:0"],
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "c3d_entanglement" in bad.stderr


@pytest.fixture(scope="module")
def ctx6000():
    from chromosome3d_amd import Solver
    n = 6000
    x = (random_coil(n, 60000) * np.float32(0.5))[None]
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        restrained(s, n, 1)
        s.set_coords(x)
        yield s, x[0].astype(np.float64)
    finally:
        s.close()


def test_6000_beads_sampled_rows_equal_the_restatement(ctx6000):
    """Beyond the default bead limit: 96 sampled rows (the first, the last, both sides of tile edges) against the restatement, and the totals
    against the sum of the device's own rows: two orders of the same S terms, each of which carries at least its own kappa >= 1 per pair."""
    s, x = ctx6000
    S = 5999
    got = s.entanglement()
    which = [0, 1, 63, 64, 65, 127, 128, 2999, 3000, 5951, 5952, S - 2, S - 1]
    for v in np.random.default_rng(6000).integers(0, S, 200):
        if len(which) < 96 and int(v) not in which:
            which.append(int(v))
    assert len(which) == 96
    w, a, kappa = E.rows(x, which=which)
    gw, ga = np.abs(got["seg_writhe"][0][which] - w), np.abs(got["seg_acn"][0][which] - a)
    tw, ta = _tol(kappa, w), _tol(kappa, a)
    print(f"n6000: writhe {got['writhe'][0]:.6f}, acn {got['acn'][0]:.6f}, {len(which)} rows, largest gap / bound {max((gw / tw).max(), (ga / ta).max()):.4f}, "
          f"device {got['device_ms']:.3f} ms")
    assert (gw <= tw).all() and (ga <= ta).all()
    terms = S * (S - 1) - 2 * (S - 1)                                           # ordered pairs |s - t| >= 2: every kappa is >= 1
    assert abs(got["writhe"][0] - got["seg_writhe"][0].sum()) <= _tol(terms, got["writhe"][0])
    assert abs(got["acn"][0] - got["seg_acn"][0].sum()) <= _tol(terms, got["acn"][0])
    assert got["acn"][0] > abs(got["writhe"][0]) > 0
