"""Loop enrichment on the device (c3d_loops; csrc/c3d_score_loop.inc k_loop_*) against the numpy restatement tests/loop_ref.py, which
tests/test_loop_ref.py holds to a direct loop and to planted inputs.

The kernels' constants: a workgroup of k_loop_scan owns a 32 x 32 tile of pixels, tile k of a tile row starting at column
i0 + min_sep - 31 + 32 k; the expected, closed and pile-up kernels walk rows or the list in steps of 256.
  small     n = 2w + min_sep + 1 (one inside pixel) and that plus one, for w = 1 and for w = 20 with p = 19 and p = 0
  tiles     n = 31, 32, 33, 65 with max_sep = n - 1 (s_hi clipped); bands of 31, 32, 33, 65 separations; B = 1 and B = 1024
  peaks     merge = 0 and merge = w; max_peaks = 0, found - 1 and 65536
  lists     1, 255, 256 and 257 pixels, some not inside; a pixel alone and in a longer list
  masks     none, one bin, a run of 2w + 1 bins, a peak's own anchor
  models    one to three rosettes with and without the consensus, as set or relaxed by a short schedule; fp64 state; extra models only
  large     16384 beads x 1 model, 257 listed pixels; IF dense at n = 4096, B = 64, w = 20, a sample held to the restatement

Bounds, u = 2^-53, c = (2w+1)^2.  expected, relative: (n + 2) u, (n + Kp + 2) u for the consensus.  ratio and at, relative:
S = (2c + 2(n + Kp + 2) + 4) u, the NaN pattern bit for bit.  apa, relative: (L + n + Kp + 4) u; p2ll: corner^2 + 2 more.  Candidates,
peaks, report and closed: the restatement's steps on the device's own ratio bytes, bit for bit; and the restatement's own wherever its
margins exceed 2 S, at most 1 % of the pixels left out.  Every check prints the largest observed fraction of its bound."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import loop_ref as R
from tests.util import SHORT, restrained

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
THR = (1.75, 1.75, 1.5, 1.5)


@pytest.fixture(scope="module")
def ctx():
    from chromosome3d_amd import Solver
    s = Solver(0)
    yield s
    s.close()


@functools.lru_cache(maxsize=None)
def _planted(name):
    n, planted = R.PLANTED_CASES[name][:2]
    return R.planted_map(n, planted)


@functools.lru_cache(maxsize=None)
def _rosette(n, r):
    return R.planted_rosette(n, 12, 100 + r).astype(np.float32)


def _state(ctx):
    return [m.astype(np.float64) for m in ctx.coords()]


def _set(ctx, n, nrep, relaxed=False):
    restrained(ctx, n, nrep)
    ctx.set_coords(np.stack([_rosette(n, r) for r in range(nrep)]))
    if relaxed:
        ctx.run()                                                               # the steps of SHORT: a model the solver left
    return _state(ctx)


def _maps(models, IF, pick, consensus):
    order = list(range(len(models))) if pick is None else list(pick)
    maps = ([("if", np.asarray(IF, dtype=np.float64))] if IF is not None else []) + [("model", models[k]) for k in order]
    if consensus:
        maps.append(("consensus", [models[k] for k in order]))
    return maps


def _rel(got, want, bound, what, worst, key):
    """got against want to a relative bound; the NaN and zero patterns bit for bit"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want) & (want != 0.0)
    assert (got[~np.isnan(want) & (want == 0.0)] == 0.0).all(), what
    if ok.any():
        frac = np.abs(got[ok] - want[ok]) / np.abs(want[ok]) / bound
        assert (frac <= 1.0).all(), (what, float(frac.max()))
        worst[key] = max(worst.get(key, 0.0), float(frac.max()))


def _check(got, maps, n, mask=None, p=2, w=5, lo=None, hi=None, thr=THR, min_obs=0.0, merge=2, corner=3, max_peaks=4096, what="", seps=None, step=1):
    """every output of a call against the restatement, to the bounds of the module's docstring; returns the largest fractions"""
    masked = np.zeros(n, dtype=bool) if mask is None else np.asarray(mask) != 0
    lo = 2 * w + 1 if lo is None else lo
    hi = n - 1 if hi is None else hi
    s_lo, s_hi = R.band_range(n, w, lo, hi)
    Q, c = len(maps), (2 * w + 1) ** 2
    has_if = maps[0][0] == "if"
    worst = {}
    assert got["expected"].shape == (Q, s_hi - s_lo + 1)
    E = np.stack([R.expected(k, src, n, masked, s_lo, s_hi) for k, src in maps])
    Kps = [len(src) if kind == "consensus" else 0 for kind, src in maps]
    for q in range(Q):
        _rel(got["expected"][q], E[q], (n + Kps[q] + 2) * U, f"{what} expected of map {q}", worst, "expected")
    if has_if:
        M = maps[0][1]
        S = (2 * c + 2 * (n + 2) + 4) * U
        vals = R.band_values(M, n, lo, hi)
        if "ratio" in got:
            ratio = got["ratio"]
            assert ratio.shape == (4, hi - lo + 1, n)
            want = R.scan(M, E[0], n, masked, p, w, lo, hi, seps, step)
            if seps is None and step == 1:
                _rel(ratio, want, S, f"{what} ratio", worst, "ratio")
            else:                                                               # a sample: the restatement has the other pixels as NaN
                held = np.zeros(ratio.shape, dtype=bool)
                for s in seps:
                    held[:, s - lo, np.arange(0, n - s, step)] = True
                _rel(ratio[held], want[held], S, f"{what} sampled ratio", worst, "ratio")
                for s in range(lo, hi + 1):                                     # and the NaN pattern of every pixel: not inside, or beyond the matrix
                    i = np.arange(n)
                    out = (i < w) | (i + s + w > n - 1)
                    assert np.isnan(ratio[:, s - lo, out]).all() and not np.isnan(ratio[:, s - lo, ~out]).any(), (what, s)
            # steps 6 on the device's own ratio bytes: bit for bit
            cand, peak, pk, report = R.call_peaks(ratio, vals, n, masked, w, lo, thr, min_obs, merge, max_peaks)
            assert np.array_equal(got["peaks"], pk), (what, got["peaks"][:8], pk[:8])
            assert [got["candidates"], got["found"], len(got["peaks"]), got["masked_pixels"]] == report.tolist(), (what, report)
            if seps is None and step == 1:                                      # and the restatement's own where its margins exceed 2 S
                rc, rp, rpk, rrep = R.call_peaks(want, vals, n, masked, w, lo, thr, min_obs, merge, max_peaks)
                sure = R.margins(want, vals, thr, min_obs) > 2 * S
                left = float((~sure).sum()) / sure.size
                assert left <= 0.01, (what, left)
                worst["left out"] = left
                assert np.array_equal(cand[sure], rc[sure]), what
                if left == 0.0:
                    assert np.array_equal(pk, rpk) and report.tolist() == rrep.tolist(), what
    if "at" in got:
        px = np.asarray(got["pixels"], dtype=np.int64).reshape(-1, 2)
        L = len(px)
        assert got["at"].shape == (Q, L, 6) and got["closed"].shape == (Q, 2) and got["apa"].shape == (Q, 2 * w + 1, 2 * w + 1) and got["p2ll"].shape == (Q,)
        for q, (kind, src) in enumerate(maps):
            S = (2 * c + 2 * (n + Kps[q] + 2) + 4) * U
            want = R.pixels(kind, src, E[q], n, masked, p, w, s_lo, px[:, 0], px[:, 1])
            at = got["at"][q]
            if L:
                if kind == "consensus":
                    _rel(at[:, 0], want[:, 0], (Kps[q] + 2) * U, f"{what} M of map {q}", worst, "at")
                else:
                    assert at[:, 0].tobytes() == want[:, 0].tobytes(), (what, q)       # an input value, or a distance with the host's bits
                assert at[:, 1].tobytes() == got["expected"][q][px[:, 1] - px[:, 0] - s_lo].tobytes(), (what, q)
                _rel(at[:, 2:], want[:, 2:], S, f"{what} at of map {q}", worst, "at")
                if q == 0 and has_if and "ratio" in got:
                    assert at[:, 2:].T.tobytes() == np.ascontiguousarray(got["ratio"][:, px[:, 1] - px[:, 0] - lo, px[:, 0]]).tobytes(), what
            assert np.array_equal(got["closed"][q], R.closed(at, has_if and q == 0)), (what, q)
            with np.errstate(invalid="ignore"):
                near = (np.abs(want[:, 2:4] - 1.0) <= 2 * S).any(axis=1)
            if not near.any():
                assert np.array_equal(got["closed"][q], R.closed(want, has_if and q == 0)), (what, q)
            A, ratio_ll = R.apa(kind, src, E[q], n, masked, w, s_lo, px[:, 0], px[:, 1], corner)
            _rel(got["apa"][q], A, (L + n + Kps[q] + 4) * U, f"{what} apa of map {q}", worst, "apa")
            _rel(got["p2ll"][q:q + 1], np.array([ratio_ll]), (L + n + Kps[q] + 4 + corner * corner + 2) * U, f"{what} p2ll of map {q}", worst, "p2ll")
    print(f"{what}: largest fraction of the bound — " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


def _if_call(ctx, name, **kw):
    n, planted, w, p, lo, hi, seps, step = R.PLANTED_CASES[name]
    if ctx.n != n or ctx.nrep != 1:
        restrained(ctx, n, 1)
    M = _planted(name)
    corner = kw.pop("corner", min(3, w))
    merge = kw.pop("merge", min(2, w))
    mask = kw.pop("mask", None)
    max_peaks = kw.pop("max_peaks", 4096)
    min_obs = kw.pop("min_obs", 0.0)
    got = ctx.loops(M, None, None, False, mask, p, w, lo, hi, THR, min_obs, merge, corner, None, max_peaks, True, False)
    assert got["maps"] == ["IF"] and got["device_ms"] > 0
    worst = _check(got, [("if", M)], n, mask, p, w, lo, hi, THR, min_obs, merge, corner, max_peaks, name, seps, step)
    return got, worst


SMALL = ["one pixel", "one pixel, clipped", "two pixels", "largest window, p = 19", "largest window, p = 0"]
TILES = ["n = 31", "n = 32", "n = 33", "n = 65", "B = 31", "B = 32", "B = 33", "B = 65", "B = 1024", "120", "80"]


@pytest.mark.parametrize("name", SMALL)
def test_small_sizes(ctx, name):
    got, _ = _if_call(ctx, name)
    n, _, w, p, lo, hi = R.PLANTED_CASES[name][:6]
    inside = sum(1 for s in range(lo, hi + 1) for i in range(w, n - s - w))
    assert int((~np.isnan(got["ratio"][0])).sum()) == inside and inside in (1, 2, 3)


@pytest.mark.parametrize("name", TILES)
def test_tile_and_band_borders(ctx, name):
    got, worst = _if_call(ctx, name)
    n, planted = R.PLANTED_CASES[name][:2]
    if name in ("120", "80"):
        assert got["peaks"].tolist() == [list(q) for q in planted] and got["closed"].tolist() == [[len(planted), len(planted)]]
        assert got["candidates"] == {"120": 27, "80": 16}[name] and got["p2ll"][0] > 2.0


def test_merge_and_max_peaks(ctx):
    name = "120"
    for merge in (0, 5):                                                        # no suppression: every candidate a peak; the widest: w
        got, _ = _if_call(ctx, name, merge=merge)
        assert got["found"] == (27 if merge == 0 else 3)
    full, _ = _if_call(ctx, name, merge=0, max_peaks=65536)
    assert len(full["peaks"]) == 27
    cut, _ = _if_call(ctx, name, merge=0, max_peaks=26)                         # found - 1: truncation keeps the order
    assert cut["found"] == 27 and np.array_equal(cut["peaks"], full["peaks"][:26]) and cut["at"].shape[1] == 26
    none, _ = _if_call(ctx, name, max_peaks=0)
    assert none["found"] == 3 and len(none["peaks"]) == 0 and none["at"].shape == (1, 0, 6)
    assert none["closed"].tolist() == [[0, 0]] and np.isnan(none["apa"]).all() and np.isnan(none["p2ll"]).all()


def test_min_obs_removes_candidates(ctx):
    """M(i,j) >= min_obs is part of the candidate rule: a value among the candidates' own removes those below it and keeps the one
    that equals it; the peaks change with the candidates.  An exact comparison of input values: no margin is involved."""
    name = "120"
    every, _ = _if_call(ctx, name, merge=0)                                     # every candidate a peak: their values are at[:, 0]
    values = np.sort(every["at"][0, :, 0])
    assert len(values) == 27
    cut = float(values[len(values) // 2])
    kept = int((values >= cut).sum())
    assert 0 < kept < 27
    got, _ = _if_call(ctx, name, merge=0, min_obs=cut)                          # held to call_peaks on the device's ratio bytes in _check
    assert got["candidates"] == kept and got["found"] == kept and (got["at"][0, :, 0] >= cut).all() and cut in got["at"][0, :, 0]
    above, _ = _if_call(ctx, name, min_obs=float(np.nextafter(values[-1], np.inf)))
    assert above["candidates"] == 0 and above["found"] == 0 and len(above["peaks"]) == 0
    merged, _ = _if_call(ctx, name, min_obs=cut)
    assert merged["candidates"] == kept and 0 < merged["found"] <= 3


def test_masks(ctx):
    name = "120"
    n, planted, w = R.PLANTED_CASES[name][:3]
    plain, _ = _if_call(ctx, name)
    for bins in ([45], list(range(56, 56 + 2 * w + 1)), [50]):                  # one bin; a run of 2w + 1; a peak's own anchor
        mask = np.zeros(n, np.int32)
        mask[bins] = 2
        got, _ = _if_call(ctx, name, mask=mask)
        assert got["masked_pixels"] > 0 and got["ratio"].tobytes() != plain["ratio"].tobytes(), bins
        assert np.isnan(got["ratio"][:, :, bins]).all()
        if bins == [50]:
            assert [50, 95] not in got["peaks"].tolist() and [30, 60] in got["peaks"].tolist()
    lone = np.ones(n, np.int32)
    lone[[30, 60]] = 0                                                          # nothing live around the pixel: SM = SE = 0, NaN
    got = ctx.loops(_planted(name), None, None, False, lone, 2, 5, 11, 50, THR, 0.0, 2, 3, [(30, 60)], 16, True, False)
    _check(got, [("if", _planted(name))], n, lone, 2, 5, 11, 50, what="a pixel without neighbours")
    assert np.isnan(got["at"][0, 0, 2:]).all() and got["at"][0, 0, 0] == _planted(name)[30, 60] and got["closed"].tolist() == [[0, 0]]


def _bases(n, w, lo, hi, count):
    """`count` pixels: the rosette's base pixels first, then pixels spread over the band, some of them not inside"""
    px = [(12 * m, 12 * m + 12 * k) for k in (1, 2) for m in range(1, n // 12 - k) if lo <= 12 * k <= hi]
    rng = np.random.default_rng(count)
    while len(px) < count:
        s = int(rng.integers(lo, hi + 1))
        px.append((int(rng.integers(0, n - s)), 0))
        px[-1] = (px[-1][0], px[-1][0] + s)
    if count >= 40:
        px[count - 1] = (0, lo)                                                 # not inside
    return np.array(px[:count], np.int32)


@pytest.mark.parametrize("n,nrep,relaxed,consensus,w,p,count", [(96, 1, False, False, 3, 1, 1), (96, 2, False, True, 3, 1, 255), (131, 3, True, True, 5, 2, 256),
                                                                 (257, 3, False, False, 2, 0, 257), (455, 2, True, True, 20, 7, 40)])
def test_models_lists_and_the_pile_up(ctx, n, nrep, relaxed, consensus, w, p, count):
    models = _set(ctx, n, nrep, relaxed)
    lo, hi = 2 * w + 1, min(n - 1, 2 * w + 64)
    px = _bases(n, w, lo, hi, count)
    corner = min(3, w)
    got = ctx.loops(None, None, None, consensus, None, p, w, lo, hi, THR, 0.0, 2, corner, px)
    assert got["maps"] == ["model %d" % k for k in range(nrep)] + (["consensus"] if consensus else []) and "peaks" not in got
    _check(got, _maps(models, None, None, consensus), n, None, p, w, lo, hi, corner=corner, what=f"n = {n} x {nrep}{' relaxed' if relaxed else ''} list of {count}")
    if not relaxed and w == 3 and count >= 5:                                   # the bases of the rosette are closed
        base = [l for l, (i, j) in enumerate(px) if j - i == 12 and i % 12 == 0]
        assert len(base) and (got["at"][:, base, 2:4] < 0.5).all()
    one = ctx.loops(None, None, None, consensus, None, p, w, lo, hi, THR, 0.0, 2, corner, px[count // 2:count // 2 + 1])      # a pixel alone: its bytes in the list
    assert one["at"][:, 0].tobytes() == got["at"][:, count // 2].tobytes()
    assert (~((px[:, 0] >= w) & (px[:, 1] + w <= n - 1))).any() or count < 40   # the longer lists hold pixels that are not inside
    assert np.isnan(got["at"][:, ~((px[:, 0] >= w) & (px[:, 1] + w <= n - 1)), 2:]).all()


def test_if_models_consensus_picks_and_extra_models(ctx):
    """IF, three replicas and two extra models, a pick list with a repeat, the consensus; then the extra models only; the report"""
    name = "120"
    n, planted, w, p, lo, hi = R.PLANTED_CASES[name][:6]
    state = _set(ctx, n, 3)
    extra = np.stack([R.planted_rosette(n, 12, 200 + r) + 0.25 for r in (5, 7)])
    models = state + list(extra)
    pick = [4, 0, 0, 3, 2]
    IF = _planted(name)
    got = ctx.loops(IF, extra, pick, True, None, p, w, lo, hi, want_ratio=True)
    assert got["maps"] == ["IF"] + ["model %d" % k for k in pick] + ["consensus"]
    _check(got, _maps(models, IF, pick, True), n, None, p, w, lo, hi, what="IF, picks, extra models, consensus")
    assert got["at"][2].tobytes() == got["at"][3].tobytes() and got["apa"][2].tobytes() == got["apa"][3].tobytes()       # the repeated pick
    only = ctx.loops(None, extra, [3, 4], False, None, p, w, lo, hi, pixels=got["peaks"])
    _check(only, _maps(models, None, [3, 4], False), n, None, p, w, lo, hi, what="extra models only")
    assert only["at"][0].tobytes() == got["at"][4].tobytes() and only["at"][1].tobytes() == got["at"][1].tobytes()       # alone or among others
    from chromosome3d_amd import pipeline
    rep = pipeline.loop_report(ctx, IF, extra, pick, p=p, w=w, min_sep=lo, max_sep=hi)
    assert rep["at"].tobytes() == got["at"].tobytes() and rep["text"].count("\n") == 1 + 3 + 1 + 7 and rep["text"].splitlines()[1].startswith("31 61 ")


def test_f64_state_is_read_in_doubles():
    """A precision-64 context whose state no float holds: coordinates near 9000 A, where a float's last place is 1e-3 A"""
    from chromosome3d_amd import Solver
    s = Solver(0)
    try:
        s.set_option("precision", 64)
        n, w, p = 96, 3, 1
        restrained(s, n, 2)
        rng = np.random.default_rng(96)
        x = np.stack([_rosette(n, r).astype(np.float64) + 9000.0 for r in range(2)]) + rng.normal(scale=1e-3, size=(2, n, 3))
        s.set_coords64(x)
        assert np.array_equal(s.coords64(), x) and not np.array_equal(x, x.astype(np.float32).astype(np.float64))
        px = _bases(n, w, 7, 30, 9)
        got = s.loops(None, None, None, True, None, p, w, 7, 30, pixels=px)
        _check(got, _maps(list(x), None, None, True), n, None, p, w, 7, 30, what="fp64 state")
        rounded = R.cells("model", x[0].astype(np.float32).astype(np.float64), px[:, 0], px[:, 1])
        assert (got["at"][0, :, 0] != rounded).any()
    finally:
        s.close()


def test_two_calls_same_bytes_and_the_solve_goes_on(ctx):
    name = "120"
    n, planted, w, p, lo, hi = R.PLANTED_CASES[name][:6]
    _set(ctx, n, 3)
    assert ctx.run_steps(20) == 20 and ctx.run_steps(15) == 15                  # an uninterrupted run
    plain = (ctx.coords().tobytes(), ctx.velocities().tobytes())
    _set(ctx, n, 3)
    assert ctx.run_steps(20) == 20                                              # velocities and parity of a solve under way
    before = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    IF = _planted(name)
    a, b = (ctx.loops(IF, None, None, True, None, p, w, lo, hi, want_ratio=True) for _ in range(2))
    for k in ("expected", "ratio", "peaks", "at", "closed", "apa", "p2ll"):
        assert a[k].tobytes() == b[k].tobytes(), k
    _check(a, _maps(_state(ctx), IF, None, True), n, None, p, w, lo, hi, what="mid-solve")
    alone = ctx.loops(None, None, [2], False, None, p, w, lo, hi, pixels=a["peaks"])         # model 2 alone: the bytes it had among IF, three and the consensus
    for k in ("expected", "at", "closed", "apa", "p2ll"):
        assert alone[k][0].tobytes() == a[k][3].tobytes(), k
    after = (ctx.coords(), ctx.velocities(), ctx.energies(), ctx.steps_done, ctx.step_kernel_name)
    for x, y in zip(before[:3], after[:3]):
        assert x.tobytes() == y.tobytes()
    assert before[3:] == after[3:] and before[4] != ""
    assert ctx.run_steps(15) == 15                                              # and the solve goes on, to the bits of the uninterrupted run
    assert (ctx.coords().tobytes(), ctx.velocities().tobytes()) == plain


def test_refusals_leave_the_context_working(ctx):
    """Every case of c3d.h's error list is C3D_ERR_INVALID with the function's name and writes nothing; the context works afterwards."""
    from chromosome3d_amd import C3DError, Solver, default_model, lib, make_stages
    n, M = 80, 2
    models = _set(ctx, n, M)
    L, h = ctx._L, ctx._h
    state = ctx.coords().tobytes()
    good = np.stack(models)
    IF = _planted("80")
    big = np.zeros((256 - M + 1, n, 3))
    thr0 = np.array(THR)

    def refused(IF=None, extra=None, n_extra=0, pick=None, n_pick=0, flags=0, mask=None, p=1, w=3, lo=7, hi=30, thr=thr0, min_obs=0.0, merge=2, corner=3,
                pixels=None, n_list=None, max_peaks=8, outs="ea", word=b""):
        buf = {k: np.full(4 * 24 * n + 300 * 64, 7.0) for k in "eraAP"}
        ibuf = {k: np.full(600, 7, np.int32) for k in "pRc"}
        ms = C.c_double(7.0)
        px = np.array(pixels, np.int32).reshape(-1) if pixels is not None else None
        d = lambda k: lib.dptr(buf[k]) if k in outs else None
        i = lambda k: lib.i32ptr(ibuf[k]) if k in outs else None
        rc = L.c3d_loops(h, lib.dptr(IF) if IF is not None else None, lib.dptr(extra) if extra is not None else None, n_extra,
                         lib.i32ptr(pick) if pick is not None else None, n_pick, flags, lib.i32ptr(mask) if mask is not None else None, p, w, lo, hi,
                         lib.dptr(thr) if thr is not None else None, min_obs, merge, corner, lib.i32ptr(px) if px is not None else None,
                         (len(px) // 2 if px is not None else 0) if n_list is None else n_list, max_peaks, d("e"), d("r"), i("p"), i("R"), d("a"), i("c"), d("A"), d("P"),
                         C.byref(ms))
        assert rc == -1 and b"c3d_loops" in L.c3d_last_error() and word in L.c3d_last_error(), (L.c3d_last_error(), word)
        assert all((v == 7.0).all() for v in buf.values()) and all((v == 7).all() for v in ibuf.values()) and ms.value == 7.0      # nothing written

    listed = [(20, 40)]
    for kw, word in ((dict(w=0), b"w outside"), (dict(w=21, lo=43, hi=50), b"w outside"), (dict(p=3), b"p outside"), (dict(p=-1), b"p outside"), (dict(lo=6), b"min_sep"),
                     (dict(hi=80), b"max_sep"), (dict(lo=20, hi=19), b"max_sep"), (dict(merge=-1), b"merge"), (dict(merge=4), b"merge"), (dict(corner=0), b"corner"),
                     (dict(corner=4), b"corner"), (dict(min_obs=-1.0), b"min_obs"), (dict(min_obs=np.nan), b"min_obs"), (dict(min_obs=np.inf), b"min_obs"),
                     (dict(max_peaks=-1), b"max_peaks"), (dict(max_peaks=65537), b"max_peaks"), (dict(flags=4), b"flag"), (dict(flags=-1), b"flag")):
        refused(pixels=listed, **kw, word=word)
    restrained(ctx, 1100, 1)                                                    # B = 1025 needs a longer chain
    h = ctx._h
    refused(pixels=[(20, 40)], w=1, p=0, lo=3, hi=1027, corner=1, merge=1, word=b"C3D_LOOP_MAX_BAND")
    models = _set(ctx, n, M)
    h = ctx._h
    state = ctx.coords().tobytes()
    for bad in ([(40, 20)], [(20, 20)], [(20, 26)], [(20, 51)], [(60, 80)], [(-1, 20)]):          # i < j, the separation, j <= n - 1
        refused(pixels=bad, word=b"list entry")
    refused(pixels=listed, n_list=-1, word=b"n_list")
    refused(pixels=listed, n_list=65537, word=b"n_list")
    refused(n_list=1, outs="e", word=b"n_list")
    refused(outs="", pixels=listed, word=b"NULL")
    for outs in ("r", "p", "R"):                                                # ratio, peaks and report without IF
        refused(outs=outs, pixels=listed, word=b"IF")
    for outs in ("a", "c", "A", "P"):                                           # a list that is empty by construction
        refused(outs=outs, word=b"list")
    refused(IF=IF, outs="p", thr=None, word=b"thr")                            # peaks without thresholds
    refused(IF=IF, outs="a", thr=None, word=b"thr")                            # the list taken from the peaks
    for bad in (0.0, -1.0, np.nan, np.inf):
        t = thr0.copy()
        t[2] = bad
        refused(IF=IF, outs="R", thr=t, word=b"threshold")
    refused(flags=2, outs="e", word=b"IF_ONLY")                                 # neither IF nor a model
    refused(IF=IF, flags=3, outs="e", word=b"IF_ONLY")                          # the consensus of no model
    one = np.array([0, 1], np.int32)
    refused(IF=IF, flags=2, pick=one, n_pick=2, outs="e", word=b"IF_ONLY")
    refused(pick=one, n_pick=0, pixels=listed)                                  # a list without a length, a length without a list
    refused(n_pick=2, pixels=listed)
    refused(pick=one, n_pick=-1, pixels=listed)
    refused(pick=np.array([0, 2], np.int32), n_pick=2, pixels=listed, word=b"pick")               # K = 2: index 2 is outside
    refused(pick=np.zeros(257, np.int32), n_pick=257, pixels=listed, word=b"256")
    refused(n_extra=1, pixels=listed)                                           # extra models without coordinates
    refused(extra=good, n_extra=-1, pixels=listed)
    for bad in (np.nan, np.inf, 1e6):                                           # what check_model_coords refuses
        e = good.copy()
        e[M - 1, n - 1, 2] = bad
        refused(extra=e, n_extra=M, pixels=listed)
    refused(extra=big, n_extra=len(big), pixels=listed)                         # K = 257
    for at, bad, word in (((3, 9), np.nan, b"finite"), ((3, 9), np.inf, b"finite"), ((3, 9), -1.0, b"negative"), ((9, 3), 5.0, b"symmetric")):
        m = IF.copy()
        m[at] = bad
        if bad < 0:
            m[at[::-1]] = bad
        refused(IF=m, outs="erpRacAP", word=word)                               # found while the host packs the band
    m = IF.copy()
    m[3, 3], m[30, 30 + 37], m[67, 30] = np.nan, -1.0, np.inf                 # the diagonal and a separation beyond s_hi = 36: not read, accepted
    ok = ctx.loops(m, None, None, True, None, 1, 3, 7, 30, want_ratio=True)
    assert ctx.coords().tobytes() == state
    got = ctx.loops(IF, None, None, True, None, 1, 3, 7, 30, want_ratio=True)   # and the context works
    _check(got, _maps(models, IF, None, True), n, None, 1, 3, 7, 30, what="after the refusals")
    assert all(ok[k].tobytes() == got[k].tobytes() for k in ("ratio", "peaks", "at", "apa"))
    s2 = Solver(0)
    try:
        s2.set_model(default_model())
        s2.set_schedule(make_stages(SHORT))
        s2.set_restraints(40, np.array([1], np.int32), np.array([2], np.int32), np.array([38], np.int32))
        with pytest.raises(C3DError, match="c3d_loops.*c3d_init_replicas"):
            s2.loops(pixels=[(5, 20)])
    finally:
        s2.close()


def test_from_the_command_line(tmp_path):
    """c3d_solve --loops on the smallest bundled matrix: the table's peaks are those of Solver.loops on the same IF, whatever the models"""
    import os
    import subprocess
    from chromosome3d_amd import Solver
    from tests.util import GOLD, load_if
    cid, n = "chr21_1mb", 37
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "chromosome3d_amd", "_lib", "c3d_solve")
    matrix = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    prefix = str(tmp_path / "lp")
    run = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "a"), "-m", "2", "--quiet", "--loops", prefix, "--loop-window", "3", "--loop-peak", "1",
                          "--loop-sep", "7:20", "--loop-thr", "1.05,1.05,1.02,1.02"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = open(prefix + "_loops.txt").read().splitlines()
    rows = [l.split() for l in lines if not l.startswith("#")]
    s = Solver(0)
    try:
        restrained(s, n, 1)
        got = s.loops(load_if(cid), None, None, False, None, 1, 3, 7, 20, (1.05, 1.05, 1.02, 1.02), models=False)
    finally:
        s.close()
    assert [[int(r[0]) - 1, int(r[1]) - 1] for r in rows] == got["peaks"].tolist() and all(len(r) == 11 for r in rows)
    for r, at in zip(rows, got["at"][0]):
        assert abs(float(r[3]) - at[2]) <= 5.000001e-5 and abs(float(r[4]) - at[3]) <= 5.000001e-5 and 0 <= int(r[10]) <= 2
    tail = [l for l in lines if l.startswith("# IF ") or l.startswith("# model ") or l.startswith("# consensus ")]
    assert len(tail) == 4 and tail[0].split()[2:4] == [str(got["closed"][0, 0]), str(got["closed"][0, 1])]
    bad = subprocess.run([exe, "--if", matrix, "--out", str(tmp_path / "c"), "-m", "2", "--quiet", "--loops", str(tmp_path / "x"), "--loop-window", "30"],
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "c3d_loops" in bad.stderr
    # --loop-list: pixels of the caller's, `#` and blank lines skipped, further columns ignored: a table of the tool's own can be fed back
    pairs = [(5, 14), (10, 25), (1, 9), (20, 37)]                               # beads from 1; the last two are not inside
    listing = tmp_path / "list.txt"
    listing.write_text("# i j and a comment\n\n" + "".join(f"{i} {j} 0.5 extra\n" if k == 1 else f"  {i}\t{j}\n" for k, (i, j) in enumerate(pairs)))
    args = [exe, "--if", matrix, "--out", str(tmp_path / "d"), "-m", "2", "--quiet", "--loop-window", "3", "--loop-peak", "1", "--loop-sep", "7:20"]
    run = subprocess.run(args + ["--loops", str(tmp_path / "ll"), "--loop-list", str(listing)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lrows = [l.split() for l in open(str(tmp_path / "ll") + "_loops.txt").read().splitlines() if not l.startswith("#")]
    assert [(int(r[0]), int(r[1])) for r in lrows] == pairs and all(len(r) == 11 for r in lrows)
    s = Solver(0)
    try:
        restrained(s, n, 1)
        want = s.loops(load_if(cid), None, None, False, None, 1, 3, 7, 20, pixels=[(i - 1, j - 1) for i, j in pairs], models=False)
    finally:
        s.close()
    for r, at in zip(lrows, want["at"][0]):
        assert all(np.isnan(float(r[3 + x])) if np.isnan(at[2 + x]) else abs(float(r[3 + x]) - at[2 + x]) <= 5.000001e-5 for x in range(4))
    assert np.isnan(want["at"][0, 2:, 2:]).all() and all(r[3] == "nan" or r[3] == "-nan" for r in lrows[2:])
    again = subprocess.run(args + ["--loops", str(tmp_path / "l2"), "--loop-list", str(tmp_path / "ll") + "_loops.txt"], capture_output=True, text=True)
    assert again.returncode == 0, again.stderr                                  # its own table, header lines and all
    assert [l.split()[:2] for l in open(str(tmp_path / "l2") + "_loops.txt").read().splitlines() if not l.startswith("#")] == [r[:2] for r in lrows]
    for text, word in (("", "holds no pair"), ("# only a header\n\n", "holds no pair"), ("3 12\nthree twelve\n", "line 2"), ("3 12x\n", "line 1"), ("3\n", "line 1")):
        listing.write_text(text)
        bad = subprocess.run(args + ["--loops", str(tmp_path / "bad"), "--loop-list", str(listing)], capture_output=True, text=True)
        assert bad.returncode != 0 and word in bad.stderr and not os.path.exists(str(tmp_path / "bad") + "_loops.txt"), (text, bad.stderr)
    bad = subprocess.run(args + ["--loops", str(tmp_path / "bad"), "--loop-list", str(tmp_path / "nowhere.txt")], capture_output=True, text=True)
    assert bad.returncode != 0 and "cannot read" in bad.stderr


def test_the_dense_scan_at_4096_beads():
    """IF dense at n = 4096, B = 64, w = 20 on planted_map: 130 x 4 tiles, the largest window; every 97th pixel of every 7th separation is
    held to the restatement, the peaks to the restatement's steps on the device's own ratio bytes"""
    from chromosome3d_amd import Solver
    name = "4096"
    n, planted, w, p, lo, hi, seps, step = R.PLANTED_CASES[name]
    s = Solver(0)
    try:
        restrained(s, n, 1)
        M = _planted(name)
        got = s.loops(M, None, None, False, None, p, w, lo, hi, THR, 0.0, 2, 3, None, 4096, True, False)
        _check(got, [("if", M)], n, None, p, w, lo, hi, what="n = 4096 dense", seps=seps, step=step)
        assert all(list(q) in got["peaks"].tolist() for q in planted), got["peaks"][:8]
        print(f"n = 4096 dense: {got['candidates']} candidates, device {got['device_ms']:.1f} ms")
    finally:
        s.close()


def test_the_index_arithmetic_at_16384_beads():
    """16384 beads x 1 model: the list pass and the pile-up on 257 pixels spread over the chain and the band ends"""
    from chromosome3d_amd import Solver, default_model, make_stages
    n, w, p, lo, hi = 16384, 20, 5, 41, 104
    s = Solver(0)
    try:
        s.set_option("max_beads", n)
        s.set_model(default_model())
        s.set_schedule(make_stages(SHORT))
        s.set_restraints(n, np.array([1, 1, 8001], np.int32), np.array([11, 16384, 16384], np.int32), np.array([100, 457, 300], np.int32))
        s.init_replicas(1, 82364, 0)
        s.set_coords(R.planted_rosette(n, 48, 3).astype(np.float32)[None])
        x = s.coords()[0].astype(np.float64)
        rows = np.linspace(0, n - 1 - hi, 129).astype(np.int64)
        px = np.array([(i, i + lo) for i in rows[:128]] + [(i, i + hi) for i in rows], np.int32)       # 257 pixels, the first and the last rows not inside
        got = s.loops(None, None, None, False, None, p, w, lo, hi, pixels=px)
        _check(got, [("model", x)], n, None, p, w, lo, hi, what="n = 16384")
        print(f"n = 16384: device {got['device_ms']:.1f} ms")
    finally:
        s.close()
