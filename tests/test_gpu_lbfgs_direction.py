"""The serial section of the L-BFGS move as a table: c3d_debug_lbfgs_direction runs c3d_lbfgs_serial.inc — the text k_lbfgs_move and
k64_lbfgs_move run between their barriers — a thread a row, on an fp32 and on a precision-64 context.  Expected values: a numpy float64
restatement (lbfgs_ref.direction_row_ref: the header comment of c3d_lbfgs.h and compact_direction, np.linalg.solve for the two
triangular systems), which tests/test_lbfgs_cases.py holds to compact_direction on real vectors.

Rows: every ring state (mem, head, cnt) with a kept and with a rejected pair, the first step for every memory, the pair test at its
edge, gamma at both clamps, F.d zero / negative / NaN, states out of range.  Integer state, slot mask and slot are exact everywhere.
gamma and the coefficients: fp32 within 4 float ulps of the row's largest coefficient (one rounding to float after fp64 arithmetic on a
system of condition number <= 100); fp64 within 8 x the gap measured on an MI355X (F64_MEASURED, profiles/r27_lbfgs_controller.md),
under a cap of 1e-10 relative to the largest coefficient.  The state's gamma is a double in both precisions: one division, 4 double ulps."""
import numpy as np
import pytest

from tests import controller_ref as R
from tests import lbfgs_ref as L

pytestmark = pytest.mark.gpu

M, Q = L.MAX_PAIRS, L.NSUMS
NAN = float("nan")
# the largest |coefficient gap| / largest |coefficient| of a row over the ring-state rows on a precision-64 context, measured on an MI355X
F64_MEASURED = 5.411e-16
F64_CAP = 1e-10


@pytest.fixture(scope="module", params=[32, 64])
def ctx(request):
    """a context of its own in the precision, model and FIRE values off default (mass 37, dt_start 0.006: the first step's gamma)"""
    from chromosome3d_amd import Solver, default_fire, default_model, make_stages
    from tests.util import load_if
    s = Solver(0)
    if request.param == 64:
        s.set_option("f64_lbfgs", 1)
        s.set_option("precision", 64)
    s.set_model(default_model(**R.TABLE_MODEL))
    s.set_if_matrix(load_if("chr21_1mb"))
    s.set_schedule(make_stages([(8, 4, 0.0, 1.0, 1.0, 0.85, 0.0)]), default_fire(**R.TABLE_FIRE))
    s.precision = request.param
    yield s
    s.close()


def first_gamma(precision):
    """gamma of a first step in float64 from the float values the context holds (the fp32 kernels form it in float arithmetic: 4 ulps)"""
    dt = float(np.float32(R.TABLE_FIRE["dt_start"]))
    return dt * dt * (418.4 / float(np.float32(R.TABLE_MODEL["mass"])))


class Rows:
    """rows of the table and what to assert of each: "all" (integers exact, gamma and coefficients within the bound), "int" (integer state,
    mask and slot only)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.sums, self.si, self.sd, self.first, self.mem0, self.check = [], [], [], [], [], []

    def state(self, gamma=None):
        """a full 8 x 8 state in which every subset of slots in every age order is well conditioned: S'Y diagonal 1 .. 2, everything else
        within 0.1 and different in every slot — a read of a slot outside the held pairs, of the wrong triangle or of a stale column shows"""
        g = self.rng
        SY = g.uniform(-0.1, 0.1, (M, M)) + np.diag(g.uniform(1.0, 2.0, M))
        B = g.uniform(-0.1, 0.1, (M, M))
        YY = 0.5 * (B + B.T) + np.diag(g.uniform(1.0, 2.0, M))
        return np.concatenate([[g.uniform(0.5, 2.0) if gamma is None else gamma], SY.reshape(-1), YY.reshape(-1)])

    def some_sums(self, nx, kept=True):
        g = self.rng
        s = np.zeros(Q)
        for j in range(M):
            s[4 * j:4 * j + 4] = g.uniform(-1, 1), g.uniform(-1, 1), g.uniform(-0.1, 0.1), g.uniform(-0.1, 0.1)
        s[4 * nx + 2] = g.uniform(1.0, 2.0) * (1 if kept else -1)
        s[4 * nx + 3] = g.uniform(1.0, 2.0)
        s[Q - 4], s[Q - 3] = g.uniform(1.0, 2.0), g.uniform(50.0, 100.0)       # s.s; F.F large: F.d > 0 with a margin
        return s

    def add(self, sums, si, sd, first=0, mem0=5, check="all"):
        self.sums.append(np.array(sums, dtype=np.float64)); self.si.append(tuple(si)); self.sd.append(np.array(sd, dtype=np.float64))
        self.first.append(first); self.mem0.append(mem0); self.check.append(check)

    def __len__(self):
        return len(self.check)


def ring_rows():
    """the 240 ring states, each with a kept and with a rejected pair"""
    t = Rows(27)
    for mem in range(1, M + 1):
        for head in range(mem):
            for cnt in range(mem + 1):
                for kept in (True, False):
                    t.add(t.some_sums((head + 1) % mem, kept), (cnt, head, mem, 3), t.state())
    assert len(t) == 480
    return t


def edge_rows():
    t = Rows(28)
    # the first step, mem0 1 .. 8 (the state is not read: out of range on purpose)
    for mem0 in range(1, M + 1):
        t.add(t.some_sums(0), (9, -3, 11, 7), t.state(), first=1, mem0=mem0)
    # the pair test at its edge: mem 1, no pair held, F.s = 0 (F.d = gamma F.F > 0 whatever the pair); s.s y.y = 4 has an exact root
    thr = 1e-12 * 2.0
    for sy, yy in ((thr, 1.0), (float(np.nextafter(thr, 1.0)), 1.0), (0.0, 1.0), (-0.0, 1.0), (-1.5, 1.0), (NAN, 1.0), (0.0, 0.0)):
        s = t.some_sums(0)
        s[0], s[2], s[3], s[Q - 4] = 0.0, sy, yy, 4.0
        t.add(s, (0, 0, 1, 0), t.state(), check="int")
    # gamma at both clamps: a kept pair with s.y / y.y just inside and just outside each bound (one pair: nothing else is in the row)
    for bound in (1e-7, 1e2):
        for f in (1.0 - 1e-6, 1.0 + 1e-6):
            s = t.some_sums(0)
            s[2], s[3] = 1.0, 1.0 / (bound * f)
            s[Q - 3] = 1e6 / bound                                                # F.F: gamma F.F dominates F.d
            t.add(s, (0, 0, 1, 0), t.state())
    # a rejection doubles gamma out of the upper bound, and below the lower one it is raised
    for g_in in (30.0, 60.0, 100.0, 2e-8):
        t.add(t.some_sums(1, kept=False), (2, 0, 3, 0), t.state(gamma=g_in))
    # F.d: F = 0 makes it exactly 0; a stored S'Y with a negative diagonal makes the form indefinite (negative with a margin); F.F = NaN
    for what in ("zero", "negative", "nan", "reject+drop"):
        s = t.some_sums(2, kept=what != "reject+drop")
        sd = t.state()
        if what == "zero":
            s[0:4 * M:4] = 0.0; s[1:4 * M:4] = 0.0; s[Q - 3] = 0.0
        elif what == "negative":
            sd[1 + 1 * M + 1] = -10.0                 # S'Y[1][1] (slot 1 is held: cnt 2, head 1 -> slots 0, 1, then 2): D + gamma Y'Y < 0 there
            s[4] = 100.0; s[Q - 3] = 1.0              # F.s_1 large: its term (F.s_1)^2 (D_11 + gamma Y'Y_11) / D_11^2 = -850 decides F.d
        elif what == "nan":
            s[Q - 3] = NAN
        else:
            s[Q - 3] = -1.0                                                       # (no force has F.F < 0: the table can ask)
        t.add(s, (2, 1, 3, 5), sd, check="int" if what == "nan" else "all")
    # state out of range: mem 0 and 9, head -1 and mem, cnt -1 and mem + 1, with a rejected and with a kept pair
    for si in ((2, 1, 0, 0), (2, 1, 9, 0), (2, -1, 4, 0), (2, 4, 4, 0), (-1, 1, 4, 0), (5, 1, 4, 0)):
        mem = min(max(si[2], 1), M)
        nx = (min(max(si[1], 0), mem - 1) + 1) % mem
        for kept in (False, True):
            t.add(t.some_sums(nx, kept), si, t.state())
    return t


def run_table(ctx, t):
    """(device outputs, reference outputs per row)"""
    si, sd, coef, ms = ctx.debug_lbfgs_direction(np.array(t.sums), np.array(t.si, dtype=np.int32), np.array(t.sd), np.array(t.first, dtype=np.int32),
                                                 np.array(t.mem0, dtype=np.int32))
    ref = [L.direction_row_ref(t.sums[r], t.si[r], t.sd[r], t.first[r], t.mem0[r], first_gamma(ctx.precision)) for r in range(len(t))]
    return (si, sd, coef, ms), ref


def check_rows(ctx, t, label):
    (si, sd, coef, ms), ref = run_table(ctx, t)
    worst = 0.0
    for r in range(len(t)):
        rsi, rsd, rcoef, rmask, rslot, rfd = ref[r]
        row = (label, r, t.si[r], t.first[r], t.mem0[r])
        assert tuple(int(a) for a in si[r]) == rsi, (row, si[r], rsi)
        assert (int(ms[r][0]), int(ms[r][1])) == (rmask, rslot), (row, ms[r], rmask, rslot)
        if t.check[r] == "int":
            continue
        # S'Y and Y'Y are copies of sums: exact; the state's gamma is one fp64 division (or a product by 2, or a bound: exact)
        assert np.array_equal(sd[r][1:], rsd[1:]), (row, np.flatnonzero(sd[r][1:] != rsd[1:]))
        grain = np.spacing(np.float32(rsd[0])) if t.first[r] and ctx.precision == 32 else np.spacing(abs(rsd[0]))    # (fp32: formed in floats)
        assert abs(sd[r][0] - rsd[0]) <= 4.0 * float(grain), (row, sd[r][0], rsd[0])
        big = float(np.abs(rcoef).max())
        gap = float(np.abs(coef[r] - rcoef).max())
        worst = max(worst, gap / big)
        if ctx.precision == 32:
            tol = 4.0 * float(np.spacing(np.float32(big)))
            assert np.array_equal(coef[r], coef[r].astype(np.float32).astype(np.float64)), row      # floats, widened
        else:
            tol = big * (F64_CAP if F64_MEASURED is None else min(F64_CAP, 8.0 * F64_MEASURED))
        assert gap <= tol, (row, gap, tol, coef[r], rcoef)
        assert np.all(coef[r][rcoef == 0.0] == 0.0), (row, coef[r], rcoef)         # a slot outside the direction: exactly 0
    print(f"TABLE {label} precision {ctx.precision}: {len(t)} rows, worst coefficient gap {worst:.3e} of the row's largest")
    return ref, worst


def test_every_ring_state_with_a_kept_and_a_rejected_pair(ctx):
    """mem 1 .. 8, head 0 .. mem - 1, cnt 0 .. mem: 240 states x (kept, rejected).  The systems are well conditioned (asserted: <= 100), every
    kept row's F.d is positive with a margin, every rejected row leaves cnt 0, resets + 1, gamma doubled and no coefficient."""
    t = ring_rows()
    ref, worst = check_rows(ctx, t, "ring")
    for r in range(len(t)):
        rsi, rsd, rcoef, rmask, rslot, rfd = ref[r]
        cnt, head, mem, resets = t.si[r]
        if r % 2 == 0:                                           # kept
            k = min(cnt + 1, mem)
            slots = [(rsi[1] - (k - 1) + i) % mem for i in range(k)]
            Rm = np.triu(rsd[1:1 + M * M].reshape(M, M)[np.ix_(slots, slots)])
            assert np.linalg.cond(Rm) <= 100.0 and rfd > 1.0 and rsi == (k, (head + 1) % mem, mem, resets), (r, rsi, rfd)
            assert bin(rmask).count("1") == k and rslot == (rsi[1] + 1) % mem
        else:
            assert rsi == (0, head, mem, resets + 1) and rmask == 0 and rsd[0] == 2.0 * t.sd[r][0] and not rcoef[1:].any(), (r, rsi)
    if ctx.precision == 64:
        assert F64_MEASURED is not None, "no measured fp64 gap: profiles/r27_lbfgs_controller.md"


def test_first_step_edges_clamps_descent_test_and_states_out_of_range(ctx):
    """The rows of edge_rows(), with what the restatement must say of them spelt out (so that a wrong restatement cannot pass them on)."""
    t = edge_rows()
    ref, _ = check_rows(ctx, t, "edges")
    r = 0
    for mem0 in range(1, M + 1):                                 # first step: kind 9
        rsi, rsd, rcoef, rmask, rslot, _ = ref[r]
        assert rsi == (0, mem0 - 1, mem0, 0) and rmask == 0 and rslot == 0 and rcoef[0] == first_gamma(ctx.precision) and not rcoef[1:].any()
        r += 1
    for kept in (False, True, False, False, False, False, False):      # at the edge, one double above, +0, -0, negative, NaN, y.y = 0
        rsi, _, _, rmask, rslot, _ = ref[r]
        assert rsi == ((1, 0, 1, 0) if kept else (0, 0, 1, 1)) and rmask == (1 if kept else 0) and rslot == 0, (r, rsi, rmask)
        r += 1
    for bound in (1e-7, 1e2):                                    # just inside / outside each bound
        for f in (1.0 - 1e-6, 1.0 + 1e-6):
            inside = (f > 1.0) == (bound == 1e-7)
            g = ref[r][1][0]
            assert (g != bound and abs(g / bound - 1.0) < 2e-6) if inside else g == bound, (r, bound, f, g)
            r += 1
    for g_out in (60.0, 100.0, 100.0, 1e-7):                     # doubling: 30 -> 60, 60 -> 120 -> 1e2, 1e2 stays, 2e-8 -> 4e-8 -> 1e-7
        assert ref[r][1][0] == g_out and ref[r][0] == (0, 0, 3, 1), (r, ref[r][1][0], ref[r][0])
        r += 1
    for what in ("zero", "negative", "nan", "reject+drop"):      # F.d <= 0 or NaN: the memory goes, gamma stays
        rsi, rsd, rcoef, rmask, rslot, rfd = ref[r]
        want_fd = {"zero": rfd == 0.0, "negative": rfd < -1.0, "nan": np.isnan(rfd), "reject+drop": rfd < 0.0}[what]
        assert want_fd and rmask == 0 and not rcoef[1:].any(), (what, rfd)
        assert rsi == ((0, 1, 3, 7) if what == "reject+drop" else (0, 2, 3, 6)), (what, rsi)
        if what not in ("nan", "reject+drop"):
            assert rsd[0] == t.sums[r][4 * 2 + 2] / t.sums[r][4 * 2 + 3]
        r += 1
    for si, want in (((2, 1, 0, 0), (1, 0)), ((2, 1, 9, 0), (8, 1)), ((2, -1, 4, 0), (4, 0)), ((2, 4, 4, 0), (4, 3)), ((-1, 1, 4, 0), (4, 1)),
                     ((5, 1, 4, 0), (4, 1))):
        mem, head = want
        cnt = min(max(si[0], 0), mem)
        assert ref[r][0] == (0, head, mem, 1), (si, ref[r][0])                                           # rejected
        assert ref[r + 1][0] == (min(cnt + 1, mem), (head + 1) % mem, mem, 0), (si, ref[r + 1][0])       # kept
        r += 2
    assert r == len(t)


def test_a_chain_of_rejections_doubles_gamma_up_to_the_bound_and_stays(ctx):
    """the state of one call fed to the next, five times from gamma = 15: 30, 60, 1e2, 1e2, 1e2, exactly; resets 1 .. 5"""
    t = Rows(29)
    si, sd = np.array([(3, 2, 4, 0)], dtype=np.int32), t.state(gamma=15.0)[None]
    seen = []
    for k in range(5):
        si, sd, coef, ms = ctx.debug_lbfgs_direction(t.some_sums(3, kept=False)[None], si, sd, np.zeros(1, dtype=np.int32), np.full(1, 4, dtype=np.int32))
        seen.append((float(sd[0][0]), float(coef[0][0]), tuple(int(a) for a in si[0]), int(ms[0][0]), int(ms[0][1])))
    assert seen == [(g, g, (0, 2, 4, k + 1), 0, 3) for k, g in enumerate((30.0, 60.0, 100.0, 100.0, 100.0))], seen
