"""tests/entangle_ref.py, the numpy restatement of c3d_entanglement's definitions (include/c3d.h), held to things that do not share its
code: a quadrature of the Gauss integral, the four-asin form of Klenin & Langowski, shapes whose answers are known, the symmetries of
the integral, the identities of the domain table, and the same code in extended precision.  tests/test_gpu_entanglement.py compares the
device with this restatement under the bound that the last test shows the restatement itself to meet with room."""
import numpy as np
import pytest

from tests import entangle_ref as E
from tests.util import random_coil

U = 2.0 ** -53


@pytest.fixture(scope="module")
def coil():
    return random_coil(40, 3).astype(np.float64)


def test_the_pair_term_is_the_gauss_integral(coil):
    """A 400 x 400 midpoint rule has a relative error of about 1 / (24 m^2) x (segment / distance)^2: 1e-6 is room for pairs a few bonds apart."""
    for s, t in ((0, 5), (3, 20), (10, 38), (20, 3)):
        g = E.row_terms(coil, s)[0][t]
        q = E.quadrature_term(coil, s, t)
        print(f"pair ({s}, {t}): g {g:.12f}, quadrature {q:.12f}, relative gap {abs(g - q) / abs(g):.2e}")
        assert abs(g - q) <= 1e-6 * abs(g)


def test_the_pair_term_is_the_four_asin_form(coil):
    """asin loses half the digits near +-1 (nearly coplanar faces), so the comparison is at 1e-12; the gap seen is 3e-15."""
    S = len(coil) - 1
    worst = 0.0
    for s in range(S):
        g = E.row_terms(coil, s)[0]
        for t in range(S):
            if abs(s - t) >= 2:
                worst = max(worst, abs(g[t] - E.asin_term(coil, s, t)))
    print(f"largest gap to the asin form {worst:.2e}")
    assert worst <= 1e-12


def test_exact_zeros():
    for x in (E.straight(), E.spiral(), E.straight(50), E.spiral(50)):
        r = E.entanglement(x, bounds=[0, 7, len(x) - 1])
        assert (r["seg_writhe"] == 0).all() and (r["seg_acn"] == 0).all() and r["writhe"] == 0 and r["acn"] == 0
        assert (r["link"] == 0).all() and (r["link_abs"] == 0).all()
    x = random_coil(12, 5).astype(np.float64)
    x[7] = x[3]                                                                 # coincident beads: triangles with 0 / 0 contribute 0
    assert np.isfinite(E.entanglement(x)["seg_acn"]).all()


def test_mirror_negates_exactly(coil):
    r = E.entanglement(coil, bounds=[0, 10, 11, 39])
    for axis in range(3):
        m = coil.copy()
        m[:, axis] = -m[:, axis]
        q = E.entanglement(m, bounds=[0, 10, 11, 39])
        for k in ("seg_writhe", "writhe", "link"):
            assert np.array_equal(np.asarray(q[k]), -np.asarray(r[k])), k
        for k in ("seg_acn", "acn", "link_abs"):
            assert np.asarray(q[k]).tobytes() == np.asarray(r[k]).tobytes(), k


def test_reversal_and_rigid_motion_keep_the_totals(coil):
    r = E.entanglement(coil)
    bound = 8 * U * r["kappa"]
    rev = E.entanglement(coil[::-1].copy())
    assert abs(rev["writhe"] - r["writhe"]) <= 2 * bound and abs(rev["acn"] - r["acn"]) <= 2 * bound
    assert np.abs(rev["seg_writhe"][::-1] - r["seg_writhe"]).max() <= 2 * 8 * U * r["seg_kappa"].max()
    rng = np.random.default_rng(4)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q *= np.sign(np.linalg.det(Q))                                              # a proper rotation
    moved = coil @ Q.T + np.array([100.0, -50.0, 25.0])
    # the moved coordinates are rounded once more: a relative 2^-53 of |x| ~ 100 against distances of a few A, times the conditioning
    m = E.entanglement(moved)
    print(f"rigid motion: writhe gap {abs(m['writhe'] - r['writhe']):.2e}, acn gap {abs(m['acn'] - r['acn']):.2e}, bound {100 * bound:.2e}")
    assert abs(m["writhe"] - r["writhe"]) <= 100 * bound and abs(m["acn"] - r["acn"]) <= 100 * bound


def test_helix_is_positive_and_has_the_issues_value():
    r = E.entanglement(E.helix())
    assert abs(r["writhe"] - 2.2047) <= 5e-5 and r["acn"] >= r["writhe"]
    left = E.helix() * np.array([1.0, -1.0, 1.0])
    assert E.entanglement(left)["writhe"] == -r["writhe"]
    local = E.entanglement(E.helix(), 2, 12)                                    # chirality at the scale of less than a turn (30 beads a turn)
    assert local["writhe"] > 0 and (local["seg_writhe"][15:-15] > 0).all()


def test_linked_rings_give_one_and_unlinked_rings_zero():
    x, b = E.two_rings(True)
    r = E.entanglement(x, bounds=b)
    assert abs(abs(r["link"][0, 2]) - 1.0) <= 1e-12 and r["link"][0, 2] == r["link"][2, 0]
    assert r["link"][0, 0] == 0 and r["link"][2, 2] == 0                        # a planar ring has no writhe
    y, _ = E.two_rings(False)
    assert abs(E.entanglement(y, bounds=b)["link"][0, 2]) <= 1e-12
    swapped = E.entanglement(x * np.array([1.0, 1.0, -1.0]), bounds=b)          # the mirror image is linked the other way
    assert swapped["link"][0, 2] == -r["link"][0, 2]


def test_table_identities(coil):
    S = len(coil) - 1
    for lo, hi in ((2, 0), (3, 10)):
        for b in ([0, S], [0, 10, 11, 25, S], list(range(S + 1))):
            r = E.entanglement(coil, lo, hi, b)
            D = len(b) - 1
            assert np.array_equal(r["link"], r["link"].T) and np.array_equal(r["link_abs"], r["link_abs"].T)
            assert abs(r["link"].sum() - r["writhe"]) <= 8 * U * r["kappa"] and abs(r["link_abs"].sum() - r["acn"]) <= 8 * U * r["kappa"]
            for p in range(D if (lo, hi) == (2, 0) else 0):                     # the diagonal: the domain's own writhe, as a chain of its own
                own = coil[b[p]:b[p + 1] + 1]
                if len(own) >= 4:
                    alone = E.entanglement(own)
                    assert abs(alone["writhe"] - r["link"][p, p]) <= 8 * U * alone["kappa"], (b, p)
                else:
                    assert r["link"][p, p] == 0                                 # fewer than three segments: no counted pair
    with_table = E.entanglement(coil, bounds=[0, 20, S])
    assert np.array_equal(with_table["seg_writhe"], E.entanglement(coil)["seg_writhe"])
    w, a, k = E.rows(coil, which=[0, 7, S - 1])
    assert np.array_equal(w, with_table["seg_writhe"][[0, 7, S - 1]]) and np.array_equal(k, with_table["seg_kappa"][[0, 7, S - 1]])


@pytest.mark.parametrize("step", [3.8, 1.9])
@pytest.mark.parametrize("n", [65, 129, 257, 1025])
def test_fp64_against_extended_precision(n, step):
    """The fp64 restatement against the same code in np.longdouble (80-bit here): every row sum within 8 x 2^-53 x the row's sum of kappa, and
    the totals within the same over all pairs.  Seen: under 0.3 % of the bound on rows.  The bound is thus a condition the reference
    meets with room, not a fitted number."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 on this host: nothing to compare with"
    x = random_coil(n, 7 * n, step).astype(np.float64)
    r, rl = E.entanglement(x), E.entanglement(x, ft=np.longdouble)
    rows_w = np.abs((r["seg_writhe"] - rl["seg_writhe"]).astype(np.float64)) / (8 * U * r["seg_kappa"])
    rows_a = np.abs((r["seg_acn"] - rl["seg_acn"]).astype(np.float64)) / (8 * U * r["seg_kappa"])
    tot_w = abs(float(r["writhe"] - rl["writhe"])) / (8 * U * r["kappa"])
    tot_a = abs(float(r["acn"] - rl["acn"])) / (8 * U * r["kappa"])
    print(f"n {n} step {step}: rows {max(rows_w.max(), rows_a.max()):.4f} of the bound, totals {max(tot_w, tot_a):.2e}")
    assert rows_w.max() <= 1 and rows_a.max() <= 1 and tot_w <= 1 and tot_a <= 1
    worst = 0.0
    for s in (0, n // 2, n - 2):                                                # per term, on three rows
        g, kappa = E.row_terms(x, s)
        gl, _ = E.row_terms(x, s, ft=np.longdouble)
        on = kappa > 0
        worst = max(worst, float((np.abs((g - gl).astype(np.float64))[on] / (8 * U * kappa[on])).max()))
    assert worst <= 1
