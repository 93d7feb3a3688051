"""The yardstick of tests/test_gpu_accessibility.py — the numpy restatement tests/accessibility_ref.py of c3d_accessibility — held to facts
outside itself: the analytic cap of two overlapping spheres, the symmetries of the definition, the lattice's own properties, and its quick
walk over j against the brute one."""
import numpy as np
import pytest

from tests import accessibility_ref as A
from tests.util import random_coil

RADIUS = PROBE = 1.965                                                          # touching beads at the default bond length 3.93 A
R = RADIUS + PROBE


def test_the_lattice_is_on_the_sphere_and_balanced():
    """unit norms to 4e-16; the centroid's norm below 1e-3 at 96 points and 1e-5 at 1024 (measured 9.8e-4 and 1.7e-6)"""
    for P, bound in ((96, 1e-3), (1024, 1e-5)):
        u = A.lattice(P)
        assert u.shape == (P, 3) and np.abs(np.linalg.norm(u, axis=1) - 1.0).max() <= 4e-16
        print(f"P = {P}: centroid norm {np.linalg.norm(u.mean(axis=0)):.3g}")
        assert np.linalg.norm(u.mean(axis=0)) < bound
    assert np.array_equal(A.lattice(1), [[1.0, 0.0, 0.0]])                      # one point: z = 0, r = 1, phi = 0


def test_a_bead_out_of_reach_of_every_other_is_fully_exposed():
    u = A.lattice(96)
    x = np.array([[0.0, 0.0, 0.0], [2.0 * R + 1e-6, 0.0, 0.0], [0.0, -2.0 * R - 1e-6, 0.0], [50.0, 50.0, 50.0]])
    assert list(A.exposed(x, u, RADIUS, PROBE, brute=True)) == [96] * 4
    x[1, 0] = 2.0 * R - 0.5                                                     # within reach: bead 0 and bead 1 lose points, the others none
    e = A.exposed(x, u, RADIUS, PROBE, brute=True)
    assert e[0] < 96 and e[1] < 96 and list(e[2:]) == [96, 96]


def test_two_beads_expose_the_analytic_cap():
    """Two spheres of radius R at distance d < 2 R: the share of either outside the other is (1 + d / 2R) / 2.  At P = 1024 the lattice gives
    it within 0.01 (0.0055 at worst over 200 random directions and distances when the bound was chosen, 0.0060 over the 200 drawn here; at
    P = 96 the worst was 0.036: nothing is asserted there)."""
    u = A.lattice(1024)
    rng = np.random.default_rng(20261020)
    worst = 0.0
    for _ in range(200):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        d = rng.uniform(0.02, 1.0) * 2.0 * R
        x = np.stack([rng.normal(scale=20.0, size=3), np.zeros(3)])
        x[1] = x[0] + d * axis
        err = np.abs(A.exposed(x, u, RADIUS, PROBE, brute=True) / 1024.0 - (1.0 + d / (2.0 * R)) / 2.0).max()
        worst = max(worst, err)
    print(f"worst deviation from the cap fraction at P = 1024: {worst:.4f}")
    assert worst <= 0.01


def test_the_order_of_the_beads_does_not_matter_and_a_bead_more_never_exposes():
    u = A.lattice(96)
    x = random_coil(150, 15).astype(np.float64)
    e = A.exposed(x, u, RADIUS, PROBE, brute=True)
    assert e.min() < 96 and e.max() > 0 and len(set(e)) > 10                    # a track, not a constant
    assert np.array_equal(A.exposed(x[::-1], u, RADIUS, PROBE, brute=True), e[::-1])
    rng = np.random.default_rng(3)
    for _ in range(5):
        more = np.concatenate([x, x[rng.integers(150)][None] + rng.normal(scale=2.0, size=(1, 3))])
        e1 = A.exposed(more, u, RADIUS, PROBE, brute=True)
        assert (e1[:150] <= e).all() and (e1[:150] < e).any()


def test_a_bead_is_left_out_by_index_and_its_twin_is_not():
    """Points a hair inside the unit sphere (squared norm 1 - 5e-10, which the entry accepts): a bead's own sphere holds all its points and
    must not bury them, a second bead at the same coordinates has the same sphere and buries every one.  A hair outside: none."""
    inside, outside = A.lattice(96) * np.sqrt(1.0 - 5e-10), A.lattice(96) * np.sqrt(1.0 + 5e-10)
    far = np.array([[3.0, -7.0, 11.0], [300.0, 0.0, 0.0]])
    assert list(A.exposed(far, inside, RADIUS, PROBE, brute=True)) == [96, 96]
    twins = np.array([[3.0, -7.0, 11.0], [300.0, 0.0, 0.0], [3.0, -7.0, 11.0]])
    assert list(A.exposed(twins, inside, RADIUS, PROBE, brute=True)) == [0, 96, 0]
    assert list(A.exposed(twins, outside, RADIUS, PROBE, brute=True)) == [96, 96, 96]
    # on the lattice itself rounding decides point by point, and the restatement follows the definition's operations one by one
    u = A.lattice(96)
    got = A.exposed(twins, u, RADIUS, PROBE, brute=True)
    Rd, count = float(np.float64(RADIUS) + np.float64(PROBE)), 0
    for p in range(96):
        c = [float(twins[0, q]) + Rd * float(u[p, q]) for q in range(3)]        # python floats: a product, then a sum, each rounded
        e = [c[q] - float(twins[2, q]) for q in range(3)]
        count += 0 if (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] < Rd * Rd else 1
    assert got[0] == got[2] == count and got[1] == 96


@pytest.mark.parametrize("name", ["coil", "dense", "tangent"])
def test_the_quick_walk_gives_the_brute_walks_integers(name):
    u = A.lattice(96)
    if name == "tangent":
        models, labels = A.tangent_table(RADIUS, PROBE)
        assert len(models) == 108
        brute = np.array([A.exposed(m, u, RADIUS, PROBE, brute=True) for m in models])
        quick = np.array([A.exposed(m, u, RADIUS, PROBE) for m in models])
        hit = brute[:, 0] < 96
        print(f"tangent table: {int(hit.sum())} cases with a buried point, {int((~hit).sum())} without")
        assert hit.any() and (~hit).any()                                       # the table decides between a tight and a loose bound
        assert (brute[:, 1:] == 96).all() and (brute[:, 0] >= 95).all()
        for shift in (0.0, 9e5):                                                # ... at the origin and far from it
            some = np.array([l[0] == shift for l in labels])
            assert hit[some].any() and (~hit[some]).any()
    else:
        x = random_coil(300, 30).astype(np.float64) * (0.01 if name == "dense" else 1.0)
        brute, quick = A.exposed(x, u, RADIUS, PROBE, brute=True), A.exposed(x, u, RADIUS, PROBE)
        assert (brute < 96).all() and ((brute == 0).sum() > 200 if name == "dense" else (brute > 0).sum() > 100)
    assert quick.dtype == np.int32 and np.array_equal(quick, brute)
