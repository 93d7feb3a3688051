"""The numpy restatement of the superposition (tests/superpose_ref.py) held to facts that need no device: it is the yardstick of
tests/test_gpu_superpose.py."""
import numpy as np
import pytest

from tests import superpose_ref as R
from tests.util import random_coil


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q if np.linalg.det(q) > 0 else -q


@pytest.mark.parametrize("n", [4, 37, 256])
def test_a_rigid_copy_fits_exactly_and_returns_the_rotation(n):
    rng = np.random.default_rng(n)
    a = random_coil(n, n).astype(np.float64)
    rot, t = _rotation(rng), rng.normal(scale=30.0, size=3)
    Q, mirrored, rmsd, _ = R.fit(a, a @ rot.T + t)
    assert mirrored == 0 and rmsd <= 1e-12 and np.abs(Q - rot).max() <= 1e-12
    Q, mirrored, rmsd, _ = R.fit(a, (-a) @ rot.T + t)               # the same with a reflection through the origin
    assert mirrored == 1 and rmsd <= 1e-12 and np.abs(Q + rot).max() <= 1e-12 and np.linalg.det(Q) < 0
    _, mirrored, rmsd, _ = R.fit(a, (-a) @ rot.T + t, mirror=False)
    assert mirrored == 0 and rmsd > 0.1


def test_rmsd_is_invariant_under_rigid_motion_of_either_side_and_no_worse_than_unfitted():
    rng = np.random.default_rng(1)
    a, b = random_coil(50, 1).astype(np.float64), random_coil(50, 2).astype(np.float64)
    base = R.fit(a, b)[2]
    assert base <= R.unfitted_rmsd(a, b)
    for _ in range(4):
        ra, rb = _rotation(rng), _rotation(rng)
        moved = R.fit(a @ ra.T + rng.normal(size=3), b @ rb.T + rng.normal(scale=100.0, size=3))[2]
        assert abs(moved - base) <= 1e-11
    assert abs(R.fit(-a, b)[2] - base) <= 1e-11                     # with the mirror allowed, the hand of a model does not matter
    assert R.fit(a, b)[1] != R.fit(-a, b)[1]


def test_superpose_and_table_agree_and_procrustes_tightens_the_ensemble():
    rng = np.random.default_rng(3)
    base = random_coil(40, 5).astype(np.float64)
    x = np.stack([(base if k % 2 == 0 else -base) @ _rotation(rng).T + rng.normal(scale=20.0, size=3) + rng.normal(scale=0.5, size=base.shape)
                  for k in range(6)])
    one = R.superpose(x, x[0], True, 0)
    table, mir = R.rmsd_table(x)
    assert np.allclose(one["rmsd"], table[:, 0], atol=1e-12) and np.array_equal(one["mirrored"], mir[:, 0])
    assert np.array_equal(one["mirrored"], [0, 1, 0, 1, 0, 1])
    assert np.allclose(table, table.T, atol=1e-10) and not np.diag(table).any()
    assert np.allclose(one["fitted"].mean(axis=(0, 1)), x[0].mean(axis=0), atol=1e-9)      # the target's frame
    gpa = R.superpose(x, x[0], True, 3)
    assert np.abs(gpa["mean"].mean(axis=0)).max() <= 1e-9                                   # the origin
    assert (gpa["rmsf"] ** 2).sum() <= (one["rmsf"] ** 2).sum() + 1e-12
    assert np.allclose(gpa["rmsd"] ** 2 * 40, ((gpa["fitted"] - gpa["mean"]) ** 2).sum(axis=(1, 2)))
    assert 0.1 < gpa["rmsf"].mean() < 1.5                                                   # the 0.5 A of noise, as the spread of a locus


def test_against_scipy_align_vectors():
    transform = pytest.importorskip("scipy.spatial.transform")
    a, b = R.centred(random_coil(60, 8)), R.centred(random_coil(60, 9))
    rot, rssd = transform.Rotation.align_vectors(b, a)             # rot applied to a ~ b
    Q, e = R.kabsch(a, b)
    assert np.abs(rot.as_matrix() - Q).max() <= 1e-9 and abs(rssd - np.sqrt(e)) <= 1e-9
