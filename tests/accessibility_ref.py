"""Numpy restatement of c3d_accessibility (include/c3d.h): Shrake-Rupley over uniform spheres, every operation written as the definition
gives it — float64 arrays, one numpy operation a rounding, no fused multiply-add anywhere.
tests/test_accessibility_ref.py holds it to facts outside itself; tests/test_gpu_accessibility.py holds the device to it with ==.

Two walks over j give the same integers.  brute=True tests every j != i: the definition as it stands, 3.4 s for one model of 1100 beads and
96 points.  The default leaves out, before any point is formed, the beads whose coordinates differ from bead i's by more than 2 R + 1 A
along some axis, which keeps a test of 2052 beads x 3 models inside a second.  Such a bead is further than 2 R + 1 A from x_i; a point lies
within R (1 + 1e-9) + 1e-9 A of x_i (the entry's limits on |u|, |x| < 1e6 and R <= 1e5, roundings included), so it is further than R + 0.99 A
from that bead and its squared distance, whatever its last bits, is not below R2.  The margin is a whole Angstrom where the device's own
neighbour bound (csrc/c3d_score_access.inc) is R 2^-20: the two share nothing, and tests/test_accessibility_ref.py holds the default walk to
the brute one on coils, a dense model and the tangent table."""
import numpy as np


def lattice(P):
    """the Fibonacci lattice of c3d_sphere_points: z = 1 - (2k+1)/P, r = sqrt(1 - z z), phi = k pi (3 - sqrt 5), u = (r cos phi, r sin phi, z)"""
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(P)
    r = np.sqrt(1.0 - z * z)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def buried_mask(x, u, radius, probe, rows=None, brute=False, chunk=128):
    """[len(rows), P] bool: point p of bead rows[a] lies strictly inside the sphere of another bead.  x [n, 3], u [P, 3] float64."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    u = np.ascontiguousarray(u, dtype=np.float64)
    n = len(x)
    rows = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    R = np.float64(radius) + np.float64(probe)
    R2 = R * R
    Ru = R * u                                                                  # [P, 3]: one product a component
    out = np.zeros((len(rows), len(u)), dtype=bool)
    everyone = np.arange(n)
    for a, i in enumerate(rows):
        c = x[i][None, :] + Ru                                                  # [P, 3]: one sum a component
        js = everyone if brute else np.nonzero(np.abs(x - x[i]).max(axis=1) <= 2.0 * R + 1.0)[0]
        js = js[js != i]                                                        # j = i is left out by index, not by distance
        alive = np.arange(len(u))                                               # a buried point stays buried: it is not tested again
        for j0 in range(0, len(js), chunk):
            xj = x[js[j0:j0 + chunk]]
            e = c[alive][:, None, :] - xj[None, :, :]                           # [points alive, J, 3]
            s = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            hit = (s < R2).any(axis=1)
            out[a, alive[hit]] = True
            alive = alive[~hit]
            if alive.size == 0:
                break
    return out


def exposed(x, u, radius, probe, rows=None, brute=False):
    """int32 [len(rows)]: the number of points of every asked bead (None: all) that no other bead buries"""
    return (len(u) - buried_mask(x, u, radius, probe, rows, brute).sum(axis=1)).astype(np.int32)


def tangent_table(radius=1.965, probe=1.965, u=None):
    """The cases that decide between a tight and a loose neighbour bound: (models [108, 3, 3], labels).  Three beads a model: the first at
    the origin or at (9e5, 9e5, 9e5), the second at 2 R (1 +- 2^-k) u_p from it, k = 20, 24, .. 52 and p in {0, 17, 95} — point p of the
    first bead then lies R (1 -+ 2^(1-k)) from the second, inside or outside its sphere by less and less until rounding decides — and a
    third 100 A off along x, which buries nothing.  u: the 96 points the directions are taken from (None: lattice(96)); a device test passes
    the library's own, so that the second bead sits on the direction the device forms its point with."""
    u = lattice(96) if u is None else u
    R = np.float64(radius) + np.float64(probe)
    models, labels = [], []
    for shift in (0.0, 9e5):
        for k in range(20, 53, 4):
            for sign in (-1.0, 1.0):
                for p in (0, 17, 95):
                    first = np.full(3, shift)
                    second = first + (2.0 * R * (1.0 + sign * 2.0 ** -k)) * u[p]
                    third = first + np.array([100.0, 0.0, 0.0])
                    models.append(np.stack([first, second, third]))
                    labels.append((shift, k, sign, p))
    return np.stack(models), labels
