#!/usr/bin/env python3
"""Model geometry and the distance against separation on the device beside the numpy loop on the host: time per call and the gaps.

    python tools/geometry.py [--out profiles/r22_geometry.txt] [--skip-large]

Sizes: 455 beads x 20 models and 16384 x 20, synthetic coordinates (random coils).  Per size: the wall time of one Solver.geometry (all four
outputs, cutoff 3.5 A, sep 1) and one Solver.separation_profile (mean, sd and contact at 7.6 A) — a warm call, then the median and range
of five (two at 16384) — beside the host loop in numpy (tests/geometry_ref.py, the read-back of the coordinates included), whether the
exact quantities are equal (clash counts, per-bead counts, nearest partners, extent, contact counts) and the largest |device - host| of
the summed ones.  At 16384 beads the host walks a sample — 64 beads of every model for the geometry, 64 separations for the profile — and
its time is scaled to all of them and marked so: 20 x 16384^2 distances in numpy are minutes and 2 GB a model."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import geometry_ref as G                                # noqa: E402
from tests.util import random_coil                                 # noqa: E402

SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]
CLASH, CONTACT = 3.5, 7.6


def rows_of_geometry(x, rows, cutoff):
    """per-bead clash partners, nearest and furthest partner of the given beads alone (sep 1), in geometry_ref's operation order"""
    u = x[rows][:, None, :] - x[None, :, :]
    d = np.sqrt(((u[..., 0] * u[..., 0]) + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2])
    other = np.arange(len(x))[None, :] != rows[:, None]
    return (other & (d <= cutoff)).sum(1), np.where(other, d, np.inf).min(1), d.max(1)


def separations_of_profile(models, seps, cutoff):
    """mean, sd and contact count of the given separations alone, in geometry_ref's operation order"""
    mean, sd, count = np.zeros(len(seps)), np.zeros(len(seps)), np.zeros(len(seps), dtype=np.int64)
    for q, s in enumerate(seps):
        v = []
        for x in models:
            u = x[s:] - x[:len(x) - s]
            v.append(np.sqrt(((u[:, 0] * u[:, 0]) + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]))
        v = np.concatenate(v)
        mean[q] = v.sum() / len(v)
        e = v - mean[q]
        sd[q] = np.sqrt((e * e).sum() / len(v))
        count[q] = (v < cutoff).sum()
    return mean, sd, count


def timed(call, repeats):
    call()                                                         # warm: code object, allocator
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = call()
        t.append(time.perf_counter() - t0)
    return out, np.median(t), min(t), max(t)


def measure(s, n, K, lines):
    from chromosome3d_amd import default_model, make_stages
    large = n > 5120
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    i = np.arange(1, n - 4, dtype=np.int32)
    s.set_restraints(n, i, i + 4, np.full(len(i), 60, np.int32))
    s.init_replicas(K)
    s.set_coords(np.stack([random_coil(n, 19 * n + k) for k in range(K)]))
    repeats = 2 if large else 5
    geo, t_geo, lo_geo, hi_geo = timed(lambda: s.geometry(None, CLASH, 1), repeats)
    prof, t_sep, lo_sep, hi_sep = timed(lambda: s.separation_profile(None, None, CONTACT), repeats)
    t0 = time.perf_counter()
    models = [m.astype(np.float64) for m in s.coords()]
    t_read = time.perf_counter() - t0
    terms = (n - np.arange(n)) * K
    if large:
        rows = np.linspace(0, n - 1, 64).astype(int)
        t0 = time.perf_counter()
        host = [rows_of_geometry(x, rows, CLASH) for x in models]
        t_hgeo = t_read + (time.perf_counter() - t0) * n / len(rows)
        exact = all(np.array_equal(geo["bead_clashes"][k][rows], h[0]) and np.array_equal(geo["nearest"][k][rows], h[1]) for k, h in enumerate(host))
        exact = exact and all(geo["chain"][k, 5] >= h[2].max() for k, h in enumerate(host))
        chain_gap = "not computed"
        seps = np.unique(np.concatenate([np.arange(0, 8), np.linspace(8, n - 1, 56).astype(int)]))
        t0 = time.perf_counter()
        hmean, hsd, hcount = separations_of_profile(models, seps, CONTACT)
        t_hsep = t_read + (time.perf_counter() - t0) * n / len(seps)
        gmean, gsd = np.abs(prof[0][seps] - hmean).max(), np.abs(prof[1][seps] - hsd).max()
        counts = np.array_equal(np.rint(prof[2][seps] * terms[seps]).astype(np.int64), hcount)
        note = " (64 sampled, scaled)"
    else:
        t0 = time.perf_counter()
        host = [G.geometry(x, CLASH, 1) for x in models]
        t_hgeo = t_read + time.perf_counter() - t0
        exact = all(geo["clashes"][k] == h["clashes"] and np.array_equal(geo["bead_clashes"][k], h["bead_clashes"]) and
                    np.array_equal(geo["nearest"][k], h["nearest"]) and geo["chain"][k, 5] == h["chain"][5] for k, h in enumerate(host))
        chain_gap = f"{max(np.abs(geo['chain'][k, :5] - h['chain'][:5]).max() for k, h in enumerate(host)):.2e}"
        t0 = time.perf_counter()
        hmean, hsd, _, hcount, _ = G.separation_profile(models, None, CONTACT)
        t_hsep = t_read + time.perf_counter() - t0
        gmean, gsd = np.abs(prof[0] - hmean).max(), np.abs(prof[1] - hsd).max()
        counts = np.array_equal(np.rint(prof[2] * terms).astype(np.int64), hcount)
        note = ""
    lines.append(f"{n} x {K}\n"
                 f"  geometry   device {1e3 * t_geo:9.2f} ms ({1e3 * lo_geo:.2f} .. {1e3 * hi_geo:.2f})   host {t_hgeo:9.3f} s{note}   "
                 f"exact quantities {'equal' if exact else 'DIFFERENT'}   chain gap {chain_gap}   clashes {int(geo['clashes'].min())} .. {int(geo['clashes'].max())}\n"
                 f"  separation device {1e3 * t_sep:9.2f} ms ({1e3 * lo_sep:.2f} .. {1e3 * hi_sep:.2f})   host {t_hsep:9.3f} s{note}   "
                 f"contact counts {'equal' if counts else 'DIFFERENT'}   gap mean {gmean:.2e}   gap sd {gsd:.2e}   "
                 f"R(1) {prof[0][1]:.3f}  R(16) {prof[0][min(16, n - 1)]:.3f}  P(2) {prof[2][2]:.4f}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_geometry.txt"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    lines = ["Model geometry and distance against separation: device against the numpy loop on the host (tools/geometry.py)",
             "",
             "Wall time per call, median (range) of five after a warm call, two at 16384.  geometry: clash count (d <= 3.5 A, sep 1), per-bead counts,",
             "nearest partners and the chain fields of every model, copies into the caller's arrays included.  separation: mean, sd and contact",
             "(d < 7.6 A) against s.  Host: the numpy loop of tests/geometry_ref.py, read-back of the coordinates included.  Gaps: largest",
             "|device - host|.  Synthetic coordinates (random coils).  No target was set for these times: this is what the first run shows.",
             ""]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    try:
        for n, K in ((455, 20),) + (() if a.skip_large else ((16384, 20),)):
            measure(s, n, K, lines)
    finally:
        s.close()
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
