#!/usr/bin/env python3
"""The ensemble's distance map on the device beside the numpy loop on the host: time per call and the largest gaps.

    python tools/ensemble_map.py [--out profiles/r19_ensemble_map.md] [--skip-large]

Sizes: 455 beads x 20 models, 2500 x 8 and 16384 x 4, synthetic coordinates (random coils).  Per size: the wall time of one
Solver.ensemble_map (mean + sd + contact, the copy into the caller's matrices included) and one Solver.ensemble_score (both coefficients) —
a warm call, then the median and range of five (one at 16384) — beside the host loop over K x n^2 distances in numpy (tests/ensemble_ref.py,
the read-back of the coordinates included), and the largest |device - host| of mean, sd and the two coefficients.  At 16384 beads the host
loop runs over a sample of 64 rows (its time is scaled to n rows and marked so) and the coefficients are not recomputed on the host
(ranking 2.7e8 pairs twice in numpy takes minutes and 10 GB): that row records that the sizes fit, and what a call costs."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ensemble_ref as R                                # noqa: E402
from tests.util import random_coil                                 # noqa: E402

SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]
CUTOFF = 7.6


def if_matrix(n, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    m = np.rint(300.0 / (1.0 + np.abs(i[:, None] - i[None, :])) * rng.lognormal(sigma=0.5, size=(n, n)))
    return np.triu(m) + np.triu(m, 1).T


def rows_of_map(models, rows, cutoff):
    """mean, sd, contact of the given rows alone, in ensemble_ref's operation order"""
    d = []
    for x in models:
        u = x[rows][:, None, :] - x[None, :, :]
        d.append(np.sqrt(((u[..., 0] * u[..., 0]) + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]))
    total = np.zeros_like(d[0])
    for k in d:
        total = total + k
    mean = total / len(d)
    dev = np.zeros_like(mean)
    for k in d:
        dev = dev + (k - mean) * (k - mean)
    return mean, np.sqrt(dev / len(d)), sum((k < cutoff).astype(np.int64) for k in d) / len(d)


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
    IF = if_matrix(n, n)
    repeats = 1 if large else 5
    maps, t_map, lo_map, hi_map = timed(lambda: s.ensemble_map(cutoff=CUTOFF), repeats)
    rho, t_rho, lo_rho, hi_rho = timed(lambda: s.ensemble_score(IF, 3, cutoff=CUTOFF), repeats)
    t0 = time.perf_counter()
    models = [m.astype(np.float64) for m in s.coords()]
    if large:
        rows = np.linspace(0, n - 1, 64).astype(int)
        hmean, hsd, hcontact = rows_of_map(models, rows, CUTOFF)
        t_host = (time.perf_counter() - t0) * n / len(rows)
        got = {k: v[rows] for k, v in maps.items()}
        host_note, grho = f"{t_host:.1f} (64 rows, scaled)", ("not computed", "not computed")
    else:
        hmean, hsd, hcontact, _ = R.ensemble_map(models, None, CUTOFF)
        t_host = time.perf_counter() - t0
        got = maps
        host_note = f"{t_host:.3f}"
        grho = tuple(f"{abs(a - R.spearman(IF, maps[k], 3)):.2e}" for a, k in zip(rho, ("mean", "contact")))
    gmean, gsd = np.abs(got["mean"] - hmean).max(), np.abs(got["sd"] - hsd).max()
    exact = np.array_equal(got["contact"], hcontact)
    lines.append(f"| {n} x {K} | {1e3 * t_map:.1f} ({1e3 * lo_map:.1f} .. {1e3 * hi_map:.1f}) | {1e3 * t_rho:.1f} ({1e3 * lo_rho:.1f} .. {1e3 * hi_rho:.1f}) | "
                 f"{host_note} | {gmean:.2e} | {gsd:.2e} | {'equal' if exact else 'DIFFERENT'} | {grho[0]} | {grho[1]} | {rho[0]:.4f} | {rho[1]:.4f} |")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_ensemble_map.md"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    lines = ["# The ensemble's distance map: device against the numpy loop on the host (tools/ensemble_map.py)\n",
             "Wall time per call in ms, median (range) of five after a warm call, one at 16384; the map call returns mean, sd and contact and",
             "includes the copy of the three n x n matrices into the caller's memory; the score call returns both coefficients.  Host: the numpy",
             "loop of tests/ensemble_ref.py in seconds, read-back of the coordinates included.  Gaps: largest |device - host|; the coefficients",
             "against the restatement's over the device's maps.  Synthetic coordinates (random coils), cutoff 7.6 A, range 3.\n",
             "| beads x models | map, ms | score, ms | host map, s | gap mean | gap sd | contact | gap rho_mean | gap rho_contact | rho_mean | rho_contact |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    try:
        for n, K in ((455, 20), (2500, 8)) + (() if a.skip_large else ((16384, 4),)):
            measure(s, n, K, lines)
    finally:
        s.close()
    lines.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
