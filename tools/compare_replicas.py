#!/usr/bin/env python3
"""Wall time of one Solver.compare() (c3d_compare_replicas: every replica against every other, on the device) against the host loop over
the same models (pipeline.model_similarity for every pair a < b), in the same process.

    python tools/compare_replicas.py [--rows chr1,2500,8192,16384] [--host-limit 60] [--out profiles/r13_compare_replicas.md]

Rows: chr1_500kb x 20 after a default solve; 2500 beads x 8, 8192 x 4 and 16384 x 4 random coils (set_coords on a chain-only context: the
time does not depend on what the models look like, only ties would shorten the look-ups).  The device call is warmed once, then timed
`--calls` times: median and min..max.  The host loop runs once; beyond 8192 beads it is skipped where the previous row's time per pair,
scaled by m log m, says it would pass --host-limit seconds.  Where both ran, the largest difference of the two tables is written beside the
times.  A record, not a gate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def coil(n, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = np.cumsum(3.8 * d, axis=0)
    return (x - x.mean(0)).astype(np.float32)


def prepare(s, row):
    """the context holding the row's models; returns (label, n, M)"""
    from chromosome3d_amd import default_model, make_stages, pipeline
    if row == "chr1":
        from tests.util import load_if
        IF = load_if("chr1_500kb")
        s.set_model(default_model())
        pipeline.IF2dist_new(s, IF)
        pipeline.build_models(s, 20)
        return "chr1_500kb x 20, default solve", len(IF), 20
    n = int(row)
    M = 8 if n <= 2500 else 4
    s.set_option("max_beads", max(n, 5120))
    s.set_model(default_model())
    s.set_schedule(make_stages([(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0)]))
    s.set_restraints(n, np.array([1], np.int32), np.array([11], np.int32), np.array([100], np.int32))
    s.init_replicas(M, 82364, 0)
    s.set_coords(np.stack([coil(n, 1000 + r) for r in range(M)]))
    return f"{n} x {M}, random coils", n, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="chr1,2500,8192,16384")
    ap.add_argument("--calls", type=int, default=5, help="timed device calls per row (3 beyond 5120 beads)")
    ap.add_argument("--host-limit", type=float, default=60.0, help="seconds the host loop of a row beyond 8192 beads may be expected to take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_compare_replicas.md"))
    a = ap.parse_args()
    from chromosome3d_amd import Solver, pipeline
    lines = ["# c3d_compare_replicas against the host loop", "",
             "One `Solver.compare()` (both K x K tables; warm call first, then the timed calls: median, min..max) and one host loop",
             "`pipeline.model_similarity` over the pairs a < b of the same models, same process (`tools/compare_replicas.py`).", "",
             "| models | pairs m | device call, s (median) | min..max, s | calls | host loop, s | host / device | max abs diff rho | max abs diff rmsd |",
             "|---|---|---|---|---|---|---|---|---|"]
    per_pair_unit = None           # host seconds per (model pair x m log2 m) of the last row whose host loop ran
    for row in a.rows.split(","):
        s = Solver(0)
        try:
            label, n, M = prepare(s, row)
            m = n * (n - 1) // 2
            s.compare()
            calls = a.calls if n <= 5120 else min(a.calls, 3)
            times = []
            for _ in range(calls):
                t0 = time.perf_counter()
                rho, rmsd = s.compare()
                times.append(time.perf_counter() - t0)
            med = statistics.median(times)
            pairs = M * (M - 1) // 2
            work = pairs * m * np.log2(m)
            expect = None if per_pair_unit is None else per_pair_unit * work
            host = "skipped"
            ratio = drho = drmsd = "-"
            if n <= 8192 or expect is None or expect <= a.host_limit:
                x = s.coords().astype(np.float64)
                t0 = time.perf_counter()
                hrho, hrmsd = np.ones((M, M)), np.zeros((M, M))
                for p in range(M):
                    for q in range(p + 1, M):
                        hrho[p, q], hrmsd[p, q] = pipeline.model_similarity(x[p], x[q])
                th = time.perf_counter() - t0
                per_pair_unit = th / work
                iu = np.triu_indices(M, 1)
                host, ratio = f"{th:.3f}", f"{th / med:.1f}"
                drho, drmsd = f"{np.abs(rho[iu] - hrho[iu]).max():.2e}", f"{np.abs(rmsd[iu] - hrmsd[iu]).max():.2e}"
            else:
                host = f"skipped (expected {expect:.0f} s)"
            lines.append(f"| {label} | {m} | {med:.4f} | {min(times):.4f}..{max(times):.4f} | {calls} | {host} | {ratio} | {drho} | {drmsd} |")
            print(lines[-1], flush=True)
        finally:
            s.close()
    lines += ["", "The host loop covers the pairs a < b only (one call gives rho and the rmsd of one direction); the device call fills both",
              "directions of both tables.  The table pass exists in its VALU form only: no MFMA form was built, so there is no second time."]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
