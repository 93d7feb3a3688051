#!/usr/bin/env python3
"""c3d_accessibility on the device beside the numpy restatement on the host: time per call, the kernel's share of it, the differing integers.

    python tools/accessibility.py [--out profiles/r29_accessibility.md] [--skip-large]

Sizes: 455 beads x 20 models, 2500 x 8 and 16384 x 2, 96 points, radius and probe at their defaults (half the bond length b0 each), every
model a random coil relaxed by the 45 steps of a short schedule.  Per size: the wall time of one Solver.accessibility (a warm call, then
the median and range of five; the gather of the state, the copy of the counts and the host's divisions included), the device time of
k_access from HIP events around its launch (the entry's device_ms), and the restatement tests/accessibility_ref.py on the host, walking
every j (brute): every row at 455 beads, 64 sampled rows a model beyond, its time scaled to all rows and marked so.  The count of integers
that differ between the device and the restatement over the rows walked must be 0."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import accessibility_ref as A                           # noqa: E402
from tests.util import SHORT, random_coil                          # noqa: E402

POINTS = 96


def measure(s, n, K, rows):
    from chromosome3d_amd import default_model, lib, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    i = np.arange(1, n - 7, dtype=np.int32)
    s.set_restraints(n, i, i + 8, np.full(len(i), 60, np.int32))
    s.init_replicas(K)
    s.set_coords(np.stack([random_coil(n, 29 * n + k) for k in range(K)]))
    s.run()
    s.accessibility()                                              # warm: the code object
    t, ms = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        got = s.accessibility()
        t.append(time.perf_counter() - t0)
        ms.append(got["device_ms"])
    u = np.empty((POINTS, 3))
    assert lib.load().c3d_sphere_points(POINTS, lib.dptr(u)) == 0  # the library's own lattice: no libm difference enters
    models = [m.astype(np.float64) for m in s.coords()]
    sampled = n > 455
    beads = np.unique(np.linspace(0, n - 1, 64).astype(int)) if sampled else np.arange(n)
    t0 = time.perf_counter()
    host = np.stack([A.exposed(m, u, 0.5 * s.b0, 0.5 * s.b0, beads, brute=True) for m in models])
    t_host = (time.perf_counter() - t0) * n / len(beads)
    differing = int((got["exposed"][:, beads] != host).sum())
    e = got["exposed"]
    rows.append(f"| {n} x {K} | {1e3 * np.median(t):.2f} ({1e3 * min(t):.2f} .. {1e3 * max(t):.2f}) | {np.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f}) | "
                f"{t_host:.1f}{' (64 rows a model sampled, scaled)' if sampled else ''} | {differing} of {host.size} | "
                f"{e.min()} .. {e.max()}, {int((e == 0).sum())} of {e.size} beads with none |")
    print(rows[-1], flush=True)
    return differing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_accessibility.md"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    rows = ["# c3d_accessibility: device against the numpy restatement on the host (tools/accessibility.py)",
            "",
            "96 points, radius = probe = b0 / 2 = 1.965 A, random coils relaxed by 45 steps.  call: wall time of one Solver.accessibility, median",
            "(range) of five after a warm call: the gather of the state, the kernel, the copy of the K x n counts and the host's divisions.",
            "k_access: device time of the launch from HIP events (device_ms), median (range) of the same five.  host: tests/accessibility_ref.py",
            "walking every j.  No target was set for these times and no speed ratio is claimed: the host column is the restatement, not a",
            "competitor.  Not profiled: the divergence of the sixteen threads of a row over lists of unequal length, LDS bank conflicts of the",
            "list appends, the kernel at two workgroups a CU against one.",
            "",
            "| beads x models | call (ms) | k_access (ms) | host (s) | differing integers | exposed points a bead |",
            "|---|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    differing = 0
    try:
        for n, K in ((455, 20), (2500, 8)) + (() if a.skip_large else ((16384, 2),)):
            differing += measure(s, n, K, rows)
    finally:
        s.close()
    rows.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows))
    print("wrote", a.out)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
