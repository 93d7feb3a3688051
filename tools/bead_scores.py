#!/usr/bin/env python3
"""c3d_bead_scores on the device beside the numpy restatement on the host: time per call, the split between the two kernels, the gap.

    python tools/bead_scores.py [--out profiles/r10_bead_scores.md] [--skip-large]

Sizes: 455 beads x 20 models, 2052 x 3 and 16384 x 1, every bead, range 3, random coils, a restraint every fourth neighbour.  Per size: the
wall time of one Solver.bead_scores with all five outputs (a warm call, then the median and range of three, two beyond 5120 beads; the
upload of IF and the host's divisions included), the device time of k_bead_if's and k_bead_model's launches from HIP events around each
pass (stats "bead_if_ms", "bead_models_ms" of the last call), and the restatement tests/bead_ref.py on the host with the largest
|rho device - rho host| and whether C, A, B and the tallies are equal.  Up to 5120 beads IF is tests/util.synthetic_if and the host walks
every row; beyond, IF is (i + j) mod 1021 (the network's work does not depend on the values) and the host walks 64 sampled rows, its time
scaled to all of them and marked so."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bead_ref as Bd                                   # noqa: E402
from tests.util import random_coil, synthetic_if                   # noqa: E402

SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]
RANGE = 3
SEP = 8                                                            # the restrained partner of bead i: i + 8 (beyond the model's min_sep)


class Targets:
    """row i of the target matrix of the restraints (i, i + SEP, 60 tenths), on demand"""

    def __init__(self, n):
        self.n = n

    def __getitem__(self, i):
        row = np.zeros(self.n, dtype=np.int64)
        for j in (i - SEP, i + SEP):
            if 0 <= j < self.n:
                row[j] = 60
        return row


def measure(s, n, K, rows):
    from chromosome3d_amd import default_model, make_stages
    large = n > 5120
    model = default_model()
    s.set_model(model)
    s.set_schedule(make_stages(SHORT))
    i = np.arange(1, n - SEP + 1, dtype=np.int32)
    s.set_restraints(n, i, i + SEP, np.full(len(i), 60, np.int32))
    s.init_replicas(K)
    s.set_coords(np.stack([random_coil(n, 19 * n + k) for k in range(K)]))
    if large:
        a = np.arange(n, dtype=np.float64)
        IF = np.add.outer(a, a)
        np.fmod(IF, 1021.0, out=IF)
    else:
        IF = synthetic_if(n, seed=n)[0]
    s.bead_scores(IF, RANGE)                                       # warm: code object, the context's IF scratch
    t, split = [], []
    for _ in range(2 if large else 3):
        t0 = time.perf_counter()
        got = s.bead_scores(IF, RANGE)
        t.append(time.perf_counter() - t0)
        split.append((s.stat("bead_if_ms"), s.stat("bead_models_ms")))
    models = [m.astype(np.float64) for m in s.coords()]
    beads = list(range(n)) if not large else sorted(set(np.linspace(0, n - 1, 64).astype(int)))
    cache = {}
    t0 = time.perf_counter()
    host = [Bd.bead_scores(IF, m, RANGE, beads, Targets(n), int(model.min_sep), cache) for m in models]
    t_host = (time.perf_counter() - t0) * n / len(beads)
    equal = all(np.array_equal(got["sums"][k][beads], h["sums"]) for k, h in enumerate(host))
    tallies = all(np.array_equal(got["restrained"][beads], h["restrained"]) and np.array_equal(got["satisfied"][k][beads], h["satisfied"]) and
                  np.array_equal(got["dev_milli"][k][beads], h["dev_milli"]) for k, h in enumerate(host))
    gap = max(np.nanmax(np.abs(got["rho"][k][beads] - h["rho"])) for k, h in enumerate(host))
    nan_same = all(np.array_equal(np.isnan(got["rho"][k][beads]), np.isnan(h["rho"])) for k, h in enumerate(host))
    ms_if, ms_models = np.median([p[0] for p in split]), np.median([p[1] for p in split])
    rows.append(f"| {n} x {K} | {1e3 * np.median(t):.1f} ({1e3 * min(t):.1f} .. {1e3 * max(t):.1f}) | {ms_if:.2f} | {ms_models:.2f} | "
                f"{t_host:.1f}{' (64 rows sampled, scaled)' if large else ''} | {'equal' if equal else 'DIFFERENT'} | {'equal' if tallies else 'DIFFERENT'} | "
                f"{gap:.1e}{'' if nan_same else ' NaN PATTERN DIFFERS'} | {np.nanmin(got['rho']):.4f} .. {np.nanmax(got['rho']):.4f} |")
    print(rows[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_bead_scores.md"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    rows = ["# c3d_bead_scores: device against the numpy restatement on the host (tools/bead_scores.py)",
            "",
            "Every bead, range 3, random coils, all five outputs.  call: wall time of one Solver.bead_scores, median (range) of three after a warm",
            "call (two beyond 5120 beads), the upload of IF (8 n^2 bytes from pageable memory) and the host's divisions included.  k_bead_if /",
            "k_bead_model: device time of each pass's launch, HIP events, median.  host: tests/bead_ref.py, one rankdata a row and model and the",
            "tallies.  No target was set for these times and no speed ratio is claimed: the host column is the restatement, not a tuned code.",
            "Not profiled: LDS bank conflicts of the vector passes, occupancy of the 64 and 128 KiB workgroups, the one P a call (a short row",
            "sorts the pad of the longest).",
            "",
            "| beads x models | call (ms) | k_bead_if (ms) | k_bead_model (ms) | host (s) | C, A, B | tallies | largest abs(rho device - rho host) | rho |",
            "|---|---|---|---|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    try:
        for n, K in ((455, 20), (2052, 3)) + (() if a.skip_large else ((16384, 1),)):
            measure(s, n, K, rows)
    finally:
        s.close()
    rows.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
