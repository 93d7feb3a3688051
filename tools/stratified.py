#!/usr/bin/env python3
"""c3d_stratified_score on the device beside the numpy restatement on the host: time per call, the split between the two kernels, the gap.

    python tools/stratified.py [--out profiles/r26_stratified.md] [--skip-large]

Sizes: 455 beads x 20 models, 2500 x 8, 8192 x 4 and 16384 x 2, every separation from 3 to n-1, random coils.  Per size: the wall time of
one Solver.stratified_score with all three outputs (a warm call, then the median and range of three, two beyond 5120 beads; the upload of
IF and the host's divisions included), the device time of k_str_if's and k_str_model's launches from HIP events around each pass (stats
"stratified_if_ms", "stratified_models_ms" of the last call), and the restatement tests/stratified_ref.py on the host with the largest
|rho device - rho host| and whether C, A, B are equal.  Up to 2500 beads IF is tests/util.synthetic_if and the host walks every stratum;
beyond, IF is (i + j) mod 1021 (the network's work does not depend on the values) and the host walks 64 sampled strata of every model, its
time scaled to all of them and marked so."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import stratified_ref as S                              # noqa: E402
from tests.util import random_coil, synthetic_if                   # noqa: E402

SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]
RANGE = 3


def measure(s, n, K, rows):
    from chromosome3d_amd import default_model, make_stages
    large = n > 5120
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    i = np.arange(1, n - 4, dtype=np.int32)
    s.set_restraints(n, i, i + 4, np.full(len(i), 60, np.int32))
    s.init_replicas(K)
    s.set_coords(np.stack([random_coil(n, 19 * n + k) for k in range(K)]))
    if large:
        a = np.arange(n, dtype=np.float64)
        IF = np.add.outer(a, a)
        np.fmod(IF, 1021.0, out=IF)
    else:
        IF = synthetic_if(n, seed=n)[0]
    s.stratified_score(IF, RANGE, 0, None, True)                   # warm: code object, the context's IF scratch
    t, split = [], []
    for _ in range(2 if large else 3):
        t0 = time.perf_counter()
        got = s.stratified_score(IF, RANGE, 0, None, True)
        t.append(time.perf_counter() - t0)
        split.append((s.stat("stratified_if_ms"), s.stat("stratified_models_ms")))
    models = [m.astype(np.float64) for m in s.coords()]
    strata = list(range(RANGE, n)) if not large else sorted(set(np.linspace(RANGE, n - 1, 64).astype(int)))
    cache = {}
    t0 = time.perf_counter()
    host = [S.stratified(IF, m, RANGE, 0, strata, cache) for m in models]
    t_host = (time.perf_counter() - t0) * (n - RANGE) / len(strata)
    equal = all(np.array_equal(got["sums"][k][strata], h["sums"][strata]) for k, h in enumerate(host))
    gap = max(np.nanmax(np.abs(got["rho"][k][strata] - h["rho"][strata])) for k, h in enumerate(host))
    nan_same = all(np.array_equal(np.isnan(got["rho"][k][strata]), np.isnan(h["rho"][strata])) for k, h in enumerate(host))
    ms_if, ms_models = np.median([p[0] for p in split]), np.median([p[1] for p in split])
    rows.append(f"| {n} x {K} | {1e3 * np.median(t):.1f} ({1e3 * min(t):.1f} .. {1e3 * max(t):.1f}) | {ms_if:.2f} | {ms_models:.2f} | "
                f"{t_host:.1f}{' (64 strata sampled, scaled)' if large else ''} | {'equal' if equal else 'DIFFERENT'} | {gap:.1e}{'' if nan_same else ' NaN PATTERN DIFFERS'} | "
                f"{np.nanmin(got['scc']):.4f} .. {np.nanmax(got['scc']):.4f} |")
    print(rows[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_stratified.md"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    rows = ["# c3d_stratified_score: device against the numpy restatement on the host (tools/stratified.py)",
            "",
            "Every separation 3 .. n-1, random coils, all three outputs.  call: wall time of one Solver.stratified_score, median (range) of three after a",
            "warm call (two beyond 5120 beads), the upload of IF (8 n^2 bytes from pageable memory) and the host's divisions included.  k_str_if /",
            "k_str_model: device time of each pass's launches, HIP events, median.  host: tests/stratified_ref.py, one rankdata a stratum and model.",
            "No target was set for these times: this is what the first run shows.  Not profiled: LDS bank conflicts of the vector passes at strides",
            "4 .. 32 keys, occupancy of the 64 and 128 KiB workgroups, the uncoalesced diagonal reads of k_str_if.",
            "",
            "| beads x models | call (ms) | k_str_if (ms) | k_str_model (ms) | host (s) | C, A, B | largest abs(rho device - rho host) | scc |",
            "|---|---|---|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    try:
        for n, K in ((455, 20), (2500, 8)) + (() if a.skip_large else ((8192, 4), (16384, 2))):
            measure(s, n, K, rows)
    finally:
        s.close()
    rows.append("")
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
