#!/usr/bin/env python3
"""The gaps tests/test_gpu_superpose.py bounds, measured, and the wall time of the on-device superposition against the numpy restatement.

    python tools/superpose.py [--out profiles/r17_superpose.md] [--skip-large]

Gaps: the test module's own cases are run (its functions, its models) and the largest |device - restatement| of every figure is printed:
the "largest" lines are what the module's MEASURED table holds.  Times: c3d_rmsd_table and one superpose(iters=3) at 455 beads x 20
models, 2500 x 8 and 16384 x 20 (random coils and moved copies), a warm call and then the median and range of five, beside the
restatement on the host for the same input, the read-back of the coordinates included (one run; the table is skipped on the host where
it would pass a minute)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import superpose_ref as R                               # noqa: E402
from tests import test_gpu_superpose as T                          # noqa: E402
from tests.util import random_coil                                 # noqa: E402


def gaps(lines):
    from chromosome3d_amd import Solver
    s32, s64 = Solver(0), Solver(0)
    for key, val in (("max_beads", 16384), ("f64_max_beads", 16384), ("precision", 64)):
        s64.set_option(key, val)
    for name in T.CASES:
        T.test_superposition_equals_the_restatement(s32, name)
    for name in T.CASES64:
        T.test_f64_state_is_fitted_and_applied_in_doubles(s64, name)
    T.test_apply_on_a_precision_32_context(s32)
    T.test_table_of_17_replicas_and_16_extras(s32)
    T.test_large_models_on_a_precision_64_context(s64)
    T.test_bundled_model_as_the_reference(s32)
    s32.close()
    s64.close()
    lines.append("## Gaps against tests/superpose_ref.py (every case of tests/test_gpu_superpose.py)\n")
    lines.append("| figure | largest gap | 8 x | bound in the test |")
    lines.append("|---|---|---|---|")
    for k, v in sorted(T.GAPS.items()):
        lines.append(f"| {k} | {v:.3e} | {8 * v:.3e} | {T.BOUND[k]:.3e} |")
    for k, v in sorted(T.GAPS.items()):
        lines.append(f"\nlargest {k}: {v:.3e}")
    lines.append("")


def ensemble(n, K, seed):
    rng = np.random.default_rng(seed)
    bases = [random_coil(n, seed + b).astype(np.float64) for b in range(3)]
    out = []
    for k in range(K):
        x = bases[k % 3]
        if k >= 3:
            x = (x if k % 2 == 0 else -x) @ T.rotation(rng).T + rng.normal(scale=40.0, size=3) + rng.normal(scale=0.3, size=x.shape)
        out.append(x)
    return np.stack(out).astype(np.float32)


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t))
    return float(np.median(ts)), min(ts), max(ts)


def times(lines, large):
    from chromosome3d_amd import Solver
    lines.append("## Wall time (ms; device: warm call, then median and min..max of 5; host: one run of the restatement, read-back included)\n")
    lines.append("| beads x models | c3d_rmsd_table | host table | superpose(iters=3) | host superpose |")
    lines.append("|---|---|---|---|---|")
    for n, K in [(455, 20), (2500, 8)] + ([(16384, 20)] if large else []):
        s = Solver(0)
        s.set_option("max_beads", 16384)
        T.restrained(s, n, K)
        s.set_coords(ensemble(n, K, 17))
        tab = timed(lambda: s.rmsd_table())
        sup = timed(lambda: s.superpose(0, iters=3))
        t = time.perf_counter()
        x = s.coords().astype(np.float64)
        R.superpose(x, x[0], True, 3)
        host_sup = 1e3 * (time.perf_counter() - t)
        t = time.perf_counter()
        x = s.coords().astype(np.float64)
        R.rmsd_table(x)
        host_tab = 1e3 * (time.perf_counter() - t)
        lines.append(f"| {n} x {K} | {tab[0]:.2f} ({tab[1]:.2f}..{tab[2]:.2f}) | {host_tab:.1f} | {sup[0]:.2f} ({sup[1]:.2f}..{sup[2]:.2f}) | {host_sup:.1f} |")
        s.close()
    lines.append("")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_superpose.md"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    lines = ["# Superposition of a run's models on the device: gaps and times (MI355X)\n"]
    gaps(lines)
    times(lines, not a.skip_large)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
