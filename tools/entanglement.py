#!/usr/bin/env python3
"""Entanglement (writhe, average crossing number, linking table) on the device beside the numpy restatement on the host: times, kernel split, gaps.

    python tools/entanglement.py [--out profiles/r34_entanglement_raw.txt] [--skip-large]

Sizes: 455 beads x 20 models and 16384 x 20, synthetic coordinates (random coils).  Per size, after a warm call, the median and range of
five calls (three at 16384) of Solver.entanglement, device time from the entry's events and wall time: the row sums and totals alone, the
64-domain table alone (the C entry with only `link`), and both.  The kernel split is the first two.  Pairs/s counts the ordered
segment pairs the row kernel evaluates.  Host: tests/entangle_ref.py on the same machine, all rows at 455 and 48 sampled rows of two
models at 16384, its time scaled to all rows of all models and marked so.  Gaps: the largest |device - host| over the compared row sums as
a fraction of its bound 8 x 2^-53 x sum of kappa (tests/test_gpu_entanglement.py)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import entangle_ref as E                                # noqa: E402
from tests.util import random_coil                                 # noqa: E402

SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]
U = 2.0 ** -53
DOMAINS = 64


def timed(call, repeats):
    """(last result, device ms: median, min, max; wall ms: median) of `repeats` calls after a warm one; call() returns (result, device_ms)"""
    call()
    dev, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out, ms = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        dev.append(ms)
    return out, np.median(dev), min(dev), max(dev), np.median(wall)


def measure(s, n, K, lines):
    from chromosome3d_amd import default_model, lib, make_stages
    large = n > 5120
    S = n - 1
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    i = np.arange(1, n - 4, dtype=np.int32)
    s.set_restraints(n, i, i + 4, np.full(len(i), 60, np.int32))
    s.init_replicas(K)
    s.set_coords(np.stack([random_coil(n, 23 * n + k) for k in range(K)]))
    bounds = np.linspace(0, S, DOMAINS + 1).astype(np.int32)
    repeats = 3 if large else 5
    link = np.empty((K, DOMAINS, DOMAINS))
    ms = C.c_double()

    def rows():
        r = s.entanglement()
        return r, r["device_ms"]

    def table():
        lib.check(s._L.c3d_entanglement(s._h, None, 0, 2, 0, lib.i32ptr(bounds), DOMAINS, None, None, None, None, lib.dptr(link), None, C.byref(ms)))
        return link, ms.value

    def both():
        r = s.entanglement(None, 2, 0, bounds)
        return r, r["device_ms"]

    got, d_rows, lo_rows, hi_rows, w_rows = timed(rows, repeats)
    _, d_tab, lo_tab, hi_tab, w_tab = timed(table, repeats)
    full, d_both, lo_both, hi_both, w_both = timed(both, repeats)
    pairs = K * (S * (S - 1) - 2 * (S - 1))
    models = [m.astype(np.float64) for m in s.coords()]
    if large:
        which = np.linspace(0, S - 1, 48).astype(int)
        t0 = time.perf_counter()
        host = [E.rows(models[k], which=which) for k in (0, K - 1)]
        t_host = (time.perf_counter() - t0) * S / len(which) * K / 2
        frac = max(max((np.abs(got[key][k][which] - h[q]) / (8 * U * h[2])).max() for q, key in enumerate(("seg_writhe", "seg_acn"))) for k, h in zip((0, K - 1), host))
        note = " (48 rows of 2 models, scaled)"
    else:
        t0 = time.perf_counter()
        host = [E.entanglement(x) for x in models]
        t_host = time.perf_counter() - t0
        frac = max(max((np.abs(got[key][k] - h[key]) / (8 * U * h["seg_kappa"])).max() for key in ("seg_writhe", "seg_acn")) for k, h in enumerate(host))
        note = ""
    sym = all(np.array_equal(full["link"][k], full["link"][k].T) for k in range(K))
    w = got["writhe"]
    lines.append(f"{n} x {K}\n"
                 f"  rows + totals   device {d_rows:9.3f} ms ({lo_rows:.3f} .. {hi_rows:.3f})   wall {w_rows:9.3f} ms   {pairs / (1e-3 * d_rows):.3e} pairs/s\n"
                 f"  {DOMAINS}-domain table device {d_tab:9.3f} ms ({lo_tab:.3f} .. {hi_tab:.3f})   wall {w_tab:9.3f} ms\n"
                 f"  both            device {d_both:9.3f} ms ({lo_both:.3f} .. {hi_both:.3f})   wall {w_both:9.3f} ms   table symmetric {'yes' if sym else 'NO'}\n"
                 f"  host (numpy)    {t_host:9.3f} s{note}   largest row gap / bound {frac:.4f}\n"
                 f"  writhe {w.min():.3f} .. {w.max():.3f} (mean {w.mean():.3f}, sd {w.std():.3f})   acn per segment {got['acn'].min() / S:.4f} .. {got['acn'].max() / S:.4f}")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r34_entanglement_raw.txt"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    lines = ["Entanglement: device against the numpy restatement on the host (tools/entanglement.py)", "",
             "Device time from the entry's own events (gather of the models, kernels, copies into the caller's arrays), median (range) of five calls after",
             "a warm one, three at 16384; wall time of the same calls.  Separations 2 .. S-1.  Synthetic coordinates (random coils).", ""]
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
