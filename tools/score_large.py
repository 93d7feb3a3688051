#!/usr/bin/env python3
"""Wall time of c3d_score_replicas on large maps with the IF ranks from the host (device_ranks -1) and from the device (1): one call
each per size, one child process per size under a time limit (a fresh context each; the host side needs about 10 GB at 16384 beads).

    python tools/score_large.py [--sizes 6000,8192,16384] [--limit 600] [--out profiles/r12_score_large.md]

The matrix is tools/large_maps.py's synthetic one, the model a compact random coil (the fixed histogram holds it), one replica, one
restraint: the time is that of ranking the matrix and of the distance side.  A record, not a gate."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def child(n):
    import numpy as np
    from chromosome3d_amd import Solver, default_model, make_stages, pipeline
    from large_maps import synthetic
    s = Solver(0)
    s.set_option("max_beads", max(n, 5120))
    s.set_model(default_model())
    s.set_schedule(make_stages([(2, 10, 0.0, 1.0, 20.0, 0.5, 0.0)]))
    s.set_restraints(n, np.array([1], np.int32), np.array([11], np.int32), np.array([100], np.int32))
    s.init_replicas(1, 82364, 0)
    rng = np.random.default_rng(5)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = np.cumsum(3.8 * d, axis=0)
    s.set_coords((x / np.abs(x).max() * 60.0).astype(np.float32)[None])
    IF = synthetic(n)
    row = {"n": n}
    s.score(None)                                  # the scoring unit's first launch is not what is timed
    for mode, label in ((-1, "host"), (1, "device")):
        s.set_option("device_ranks", mode)
        runs = s.stat("device_rank_runs")
        t0 = time.perf_counter()
        rho = s.score(IF, 3)[2]
        row[label + "_s"] = time.perf_counter() - t0
        row[label + "_rho"] = float(rho[0])
        assert s.stat("device_rank_runs") - runs == (1 if mode == 1 else 0)
    t0 = time.perf_counter()
    row["host_function_rho"] = float(pipeline.spearman_IF_models(IF, s.coords())[0])
    row["host_function_s"] = time.perf_counter() - t0
    print("ROW " + json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6000,8192,16384")
    ap.add_argument("--limit", type=float, default=600.0, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_score_large.md"))
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    lines = ["# c3d_score_replicas on large maps: IF ranks from the host and from the device", "",
             "`python tools/score_large.py`: one call per rank source and size, wall time of the call as the caller sees it (matrix upload",
             "included), one replica, a compact coil, synthetic matrix.  Neither side had been timed at these sizes before this file; the",
             "numbers below are what one run gave, not a bound anything is held to.", "",
             "| beads | host ranks (device_ranks -1), s | device ranks (device_ranks 1), s | rho device - rho host ranks | rho device - host function | host function, s |",
             "|---|---|---|---|---|---|"]
    for n in (int(v) for v in a.sizes.split(",")):
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n)], capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            lines.append(f"| {n} | not finished within {a.limit:.0f} s; nothing larger was started | | | | |")
            print(lines[-1], flush=True)
            break                                   # after a time limit nothing more is started on the device
        rows = [l for l in out.stdout.splitlines() if l.startswith("ROW ")]
        if out.returncode != 0 or not rows:
            lines.append(f"| {n} | failed (exit status {out.returncode}); nothing larger was started | | | | |")
            print(lines[-1], out.stderr[-2000:], flush=True)
            break                                   # after a failing child nothing more is started on the device
        r = json.loads(rows[0][4:])
        lines.append(f"| {n} | {r['host_s']:.3f} | {r['device_s']:.3f} | {r['device_rho'] - r['host_rho']:.3g} | "
                     f"{r['device_rho'] - r['host_function_rho']:.3g} | {r['host_function_s']:.3f} |")
        print(lines[-1], flush=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
