#!/usr/bin/env python3
"""Step time of the fp32 per-step path on large maps: the staged form against the chunked form (option column_chunk) where both run,
and the chunked form up to 16384 beads.  One child process per size (a fresh context and a fresh code-object load each), device-event
timing (c3d_last_timing: the event pair around c3d_run_steps), a warm-up that captures the graphs, then at least 200 timed steps.

    python tools/large_maps.py [--sizes 4096,5120,8192,12288,16384] [--chunks 0,256,1024,2048] [--replicas 8] [--steps 200]
                               [--warmup 30] [--whole 8192] [--json OUT] [--precision 32]

--precision 64 measures the fp64 step instead (k64_step against k64_step_chunked, option f64_column_chunk: chunks 0, 256, 512, 1024;
chunk 0 is the staged kernel up to 2560 beads and is left out beyond).

Prints one line per (n, chunk, kind) and, with --whole N, the time of the library's default schedule at N x replicas.  Chunk 0 is the
library's choice (staged up to 5120 beads, chunked beyond): at sizes beyond 5120 it is left out, its kernel is one of the others.
The matrix is a config-5 style synthetic one (every pair restrained; the step's cost does not depend on the targets' values)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIRE = (2, 0, 0.0, 1.0, 20.0, 0.5, 0.0)
MD = (0, 0, 0.003, 0.4, 0.003, 0.9, 2000.0)


def synthetic(n, seed=20161015, K=11.0):
    """IF = (K / d)^2 of a confined random walk, computed in row blocks (no noise: the step's cost does not depend on it)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = np.cumsum(3.8 * d, axis=0)
    x = x / np.abs(x).max() * 2.2 * n ** (1.0 / 3.0) * 2.0          # squeezed into the confinement radius of tests.util.synthetic_if
    IF = np.empty((n, n))
    for a in range(0, n, 512):
        r = np.linalg.norm(x[a:a + 512, None, :] - x[None, :, :], axis=-1)
        r[r < 1.0] = 1.0
        IF[a:a + 512] = (K / r) ** 2
    np.fill_diagonal(IF, 10.0 * IF.max(axis=1))
    return IF


def child(n, chunks, nrep, steps, warmup, whole, precision=32):
    from chromosome3d_amd import Solver, default_model, default_schedule, make_stages
    s = Solver(0)
    s.set_option("max_beads", max(n, 5120))
    chunk_option = "column_chunk"
    if precision == 64:
        s.set_option("precision", 64)
        s.set_option("f64_max_beads", max(n, 2560))
        chunk_option = "f64_column_chunk"
    s.set_model(default_model())
    IF = synthetic(n)
    s.set_if_matrix(IF)
    del IF
    out = []
    for chunk in chunks:
        s.set_option(chunk_option, chunk)
        for label, st in (("FIRE", FIRE), ("MD", MD)):
            row = list(st)
            row[1] = warmup + steps
            s.set_schedule(make_stages([tuple(row)]))
            s.init_replicas(nrep, 82364, 0)
            s.run_steps(warmup)
            s.run_steps(steps)
            ms, done, launches = s.last_timing()
            out.append(dict(n=n, chunk=chunk, kind=label, replicas=nrep, steps=done, us_per_step=1000.0 * ms / done,
                            kernel=s.step_kernel_name, pair_terms_per_us=nrep * n * n / (1000.0 * ms / done)))
            print(json.dumps(out[-1]), flush=True)
    if whole:
        s.set_option(chunk_option, 0)
        sched = default_schedule(3000)
        s.set_schedule(sched, None, 0.0, 250)
        s.init_replicas(nrep, 82364, 0)
        s.run()
        ms, done, launches = s.last_timing()
        out.append(dict(n=n, chunk=0, kind="default schedule", replicas=nrep, steps=done, ms=ms, us_per_step=1000.0 * ms / done,
                        kernel=s.step_kernel_name))
        print(json.dumps(out[-1]), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="4096,5120,8192,12288,16384")
    ap.add_argument("--chunks", default="0,256,1024,2048")
    ap.add_argument("--replicas", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--whole", type=int, default=0, help="also run the default schedule at this size")
    ap.add_argument("--precision", type=int, default=32, choices=(32, 64))
    ap.add_argument("--json")
    ap.add_argument("--child", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(",")]
    if a.child:
        child(a.child, chunks, a.replicas, max(a.steps, 200), a.warmup, a.whole == a.child, a.precision)
        return 0
    rows = []
    for n in (int(v) for v in a.sizes.split(",")):
        cs = [c for c in chunks if c != 0 or n <= (5120 if a.precision == 32 else 2560)]
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--chunks", ",".join(map(str, cs)), "--replicas",
               str(a.replicas), "--steps", str(a.steps), "--warmup", str(a.warmup), "--whole", str(a.whole), "--precision", str(a.precision)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                rows.append(json.loads(line))
                r = rows[-1]
                print("n %5d  chunk %4d  %-16s %8.1f us/step  %7.0f pair terms/us  %s" % (r["n"], r["chunk"], r["kind"], r["us_per_step"],
                      r.get("pair_terms_per_us", 0.0), r["kernel"]), flush=True)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-3000:])
            print("child for n = %d failed: %d" % (n, p.returncode))
            return p.returncode
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
