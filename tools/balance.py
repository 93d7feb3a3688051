#!/usr/bin/env python3
"""c3d_balance_matrix on the device beside the numpy restatement on the host: times, the time per round, the rate at which a round reads
the matrix, and the largest gaps.

    python tools/balance.py [--out profiles/r32_balance.md] [--sizes 455,2048,5792,8192,16384]

Sizes: 455 beads (chr1_500kb turned into biased counts with one unmappable bin, the worked example of tests/test_balance_ref.py) and
2048, 5792, 8192 and 16384 beads of a synthetic matrix (a decay with the separation times b b^T).  5792 is the largest size whose
padded copy (8 n np bytes) fits the 256 MiB Infinity Cache.  Per size: the device time of a call (the entry's device_ms: HIP events from
the first count of non-zeros to the last kernel, uploads and read-backs excluded; median and range of the repeats after a warm call) at
two numbers of rounds with tol 0, the time per round from their difference, the bytes of the padded matrix over that time beside the
6.3 TB/s a streaming read achieves from HBM (profiles/r02_hbm_stream_microbench.txt measured 6.47), device_ms / (T + 1) of the longer call (which carries the mask's passes too), the wall
time of one round of the restatement (tests/balance_ref.py: a matrix-vector product and the update in numpy) on the host, and the largest
relative gap of the weights after two rounds against the restatement beside the tests' bound 2 (4n + 12) 2^-53."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import balance_ref as R                                                 # noqa: E402

ACHIEVABLE = 6.3e12                                                                # bytes per second a streaming read achieves from HBM on an MI355X
U = 2.0 ** -53


def matrix(n):
    if n == 455:
        S = np.loadtxt(os.path.join(ROOT, "tests", "golden", "all45", "txt", "chr1_500kb_matrix.txt"))
        return R.worked_example(S, seed=1)[0]
    rng = np.random.default_rng(n)
    b = np.exp(rng.normal(0.0, 0.3, n))
    decay = 1.0 / (1.0 + np.arange(n)) ** 0.9 + 1e-3
    both = np.concatenate((decay[:0:-1], decay))
    toeplitz = np.lib.stride_tricks.as_strided(both[n - 1:], shape=(n, n), strides=(-both.strides[0], both.strides[0]))
    M = np.multiply.outer(b, b)                                                     # b_i b_j first: symmetric bit for bit
    M *= toeplitz
    return M


def device_ms(s, M, rounds, repeats):
    call = lambda: s.balance(M, "ice", ignore_diags=2, min_nnz=1, tol=0.0, max_iters=rounds, want_matrix=False)["device_ms"]
    call()
    t = [call() for _ in range(repeats)]
    return float(np.median(t)), min(t), max(t)


def host_round(M, repeats=3):
    """one round as the restatement makes it: s = w (A' w), mbar, r, var, w / r"""
    A = R.seen_by_marginals(M, 2)
    kept = (A > 0).any(axis=1)
    k = float(kept.sum())
    w = kept.astype(np.float64)
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        s = w * (A @ w)
        mbar = s[kept].sum() / k
        r = s[kept] / mbar
        var = ((r - 1) ** 2).sum() / k
        w[kept] = w[kept] / r
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), var


def measure(s, n, rows):
    M = matrix(n)
    np_ = (n + 1) & ~1
    few, many = 10, 110
    repeats = 5 if n <= 8192 else 3
    a, b = device_ms(s, M, few, repeats), device_ms(s, M, many, repeats)
    per_round = (b[0] - a[0]) / (many - few)                                        # ms
    rate = 8.0 * n * np_ / (per_round * 1e-3)
    t_host, _ = host_round(M)
    got = s.balance(M, "ice", ignore_diags=2, min_nnz=1, tol=0.0, max_iters=2, want_matrix=False)
    want = R.balance(M, "ice", ignore_diags=2, min_nnz=1, tol=0.0, max_iters=2, want_matrix=False)
    kept = want["masked"] == 0
    same_mask = bool(np.array_equal(got["masked"], want["masked"]))
    gap = float(np.abs(got["weights"][kept] / want["weights"][kept] - 1).max())
    bound = 2 * (4 * n + 12) * U
    rows.append(f"| {n} | {8.0 * n * np_ / 2 ** 20:.0f} | {a[0]:.3f} ({a[1]:.3f} .. {a[2]:.3f}) | {b[0]:.3f} ({b[1]:.3f} .. {b[2]:.3f}) | {1e3 * per_round:.1f} | "
                f"{rate / 1e12:.2f} ({100.0 * rate / ACHIEVABLE:.0f} %) | {1e3 * b[0] / (many + 1):.1f} | {1e3 * t_host:.1f} | {'equal' if same_mask else 'DIFFERENT'} | "
                f"{gap:.1e} | {gap / bound:.2g} |")
    print(rows[-1], flush=True)
    return gap > bound or not same_mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_balance.md"))
    ap.add_argument("--sizes", default="455,2048,5792,8192,16384")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    rows = ["# c3d_balance_matrix: device against the numpy restatement on the host (tools/balance.py)",
            "",
            "call: the entry's device_ms (HIP events from the first count of non-zeros to the last kernel: the mask's passes and the rounds,",
            "with the host's looks at the round record every 16 rounds; the upload of the matrix and the read-backs are not in it), ICE with",
            "tol 0, ignore_diags 2, no `balanced`; median (range) of the repeats after a warm call, at 10 and at 110 updates.  round: the",
            "difference of the two over 100: one pass of k_bal_marginals over the padded matrix and one k_bal_update.  matrix read: 8 n np bytes",
            "over that time, beside the 6.3 TB/s a streaming read achieves from HBM (profiles/r02_hbm_stream_microbench.txt: 6.47); up to 5792 beads the copy fits the 256 MiB Infinity",
            "Cache and the figure is not an HBM rate.  call / (T + 1): the longer call over its 111 passes, the mask's passes included.",
            "restatement: one round of tests/balance_ref.py on the host (numpy: a matrix-vector product and the update).  gap: the largest",
            "relative difference of the weights after two rounds against the restatement; of bound: over 2 (4n + 12) 2^-53, the tests' bound.",
            "No ratio was fixed in advance and none is claimed: the host column is the restatement, not a competitor.",
            "",
            "| beads | matrix (MiB) | call, 10 updates (ms) | call, 110 updates (ms) | round (us) | matrix read (TB/s, of 6.3) | call / (T + 1) (us) | restatement round (ms) | mask | gap | of bound |",
            "|---|---|---|---|---|---|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    bad = False
    try:
        for n in (int(v) for v in a.sizes.split(",")):
            bad = measure(s, n, rows) or bad
    finally:
        s.close()
    rows += ["", "A gap above the bound, or a mask that differs: " + ("yes, see the table." if bad else "none."), ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows))
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
