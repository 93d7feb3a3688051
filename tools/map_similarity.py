#!/usr/bin/env python3
"""c3d_map_similarity on the device beside the numpy restatement on the host: times, the kernel split and the gaps.

    python tools/map_similarity.py [--out profiles/r35_map_similarity.md] [--cases 0,1,2]

Cases: 455 bins x 2 maps (chr1_500kb and a noisy copy), h = 0..5, all strata; 4096 x 4 synthetic maps, separations 1..500, h = 3;
16384 x 2, separations 1..2000, h = 5 (synthetic: a decay with the separation times b b^T times a symmetric noise).  Per case: the
device time of a call (the entry's device_ms: HIP events around the kernels of every half-width, the upload, the check and the read-backs
excluded; median and range of the repeats after a warm call); the kernel split from two calls that differ in the number of maps — a call
of Q maps costs Q a + Q (Q - 1) / 2 b, a the smoothing of one map (its share of the band's memset included), b the strata of one pair —
solved from the call of the case and a call of 3 maps (of 2 where the case has more); the rate at which the smoothing kernel reads the
band — 8 bytes a cell with lo - h <= j - i <= hi + h, once, over a / n_h — as a share of the 4.65 TB/s profiles/r32_balance.md measured
for a streaming pass over a matrix; the wall time of the restatement tests/mapsim_ref.py on the same host (beyond 455 bins scaled from a
sample of strata, and the table says so); and the gaps on the sampled strata: `smoothed` values that differ in a bit, `counts` that differ,
the largest |moment - restatement| over sqrt(Cxx Cyy), the largest |scc - restatement| where every stratum was restated."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import mapsim_ref as R                                                  # noqa: E402

STREAM = 4.65e12                                                                   # bytes per second: k_bal_marginals at 16384 beads (profiles/r32_balance.md)
CASES = [(455, 2, tuple(range(6)), 0, 0), (4096, 4, (3,), 1, 500), (16384, 2, (5,), 1, 2000)]


def make_maps(n, Q):
    rng = np.random.default_rng(n)
    if n == 455:
        S = np.loadtxt(os.path.join(ROOT, "tests", "golden", "all45", "txt", "chr1_500kb_matrix.txt"))
        out = [S]
        for _ in range(Q - 1):
            noise = np.triu(np.exp(rng.normal(0.0, 0.3, S.shape)))
            out.append(S * (noise + np.triu(noise, 1).T))
        return np.stack(out)
    decay = 1.0 / (1.0 + np.arange(n)) ** 0.9 + 1e-3
    both = np.concatenate((decay[:0:-1], decay))
    toeplitz = np.lib.stride_tricks.as_strided(both[n - 1:], shape=(n, n), strides=(-both.strides[0], both.strides[0]))
    maps = np.empty((Q, n, n))
    for m in range(Q):
        b = np.exp(rng.normal(0.0, 0.3, n))
        np.multiply.outer(b, b, out=maps[m])                                        # b_i b_j first: symmetric bit for bit
        maps[m] *= toeplitz
        for d in range(0, min(n, 2100), 7):                                         # a symmetric ripple on some diagonals, so that the maps differ in more than b
            v = 1.0 + 0.2 * rng.random(n - d)
            i = np.arange(n - d)
            maps[m, i, i + d] *= v
            if d:
                maps[m, i + d, i] = maps[m, i, i + d]
    return maps


def device_ms(s, maps, h, lo, hi, repeats):
    call = lambda: s.map_similarity(maps, h, lo, hi)["device_ms"]
    call()
    t = [call() for _ in range(repeats)]
    return float(np.median(t)), min(t), max(t)


def measure(s, case, rows, raw):
    n, Q, hs, lo, hi = case
    top = hi if hi else n - 1
    S = top - lo + 1
    Q2 = 3 if Q == 2 else 2
    maps = make_maps(n, max(Q, Q2))
    repeats = 5 if n <= 4096 else 2
    t1 = device_ms(s, maps[:Q], hs, lo, hi, repeats)
    t2 = device_ms(s, maps[:Q2], hs, lo, hi, repeats)
    p1, p2 = Q * (Q - 1) / 2, Q2 * (Q2 - 1) / 2
    det = Q * p2 - Q2 * p1
    a = (t1[0] * p2 - t2[0] * p1) / det                                             # ms: smoothing, one map, all half-widths
    b = (Q * t2[0] - Q2 * t1[0]) / det                                              # ms: strata, one pair, all half-widths
    raw.append(f"n {n} maps {Q}: device_ms {t1}; maps {Q2}: device_ms {t2}; smoothing a map {a:.4f} ms, strata a pair {b:.4f} ms")
    rates = []
    for hk in hs:
        cells = sum(n - abs(d) for d in range(lo - hk, top + hk + 1) if abs(d) < n)
        rates.append(8.0 * cells / (a / len(hs) * 1e-3))
    rate = float(np.mean(rates))
    # the restatement on the same host: every stratum at 455, a sample beyond, scaled
    sample = list(range(lo, top + 1)) if n <= 455 else sorted(set(np.linspace(lo, top, 6).astype(int)))
    got = s.map_similarity(maps[:Q], hs, lo, hi, want_smoothed=True)
    t0 = time.perf_counter()
    bits = cnt_diff = 0
    gap_m = 0.0
    for k, hk in enumerate(hs):
        for sep in sample:
            want = [R.smooth_stratum(maps[m], hk, sep) for m in range(Q)]
            for m in range(Q):
                bits += int((want[m].view(np.uint64) != got["smoothed"][k, m, sep - lo, :n - sep].view(np.uint64)).sum())
            for e, (p, q) in enumerate(R.pairs(Q)):
                mo, co = R.stratum(want[p], want[q])
                cnt_diff += int(tuple(int(v) for v in got["counts"][k, e, sep - lo]) != co)
                scale = np.sqrt(mo[1] * mo[2])
                if scale > 0:
                    gap_m = max(gap_m, float(np.abs(got["moments"][k, e, sep - lo] - mo).max() / scale))
    t_host = (time.perf_counter() - t0) * (S / len(sample))
    gap_scc = None
    if len(sample) == S:
        want = R.map_similarity(maps[:Q], hs, lo, hi)
        gap_scc = float(np.nanmax(np.abs(want["scc"] - got["scc"])))
    raw.append(f"n {n}: restatement {t_host:.2f} s ({'all' if len(sample) == S else 'scaled from %d of %d' % (len(sample), S)} strata); smoothed values differing {bits}, "
               f"counts differing {cnt_diff}, moments gap {gap_m:.3g}, scc gap {gap_scc}; scc {got['scc'][-1, 0, 1]:.6f}")
    split = a > 0 and b > 0                                                         # a small call is bound by its launches, not by Q: no split to report
    rows.append(f"| {n} x {Q} | {','.join(str(v) for v in hs)} | {lo}..{top} | {t1[0]:.3f} ({t1[1]:.3f} .. {t1[2]:.3f}) | {'%.3f' % (Q * a) if split else 'not separable'} | "
                f"{'%.3f' % (p1 * b) if split else 'not separable'} | {'%.2f (%.0f %%)' % (rate / 1e12, 100.0 * rate / STREAM) if split else 'n/a'} | {t_host:.1f}{'' if len(sample) == S else ' (scaled from %d strata)' % len(sample)} | {bits} | {cnt_diff} | {gap_m:.1e} | "
                f"{'%.1e' % gap_scc if gap_scc is not None else 'not restated'} |")
    print(raw[-2], raw[-1], rows[-1], sep="\n", flush=True)
    return bits != 0 or cnt_diff != 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_map_similarity.md"))
    ap.add_argument("--cases", default="0,1,2")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    rows = ["# c3d_map_similarity: device against the numpy restatement on the host (tools/map_similarity.py)",
            "",
            "call: the entry's device_ms (HIP events around the kernels of every half-width; the upload of the maps, the check and the read-backs are",
            "not in it); median (range) of the repeats after a warm call.  smoothing, strata: the split of that time from a second call with another",
            "number of maps (a call of Q maps costs Q a + Q (Q - 1) / 2 b), the band's memset counted with the smoothing.  band read: 8 bytes a cell",
            "with lo - h <= j - i <= hi + h, once, over the smoothing time of a map and half-width, as a share of the 4.65 TB/s profiles/r32_balance.md",
            "measured for a streaming pass; the tiles' halos are read on top of that and are not counted.  restatement: tests/mapsim_ref.py on the same",
            "host, every stratum at 455 bins and a sample scaled to all beyond.  differing: `smoothed` values that differ in a bit and `counts` triples that",
            "differ on the restated strata; moments gap: the largest |moment - restatement| / sqrt(Cxx Cyy).  not separable: the second call did not cost",
            "more per map and pair (a call of a few hundred bins is bound by its launches).  No ratio was fixed in advance and none is claimed: the host",
            "column is the restatement, not a competitor.",
            "",
            "| bins x maps | h | separations | call (ms) | smoothing (ms) | strata (ms) | band read (TB/s, of 4.65) | restatement (s) | smoothed differing | counts differing | moments gap | scc gap |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    raw = []
    s = Solver(0)
    s.set_option("max_beads", 16384)
    bad = False
    try:
        for c in (int(v) for v in a.cases.split(",")):
            bad = measure(s, CASES[c], rows, raw) or bad
    finally:
        s.close()
    rows += ["", "A smoothed value or a count that differs: " + ("yes, see the table." if bad else "none."), ""]
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows))
    with open(os.path.splitext(a.out)[0] + "_raw.txt", "w") as fh:
        fh.write("\n".join(raw) + "\n")
    print("wrote", a.out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
