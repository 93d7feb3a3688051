#!/usr/bin/env python3
"""c3d_loops on the device beside the numpy restatement on the host: times, the kernel split and the gaps.

    python tools/loops.py [--out profiles/r33_loops.md] [--skip-large | --large-only]

Sizes: 455 beads x 20 models with IF and the consensus (chr1_500kb's matrix, the models its bundled model scaled and jittered; w = 5,
separations 11..200); 4096 x 20 rosettes with a planted IF (w = 10, B = 512); 16384 x 20 without IF, a list of 4096 pixels (w = 20);
16384 with IF only (w = 20, B = 512) unless --skip-large or the host lacks the memory for the matrix.  Per size: the device time of the
whole call (the entry's device_ms: HIP events around the uploads, the kernels and the read-backs; median and range of five after a warm
call) and of calls that ask for one group of outputs — `expected` alone (uploads, k_loop_band, k_loop_expected), `peaks` alone (the
same, k_loop_scan without the ratio store and the suppression and compaction kernels), `at` alone and `apa` alone on the same list — so
that a difference of two is a kernel group; the restatement's (tests/loop_ref.py) wall time for the same outputs, scaled from a sample of
pixels; the largest gaps against the restatement as fractions of the bounds of tests/test_gpu_loops.py; and for k_loop_scan the cells
walked per second."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import loop_ref as R                                                   # noqa: E402
from tests.util import SHORT, load_if, load_pdb_xyz, model_pdb                     # noqa: E402

U = 2.0 ** -53
THR = (1.75, 1.75, 1.5, 1.5)


def device_ms(call, repeats=5):
    call()
    t = [call()["device_ms"] for _ in range(repeats)]
    return float(np.median(t)), min(t), max(t)


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def inside_pixels(n, w, lo, hi):
    return sum(max(0, n - s - 2 * w) for s in range(lo, hi + 1))


def restatement(maps, n, p, w, lo, hi, px, scan_sample, masked=None):
    """wall time of the restatement scaled to the whole call, and the largest gap fractions of `at` given the device's rows"""
    masked = np.zeros(n, dtype=bool) if masked is None else masked
    s_lo, s_hi = R.band_range(n, w, lo, hi)
    t0 = time.perf_counter()
    E = [R.expected(k, src, n, masked, s_lo, s_hi) for k, src in maps[:2]]
    t_e = (time.perf_counter() - t0) * len(maps) / len(E)
    t_scan = 0.0
    if maps[0][0] == "if" and scan_sample:
        t0 = time.perf_counter()
        rng = np.random.default_rng(1)
        s = rng.integers(lo, hi + 1, size=scan_sample)
        i = np.array([rng.integers(w, max(w + 1, n - v - w)) for v in s])
        R.pixels("if", maps[0][1], E[0], n, masked, p, w, s_lo, i, i + s)
        t_scan = (time.perf_counter() - t0) * inside_pixels(n, w, lo, hi) / scan_sample
    t0 = time.perf_counter()
    sample = px[:: max(1, len(px) // 64)]
    want = R.pixels(maps[1][0], maps[1][1], E[1], n, masked, p, w, s_lo, sample[:, 0], sample[:, 1]) if len(maps) > 1 and len(px) else None
    t_list = (time.perf_counter() - t0) * (len(px) / max(1, len(sample))) * len(maps)
    return t_e, t_scan, t_list, E, want, sample


def group_call(s, group, IF, consensus, p, w, lo, hi, use_models, px=None, max_peaks=4096):
    """One call of the C entry that asks for one group of outputs only — "expected", "peaks", "at" or "apa" (the last two on the list
    px) — so that the call launches that group's kernels and no other; returns {"device_ms"}."""
    from chromosome3d_amd import lib
    import ctypes as C
    n = s.n
    Kp = s.nrep if use_models else 0
    Q = (1 if IF is not None else 0) + Kp + (1 if consensus else 0)
    S, side = min(hi + 2 * w, n - 1) - (lo - 2 * w) + 1, 2 * w + 1
    L = len(px) if px is not None else 0
    lst = np.ascontiguousarray(px, dtype=np.int32) if L else None
    thr = np.array(THR)
    exp = np.empty((Q, S)) if group == "expected" else None
    peaks = np.empty((max_peaks, 2), np.int32) if group == "peaks" else None
    report = np.zeros(4, np.int32) if group == "peaks" else None
    at = np.empty((Q, max(L, 1), 6)) if group == "at" else None
    closed = np.empty((Q, 2), np.int32) if group == "at" else None
    apa = np.empty((Q, side, side)) if group == "apa" else None
    p2ll = np.empty(Q) if group == "apa" else None
    d = lambda x: lib.dptr(x) if x is not None else None
    i = lambda x: lib.i32ptr(x) if x is not None else None
    flags = (lib.LOOP_CONSENSUS if consensus else 0) | (0 if use_models else lib.LOOP_IF_ONLY)
    ms = C.c_double()
    lib.check(s._L.c3d_loops(s._h, d(IF), None, 0, None, 0, flags, None, p, w, lo, hi, lib.dptr(thr), 0.0, min(2, w), min(3, w), i(lst), L, max_peaks,
                             d(exp), None, i(peaks), i(report), d(at), i(closed), d(apa), d(p2ll), C.byref(ms)))
    return {"device_ms": ms.value}


def measure(s, rows, name, IF, models, consensus, p, w, lo, hi, pixels=None, scan_sample=64, use_models=True):
    n = s.n
    call = lambda: s.loops(IF, None, None, consensus, None, p, w, lo, hi, pixels=pixels, max_peaks=4096, models=use_models)
    group = lambda g, px=None: group_call(s, g, IF, consensus, p, w, lo, hi, use_models, px)
    whole = device_ms(call)
    got = call()
    px = np.asarray(got.get("pixels", np.zeros((0, 2), np.int32)), dtype=np.int64).reshape(-1, 2)
    t_exp = device_ms(lambda: group("expected"))
    t_peaks = device_ms(lambda: group("peaks")) if IF is not None else None
    t_at = device_ms(lambda: group("at", px)) if len(px) else None
    t_apa = device_ms(lambda: group("apa", px)) if len(px) else None
    maps = ([("if", IF)] if IF is not None else []) + ([("model", m) for m in models[:1]] if use_models else [])
    Q = len(got["maps"])
    t_e, t_scan, t_list, E, want, sample = restatement(maps + maps[:1] if len(maps) == 1 else maps, n, p, w, lo, hi, px, scan_sample if IF is not None else 0)
    gap_e = max(float(np.max(np.abs(got["expected"][q][E[q] != 0] - E[q][E[q] != 0]) / E[q][E[q] != 0])) / ((n + 2) * U) for q in range(min(len(maps), 2)))
    gap_at = float("nan")
    if want is not None and use_models and len(px):
        q = 1 if IF is not None else 0
        k = np.arange(len(px))[:: max(1, len(px) // 64)]
        ok = ~np.isnan(want[:, 2:])
        if ok.any():
            gap_at = float(np.max(np.abs(got["at"][q][k][:, 2:][ok] - want[:, 2:][ok]) / np.abs(want[:, 2:][ok]))) / ((2 * (2 * w + 1) ** 2 + 2 * (n + 2) + 4) * U)
    rate = ""
    if t_peaks is not None:
        cells = inside_pixels(n, w, lo, hi) * (2 * w + 1) ** 2
        rate = f"{cells / ((t_peaks[0] - t_exp[0]) * 1e-3):.3g}"
    ref = t_e * Q / max(1, len(maps)) + t_scan + t_list * Q / max(1, len(maps))
    cell = lambda t: fmt(t) if t is not None else "-"
    rows.append(f"| {name} | {Q} | {len(px)} | {fmt(whole)} | {fmt(t_exp)} | {cell(t_peaks)} | {cell(t_at)} | {cell(t_apa)} | {rate or '-'} | "
                f"{ref:.1f} (E {t_e:.2f}, scan {t_scan:.1f}, list {t_list:.2f}) | {gap_e:.3f} | {gap_at:.3f} |")
    print(rows[-1], flush=True)
    if IF is not None:
        print(f"  {got['candidates']} candidates, {got['found']} peaks; closed:", got["closed"].tolist()[:4] if "closed" in got else "-", flush=True)


def rosettes(s, n, K, petal):
    from chromosome3d_amd import default_model, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, np.array([1, 1, n // 2 + 1], np.int32), np.array([11, n, n], np.int32), np.array([100, 457, 300], np.int32))
    s.init_replicas(K, 82364, 0)
    s.set_coords(np.stack([R.planted_rosette(n, petal, r).astype(np.float32) for r in range(K)]))
    return [m.astype(np.float64) for m in s.coords()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_loops.md"))
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--large-only", action="store_true", help="only the 16384 x IF case (2 GiB of matrix and as much again while it is built)")
    a = ap.parse_args()
    from chromosome3d_amd import Solver, default_model, make_stages
    rows = ["# c3d_loops: device against the numpy restatement on the host (tools/loops.py)",
            "",
            "Times are the entry's device_ms (HIP events around the uploads, the kernels and the read-backs), median (range) of five after a",
            "warm call, in ms.  whole: every output but `ratio`, the list taken from the peaks where there is IF.  expected / peaks / at / apa:",
            "calls that ask for that group alone (each includes the uploads, k_loop_band and k_loop_expected; `peaks` adds k_loop_scan without",
            "the ratio store and the four suppression and compaction kernels and the host's look at the report; `at` adds k_loop_list and",
            "k_loop_closed, `apa` k_loop_apa and k_loop_p2ll), so the difference to `expected` is that kernel group.  cells/s: the inside",
            "pixels x (2w+1)^2 cells over (peaks - expected), a lower bound for k_loop_scan alone.  restatement: tests/loop_ref.py (numpy, one",
            "host thread) for the same outputs, in seconds, scaled from a sample of 64 pixels and two maps.  gaps: the largest relative gap of",
            "`expected` and of the ratios in `at` as fractions of the bounds of tests/test_gpu_loops.py.  Not profiled: LDS bank conflicts and",
            "occupancy of k_loop_scan (43 KiB of LDS a workgroup: 3 workgroups a CU), the idle lanes of tiles that straddle the band's edges.",
            "",
            "| case | maps | listed | whole | expected | peaks | at | apa | scan cells/s | restatement (s) | E gap / bound | at gap / bound |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    try:
        if a.large_only:
            measure_if_alone(s, rows, rosettes(s, 16384, 1, 48))
        else:
            measure_sizes(s, rows, a.skip_large)
    finally:
        s.close()
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows) + "\n")
    print("wrote", a.out)
    return 0


def measure_if_alone(s, rows, models):
    n = 16384
    try:
        IF = R.planted_map(n, [(1000 + 151 * k, 1000 + 151 * k + 45 + (13 * k) % 500) for k in range(100)])
        measure(s, rows, "16384, IF only, w = 20, B = 512", IF, models, False, 5, 20, 41, 552, use_models=False)
    except MemoryError:
        rows.append("| 16384, IF only, w = 20, B = 512 | the host has no memory for the matrix | | | | | | | | | | |")


def measure_sizes(s, rows, skip_large):
    from chromosome3d_amd import default_model, make_stages
    K = 20
    cid = "chr1_500kb"
    IF, bundled = load_if(cid), load_pdb_xyz(model_pdb(cid))
    n = len(IF)
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_if_matrix(IF)
    s.init_replicas(K)
    rng = np.random.default_rng(n)
    s.set_coords(np.stack([(bundled * (1.0 + 0.01 * (r + 1)) + rng.normal(scale=0.05, size=bundled.shape)).astype(np.float32) for r in range(K)]))
    models = [m.astype(np.float64) for m in s.coords()]
    measure(s, rows, "455 x 20 + IF + consensus, w = 5, separations 11..200", IF, models, True, 2, 5, 11, 200)
    n = 4096
    models = rosettes(s, n, K, 48)
    IF = R.planted_map(n, [(100 + 37 * k, 100 + 37 * k + 25 + (11 * k) % 480) for k in range(100)])
    measure(s, rows, "4096 x 20 + IF + consensus, w = 10, B = 512", IF, models, True, 3, 10, 21, 532)
    n = 16384
    models = rosettes(s, n, K, 48)
    rng = np.random.default_rng(5)
    sep = rng.integers(41, 553, size=4096)
    i = np.array([rng.integers(20, n - v - 20) for v in sep])
    measure(s, rows, "16384 x 20 + consensus, no IF, w = 20, a list of 4096", None, models, True, 5, 20, 41, 552, np.stack([i, i + sep], axis=1).astype(np.int32))
    if not skip_large:
        measure_if_alone(s, rows, models)


if __name__ == "__main__":
    sys.exit(main())
