#!/usr/bin/env python3
"""c3d_insulation on the device beside the numpy restatement on the host: times, the kernel split, the staged form against the recompute
form, and the gaps.

    python tools/insulation.py [--out profiles/r31_insulation.md] [--skip-large]

Sizes: 455 beads x 20 models with IF and the consensus (22 maps; chr1_500kb's matrix, the models its bundled model scaled and jittered)
with windows {5, 10, 25}, and 16384 beads x 20 planted models with windows {8, 32, 128}.  Per size: the device time of the call (the
entry's device_ms: HIP events around the uploads, the kernels and the read-backs; median and range of five after a warm call); the kernel
split from calls that differ by one kernel — models alone against models and consensus (k_ins_band and the consensus' squares), one
window against the list (k_ins_squares' walk); the restatement's (tests/insulation_ref.py) wall time on the same maps, scaled from a
sample of the beads beyond 455; and the largest gaps of mean and score against the restatement beside the bounds of
tests/test_gpu_insulation.py.  Then the staged form (C3D_INSULATION_STAGE) against plain recomputation at w_max = 8, 32 and 128 on
2048 beads x 20 models, models only: the difference is k_ins_squares alone."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import insulation_ref as R                                             # noqa: E402
from tests.util import SHORT, load_if, load_pdb_xyz, model_pdb                     # noqa: E402

U = 2.0 ** -53


def device_ms(call, repeats=5):
    call()
    t = [call()["device_ms"] for _ in range(repeats)]
    return float(np.median(t)), min(t), max(t)


def fmt(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def gaps(got, maps, n, windows, beads=None):
    """largest |mean gap| / bound and |score gap| / bound over the maps; the restatement's wall time"""
    t0 = time.perf_counter()
    worst_mean = worst_score = 0.0
    for q, (kind, src) in enumerate(maps):
        Kp = len(src) if kind == "consensus" else 0
        for k, w in enumerate(windows):
            wm = R.mean_row(kind, src, n, w, None, beads)
            ok = ~np.isnan(wm) & (wm > 0)
            worst_mean = max(worst_mean, float((np.abs(got["mean"][q, k][ok] - wm[ok]) / wm[ok]).max() / ((w * w + Kp + 2) * U)))
            ws = R.score_row(got["mean"][q, k] if beads is not None else wm)
            S = (2 * w * w + Kp + n + 8) * U / np.log(2.0) + 2.0 * U * np.abs(np.nan_to_num(ws))
            v = ~np.isnan(ws)
            worst_score = max(worst_score, float((np.abs(got["score"][q, k][v] - ws[v]) / S[v]).max()))
    return worst_mean, worst_score, time.perf_counter() - t0


def measure_455(s, rows):
    from chromosome3d_amd import default_model, make_stages
    cid, K, windows = "chr1_500kb", 20, [5, 10, 25]
    IF, bundled = load_if(cid), load_pdb_xyz(model_pdb(cid))
    n = len(IF)
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_if_matrix(IF)
    s.init_replicas(K)
    rng = np.random.default_rng(n)
    s.set_coords(np.stack([(bundled * (1.0 + 0.01 * (r + 1)) + rng.normal(scale=0.05, size=bundled.shape)).astype(np.float32) for r in range(K)]))
    models = [m.astype(np.float64) for m in s.coords()]
    full = device_ms(lambda: s.insulation(IF, None, None, True, windows))
    no_cons = device_ms(lambda: s.insulation(IF, None, None, False, windows))
    one = device_ms(lambda: s.insulation(IF, None, None, True, windows[:1]))
    got = s.insulation(IF, None, None, True, windows)
    maps = [("if", IF)] + [("model", m) for m in models] + [("consensus", models)]
    gm, gs, t_ref = gaps(got, maps, n, windows)
    rows.append(f"| 455 x 20 + IF + consensus, windows 5,10,25 | {fmt(full)} | {fmt(no_cons)} | {fmt(one)} | {t_ref:.1f} | {gm:.3f} | {gs:.3f} |")
    print(rows[-1], flush=True)
    print("fit_r of the models (window 10):", np.round(got["fit_r"][:-1, 1], 3), flush=True)


def planted_set(s, n, K):
    from chromosome3d_amd import default_model, make_stages
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, np.array([1, 1, n // 2 + 1], np.int32), np.array([11, n, n], np.int32), np.array([100, 457, 300], np.int32))
    s.init_replicas(K, 82364, 0)
    s.set_coords(np.stack([R.planted_domains(n, 64, r).astype(np.float32) for r in range(K)]))
    return [m.astype(np.float64) for m in s.coords()]


def measure_large(s, rows):
    n, K, windows = 16384, 20, [8, 32, 128]
    models = planted_set(s, n, K)
    IF = None                                                                   # (a 2 GiB matrix of which the call reads a band: left out of the timing run)
    full = device_ms(lambda: s.insulation(IF, None, None, True, windows))
    no_cons = device_ms(lambda: s.insulation(IF, None, None, False, windows))
    one = device_ms(lambda: s.insulation(IF, None, None, True, windows[:1]))
    got = s.insulation(IF, None, None, True, windows)
    beads = list(range(0, n, 509)) + [127, 128, n - 129, n - 128]
    maps = [("model", models[0]), ("model", models[K - 1])]
    sub = {k: got[k][[0, K - 1]] for k in ("mean", "score")}
    gm, gs, t_ref = gaps(sub, maps, n, windows, beads)
    inside = sum(1 for b in beads if 128 <= b <= n - 129)
    scaled = t_ref * (n / max(inside, 1)) * (K + 1) / 2.0
    rows.append(f"| 16384 x 20 + consensus, windows 8,32,128 | {fmt(full)} | {fmt(no_cons)} | {fmt(one)} | {scaled:.0f} (scaled from {len(beads)} beads of 2 maps) | {gm:.3f} | {gs:.3f} |")
    print(rows[-1], flush=True)


def measure_forms(s, rows):
    n, K = 2048, 20
    planted_set(s, n, K)
    for wmax in (8, 32, 128):
        windows = [wmax]
        recompute = device_ms(lambda: s.insulation(None, None, None, False, windows))
        if wmax <= 40:
            staged = device_ms(lambda: s.insulation(None, None, None, False, windows, None, 0.0, 1, True))
            a, b = s.insulation(None, None, None, False, windows), s.insulation(None, None, None, False, windows, None, 0.0, 1, True)
            same = all(a[k].tobytes() == b[k].tobytes() for k in ("mean", "score", "boundary", "strength"))
            keep = "staged" if staged[0] <= recompute[0] else "recompute"
            rows.append(f"| {wmax} | {fmt(staged)} | {fmt(recompute)} | {keep} is faster; the library's default is recompute | {'equal' if same else 'DIFFERENT'} |")
        else:
            rows.append(f"| {wmax} | does not fit the 64 KiB a launch gets ({8 * (31 + wmax) ** 2} bytes) | {fmt(recompute)} | recompute, the only form | - |")
        print(rows[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_insulation.md"))
    ap.add_argument("--skip-large", action="store_true")
    a = ap.parse_args()
    from chromosome3d_amd import Solver
    rows = ["# c3d_insulation: device against the numpy restatement on the host (tools/insulation.py)",
            "",
            "call: the entry's device_ms (HIP events around the uploads, the kernels and the read-backs), median (range) of five after a warm",
            "call, in ms.  The kernel split comes from calls that differ by one kernel: without the consensus (no k_ins_band, one map fewer for",
            "k_ins_squares), and with the first window alone (k_ins_squares walks w_1^2 cells a bead instead of w_max^2; the small kernels",
            "shrink with the rows).  restatement: tests/insulation_ref.py on the same maps, numpy on the host — the loop the call replaces.",
            "gaps: the largest |device - restatement| of mean and score as a fraction of the bounds of tests/test_gpu_insulation.py",
            "((w^2 + Kp + 2) u relative, ((2 w^2 + Kp + n + 8) u) / ln 2 + 2 u |score| absolute).  No ratio is claimed.  Not profiled: LDS bank",
            "conflicts of the staged walk, the occupancy of the staged form (2 or 3 workgroups a CU at 50 - 64 KiB of LDS), the idle threads of",
            "a walk over fewer than 256 cells (w < 16).",
            "",
            "| case | call | without consensus | first window alone | restatement (s) | mean gap / bound | score gap / bound |",
            "|---|---|---|---|---|---|---|"]
    forms = ["", "## The staged form against plain recomputation (2048 beads x 20 models, models only, one window = w_max)", "",
             "| w_max | staged (ms) | recompute (ms) | kept | bytes |", "|---|---|---|---|---|"]
    s = Solver(0)
    s.set_option("max_beads", 16384)
    try:
        measure_455(s, rows)
        if not a.skip_large:
            measure_large(s, rows)
        measure_forms(s, forms)
    finally:
        s.close()
    with open(a.out, "w") as fh:
        fh.write("\n".join(rows + forms) + "\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
