#!/usr/bin/env python3
"""The gaps tests/test_gpu_f64_boundary.py bounds, measured: c3d_eval_f64's forces and energies against the oracle at the same doubles, and
the fp64 step kernels against the restatement over the test's schedules, at the test's sizes.  Prints them and writes
profiles/r16_f64_boundary.md.

    python tools/f64_boundary.py                 the GPU measurements (the test module's own measure_* functions, so the same cases)
    python tools/f64_boundary.py --cpu-check     no GPU: the restatement against a copy of itself whose force sums run in REVERSE order
                                                 (the oracle's pair loop over the beads numbered backwards), over the same schedules:
                                                 what re-ordered sums alone do to these trajectories — the step counts are chosen so
                                                 that this stays under the 1e-8 cap
    python tools/f64_boundary.py --energy-large  also time k64_energy (one workgroup a replica) at 16384 beads, one replica
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O                                     # noqa: E402
from tests import lbfgs_ref as L                                   # noqa: E402
from tests import test_gpu_f64_boundary as B                       # noqa: E402
from tests.util import oracle_fire_from, oracle_model_from, random_coil   # noqa: E402

ACCEL, KBOLTZ = 418.4, 0.0019872


def py_schedule(force, om, fp, stages, x0, v_maxwell):
    """oracle/c3d_oracle.c's c3o_run_schedule for kinds 0, 2 and 5 (all two-point), statement by statement, around force(x, w_all, w_vdw,
    repel_s); returns (x centred, v)"""
    n = x0.shape[0]
    x, v, prev = x0.copy(), np.zeros_like(x0), -1
    for kind, nsteps, dt, w_all, w_vdw, repel_s, t_bath in stages:
        if kind in (2, 5):
            fdt, alpha, npos = fp.dt_start, fp.alpha_start, 0
            Ls = np.zeros(4)
            v[:] = 0
            for _ in range(nsteps):
                F = force(x, w_all, w_vdw, repel_s)
                if kind == 2:
                    vf, ff, vv = (v * F).sum(), (F * F).sum(), (v * v).sum()
                    if Ls[0] > 0:
                        v = (1.0 - alpha) * v + alpha * np.sqrt(Ls[2] / max(Ls[1], 1e-30)) * F
                        if npos > fp.n_min:
                            fdt, alpha = min(fdt * fp.f_inc, fp.dt_max), alpha * fp.f_alpha
                        npos += 1
                    else:
                        v[:] = 0
                        alpha, fdt, npos = fp.alpha_start, fdt * fp.f_dec, 0
                    v = v + fdt * ACCEL / om.mass * F
                    dr = fdt * v
                    d2 = (dr * dr).sum(1)
                    x = x + np.where(d2 > fp.max_step ** 2, fp.max_step / np.sqrt(np.maximum(d2, 1e-300)), 1.0)[:, None] * dr
                    Ls[:3] = vf, ff, vv
                else:
                    k, a_prev = npos, fdt
                    a = a_prev
                    if k == 0:
                        a = fp.dt_start * fp.dt_start * ACCEL / om.mass
                    elif k >= 2:
                        a = (Ls[3] / Ls[0] if k % 2 == 0 else Ls[0] / Ls[2]) if Ls[0] > 0 else 2.0 * a_prev
                        a = min(max(a, 1e-7), 1e2)
                    q = np.zeros(4)
                    if k > 0:
                        sv = a_prev * v
                        d2 = (sv * sv).sum(1)
                        sv = sv * np.where(d2 > fp.max_step ** 2, fp.max_step / np.sqrt(np.maximum(d2, 1e-300)), 1.0)[:, None]
                        y = v - F
                        q[0], q[2], q[3] = (sv * y).sum(), (y * y).sum(), (sv * sv).sum()
                    q[1] = (F * F).sum()
                    dr = a * F
                    d2 = (dr * dr).sum(1)
                    x = x + np.where(d2 > fp.max_step ** 2, fp.max_step / np.sqrt(np.maximum(d2, 1e-300)), 1.0)[:, None] * dr
                    v = F.copy()
                    fdt, npos, Ls = a, k + 1, q
        else:
            if prev in (2, 5, -1):
                v = v_maxwell.copy()
            for _ in range(nsteps):
                F = force(x, w_all, w_vdw, repel_s)
                tprev = max(om.mass * (v * v).sum() / ACCEL / (max(3 * n - 3, 1) * KBOLTZ), 1e-2)
                lam = np.sqrt(max(1.0 + dt * om.fbeta * (t_bath / tprev - 1.0), 0.0)) if kind == 0 else np.sqrt(t_bath / tprev)
                v = lam * (v - v.mean(0)) + dt * ACCEL / om.mass * F
                x = x + dt * v
        prev = kind
    return x - x.mean(0), v


def cpu_check(sizes):
    """the restatement against itself with the force's pair sums reversed: (x gap, v gap) per size and schedule, as the test forms them"""
    from chromosome3d_amd import default_fire, default_model
    m, fire = default_model(), default_fire()
    rows = []
    for n in sizes:
        om, fp = oracle_model_from(m, n), oracle_fire_from(fire)
        d10 = O.if_to_dist10(B.matrix(n))
        d10r = np.ascontiguousarray(d10[::-1, ::-1])
        fwd = lambda u, *w: O.energy_force(om, d10, u, *w)[0]
        rev = lambda u, *w: O.energy_force(om, d10r, np.ascontiguousarray(u[::-1]), *w)[0][::-1]
        x0 = B.start64(n, 1)[0]
        vm = O.init_velocities(om, 82364, 0)
        for which, sched in B.SCHEDULES.items():
            stages = [(k, c) + B.F32(*rest) for (k, c, *rest) in sched]
            if which == "lbfgs":
                w = stages[0][3:6]
                g0 = float(fire.dt_start) ** 2 * (ACCEL / float(m.mass))
                res = []
                for f in (fwd, rev):
                    xl, _ = L.lbfgs_run(lambda u: f(u, *w), x0, stages[0][1] - 1, m=5, g0=g0, max_step=float(fire.max_step))
                    xe, _ = L.lbfgs_run(lambda u: f(u, *w), x0, stages[0][1], m=5, g0=g0, max_step=float(fire.max_step))
                    res.append((xe, f(xl, *w)))
            else:
                res = [py_schedule(f, om, fp, stages, x0, vm) for f in (fwd, rev)]
                xo, vo, _ = O.run_schedule(om, d10, O.make_stages(stages), fp, 82364, 0, x0=x0)     # (and the C restatement itself)
                rows.append((n, which + " (python restatement against the oracle's)", float(np.abs(res[0][0] - xo).max()),
                             float(np.abs(res[0][1] - vo).max() / max(1.0, np.abs(vo).max()))))
            (xa, va), (xb, vb) = res
            rows.append((n, which, float(np.abs(xa - xb).max()), float(np.abs(va - vb).max() / max(1.0, np.abs(va).max()))))
            for r in rows[-2 if which != "lbfgs" else -1:]:
                print("cpu-check n=%d %-60s x %.2e A  v %.2e" % r, flush=True)
    return rows


def energy_large(s):
    """k64_energy at 16384 beads, one replica: wall time of c3d_eval_f64(energies only) around its synchronising read-back"""
    from chromosome3d_amd import default_fire, default_model, make_stages
    n = 16384
    truth = random_coil(n, 7) * 0.25
    ri = np.concatenate([np.arange(n - k) for k in range(5, 65)])
    rj = np.concatenate([np.arange(k, n) for k in range(5, 65)])
    t10 = np.maximum(np.round(np.linalg.norm(truth[ri] - truth[rj], axis=1) * 10.0), 10).astype(np.int32)
    s.set_model(default_model())
    s.set_restraints(n, (ri + 1).astype(np.int32), (rj + 1).astype(np.int32), t10)
    s.set_schedule(make_stages([(2, 10, 0.0, 1.0, 1.0, 0.85, 0.0)]), default_fire())
    s.init_replicas(1, 82364, 0)
    s.set_coords64((truth * 1.1).astype(np.float64)[None])
    s.eval64(forces=False)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        s.eval64(forces=False)
        t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    s.eval64(energies=False)
    tf = time.perf_counter() - t0
    return min(t), tf


HEADER = ["# c3d_eval_f64 and the fp64 step kernels against the oracle in doubles", "",
          "Written by tools/f64_boundary.py: the MI355X section by a plain run, the CPU section by --cpu-check; each run keeps the other's section.",
          "Force gap: max |F - Fo| / (|Fo| + 0.1 max|Fo|) (cap 1e-10); energy gap: max |e - eo| / |eo| (cap 1e-11); x gap in Angstrom, v gap",
          "relative to max(1, max|v|) (cap 1e-8 each).  The bounds of tests/test_gpu_f64_boundary.py are 8 x the \"largest\" lines of the MI355X section (trajectories: schedule by schedule).", ""]
MARK = "<!-- section: %s -->"


def write_section(path, key, lines):
    """the report with section `key` ("gpu" or "cpu") replaced; the other one is kept from `path`, or from the committed profile"""
    sections = {"gpu": [], "cpu": []}
    for src in (path, os.path.join(ROOT, "profiles", "r16_f64_boundary.md")):
        if os.path.exists(src):
            cur = None
            for line in open(src).read().splitlines():
                if line.startswith("<!-- section: "):
                    cur = line[len("<!-- section: "):-len(" -->")]
                    sections[cur] = []
                elif cur in sections:
                    sections[cur].append(line)
            break
    sections[key] = lines
    with open(path, "w") as f:
        f.write("\n".join(HEADER + [MARK % "gpu"] + sections["gpu"] + [MARK % "cpu"] + sections["cpu"]).rstrip("\n") + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cpu-check", action="store_true")
    ap.add_argument("--energy-large", action="store_true")
    ap.add_argument("--sizes", type=int, nargs="*", default=None)
    ap.add_argument("--report", default=os.path.join(ROOT, "profiles", "r16_f64_boundary.md"))
    a = ap.parse_args()
    if a.cpu_check:
        rows = cpu_check(a.sizes or [113, 455, 300, 2561])
        rev = [r for r in rows if "python" not in r[1]]
        out = ["## On the CPU: the restatement against itself, the force's pair sums reversed", "",
               "The oracle's pair loop over the beads numbered backwards, the test's schedules from the test's start (replica 0, the default model):",
               "what re-ordered sums alone do over these step counts.  The anneal and the two-point stage are stepped by this tool's Python",
               "restatement of the oracle's schedule around either force; its rows against the oracle's own c3o_run_schedule stand beside them.", "",
               "| n | schedule | x gap (A) | v gap |", "|---|---|---|---|"]
        out += ["| %d | %s | %.2e | %.2e |" % r for r in rows]
        out += ["", "largest, reversed sums: x %.2e A, v %.2e" % (max(r[2] for r in rev), max(r[3] for r in rev)), ""]
        print(out[-2])
        write_section(a.report, "cpu", out)
        return 0
    from chromosome3d_amd import Solver
    s = Solver(0)
    for key, val in (("max_beads", 16384), ("f64_max_beads", 16384), ("f64_lbfgs", 1), ("precision", 64)):
        s.set_option(key, val)
    out = ["## On an MI355X: forces and energies (worst replica; every column form of a size returns the same bits)", "",
           "| n | model | w_all | force gap | energy gap |", "|---|---|---|---|---|"]
    fmax = emax = xmax = vmax = 0.0
    sizes = a.sizes or sorted(B.FORMS)
    for n in sizes:
        for (name, w), (gf, ge) in B.measure_forces_energies(s, O, n).items():
            out.append("| %d | %s | %g | %.2e | %.2e |" % (n, name, w, gf, ge))
            print(out[-1], flush=True)
            fmax, emax = max(fmax, gf), max(emax, ge)
    out += ["", "largest: force %.2e, energy %.2e" % (fmax, emax), "", "## On an MI355X: trajectories (worst replica)", "",
            "| n | schedule | steps | x gap (A) | v gap |", "|---|---|---|---|---|"]
    for n in [k for k in (113, 455, 300, 2561) if k in sizes]:
        for which in sorted(B.SCHEDULES):
            gx, gv = B.measure_trajectory(s, O, n, which)
            out.append("| %d | %s | %d | %.2e | %.2e |" % (n, which, sum(st[1] for st in B.SCHEDULES[which]), gx, gv))
            print(out[-1], flush=True)
            xmax, vmax = max(xmax, gx), max(vmax, gv)
    out += ["", "largest: x %.2e A, v %.2e" % (xmax, vmax)]
    for which in sorted(B.SCHEDULES):
        rows = [ln.split("|") for ln in out if ln.startswith("|") and "| %s |" % which in ln]
        if rows:
            out.append("largest, %s: x %.2e A, v %.2e" % (which, max(float(r[4]) for r in rows), max(float(r[5]) for r in rows)))
    out.append("")
    if a.energy_large:
        te, tf = energy_large(s)
        out += ["## On an MI355X: k64_energy at 16384 beads, one replica", "",
                "c3d_eval_f64, energies only (one workgroup of 256 threads): %.1f ms a call; forces only (k64_eval_forces_chunked): %.1f ms." % (1e3 * te, 1e3 * tf), ""]
        print(out[-2], flush=True)
    s.close()
    write_section(a.report, "gpu", out)
    print("MEASURED F %.3e E %.3e X %.3e V %.3e" % (fmax, emax, xmax, vmax))
    return 0


if __name__ == "__main__":
    sys.exit(main())
