"""The final stage in fp64 as kind 8 (L-BFGS: k64_lbfgs_eval + k64_lbfgs_move, option f64_lbfgs) against kind 5 (two-point step sizes:
k64_step), both on a precision-64 context, from the device's own annealed coordinates (the default schedule without its final stage),
exit test RMS force < 1e-2 every 10 steps: steps to the exit, and microseconds per step of each method over a fixed range.
    python tools/f64_lbfgs.py [--report profiles/r15_f64_lbfgs.md]   the table (GPU): chr1_500kb x 20 and synthetic N = 8192 x 2
    python tools/f64_lbfgs.py profile                                 200 steps of each method at both sizes, for
                                                                      rocprofv3 --kernel-trace --stats (the eval / move split)"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chromosome3d_amd import Solver, default_fire, default_model, default_schedule, make_stages
from tests.util import load_if, synthetic_if

GT, EVERY = 1e-2, 10


def _rows(kind):
    return [(t.kind, t.nsteps, t.dt, t.w_all, t.w_vdw, t.repel_s, t.t_bath) for t in default_schedule(3000, final_kind=kind)]


def context():
    s = Solver(0)
    s.set_option("max_beads", 16384)
    s.set_option("f64_max_beads", 16384)
    s.set_option("f64_lbfgs", 1)
    s.set_option("precision", 64)
    s.set_model(default_model())
    return s


def annealed(s, IF, nrep):
    s.set_if_matrix(IF)
    s.set_schedule(make_stages(_rows(5)[:-1]), default_fire(), 0.0, 250)
    s.init_replicas(nrep, 82364, 0)
    s.run()
    return s.coords()


def final_stage(s, x, kind):
    """(steps to the exit, device ms, L-BFGS steps among them) of the final stage from x"""
    s.set_schedule(make_stages([_rows(kind)[-1]]), default_fire(), GT, EVERY)
    s.init_replicas(x.shape[0], 82364, 0)
    s.set_coords(x)
    before = s.stat("lbfgs_steps")
    s.run()
    ms, steps, _ = s.last_timing()
    return steps, ms, int(s.stat("lbfgs_steps") - before)


def us_per_step(s, x, kind, nsteps=200):
    """device time per step over nsteps steps of the method alone (no FIRE part), after a warm-up range (graphs captured)"""
    s.set_option("final_minimiser_steps", 10 ** 6)
    try:
        s.set_schedule(make_stages([(kind, 2 * nsteps + 20) + _rows(kind)[-1][2:]]), default_fire(), 0.0, 250)
        s.init_replicas(x.shape[0], 82364, 0)
        s.set_coords(x)
        s.run_steps(20 + nsteps)
        s.run_steps(nsteps)
        ms, steps, _ = s.last_timing()
        return 1e3 * ms / steps, s.step_kernel_name
    finally:
        s.set_option("final_minimiser_steps", 1000)


def problems():
    yield "chr1_500kb", load_if("chr1_500kb"), 20
    yield "synthetic", synthetic_if(8192)[0], 2


def table(report):
    lines = ["# The final stage in fp64: kind 8 (L-BFGS) against kind 5 (two-point step sizes)", "",
             "Tool: `python tools/f64_lbfgs.py` on one MI355X; precision 64, f64_lbfgs 1, the default schedule without its final stage, then the",
             "final stage from those coordinates with the exit test RMS force < 1e-2 every 10 steps.  us/step: device time (events) over 200",
             "steps of the method alone after a warm-up range, replica groups and graphs as shipped.  One run, no repetitions.", "",
             "| problem | N | replicas | kind 5 steps | kind 8 steps (L-BFGS among them) | ratio | kind 5 device ms | kind 8 device ms | kind 5 us/step | kind 8 us/step (eval + move) |",
             "|" + "---|" * 10]
    s = context()
    for name, IF, nrep in problems():
        x = annealed(s, IF, nrep)
        a, b = final_stage(s, x, 5), final_stage(s, x, 8)
        ua, ka = us_per_step(s, x, 5)
        ub, kb = us_per_step(s, x, 8)
        lines.append(f"| {name} | {IF.shape[0]} | {nrep} | {a[0]} | {b[0]} ({b[2]}) | {a[0] / max(b[0], 1):.2f} | {a[1]:.2f} | {b[1]:.2f} | "
                     f"{ua:.2f} (`{ka}`) | {ub:.2f} (`{kb}`) |")
        print(lines[-1], flush=True)
    s.close()
    text = "\n".join(lines) + "\n"
    if report:
        with open(report, "w") as f:
            f.write(text)
    else:
        print(text)


def profile():
    s = context()
    for name, IF, nrep in problems():
        s.set_if_matrix(IF)
        s.init_replicas(nrep, 82364, 0)
        x = s.coords()
        for kind in (5, 8):
            print(name, IF.shape[0], nrep, kind, "%.2f us/step" % us_per_step(s, x, kind)[0], s.step_kernel_name, flush=True)
    s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="table")
    ap.add_argument("--report")
    a = ap.parse_args()
    profile() if a.mode == "profile" else table(a.report)
