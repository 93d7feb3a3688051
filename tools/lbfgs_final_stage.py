"""The final stage as kind 5 (two-point step sizes, FIRE after 1000; what ships) against kind 8 (L-BFGS m = 5 on the per-step path, FIRE
after 1000) from the device's own annealed coordinates (the default schedule without its final stage), exit test RMS force < 1e-2 every
10 steps: steps (= force evaluations) to the exit, the final stage's wall time, and microseconds per step of each method over a fixed range.
    python tools/lbfgs_final_stage.py            the table (GPU): the 15 problems of tools/minimiser_study.py fixed (five matrices x
                                                 replicas 0-2, one replica a context), chr1_500kb x 20, synthetic N = 2500 x 8
    python tools/lbfgs_final_stage.py profile    200 steps each of k_lbfgs_eval / k_lbfgs_move and of k_step (FIRE, the same form) at
                                                 chr1_500kb x 20 and N = 2500 x 8, for rocprofv3 --kernel-trace --stats"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from chromosome3d_amd import Solver, default_fire, default_model, default_schedule, make_stages, pipeline
from tests.util import load_if, synthetic_if
from tools.parity_sweep import load as load_matrix

GT, EVERY = 1e-2, 10


def _rows(kind):
    return [(t.kind, t.nsteps, t.dt, t.w_all, t.w_vdw, t.repel_s, t.t_bath) for t in default_schedule(3000, final_kind=kind)]


def annealed(s, IF, nrep):
    s.set_model(default_model())
    pipeline.IF2dist_new(s, IF)
    s.set_schedule(make_stages(_rows(5)[:-1]), default_fire(), 0.0, 250)
    s.init_replicas(nrep, 82364, 0)
    s.run()
    return s.coords()


def final_stage(s, x, kind):
    """(steps to the exit, wall ms of c3d_run, device ms) of the final stage from x."""
    s.set_schedule(make_stages([_rows(kind)[-1]]), default_fire(), GT, EVERY)
    s.init_replicas(x.shape[0], 82364, 0)
    s.set_coords(x)
    t0 = time.perf_counter()
    s.run()
    wall = 1e3 * (time.perf_counter() - t0)
    ms, steps, _ = s.last_timing()
    return steps, wall, ms


def us_per_step(s, x, kind, nsteps=200):
    """Device time per step over nsteps steps of the method alone (no FIRE part), after a warm-up range (graphs captured)."""
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


def table():
    s = Solver(0)
    print("| problem | N | replicas | kind 5 steps | kind 8 steps | ratio | kind 5 final stage ms (wall / device) | kind 8 final stage ms (wall / device) |"
          " kind 5 us/step | kind 8 us/step |\n|" + "---|" * 10, flush=True)
    tot = np.zeros(2)
    for cid in ("chr21_1mb", "chr13_1mb", "chr4_1mb", "chr10_500kb", "chr1_500kb"):
        IF = load_matrix(cid)
        x = annealed(s, IF, 3)
        for r in range(3):
            a, b = final_stage(s, x[r:r + 1], 5), final_stage(s, x[r:r + 1], 8)
            tot += (a[0], b[0])
            print(f"| {cid} r{r} | {IF.shape[0]} | 1 | {a[0]} | {b[0]} | {a[0] / b[0]:.2f} | {a[1]:.2f} / {a[2]:.2f} | {b[1]:.2f} / {b[2]:.2f} | | |", flush=True)
    print(f"# 15 problems: kind 5 {tot[0]:.0f} steps, kind 8 {tot[1]:.0f} ({tot[0] / tot[1]:.2f}x fewer)", flush=True)
    for name, IF, nrep in (("chr1_500kb", load_if("chr1_500kb"), 20), ("synthetic", synthetic_if(2500)[0], 8)):
        x = annealed(s, IF, nrep)
        a, b = final_stage(s, x, 5), final_stage(s, x, 8)
        ua, ka = us_per_step(s, x, 5)
        ub, kb = us_per_step(s, x, 8)
        print(f"| {name} | {IF.shape[0]} | {nrep} | {a[0]} | {b[0]} | {a[0] / b[0]:.2f} | {a[1]:.2f} / {a[2]:.2f} | {b[1]:.2f} / {b[2]:.2f} | {ua:.2f} ({ka}) | {ub:.2f} ({kb}) |",
              flush=True)
    s.close()


def profile():
    """k_lbfgs_eval / k_lbfgs_move against k_step of the same form (FIRE steps, per-step path) at both sizes, 420 steps each from the coil."""
    s = Solver(0)
    s.set_option("resident", 0)
    for IF, nrep in ((load_if("chr1_500kb"), 20), (synthetic_if(2500)[0], 8)):
        s.set_model(default_model())
        pipeline.IF2dist_new(s, IF)
        s.init_replicas(nrep, 82364, 0)
        x = s.coords()                      # the coil: no other step kernel runs in this process (the profile's k_step is FIRE's alone)
        for kind in (2, 8):
            print(IF.shape[0], nrep, kind, "%.2f us/step" % us_per_step(s, x, kind)[0], s.step_kernel_name, flush=True)
    s.close()


if __name__ == "__main__":
    profile() if len(sys.argv) > 1 and sys.argv[1] == "profile" else table()
