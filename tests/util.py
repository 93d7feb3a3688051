"""Shared helpers of the test-suite (fixtures live in tests/golden)."""
import functools
import glob
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")

# Spearman(IF, d) of the bundled reference models
REF_SPEARMAN = {"chr21_1mb": -0.8447, "chr22_1mb": -0.7393, "chr20_1mb": -0.8353, "chr13_1mb": -0.9152,
                "chr19_500kb": -0.8311, "chr4_1mb": -0.9488, "chr1_500kb": -0.8722, "chr21_500kb": -0.9090}


def golden():
    with open(os.path.join(GOLD, "front_half_golden.json")) as fh:
        return json.load(fh)


def load_if(cid):
    """IF matrix of a bundled chromosome as float64 (verbatim text or packed upper triangle)."""
    p = os.path.join(GOLD, "inputs", f"{cid}_matrix.txt")
    if os.path.exists(p):
        rows = [[float(t) for t in line.split()] for line in open(p) if line.strip()]
        return np.array(rows, dtype=np.float64)
    z = np.load(os.path.join(GOLD, "inputs", f"{cid}_upper.npz"))
    n = int(z["n"])
    m = np.zeros((n, n))
    iu = np.triu_indices(n)
    m[iu] = z["upper"]
    m.T[iu] = z["upper"]
    return m


def write_if_text(IF, path, crlf=True):
    """Text file in the bundled format: numbers separated by single spaces, lines end ' \\r\\n'."""
    with open(path, "w", newline="") as fh:
        for row in IF:
            fh.write(" ".join(repr(float(v)) for v in row) + (" \r\n" if crlf else "\n"))


def model_pdb(cid):
    return glob.glob(os.path.join(GOLD, "models", f"{cid}_rank*_a11.pdb"))[0]


def load_pdb_xyz(path):
    return np.array([[float(l[30:38]), float(l[38:46]), float(l[46:54])] for l in open(path) if l.startswith("ATOM")])


def oracle_model_from(m, n):
    """oracle Model (fp64) holding exactly the float32 parameter values of a c3d_model."""
    from oracle import oracle as O
    return O.default_model(n, min_sep=m.min_sep, noe_pot=m.noe_pot, rep_sep=m.rep_sep, ang_mode=m.ang_mode,
                           s_noe=float(m.s_noe), rswitch=float(m.rswitch), asym=float(m.asym), masym=float(m.masym), mrswitch=float(m.mrswitch),
                           k_bond=float(m.k_bond), b0=float(m.b0), k_ang=float(m.k_ang), a0=float(m.a0),
                           r0_rep=float(m.r0_rep), k_rep=float(m.k_rep), mass=float(m.mass), fbeta=float(m.fbeta), msoexp=int(m.msoexp))


def oracle_fire_from(f):
    from oracle import oracle as O
    return O.default_fire(dt_start=float(f.dt_start), dt_max=float(f.dt_max), f_inc=float(f.f_inc),
                          f_dec=float(f.f_dec), alpha_start=float(f.alpha_start), f_alpha=float(f.f_alpha),
                          max_step=float(f.max_step), n_min=int(f.n_min))


def random_coil(n, seed, step=3.8):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    x = np.cumsum(step * d, axis=0)
    return (x - x.mean(0)).astype(np.float32)


# ---- what the GPU tests of the output side (compare, superpose, ensemble) share ----
# a schedule of 45 steps: enough for a context that only has to hold replicas
SHORT = [(2, 15, 0.0, 1.0, 20.0, 0.5, 0.0), (0, 15, 0.003, 0.4, 0.003, 0.9, 2000.0), (2, 15, 0.0, 1.0, 1.0, 0.85, 0.0)]


def restrained(s, n, nrep, seed=7):
    """a context of n beads with a small random restraint set and nrep replicas"""
    from chromosome3d_amd import default_model, make_stages
    rng = np.random.default_rng(seed)
    R = max(1, min(3 * n, n * (n - 1) // 2 // 2))
    i = rng.integers(1, n, size=R)
    j = np.minimum(i + rng.integers(1, 12, size=R), n)
    keep = j > i
    s.set_model(default_model())
    s.set_schedule(make_stages(SHORT))
    s.set_restraints(n, i[keep].astype(np.int32), j[keep].astype(np.int32), rng.integers(30, 120, size=int(keep.sum())).astype(np.int32))
    s.init_replicas(nrep)


def pair_distances(x):
    """the i<j distances of one model [n, 3] in row order, sqrt(((ux ux) + uy uy) + uz uz) in float64: the host's, operation for operation"""
    x = np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(len(x), 1)
    u = x[i] - x[j]
    return np.sqrt(((u[:, 0] * u[:, 0]) + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def average_ranks(d):
    """average ranks 1..m of a vector, ties sharing the mean of their first and last position: the host's avg_ranks"""
    _, inv, cnt = np.unique(d, return_inverse=True, return_counts=True)
    below = np.cumsum(cnt) - cnt
    return (0.5 * (below + (below + cnt - 1)) + 1.0)[inv]


def host_ranks(x):
    """average ranks of the i<j distances of one model, pairs in row order: the host's avg_ranks over the host's distances"""
    return average_ranks(pair_distances(x))


def shared_models(name):
    """(replica coordinates [M, n, 3] float32, extra models [E, n, 3] float64 or None) of the cases the compare and ensemble modules share:
    n257 = 257 beads x 5 + 2 extra models that no float holds, k17 = 64 beads x 17"""
    if name == "k17":
        return np.stack([random_coil(64, 400 + r) for r in range(17)]), None
    assert name == "n257"
    x = np.stack([random_coil(257, 300 + r) for r in range(5)])
    rng = np.random.default_rng(257)
    extra = np.stack([random_coil(257, 310 + e).astype(np.float64) * (1.5 + e) + rng.normal(scale=1e-3, size=(257, 3)) for e in range(2)])
    assert not np.array_equal(extra, extra.astype(np.float32))
    return x, extra


def synthetic_if(n, seed=20161015, K=11.0, alpha=0.5, sigma=0.2, radius=None):
    """Config-5 style synthetic Hi-C matrix: ground truth = confined random walk with
    3.8 A steps; IF_ij = (K / d_ij)^(1/alpha) * lognormal noise, symmetric, diagonal = 10 x row max.
    Returns (IF, xyz_truth)."""
    rng = np.random.default_rng(seed)
    radius = radius if radius is not None else 2.2 * n ** (1.0 / 3.0) * 2.0
    x = np.zeros((n, 3))
    for i in range(1, n):
        for _ in range(100):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            cand = x[i - 1] + 3.8 * d
            if np.linalg.norm(cand) <= radius:
                break
        x[i] = cand
    # element for element the arithmetic of the whole-matrix form, in row chunks: at most three n x n arrays live at once (630 MB at
    # n = 5120, where the n x n x 3 difference tensor alone would take 630 MB)
    ch = 256
    IF = np.empty((n, n))
    for a in range(0, n, ch):
        d = np.linalg.norm(x[a:a + ch, None, :] - x[None, :, :], axis=-1)
        np.fill_diagonal(d[:, a:], 1.0)
        IF[a:a + ch] = (K / d) ** (1.0 / alpha)
    del d
    g = rng.normal(size=(n, n))
    gs = np.empty((n, n))
    for a in range(0, n, ch):
        gs[a:a + ch] = (g[a:a + ch] + g[:, a:a + ch].T) / np.sqrt(2.0)
    del g
    for a in range(0, n, ch):
        IF[a:a + ch] = IF[a:a + ch] * np.exp(sigma * gs[a:a + ch])
    for a in range(0, n, ch):
        gs[a:a + ch] = (IF[a:a + ch] + IF[:, a:a + ch].T) / 2.0
    IF = gs
    np.fill_diagonal(IF, 0.0)
    np.fill_diagonal(IF, 10.0 * IF.max(axis=1))
    return IF, x - x.mean(0)


# ---- structure-level comparison of a solver model with the bundled reference model of the same matrix ----------
def bundled_rank(path):
    """`chr1_500kb_rank03_a11.pdb` -> 3: the rank (by the reference's own NOE energy) of the one model the reference ships."""
    import re
    m = re.search(r"_rank(\d+)_a(\d+)\.pdb$", os.path.basename(path))
    return int(m.group(1)) if m else 1


def chain_stats(x):
    """(bond mean, bond sd, |i-j|=2 mean, |i-j|=2 sd, radius of gyration, |i-j|=2 5 % and 95 % quantiles) of one model [N, 3] — the
    envelope SURVEY 8a/8c names."""
    x = np.asarray(x, dtype=np.float64)
    b = np.linalg.norm(x[1:] - x[:-1], axis=1)
    a = np.linalg.norm(x[2:] - x[:-2], axis=1)
    rg = float(np.sqrt(((x - x.mean(0)) ** 2).sum(1).mean()))
    return float(b.mean()), float(b.std()), float(a.mean()), float(a.std()), rg, float(np.quantile(a, 0.05)), float(np.quantile(a, 0.95))


def structure_report(IF, x, e_noe, ref_xyz, ref_rank=1, rows=None):
    """Everything the parity table holds for one matrix: x [M, N, 3] our replicas, e_noe [M], ref_xyz [N, 3] the bundled
    model, ref_rank its rank in the reference's run.  Scoring through the product's pinned host routines
    (spearman_IF_pdb.pl:42-70 = c3d_spearman_if_dist; output_models/similarity.txt = c3d_model_similarity)."""
    from chromosome3d_amd import pipeline
    x = np.asarray(x)
    M = x.shape[0]
    rho = -pipeline.spearman_IF_models(IF, x)
    order = np.argsort(np.asarray(e_noe).astype(np.int64), kind="stable")       # ascending int(E_noe), chromosome3D.pl:796-802
    best = int(order[0])
    matched = int(order[min(ref_rank, M) - 1])
    rho_ref = -pipeline.spearman_IF_pdb(IF, np.asarray(ref_xyz, dtype=np.float32))
    sim_best = pipeline.model_similarity(x[best], ref_xyz)
    sim_match = pipeline.model_similarity(x[matched], ref_xyz)
    # how alike two of OUR replicas are: the scale on which "same structure as the reference's" has to be read
    sim_own = pipeline.model_similarity(x[best], x[int(order[1])]) if M > 1 else (1.0, 0.0)
    ours, ref = chain_stats(x[best]), chain_stats(ref_xyz)
    # the reference's own final assessment of a model (chromosome3D.pl:447-485, :581-600 = c3d_assess): restraints satisfied within
    # the relaxation and the summed violation, of OUR best-ranked model and of the bundled one, on the same contact.tbl rows
    assess = None
    if rows is not None:
        assess = dict(best=pipeline.assess(x[best], rows), ref=pipeline.assess(np.asarray(ref_xyz, dtype=np.float32), rows), R=len(rows[0]))
    return dict(assess=assess, rho=rho, order=order, best=best, matched=matched, rho_best=float(rho[best]), rho_matched=float(rho[matched]),
                rho_mean=float(rho.mean()), rho_ref=float(rho_ref), delta=float(rho[best] - rho_ref),
                delta_matched=float(rho[matched] - rho_ref),
                # The bundled model of a chromosome is NOT the reference's energy-best (its file name carries ranks 1..10 of 20): it was
                # picked from the run, by all appearance for its Spearman (spearman_IF_pdb.pl:73-76 prints the models sorted by it).  The
                # like-for-like figure is therefore our BEST-SPEARMAN replica; `delta_closest` = the replica nearest to the reference's value
                # ... and ranks 1..10 ONLY, never 11..20 (46 files: a uniform pick from 20 would do that with probability 2^-46): the pick was
                # made among the ten lowest-energy models.  `delta_max_top10` = the best Spearman among OUR ten lowest-energy replicas
                delta_max_top10=float(rho[order[:min(10, M)]].max() - rho_ref),
                delta_max=float(rho.max() - rho_ref), delta_closest=float(rho[np.argmin(np.abs(rho - rho_ref))] - rho_ref), rho_sd=float(rho.std()),
                ref_percentile=float((rho < rho_ref).mean()),      # fraction of our replicas below the reference's value
                sim_best=sim_best, sim_matched=sim_match, sim_own=sim_own, chain=ours, chain_ref=ref,
                rg_ratio=ours[4] / ref[4])


def relax_reference_model(solver, ref_xyz, e_noe_ours, min_steps=3000, gtol=1e-2):
    """The one reference-held datum on ENERGY ORDERING: every bundled file name carries the model's rank by
    CNS NOE energy inside the reference's own run of 20 (chr22_1mb_rank08, ...; ranking rule chromosome3D.pl:796-802, 822-828).
    Relax the bundled model under OUR energy — the final minimisation stage alone (deck :1790-1803; weights * 1, repel 0.85), started
    from the bundled coordinates — and ask which rank its int(E_noe) takes among the int(E_noe) of our 20 annealed replicas.
    The solver must hold the matrix (and model) the replicas were annealed with; its replicas are replaced.
    Returns dict(e_noe, rank_in_ours (1 = below all of ours ... M+1 = above all), moved = (distance-Spearman, scaled dRMSD) of the
    relaxed against the bundled model, xyz)."""
    from chromosome3d_amd import default_fire, make_stages, pipeline
    ref_xyz = np.asarray(ref_xyz, dtype=np.float32)
    solver.set_schedule(make_stages([(2, min_steps, 0.0, 1.0, 1.0, 0.85, 0.0)]), default_fire(), gtol, 250)
    solver.init_replicas(1, 82364, 0)
    solver.set_coords(ref_xyz[None])
    solver.run()
    e3 = solver.energies()[0].copy()              # (E_noe, bond + angle, repel), unweighted, at the final stage's weights
    e = float(e3[0])
    x = solver.coords()[0]
    ours = np.asarray(e_noe_ours).astype(np.int64)
    return dict(e_noe=e, rank_in_ours=int(1 + (ours < int(e)).sum()), moved=pipeline.model_similarity(x, ref_xyz), xyz=x,
                rel_gap=float((e - ours.min()) / ours.min()), e3=e3)


# ---- the host units on the CPU, against the fake HIP layer of tools/sanitize (plain g++ -O0: no sanitizer, nothing preloaded) ----
HOST_UNITS = ("api", "config", "gate", "run", "analysis", "host")     # every translation unit of libc3d without device code


def link_fake_hip(out_dir, mains, exe):
    """Compiles the host units of csrc/, tools/sanitize/hip_stub.cpp and `mains` [(source, object name, extra flags)] side by side and
    links them into out_dir/exe.  Returns the program's path, or None where there is no host C++ compiler; a compiler or linker error fails."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        return None
    root = os.path.dirname(HERE)
    csrc, san = os.path.join(root, "chromosome3d_amd", "csrc"), os.path.join(root, "tools", "sanitize")
    flags = ["-std=c++17", "-O0", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), "-Wno-unused-result"]
    jobs = [(os.path.join(csrc, "c3d_%s.cpp" % u), u + ".o", []) for u in HOST_UNITS] + [(os.path.join(san, "hip_stub.cpp"), "stub.o", [])] + list(mains)
    procs = [subprocess.Popen([cxx] + flags + extra + ["-c", src, "-o", os.path.join(out_dir, obj)], stderr=subprocess.PIPE, text=True) for src, obj, extra in jobs]
    for p in procs:
        err = p.communicate()[1]
        assert p.returncode == 0, err[-2000:]
    out = os.path.join(out_dir, exe)
    link = subprocess.run([cxx] + [os.path.join(out_dir, obj) for _, obj, _ in jobs] + ["-o", out, "-lpthread"], capture_output=True, text=True)
    assert link.returncode == 0, link.stderr[-2000:]
    return out


@functools.lru_cache(maxsize=None)
def config_transcript():
    """(transcript, key lists) as tests/harness/config_transcript.cpp prints them, built and run once per session; None without a compiler."""
    tmp = tempfile.mkdtemp(prefix="c3d_config_transcript_")
    try:
        exe = link_fake_hip(tmp, [(os.path.join(HERE, "harness", "config_transcript.cpp"), "main.o", [])], "config_transcript")
        if exe is None:
            return None
        runs = [subprocess.run([exe] + args, capture_output=True, text=True, timeout=120) for args in ([], ["keys"])]
        for r in runs:
            assert r.returncode == 0, r.stderr[-2000:]
        return runs[0].stdout, runs[1].stdout
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def transcript_calls(text):
    """[(context, state, what, call, return code, refusal, what changed)] of a transcript's call lines: `context` counts the `# <state> <what>`
    lines, each of which opens a fresh context in state "A" / "B" / "C"; `"` is resolved to the refusal of the line before."""
    out, ctx, state, what, last = [], -1, None, None, ""
    for line in text.splitlines():
        if line.startswith("# "):
            ctx, state, what, last = ctx + 1, line[2], line[4:], ""
            continue
        f = line.split("\t") + ["", "", ""]
        if f[0] == "default" or f[0] == "set-up differs":
            continue
        rc = int(f[1])
        if rc and f[2] != '"':
            last = f[2]
        out.append((ctx, state, what, f[0], rc, last if rc else "", f[3]))
    return out


def stub_context_knows_stat(key):
    """c3d_get_stat(key) returned C3D_OK on a live context of the harness (state A and state B); skips without a host compiler"""
    import pytest
    got = config_transcript()
    if got is None:
        pytest.skip("no host C++ compiler")
    rcs = [c[4] for c in transcript_calls(got[0]) if c[3] == "get_stat " + key]
    return len(rcs) == 2 and rcs == [0, 0]
