"""Host-side mirror of the reference driver's interface for the hot path.

Same names, argument meaning and artefacts as chromosome3D.pl so that tests read like the
reference's flow (file:line under the reference tree):

    calc_len_IF      :164-179      IF2dist_new :110-162     dist2rr :181-206
    carr2tbl         :340-362      build_models :254-289    assess_dgsa :769-829
    spearman_IF_pdb  spearman_IF_pdb.pl:15-76

All arithmetic happens in libc3d.so (HIP kernels + host C++); this file only moves buffers and
file names around.
"""
import ctypes as C
import os

import numpy as np

from . import lib as _l
from .solver import Solver, default_fire, default_model, default_schedule

KSCALING = 11       # chromosome3D.pl:18
ALPHA = 0.5         # :19
SEPARATION = 5      # :20
MODELCOUNT = 20     # :21
MD_SEED = 82364     # :980
DISTRELAX = 0.5     # :74


def parse_if_file(path):
    """N x N float64 matrix from the whitespace-separated text format (:116-129)."""
    L = _l.load()
    p = C.POINTER(C.c_double)()
    n = C.c_int()
    _l.check(L.c3d_parse_if_file(os.fsencode(path), C.byref(p), C.byref(n)))
    m = np.ctypeslib.as_array(p, shape=(n.value, n.value)).copy()
    L.c3d_free(p)
    return m


def calc_len_IF(path):
    return parse_if_file(path).shape[0]


def IF2dist_new(solver, IF, K=KSCALING, alpha=ALPHA):
    """K1 on the GPU.  Returns the quantised distances in tenths of an Angstrom (int32 N x N),
    i.e. the numbers the reference prints into <ID>.dist."""
    solver.set_if_matrix(IF, alpha=float(alpha), K=float(K))
    return solver.dist10()


def write_front_half(dist10, out_dir, ID, min_sep=SEPARATION):
    """<ID>.dist, <ID>.rr (dist2rr) and contact.tbl (carr2tbl) byte-for-byte as the reference."""
    L = _l.load()
    d = np.ascontiguousarray(dist10, dtype=np.int32)
    nres = C.c_int()
    _l.check(L.c3d_write_front_half(_l.i32ptr(d), d.shape[0], min_sep,
                                    os.fsencode(os.path.join(out_dir, f"{ID}.dist")),
                                    os.fsencode(os.path.join(out_dir, f"{ID}.rr")),
                                    os.fsencode(os.path.join(out_dir, "contact.tbl")), C.byref(nres)))
    return nres.value


def read_tbl(path):
    L = _l.load()
    pi, pj, pt = (C.POINTER(C.c_int32)() for _ in range(3))
    R = C.c_int()
    _l.check(L.c3d_read_tbl(os.fsencode(path), C.byref(pi), C.byref(pj), C.byref(pt), C.byref(R)))
    r = max(R.value, 1)
    out = tuple(np.ctypeslib.as_array(p, shape=(r,))[:R.value].copy() for p in (pi, pj, pt))
    for p in (pi, pj, pt):
        L.c3d_free(p)
    return out


def restraints_from_dist10(dist10, min_sep=SEPARATION):
    """(i, j, t10) rows i<j, 1-based, row-major order (order does not matter to the solver)."""
    n = dist10.shape[0]
    i, j = np.triu_indices(n, min_sep)
    m = dist10[i, j] > 0
    return (i[m] + 1).astype(np.int32), (j[m] + 1).astype(np.int32), dist10[i, j][m].astype(np.int32)


REFSEQUENCE_FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "refsequence.fasta")


def read_fasta(path):
    """letters of a FASTA / plain sequence file (header lines skipped) — seq_fasta, chromosome3D.pl:731-744"""
    return "".join(l.strip() for l in open(path) if not l.startswith(">"))


def set_residue_sequence(seq1):
    """Residue names of the models written from now on: None -> all MET (the bundled output_models), a string of one-letter
    codes -> residue i named after letter i as a reference run does (chromosome3D.pl:93-98); read_fasta(REFSEQUENCE_FASTA) is
    the reference's pseudo-protein."""
    _l.check(_l.load().c3d_set_residue_sequence(seq1.encode() if seq1 else None))


def write_pdb(path, xyz, e_noe=0.0, e_bond=0.0, e_rep=0.0, title=None):
    x = _l.as_f32(xyz)
    _l.check(_l.load().c3d_write_pdb(os.fsencode(path), _l.fptr(x), x.shape[0], e_noe, e_bond, e_rep,
                                     title.encode() if title else None))


def shape_pdb(in_path, out_path=None, log_path=None):
    """A16: filter_nonCA + reindex_chain + sed + add_connect_rows (:813-820) — the file assess_dgsa leaves behind."""
    _l.check(_l.load().c3d_shape_pdb(os.fsencode(in_path), os.fsencode(out_path or in_path),
                                     os.fsencode(log_path) if log_path else None))


def read_pdb_ca(path):
    L = _l.load()
    p = C.POINTER(C.c_float)()
    n = C.c_int()
    _l.check(L.c3d_read_pdb_ca(os.fsencode(path), C.byref(p), C.byref(n)))
    x = np.ctypeslib.as_array(p, shape=(n.value, 3)).copy()
    L.c3d_free(p)
    return x


def assess(xyz, rows, relax=DISTRELAX):
    """count_satisfied_tbl_rows + sum_noe_dev (:447-485, :581-600) -> (satisfied, sum_dev)."""
    ri, rj, rt = (np.ascontiguousarray(a, dtype=np.int32) for a in rows)
    x = _l.as_f32(xyz)
    sat, dev = C.c_int(), C.c_double()
    _l.check(_l.load().c3d_assess(_l.fptr(x), x.shape[0], len(ri), _l.i32ptr(ri), _l.i32ptr(rj), _l.i32ptr(rt),
                                  relax, C.byref(sat), C.byref(dev)))
    return sat.value, dev.value


def write_violations(xyz, rows, path, pdb_label="model.pdb", tbl_label="contact.tbl", relax=DISTRELAX):
    """assess() plus the violation table count_satisfied_tbl_rows leaves behind (:475-483), appended to `path`."""
    ri, rj, rt = (np.ascontiguousarray(a, dtype=np.int32) for a in rows)
    x = _l.as_f32(xyz)
    sat, dev = C.c_int(), C.c_double()
    _l.check(_l.load().c3d_write_violations(_l.fptr(x), x.shape[0], len(ri), _l.i32ptr(ri), _l.i32ptr(rj), _l.i32ptr(rt), relax,
                                            pdb_label.encode(), tbl_label.encode(), path.encode(), C.byref(sat), C.byref(dev)))
    return sat.value, dev.value


def spearman_IF_pdb(IF, xyz, rng=3):
    """Spearman(IF_ij, d_ij) over ordered pairs |i-j| >= rng; negative for good models."""
    IF = np.ascontiguousarray(IF, dtype=np.float64)
    x = _l.as_f32(xyz)
    rho = C.c_double()
    _l.check(_l.load().c3d_spearman_if_dist(_l.dptr(IF), _l.fptr(x), IF.shape[0], rng, C.byref(rho)))
    return rho.value


def spearman_IF_models(IF, xyz, rng=3):
    """spearman_IF_pdb for a stack of models [M, N, 3] of one matrix (IF ranked once)."""
    IF = np.ascontiguousarray(IF, dtype=np.float64)
    x = _l.as_f32(xyz)
    rho = np.empty(x.shape[0], dtype=np.float64)
    _l.check(_l.load().c3d_spearman_if_dist_batch(_l.dptr(IF), _l.fptr(x), IF.shape[0], x.shape[0], rng, _l.dptr(rho)))
    return rho


def reduce_model(xyz):
    """500 kb model -> 1 Mb resolution as the reference's `*_reduced.pdb` files: mean of consecutive bead pairs."""
    x = np.ascontiguousarray(xyz, dtype=np.float64)
    out = np.empty(((x.shape[0] + 1) // 2, 3), dtype=np.float64)
    _l.check(_l.load().c3d_reduce_model(_l.dptr(x), x.shape[0], _l.dptr(out)))
    return out


def model_similarity(xa, xb):
    """(Spearman, "RMSD") of two models' pairwise distances as in output_models/similarity.txt; the longer
    model is cut to the shorter one's length (a reduced 500 kb model can have one bead more or less)."""
    n = min(len(xa), len(xb))
    a = np.ascontiguousarray(np.asarray(xa, dtype=np.float64)[:n])
    b = np.ascontiguousarray(np.asarray(xb, dtype=np.float64)[:n])
    rho, rmsd = C.c_double(), C.c_double()
    _l.check(_l.load().c3d_model_similarity(_l.dptr(a), _l.dptr(b), n, C.byref(rho), C.byref(rmsd)))
    return rho.value, rmsd.value


def compare_models(solver, extra=None):
    """model_similarity for every ordered pair of the solver's replicas (and the models of `extra`, [E, n, 3]) at once, on the device:
    (spearman [K, K], rmsd [K, K]), entry [a][b] = model_similarity(model a, model b).  See Solver.compare."""
    return solver.compare(extra)


def superpose_models(solver, reference=0, ref_xyz=None, mirror=True, apply=False, iters=0):
    """The solver's replicas in one frame and one hand, on the device: (rmsd [M], mirrored [M], mean [n, 3], rmsf [n]) of fitting every
    replica onto replica `reference` (or the model ref_xyz), reflecting the mirror images; iters > 0 refines against the ensemble mean.
    rmsf is the per-bead spread of the ensemble.  apply=True leaves the replicas superposed.  See Solver.superpose."""
    return solver.superpose(reference, ref_xyz, mirror, apply, iters)


def rmsd_table(solver, extra=None, mirror=True):
    """Coordinate RMSD after superposition for every ordered pair of the solver's replicas (and the models of `extra`, [E, n, 3]), on the
    device: (rmsd [K, K] in Angstrom, mirrored [K, K]).  See Solver.rmsd_table."""
    return solver.rmsd_table(extra, mirror)


def ensemble_maps(solver, IF=None, rng=3, extra=None, pick=None, cutoff=None):
    """The ensemble's distance map on the device: a dict with "mean" and "sd" [n, n] — the mean of every pair distance over the solver's
    replicas (and the models of `extra`) and its spread from model to model — and, with a cutoff in Angstrom, "contact", the share of
    models in which the pair is closer than that (2 x the model's b0 is a common convention).  With IF also "rho_mean" and "rho_contact":
    Spearman(IF, mean distance) and Spearman(IF, contact frequency) over |i-j| >= rng.  pick: the models that count, e.g. the best-ranked
    few of solver.rank().  See Solver.ensemble_map / Solver.ensemble_score."""
    out = solver.ensemble_map(extra, pick, cutoff)
    if IF is not None:
        out["rho_mean"], out["rho_contact"] = solver.ensemble_score(IF, rng, extra, pick, cutoff)
    return out


def geometry_report(solver, extra=None, pick=None, clash_cutoff=3.5, sep=1, contact_cutoff=None):
    """Model quality and polymer diagnostics of a run's models on the device: Solver.geometry's dict ("clashes", "bead_clashes", "nearest",
    "chain" per model; clash_cutoff 3.5 A and sep 1 are the reference's clash count) with "separation_mean", "separation_sd" [n] and, with
    a contact_cutoff, "separation_contact" [n] of Solver.separation_profile over the models of `pick` (None: all)."""
    out = solver.geometry(extra, clash_cutoff, sep)
    out["separation_mean"], out["separation_sd"], contact = solver.separation_profile(extra, pick, contact_cutoff)
    if contact is not None:
        out["separation_contact"] = contact
    return out


def stratified_report(solver, IF, rng=3, max_sep=0, extra=None, sums=False):
    """A quality number that the distance decay does not dominate, on the device: {"rho" [K, n], "scc" [K][, "sums" [K, n, 3]]} of
    Solver.stratified_score — per model the Spearman coefficient of IF against distance inside every separation s = |i-j| (rng <= s <=
    max_sep, 0: n-1) and their combination with HiCRep's weights — with "strata" [n], the number of pairs n - s of every separation
    (0 outside the strata asked for).  rng 3 is the reference's range."""
    out = solver.stratified_score(IF, rng, max_sep, extra, sums)
    n = out["rho"].shape[1]
    s = np.arange(n)
    out["strata"] = np.where((s >= rng) & (s <= (max_sep if max_sep else n - 1)), n - s, 0)
    return out


def bead_report(solver, IF, rng=3, beads=None, extra=None):
    """Which bins are placed badly, on the device: Solver.bead_scores' dict — per model and bead "rho" (the Spearman coefficient of the
    bead's row of IF against its distances over |i-j| >= rng; 3 is the reference's range), "sums", "restrained", "satisfied" and
    "dev_milli" — with "beads" [B], the 0-based indices the columns stand for, "partners" [B], the number of pairs N_i of every row, and
    "dev" [K, B], the deviation in Angstrom."""
    out = solver.bead_scores(IF, rng, beads, extra)
    n = solver.n
    i = np.arange(n) if beads is None else np.asarray(beads, dtype=np.int64)
    out["beads"] = i
    out["partners"] = np.maximum(0, i - rng + 1) + np.maximum(0, n - i - rng)
    out["dev"] = out["dev_milli"] / 1000.0
    return out


def accessibility_report(solver, extra=None, radius=None, probe=None, n_points=96, points=None):
    """Where every locus sits in the fold, on the device: Solver.accessibility's dict ("exposed", "fraction", "area" per model and bead,
    "model_area" per model, "mean_fraction" per bead, "device_ms") with "radius" and "probe", the values the call used (each defaults to half
    the model's bond length b0: a convention), "points", the number of sphere points P, and "buried" [K], the number of a model's beads
    without an exposed point."""
    out = solver.accessibility(extra, radius, probe, n_points, points)
    out["radius"] = 0.5 * solver.b0 if radius is None else float(radius)
    out["probe"] = 0.5 * solver.b0 if probe is None else float(probe)
    out["points"] = int(n_points) if points is None else int(np.asarray(points).shape[0])
    out["buried"] = (out["exposed"] == 0).sum(axis=1)
    return out


def compartment_report(solver, IF, extra=None, pick=None, min_sep=1, n_vec=1, iters=200):
    """Do the models reproduce the A/B compartment pattern of the data?  Solver.compartments' dict for IF, every picked model and the
    consensus map, with "calls" [Q, n] int8, the sign of every map's first vector (the compartment call; 0 for a bead without spread),
    "converged" [Q], whether every residual is below 1e-9, and "best" — the index into "maps" of the model map (not the consensus) whose
    first vector agrees best with IF's."""
    out = solver.compartments(IF, extra, pick, True, min_sep, n_vec, iters)
    out["calls"] = np.sign(out["vectors"][:, 0, :]).astype(np.int8)
    out["converged"] = (out["residual"] < 1e-9).all(axis=1)
    out["best"] = 1 + int(np.argmax(out["agreement"][:-1, 0, 0]))
    return out


def insulation_report(solver, IF, extra=None, pick=None, windows=(5, 10, 25), contact=None, min_strength=0.1, tol=1):
    """Do the models reproduce the domain boundaries of the data?  Solver.insulation's dict for IF, every picked model and the consensus
    map over the windows that fit the chain (2w + 1 <= n), with "support" [W, n] int32 — the number of model maps (not the consensus)
    with a boundary of strength >= min_strength within tol beads of the bead — and "best" [W], per window the index into "maps" of the
    model map whose score fits IF's best (the most negative fit_r for distance maps, the most positive for contact maps)."""
    fit = [int(w) for w in windows if 2 * int(w) + 1 <= solver.n]
    out = solver.insulation(IF, extra, pick, True, fit, contact, min_strength, tol)
    marks = (out["boundary"][1:-1] == 1) & (out["strength"][1:-1] >= min_strength)                 # [models, W, n]
    near = marks.copy()
    for d in range(1, min(int(tol), solver.n - 1) + 1):
        near[:, :, d:] |= marks[:, :, :-d]
        near[:, :, :-d] |= marks[:, :, d:]
    out["support"] = near.sum(axis=0).astype(np.int32)
    r = out["fit_r"][:-1] * (1.0 if contact is not None else -1.0)
    out["best"] = [1 + int(np.nanargmax(r[:, k])) if np.isfinite(r[:, k]).any() else -1 for k in range(len(fit))]
    return out


def loop_report(solver, IF, extra=None, pick=None, mask=None, pixels=None, **kw):
    """Which pixels of IF are loops, and do the models close them?  Solver.loops' dict for IF, every picked model and the consensus
    (kw: its p, w, min_sep, max_sep, thr, min_obs, merge, corner, max_peaks), with "text": a table of the listed pixels — bead numbers
    from 1, IF's value and four ratios, the consensus' distance and its donut and lower-left ratios, and the number of models that
    close the pixel (both ratios below 1) — and below it, per map, `closed` and P2LL."""
    out = solver.loops(IF, extra, pick, True, mask, pixels=pixels, **kw)
    at, names = out["at"], out["maps"]
    model_rows = at[1:-1]
    shut = ((model_rows[:, :, 2] < 1.0) & (model_rows[:, :, 3] < 1.0)).sum(axis=0)
    lines = ["# i j IF r_donut r_ll r_h r_v consensus_d consensus_r_donut consensus_r_ll models_closed   (%d of %d candidates are peaks, %d listed; %d models)"
             % (out["found"], out["candidates"], len(out["pixels"]), len(model_rows))]
    for l, (i, j) in enumerate(out["pixels"]):
        lines.append("%d %d %.6g %.4f %.4f %.4f %.4f %.3f %.4f %.4f %d" % ((i + 1, j + 1) + tuple(at[0, l, [0, 2, 3, 4, 5]]) + tuple(at[-1, l, [0, 2, 3]]) + (shut[l],)))
    lines.append("# map scored closed P2LL")
    for q, name in enumerate(names):
        lines.append("# %s %d %d %.4f" % (name, out["closed"][q, 0], out["closed"][q, 1], out["p2ll"][q]))
    out["models_closed"] = shut.astype(np.int32)
    out["text"] = "\n".join(lines) + "\n"
    return out


def entanglement_report(solver, extra=None, min_sep=2, max_sep=0, bounds=None):
    """How entangled are the models, and do they agree in it?  Solver.entanglement's dict with "order" — the replicas in rank order
    (Solver.rank), then the extra models — "acn_per_segment" [K], "writhe_mean" and "writhe_sd" (population) over the models,
    "sign_agreement" — the share of models whose writhe has the sign of the mean — and "text": one row per model in that order
    (model number from 1, writhe, ACN, ACN per segment) under a header line with the ensemble's figures."""
    out = solver.entanglement(extra, min_sep, max_sep, bounds)
    K = len(out["writhe"])
    order = [int(k) for k in solver.rank()] + list(range(solver.nrep, K))
    S = solver.n - 1
    w = out["writhe"]
    out["order"] = np.array(order, dtype=np.int32)
    out["acn_per_segment"] = out["acn"] / S
    out["writhe_mean"], out["writhe_sd"] = float(w.mean()), float(w.std())
    out["sign_agreement"] = float((np.sign(w) == np.sign(out["writhe_mean"])).mean())
    lines = ["# model writhe acn acn_per_segment   (%d models of %d segments, separations %d..%d; writhe mean %.6f sd %.6f, sign agreement %.3f)"
             % (K, S, min_sep, max_sep if max_sep else S - 1, out["writhe_mean"], out["writhe_sd"], out["sign_agreement"])]
    for k in order:
        lines.append("%d %.9f %.9f %.9f" % (k + 1, w[k], out["acn"][k], out["acn_per_segment"][k]))
    out["text"] = "\n".join(lines) + "\n"
    return out


def balance_if(path_or_matrix, solver=None, device=0, **kw):
    """A raw contact matrix (a path in the text format of parse_if_file, or an array) balanced on the device and ready for set_if_matrix:
    Solver.balance's "balanced", rows of bins that cannot be balanced all 0 (set_if_matrix reads 0 as no restraint).  kw: the arguments of
    Solver.balance (method, ignore_diags, min_nnz, mask, w0, tol, max_iters, target).  Without a solver a context is opened on `device`
    for the call, with max_beads raised to the matrix where it is beyond the default."""
    M = parse_if_file(path_or_matrix) if isinstance(path_or_matrix, (str, bytes, os.PathLike)) else np.asarray(path_or_matrix, dtype=np.float64)
    own = solver is None
    s = Solver(device) if own else solver
    try:
        if own and M.shape[0] > 5120:
            s.set_option("max_beads", M.shape[0])
        return s.balance(M, want_matrix=True, **kw)["balanced"]
    finally:
        if own:
            s.close()


def map_similarity_report(solver, maps, names=None, h=(0,), min_sep=0, max_sep=0, keep_zeros=False):
    """Do the maps agree?  Solver.map_similarity's dict with "names", "counted" [n_h, P] (how many strata count in every pair) and "text":
    per half-width a header line and the n_maps x n_maps table of the stratum-adjusted coefficient, one row a map, then one line a pair
    with its coefficient and its counted strata."""
    out = solver.map_similarity(maps, h, min_sep, max_sep, keep_zeros)
    Q = out["scc"].shape[1]
    names = ["map %d" % (m + 1) for m in range(Q)] if names is None else [str(x) for x in names]
    assert len(names) == Q
    out["names"] = names
    out["counted"] = np.isfinite(out["rho"]).sum(axis=2)
    n, S = np.asarray(maps).shape[-1], out["rho"].shape[2]
    lines = []
    for k, hk in enumerate(out["h"]):
        lines.append("# h = %d   (%d maps of %d bins, separations %d..%d%s)" % (hk, Q, n, min_sep, min_sep + S - 1, ", zeros kept" if keep_zeros else ""))
        for m in range(Q):
            lines.append(" ".join(["%s" % names[m]] + ["%.9f" % v for v in out["scc"][k, m]]))
        for pr, (p, q) in enumerate(out["pairs"]):
            lines.append("# %s : %s  scc %.9f  strata %d of %d" % (names[p], names[q], out["scc"][k, p, q], out["counted"][k, pr], S))
    out["text"] = "\n".join(lines) + "\n"
    return out


def choose_smoothing(scc_by_h, gain=0.01):
    """HiCRep's rule for the half-width: the smallest listed h whose successor gains less than `gain` — scc(h_next) - scc(h) < gain — or
    the largest listed h if every step still gains.  scc_by_h: a dict h -> scc, or pairs (h, scc); read in ascending h.  Host only."""
    table = sorted((int(h), float(v)) for h, v in (scc_by_h.items() if hasattr(scc_by_h, "items") else scc_by_h))
    assert table, "no half-width listed"
    for (h0, v0), (_, v1) in zip(table, table[1:]):
        if v1 - v0 < gain:
            return h0
    return table[-1][0]


def build_models(solver, model_count=MODELCOUNT, seed=MD_SEED, first_replica=0, model=None, stages=None, fire=None,
                 gtol=1e-2, check_every=250, final_kind=5):
    """The replacement of `cns_solve < dgsa.inp` (:254-289): runs the whole annealing schedule
    for model_count replicas on the GPU and returns (xyz [M,N,3], energies [M,3])."""
    solver.set_model(model if model is not None else default_model())
    solver.set_schedule(stages if stages is not None else default_schedule(final_kind=final_kind), fire or default_fire(), gtol, check_every)
    solver.init_replicas(model_count, seed, first_replica)
    solver.run()
    return solver.coords(), solver.energies()


def assess_dgsa(out_dir, ID, xyz, energies, rows, top=5, quiet=False):
    """Rank by int(E_noe) ascending (:796-802), print the satisfaction table (:804-810), write every
    model as <ID>_<k>.pdb, shape it as :813-820 does (CA rows renumbered, CONECT, REMARKs to model_info.log)
    and rename the best `top` to <ID>_model<i>.pdb (:822-828)."""
    M = xyz.shape[0]
    order = sorted(range(M), key=lambda r: (int(energies[r, 0]), r))
    report = []
    names = {}
    for r in range(M):
        names[r] = os.path.join(out_dir, f"{ID}_{r + 1}.pdb")
        write_pdb(names[r], xyz[r], *energies[r], title=os.path.basename(names[r]))
    say = (lambda *a: None) if quiet else print
    say(f"NOE_SATISFIED(+-{DISTRELAX}A)  SUM_OF_DEVIATIONS>= 0.2  PDB")
    for r in reversed(order):
        sat, dev = assess(xyz[r], rows)
        report.append((r, sat, dev))
        say("%-9s             %-9s                %-25s" % (f"{sat}/{len(rows[0])}", "%.2f" % dev,
                                                            os.path.basename(names[r])[:-4]))
    for r in reversed(order):
        shape_pdb(names[r], None, os.path.join(out_dir, "model_info.log"))
    for k, r in enumerate(order[:top]):
        dst = os.path.join(out_dir, f"{ID}_model{k + 1}.pdb")
        os.replace(names[r], dst)
        say(f"model{k + 1}.pdb <= {os.path.basename(names[r])}")
    return order, report


def reconstruct(matrix_path, out_dir, K=KSCALING, alpha=ALPHA, model_count=MODELCOUNT, device=0, **kw):
    """chromosome3D.pl top level (:86-106) for one matrix: front half, models, assessment."""
    os.makedirs(out_dir, exist_ok=True)
    ID = os.path.basename(matrix_path)
    ID = ID[:-4] if ID.endswith(".txt") else ID
    IF = parse_if_file(matrix_path)
    s = Solver(device)
    try:
        d10 = IF2dist_new(s, IF, K, alpha)
        nres = write_front_half(d10, out_dir, ID)
        print(f"Restraints : {nres} lines in tbl file")
        xyz, en = build_models(s, model_count, **kw)
        rows = restraints_from_dist10(d10)
        order, _ = assess_dgsa(out_dir, ID, xyz, en, rows)
        rho = list(spearman_IF_models(IF, xyz))
        return dict(ID=ID, n=IF.shape[0], restraints=nres, order=order, spearman=rho, energies=en, xyz=xyz)
    finally:
        s.close()
