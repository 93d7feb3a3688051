// c3d_solve — command-line stand-in for the `cns_solve < dgsa.inp` line of the reference's
// job.sh (chromosome3D.pl:258-284).  It is a thin shell over the C ABI (include/c3d.h):
//
//   c3d_solve --if <matrix.txt> --out <dir> [--id ID] [-k 11] [-a 0.5] [-m 20] ...
//       front half on the GPU (K1) + <ID>.dist/.rr/contact.tbl + M models <ID>_<k>.pdb
//   c3d_solve --tbl contact.tbl --n N --out <dir> --id ID [-m 20] ...
//       exactly the cns_solve role: restraints in, <ID>_<k>.pdb out
//   --similarity <path> adds the replicas' similarity table (Spearman and scaled RMSD of the pair distances, on the device)
//   --superpose writes the models in one frame and one hand, the best-ranked model's; --rmsf <path> adds the mean model and per-bead spread
//   --ensemble <prefix> writes the ensemble's distance map — <prefix>_mean.txt, _sd.txt, _contact.txt: mean, spread and contact frequency of
//       every bead pair over the models (or the --ensemble-top best) — and prints how that map follows the input matrix
//   --geometry <prefix> writes <prefix>_geometry.txt — per model the reference's clash count, closest counted pair and chain envelope — and
//       <prefix>_separation.txt, distance and contact share against genomic separation over the models (or the --ensemble-top best)
//   --stratified <prefix> writes <prefix>_scc.txt — per model the stratum-adjusted rank correlation of IF and distance — and
//       <prefix>_strata.txt, the Spearman coefficient inside every genomic separation, one column a model
//   --per-bead <prefix> writes <prefix>_beads.txt — per bead and model the Spearman coefficient of the bead's row of IF against its distances,
//       and how many of the bead's restraints the model satisfies and by how much it misses them
//   --accessibility <prefix> writes <prefix>_accessibility.txt — per bead and model the share of the bead's sphere that a probe can reach:
//       which loci lie on the surface of the fold and which are buried in it
//   --compartments <prefix> writes <prefix>_compartments.txt — the first compartment eigenvector (PC1 of the correlation of the observed/expected
//       map) of IF, of the models' consensus distance map and of every model, and how well each agrees with IF's
//   --loops <prefix> writes <prefix>_loops.txt — the peaks of IF with their local-background ratios, and whether the models close them
//   --insulation <prefix> writes <prefix>_insulation.txt — the insulation profile and the domain boundaries of IF and of the models' consensus
//       map per window, how many models place a boundary at each bead, and how well every model's profile fits IF's
//   --entanglement <prefix> writes <prefix>_entanglement.txt — per model the writhe and the average crossing number of the chain (Gauss
//       integrals) with the ensemble's mean, sd and sign agreement — and <prefix>_segments.txt, every segment's share; with --entangle-bounds
//       also <prefix>_link.txt, the linking table of the given domains
//   --balance <ice|vc|sqrt-vc> balances the matrix of --if on the device first (raw contact counts in, a normalised matrix out): the solve and
//       every analysis option of the run use the balanced matrix; --balance-out <prefix> writes the weights and the matrix
//   --map-similarity <file> (repeatable) compares the matrix of --if as read, before any --balance, with the listed matrices on the device:
//       HiCRep's stratum-adjusted correlation coefficient of every pair, printed as a table per half-width (c3d_map_similarity)
//
// Success convention of the reference: <ID>_<M>.pdb exists, iam.running removed; on failure
// iam.running is renamed iam.failed and the exit code is non-zero (:266-283).
#include <sys/stat.h>

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/c3d.h"

static void usage() {
    fprintf(stderr,
            "usage: c3d_solve (--if <IF matrix> | --tbl <contact.tbl> --n <beads>) --out <dir> [--id <ID>]\n"
            "                 [-k <K=11>] [-a <alpha=0.5>] [-m <models=20>] [--seed <82364>] [--first-replica <0>]\n"
            "                 [--device <0>] [--min-steps <3000>] [--gtol <1e-2>] [--final-minimiser <1>] [--lbfgs] [--embed] [--no-graph] [--quiet]\n"
            "                 [--precision <32>   64: anneal with the fp64 step kernels (the reference's arithmetic; with --lbfgs the final stage is\n"
            "                                     L-BFGS in fp64); beyond 2560 beads the fp64 target matrix takes 8 n^2 bytes more]\n"
            "                 [--embed-max-beads <4549>   the largest matrix --embed takes, up to 16384 (memory: 8 n^2 bytes + 4 n^2 per replica of a batch)]\n"
            "                 [--seq <one-letter residue codes | @fasta file>   residue names of the models (default: all MET)]\n"
            "                 [--similarity <path>   after the solve, the replicas against one another: one row `a b spearman rmsd` per ordered pair of\n"
            "                                        replica ids (Spearman and scaled RMSD of the pair distances, computed on the device)]\n"
            "                 [--superpose   write the models superposed on the best-ranked one, mirror images reflected onto its hand: the files overlay;\n"
            "                                only the coordinates move (rotation, reflection, translation), every REMARK row stays]\n"
            "                 [--rmsf <path>   mean model and per-bead spread of the superposed ensemble: one row `bead mean_x mean_y mean_z rmsf`\n"
            "                                  (generalized Procrustes from the best-ranked model, 3 iterations, on the device)]\n"
            "                 [--ensemble <prefix>   the ensemble's distance map, computed on the device: <prefix>_mean.txt and <prefix>_sd.txt hold the mean of\n"
            "                                        every bead pair's distance over the models and its standard deviation from model to model (%%.3f),\n"
            "                                        <prefix>_contact.txt the share of models with the pair closer than the cutoff (%%.4f); n lines of n\n"
            "                                        numbers, the layout of the input matrix.  With --if one line `ensemble: ...` gives Spearman(IF, mean d)\n"
            "                                        and Spearman(IF, contact); a run started from --tbl has no matrix and writes the maps alone]\n"
            "                 [--ensemble-top <M>   the map of the M best-ranked models only (lowest int(E_noe) first; default: all models)]\n"
            "                 [--ensemble-cutoff <A>   contact distance in Angstrom; default 2 x the model's bond length b0 — a convention, not a\n"
            "                                          measured value; 0: no contact map]\n"
            "                 [--geometry <prefix>   model geometry, computed on the device.  <prefix>_geometry.txt: one row per model in rank order (lowest\n"
            "                                        int(E_noe) first), `rank model clashes nearest bond_mean bond_sd i2_mean i2_sd rg extent` — the pairs i < j,\n"
            "                                        j - i >= --clash-sep, no further apart than --clash-cutoff (the reference's clash_count), the smallest\n"
            "                                        distance among the pairs at that separation, mean and sd of the bond and (i,i+2) distances, radius of\n"
            "                                        gyration and largest pair distance (A).  <prefix>_separation.txt: one row `s mean sd contact` per\n"
            "                                        separation s = |i-j|, over the models --ensemble-top selects: mean distance, its sd and the share of\n"
            "                                        pairs closer than --ensemble-cutoff (`s mean sd` when that is 0)]\n"
            "                 [--clash-cutoff <A>   clash distance in Angstrom, `<=` as the reference compares; default 3.5]\n"
            "                 [--clash-sep <k>   smallest |i-j| of a counted pair; default 1: bonded neighbours count, as in the reference]\n"
            "                 [--stratified <prefix>   IF against model distance inside every genomic separation s = |i-j| >= 3 (the reference's range), sorted\n"
            "                                          and summed on the device; needs --if.  <prefix>_scc.txt: one row `rank model scc` per model in rank\n"
            "                                          order (lowest int(E_noe) first), scc the strata's Spearman coefficients combined with HiCRep's weights:\n"
            "                                          the rank correlation with the distance decay taken out, negative for a good model (%%.6f).\n"
            "                                          <prefix>_strata.txt: one row `s N rho_1 ... rho_M` per separation, N = n - s pairs, the models' columns\n"
            "                                          in rank order (%%.6f; `nan` where IF or the distances of the stratum are constant)]\n"
            "                 [--stratified-max-sep <S>   the largest separation of --stratified; default 0: n-1]\n"
            "                 [--per-bead <prefix>   which bins are placed badly, computed on the device; needs --if.  <prefix>_beads.txt: one row per bead,\n"
            "                                        `bead restrained rho_1 satisfied_1 dev_1 ... rho_M satisfied_M dev_M`, the models' columns in rank order\n"
            "                                        (lowest int(E_noe) first): the bead's 1-based index, the number of its restraints, and per model the\n"
            "                                        Spearman coefficient of the bead's row of IF against its distances over |i-j| >= 3 (%%.6f; `nan` where a\n"
            "                                        side is constant, e.g. an unmappable bin), the reference's net count of satisfied restraints of the bead\n"
            "                                        and the summed deviation of the others in A (%%.3f)]\n"
            "                 [--accessibility <prefix>   where every locus sits in the fold, computed on the device.  <prefix>_accessibility.txt: one row per bead,\n"
            "                                             `bead mean f_1 ... f_M`: the bead's 1-based index, the mean over the models and per model, in rank order\n"
            "                                             (lowest int(E_noe) first), the exposed share of the P points on the sphere of radius R = bead radius +\n"
            "                                             probe radius about the bead — those inside no other bead's sphere of that radius (%%.4f; Shrake-Rupley).\n"
            "                                             A header line gives R, P and every model's accessible area 4 pi R^2 sum f in A^2]\n"
            "                 [--bead-radius <A>   radius of a bead; default half the model's bond length b0: touching beads — a convention]\n"
            "                 [--probe-radius <A>   radius of the probe; default half of b0: a probe of a bead's size — a convention]\n"
            "                 [--sphere-points <P>   points on a bead's sphere, 1..1024; default 96]\n"
            "                 [--compartments <prefix>   do the models reproduce the A/B compartment pattern of the data?  Computed on the device.\n"
            "                                            <prefix>_compartments.txt: header lines `# IF|consensus|model <r>: share residual agreement same_side` (the first\n"
            "                                            eigenvector's share of the correlation's trace, |C v - lambda v|, |Pearson r| against IF's first eigenvector and\n"
            "                                            the share of beads on IF's side of zero; with more vectors one such group per vector), then one row per bead,\n"
            "                                            `bead IF consensus pc1_1 ... pc1_M`: the bead's 1-based index and the entry of the first eigenvector (%%.6f) of IF,\n"
            "                                            of the models' mean distance map and of every model in rank order; its sign is the compartment call]\n"
            "                 [--compartment-vectors <1..3>   eigenvectors computed and reported in the header lines; default 1]\n"
            "                 [--compartment-iters <k>   rounds of orthogonal iteration, 0..10000; default 200]\n"
            "                 [--compartment-min-sep <s>   pairs closer than s bins along the chain count as 1 in the observed/expected map; default 1]\n"
            "                 [--insulation <prefix>   do the models reproduce the domain (TAD) boundaries of the data?  Computed on the device.\n"
            "                                          <prefix>_insulation.txt: header lines `# window <w> consensus|model <r>: fit_r n_IF n_map IF_matched map_matched`\n"
            "                                          (Pearson r of the map's insulation score against IF's — negative is good for distances, positive for contacts —\n"
            "                                          and the boundaries of strength >= 0.1: IF's, the map's, IF's with one of the map's within tol beads, the map's\n"
            "                                          with one of IF's), then one row per bead per window,\n"
            "                                          `window bead IF consensus IF_boundary IF_strength consensus_boundary consensus_strength models`: the scores\n"
            "                                          (log2 of the mean over the w x w square that straddles the bead over the row's mean; nan where the square does\n"
            "                                          not fit), the boundary marks and their prominences, and the number of models with a boundary within tol beads]\n"
            "                 [--insulation-windows <a,b,c>   half-widths of the squares in beads, ascending, 1..128; default 5,10,25, those that fit (2w + 1 <= n)]\n"
            "                 [--insulation-contact <cutoff>   models and consensus: count contacts (distance < cutoff, in A) in the square instead of averaging the distance]\n"
            "                 [--insulation-tol <beads>   how far apart two boundaries may lie and still match; default 1]\n"
            "                 [--loops <prefix>   which pixels of IF are loops, and do the models close them?  Computed on the device.\n"
            "                                          <prefix>_loops.txt: a line a peak of IF, `i j IF r_donut r_ll r_h r_v consensus_d consensus_r_donut consensus_r_ll models_closed`\n"
            "                                          (beads from 1; the four local-background ratios of the pixel; the consensus' distance and ratios, below 1 where\n"
            "                                          the models close the loop; how many models have both ratios below 1), then per map `# <map> scored closed P2LL`]\n"
            "                 [--loop-window <w>   half-width of a pixel's window in beads, 1..20; default 5]\n"
            "                 [--loop-peak <p>   half-width of the peak square left out of the backgrounds, 0..w-1; default 2]\n"
            "                 [--loop-sep <MIN:MAX>   separations j - i that are scanned; default 2w+1 : min(n-1, 2w+1024)]\n"
            "                 [--loop-thr <a,b,c,d>   least ratio against the donut, lower-left, horizontal and vertical background; default 1.75,1.75,1.5,1.5]\n"
            "                 [--loop-list <FILE>   score these pixels (lines `i j`, beads from 1) instead of the peaks of IF]\n"
            "                 [--entanglement <prefix>   how entangled are the models, and with which handedness?  Gauss integrals over the chain, on the device.\n"
            "                                          <prefix>_entanglement.txt: one row per model in rank order, `rank model writhe acn acn_per_segment`, under a header\n"
            "                                          with the writhe's mean, sd and sign agreement over the models; <prefix>_segments.txt: `model segment seg_writhe seg_acn`\n"
            "                                          (segment s joins beads s and s+1, from 1)]\n"
            "                 [--entangle-sep <a:b>   the segment pairs that count: a <= |s-t| <= b, a >= 2; b = 0: all; default 2:0.  A small b gives the local writhe]\n"
            "                 [--entangle-bounds <FILE>   domain bounds in segments, ascending whole numbers from 0 to n-1 separated by white space; adds\n"
            "                                          <prefix>_link.txt: `model p q link link_abs` for p <= q (the Gauss linking integral of domains p and q, from 1;\n"
            "                                          p = q: the domain's own writhe)]\n"
            "                 [--balance <ice|vc|sqrt-vc>   the matrix of --if holds raw contact counts: balance it on the device first (iterative correction, vanilla\n"
            "                                          coverage or its square root); the solve and every analysis option of the run use the balanced matrix.  Bins that\n"
            "                                          cannot be balanced get weight 0 and no restraints]\n"
            "                 [--balance-ignore-diags <k>   the diagonals |i-j| < k do not count in the marginals; default 2]\n"
            "                 [--balance-min-nnz <m>   bins with fewer non-zero entries are masked; default 10]\n"
            "                 [--balance-tol <v>   ice stops when the variance of the relative marginals is below v; default 1e-5]\n"
            "                 [--balance-iters <k>   at most k updates of ice, 0..10000; default 200]\n"
            "                 [--balance-out <prefix>   writes <prefix>_weights.txt (header `bead weight masked`; masked: 0 kept, 1 listed, 2 too few non-zeros,\n"
            "                                          3 no kept partner) and <prefix>_matrix.txt, the balanced matrix in the format --if reads, with 17 digits]\n"
            "                 [--map-similarity <file>   repeatable, up to 15: compare the matrix of --if as read (before any --balance) with these matrices of the same\n"
            "                                          size, before the solve: the stratum-adjusted correlation coefficient (HiCRep's SCC) of every pair of maps, map 1 the\n"
            "                                          matrix of --if, printed as `Similarity : h <h> map <m> : <scc to every map>` a half-width and map]\n"
            "                 [--map-similarity-h <list>   half-widths of the box mean, ascending, each 0..20, at most 8; default 0]\n"
            "                 [--map-similarity-sep <lo>:<hi>   the separations correlated; default 1:0, 0 meaning n - 1]\n"
            "                 [--map-similarity-out <prefix>   writes <prefix>_scc.txt (header `h map scc...`, the tables with 17 digits) and <prefix>_strata.txt\n"
            "                                          (header `h map_p map_q separation kept rho`, one row a half-width, pair and separation)]\n"
            "                 [--accepted   also write <ID>a_<k>.pdb beside every <ID>_<k>.pdb, as CNS does for structures it accepts]\n");
}

#define CHECK(call)                                                              \
    do {                                                                         \
        int rc__ = (call);                                                       \
        if (rc__ != C3D_OK) {                                                    \
            fprintf(stderr, "c3d_solve: %s failed (%d): %s\n", #call, rc__, c3d_last_error()); \
            return fail_exit(out_dir);                                           \
        }                                                                        \
    } while (0)

static int fail_exit(const std::string& out_dir) {
    if (!out_dir.empty()) {
        const std::string a = out_dir + "/iam.running", b = out_dir + "/iam.failed";
        if (rename(a.c_str(), b.c_str()) != 0) { FILE* f = fopen(b.c_str(), "w"); if (f) fclose(f); }
    }
    fprintf(stderr, "ERROR! Final structures not found!\nC3D FAILED!\n");
    return 1;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int main(int argc, char** argv) {
    // A device exception (memory fault, queue error) must reach stderr in the runtime's own words: by default ROCr first pipes a GPU core
    // dump to the helper named in /proc/sys/kernel/core_pattern, and where that helper does not exist the process dies on the broken pipe
    // (rc -13, "GPU coredump: execvp failed") before the runtime has said WHICH exception — round 5 lost the only evidence of one that way.
    setenv("HSA_DISABLE_COREDUMP_ON_EXCEPTION", "1", 0);          // (0: a user's own setting wins)
    const double t_start = now_s();
    std::string if_path, tbl_path, out_dir, id, seq_arg, similarity_path, rmsf_path, ensemble_prefix, geometry_prefix, stratified_prefix, per_bead_prefix, accessibility_prefix, compartments_prefix;
    int compartment_vectors = 1, compartment_iters = 200, compartment_min_sep = 1;
    std::string insulation_prefix, insulation_windows = "5,10,25";
    bool insulation_windows_given = false;
    double insulation_contact = 0;                   // 0: mean distance
    int insulation_tol = 1;
    std::string loops_prefix, loop_sep, loop_thr = "1.75,1.75,1.5,1.5", loop_list;
    int loop_window = 5, loop_peak = 2;
    std::string entanglement_prefix, entangle_sep, entangle_bounds;
    std::string balance_method, balance_out;          // empty: the matrix of --if is taken as it is
    std::vector<std::string> mapsim_files;             // matrices to compare the one of --if with (c3d_map_similarity)
    std::string mapsim_h = "0", mapsim_sep, mapsim_out;
    int balance_ignore_diags = 2, balance_min_nnz = 10, balance_iters = 200;
    double balance_tol = 1e-5;
    double bead_radius = -1, probe_radius = -1;      // < 0: half of b0
    int sphere_points = 96;
    int superpose = 0, ensemble_top = 0, stratified_max_sep = 0;
    double ensemble_cutoff = -1;      // < 0: 2 x b0
    double clash_cutoff = 3.5;        // the figure of the reference's assessment
    int clash_sep = 1;
    double K = 11, alpha = 0.5, gtol = 1e-2;
    int final_min = 1;
    int lbfgs = 0;
    int models = 20, device = 0, n_beads = 0, min_steps = 3000, use_graph = 1, quiet = 0, embed = 0, embed_max_beads = 0, accepted = 0, precision = 32;
    unsigned long long seed = 82364ULL;
    unsigned first_rep = 0;
    for (int a = 1; a < argc; ++a) {
        const std::string s = argv[a];
        auto next = [&](const char* what) -> const char* {
            if (a + 1 >= argc) { fprintf(stderr, "c3d_solve: %s needs a value\n", what); exit(2); }
            return argv[++a];
        };
        if (s == "--if" || s == "-i" || s == "-if") if_path = next("--if");
        else if (s == "--tbl") tbl_path = next("--tbl");
        else if (s == "--n") n_beads = atoi(next("--n"));
        else if (s == "--out" || s == "-o") out_dir = next("--out");
        else if (s == "--id") id = next("--id");
        else if (s == "-k") K = atof(next("-k"));
        else if (s == "-a") alpha = atof(next("-a"));
        else if (s == "-m") models = atoi(next("-m"));
        else if (s == "--seed") seed = strtoull(next("--seed"), nullptr, 10);
        else if (s == "--first-replica") first_rep = (unsigned)strtoul(next("--first-replica"), nullptr, 10);
        else if (s == "--device") device = atoi(next("--device"));
        else if (s == "--min-steps") min_steps = atoi(next("--min-steps"));
        else if (s == "--gtol") gtol = atof(next("--gtol"));
        else if (s == "--final-minimiser") final_min = atoi(next("--final-minimiser"));   // 0 = FIRE throughout (rounds 1-4), 1 = two-point steps then FIRE (default)
        else if (s == "--lbfgs") lbfgs = 1;   // the final stage as kind 8: L-BFGS, then FIRE (opt-in; the default stays kind 5)
        else if (s == "--embed") embed = 1;   // distance-geometry start (deck :1471-1525) instead of the random coil
        else if (s == "--embed-max-beads") embed_max_beads = atoi(next("--embed-max-beads"));   // consent to the memory of an embedding beyond 4549 beads
        else if (s == "--precision") precision = atoi(next("--precision"));   // 64: the fp64 step kernels (c3d_f64.hip)
        else if (s == "--no-graph") use_graph = 0;
        else if (s == "--quiet") quiet = 1;
        else if (s == "--accepted") accepted = 1;   // the deck's printaccept writes <ID>a_<k>.pdb for structures CNS accepts, beside the trial file (:1818-1828)
        else if (s == "--seq") seq_arg = next("--seq");
        else if (s == "--similarity") similarity_path = next("--similarity");   // the ensemble table (c3d_compare_replicas)
        else if (s == "--superpose") superpose = 1;   // the models in the best-ranked model's frame and hand before they are written (c3d_superpose_replicas)
        else if (s == "--rmsf") rmsf_path = next("--rmsf");   // mean model and per-bead spread of the superposed ensemble
        else if (s == "--ensemble") ensemble_prefix = next("--ensemble");   // mean / sd / contact maps of the ensemble (c3d_ensemble_map, c3d_ensemble_score)
        else if (s == "--ensemble-top") ensemble_top = atoi(next("--ensemble-top"));
        else if (s == "--ensemble-cutoff") ensemble_cutoff = atof(next("--ensemble-cutoff"));
        else if (s == "--geometry") geometry_prefix = next("--geometry");   // clashes, chain envelope, distance against separation (c3d_geometry_replicas, c3d_separation_profile)
        else if (s == "--stratified") stratified_prefix = next("--stratified");   // per-separation Spearman and their combination (c3d_stratified_score)
        else if (s == "--stratified-max-sep") stratified_max_sep = atoi(next("--stratified-max-sep"));
        else if (s == "--per-bead") per_bead_prefix = next("--per-bead");   // per-bead Spearman and restraint tallies (c3d_bead_scores)
        else if (s == "--accessibility") accessibility_prefix = next("--accessibility");   // exposed share of every bead's sphere (c3d_accessibility)
        else if (s == "--compartments") compartments_prefix = next("--compartments");   // compartment eigenvectors of IF, consensus and models (c3d_compartments)
        else if (s == "--compartment-vectors") compartment_vectors = atoi(next("--compartment-vectors"));
        else if (s == "--compartment-iters") compartment_iters = atoi(next("--compartment-iters"));
        else if (s == "--compartment-min-sep") compartment_min_sep = atoi(next("--compartment-min-sep"));
        else if (s == "--insulation") insulation_prefix = next("--insulation");   // insulation profiles and domain boundaries (c3d_insulation)
        else if (s == "--insulation-windows") { insulation_windows = next("--insulation-windows"); insulation_windows_given = true; }
        else if (s == "--insulation-contact") insulation_contact = atof(next("--insulation-contact"));
        else if (s == "--insulation-tol") insulation_tol = atoi(next("--insulation-tol"));
        else if (s == "--entanglement") entanglement_prefix = next("--entanglement");   // writhe, average crossing number, linking (c3d_entanglement)
        else if (s == "--entangle-sep") entangle_sep = next("--entangle-sep");
        else if (s == "--entangle-bounds") entangle_bounds = next("--entangle-bounds");
        else if (s == "--loops") loops_prefix = next("--loops");                  // loop enrichment of IF and the models (c3d_loops)
        else if (s == "--loop-window") loop_window = atoi(next("--loop-window"));
        else if (s == "--loop-peak") loop_peak = atoi(next("--loop-peak"));
        else if (s == "--loop-sep") loop_sep = next("--loop-sep");
        else if (s == "--loop-thr") loop_thr = next("--loop-thr");
        else if (s == "--loop-list") loop_list = next("--loop-list");
        else if (s == "--balance") balance_method = next("--balance");   // balance the raw matrix first (c3d_balance_matrix)
        else if (s == "--balance-ignore-diags") balance_ignore_diags = atoi(next("--balance-ignore-diags"));
        else if (s == "--balance-min-nnz") balance_min_nnz = atoi(next("--balance-min-nnz"));
        else if (s == "--balance-tol") balance_tol = atof(next("--balance-tol"));
        else if (s == "--balance-iters") balance_iters = atoi(next("--balance-iters"));
        else if (s == "--balance-out") balance_out = next("--balance-out");
        else if (s == "--map-similarity") mapsim_files.push_back(next("--map-similarity"));   // compare contact maps (c3d_map_similarity)
        else if (s == "--map-similarity-h") mapsim_h = next("--map-similarity-h");
        else if (s == "--map-similarity-sep") mapsim_sep = next("--map-similarity-sep");
        else if (s == "--map-similarity-out") mapsim_out = next("--map-similarity-out");
        else if (s == "--bead-radius") bead_radius = atof(next("--bead-radius"));
        else if (s == "--probe-radius") probe_radius = atof(next("--probe-radius"));
        else if (s == "--sphere-points") sphere_points = atoi(next("--sphere-points"));
        else if (s == "--clash-cutoff") clash_cutoff = atof(next("--clash-cutoff"));
        else if (s == "--clash-sep") clash_sep = atoi(next("--clash-sep"));
        else if (s == "-h" || s == "--help") { usage(); return 0; }
        else { fprintf(stderr, "c3d_solve: unknown option %s\n", s.c_str()); usage(); return 2; }
    }
    if (out_dir.empty() || (if_path.empty() == tbl_path.empty()) || models < 1) { usage(); return 2; }
    if (!stratified_prefix.empty() && if_path.empty()) { fprintf(stderr, "c3d_solve: --stratified needs --if: a run started from --tbl has no IF matrix\n"); return 2; }
    if (!per_bead_prefix.empty() && if_path.empty()) { fprintf(stderr, "c3d_solve: --per-bead needs --if: a run started from --tbl has no IF matrix\n"); return 2; }
    if (!compartments_prefix.empty() && if_path.empty()) { fprintf(stderr, "c3d_solve: --compartments needs --if: a run started from --tbl has no IF matrix\n"); return 2; }
    if (!insulation_prefix.empty() && if_path.empty()) { fprintf(stderr, "c3d_solve: --insulation needs --if: a run started from --tbl has no IF matrix\n"); return 2; }
    if (!loops_prefix.empty() && if_path.empty()) { fprintf(stderr, "c3d_solve: --loops needs --if: a run started from --tbl has no IF matrix\n"); return 2; }
    if ((!balance_method.empty() || !balance_out.empty()) && if_path.empty()) { fprintf(stderr, "c3d_solve: --balance needs --if: a run started from --tbl has no matrix to balance\n"); return 2; }
    if (!mapsim_files.empty() && if_path.empty()) { fprintf(stderr, "c3d_solve: --map-similarity needs --if: a run started from --tbl has no matrix to compare\n"); return 2; }
    if (mapsim_files.empty() && !mapsim_out.empty()) { fprintf(stderr, "c3d_solve: --map-similarity-out needs --map-similarity <file>\n"); return 2; }
    if ((int)mapsim_files.size() > C3D_MAPSIM_MAX_MAPS - 1) { fprintf(stderr, "c3d_solve: --map-similarity: at most %d files\n", C3D_MAPSIM_MAX_MAPS - 1); return 2; }
    if (!balance_out.empty() && balance_method.empty()) { fprintf(stderr, "c3d_solve: --balance-out needs --balance <ice|vc|sqrt-vc>\n"); return 2; }
    if (!balance_method.empty() && balance_method != "ice" && balance_method != "vc" && balance_method != "sqrt-vc") {
        fprintf(stderr, "c3d_solve: --balance takes ice, vc or sqrt-vc\n");
        return 2;
    }
    if (id.empty()) {
        std::string base = if_path.empty() ? std::string("model") : if_path.substr(if_path.find_last_of('/') + 1);
        if (base.size() > 4 && base.substr(base.size() - 4) == ".txt") base.resize(base.size() - 4);
        id = base;
    }
    if (!seq_arg.empty()) {           // residue names: letters, or @file in FASTA form (header lines skipped)
        std::string letters = seq_arg;
        if (seq_arg[0] == '@') {
            FILE* f = fopen(seq_arg.c_str() + 1, "r");
            if (!f) { fprintf(stderr, "c3d_solve: cannot read %s\n", seq_arg.c_str() + 1); return 2; }
            letters.clear();
            char line[4096];
            while (fgets(line, sizeof line, f)) if (line[0] != '>') letters += line;
            fclose(f);
        }
        c3d_set_residue_sequence(letters.c_str());
    }
    mkdir(out_dir.c_str(), 0755);   // like the reference (:45): create the output directory if missing
    { FILE* f = fopen((out_dir + "/iam.running").c_str(), "w"); if (!f) { fprintf(stderr, "c3d_solve: cannot write into %s\n", out_dir.c_str()); return 1; } fclose(f); }
    remove((out_dir + "/iam.failed").c_str());

    c3d_ctx* ctx = nullptr;
    CHECK(c3d_create(device, &ctx));
    const double t_ctx = now_s();
    c3d_model model;
    c3d_default_model(&model);
    CHECK(c3d_set_model(ctx, &model));

    int n = 0, R = 0;
    std::vector<int32_t> ri, rj, rt;
    double* IF = nullptr;
    if (!if_path.empty()) {
        CHECK(c3d_parse_if_file(if_path.c_str(), &IF, &n));
        // a matrix beyond the default limit is what the user asked for: raise the limit to it (the library refuses beyond its ceiling)
        if (n > C3D_MAX_BEADS_DEFAULT && n <= C3D_MAX_BEADS_LIMIT) CHECK(c3d_set_option(ctx, "max_beads", n));
        if (!mapsim_files.empty()) {
            // the matrix as read against the listed ones, before anything changes it
            const int Q = 1 + (int)mapsim_files.size();
            std::vector<double> maps((size_t)Q * n * n);
            memcpy(maps.data(), IF, sizeof(double) * (size_t)n * n);
            for (int m = 1; m < Q; ++m) {
                double* other = nullptr;
                int no = 0;
                CHECK(c3d_parse_if_file(mapsim_files[m - 1].c_str(), &other, &no));
                if (no != n) { fprintf(stderr, "c3d_solve: --map-similarity %s has %d bins, the matrix of --if %d\n", mapsim_files[m - 1].c_str(), no, n); c3d_free(other); return fail_exit(out_dir); }
                memcpy(maps.data() + (size_t)m * n * n, other, sizeof(double) * (size_t)n * n);
                c3d_free(other);
            }
            std::vector<int32_t> hw;
            for (const char* q = mapsim_h.c_str(); *q;) {
                char* end = nullptr;
                const long v = strtol(q, &end, 10);
                if (end == q) { fprintf(stderr, "c3d_solve: --map-similarity-h takes a list such as 0,1,2\n"); return fail_exit(out_dir); }
                hw.push_back((int32_t)v);
                q = *end == ',' ? end + 1 : end;
                if (*end && *end != ',') { fprintf(stderr, "c3d_solve: --map-similarity-h takes a list such as 0,1,2\n"); return fail_exit(out_dir); }
            }
            int lo = 1, hi = 0;
            if (!mapsim_sep.empty() && sscanf(mapsim_sep.c_str(), "%d:%d", &lo, &hi) != 2) { fprintf(stderr, "c3d_solve: --map-similarity-sep takes lo:hi\n"); return fail_exit(out_dir); }
            const int H = (int)hw.size(), top = hi ? hi : n - 1, S = top >= lo ? top - lo + 1 : 1, P = Q * (Q - 1) / 2;
            std::vector<double> scc((size_t)H * Q * Q), rho((size_t)H * P * S);
            std::vector<int64_t> counts((size_t)H * P * S * 3);
            CHECK(c3d_map_similarity(ctx, maps.data(), Q, n, hw.data(), H, lo, hi, 0, scc.data(), rho.data(), nullptr, counts.data(), nullptr, nullptr));
            for (int k = 0; k < H; ++k)
                for (int m = 0; m < Q; ++m) {
                    printf("Similarity : h %d map %d :", hw[k], m + 1);
                    for (int q = 0; q < Q; ++q) printf(" %.17g", scc[((size_t)k * Q + m) * Q + q]);
                    printf("\n");
                }
            if (!mapsim_out.empty()) {
                const std::string spath = mapsim_out + "_scc.txt", tpath = mapsim_out + "_strata.txt";
                FILE* f = fopen(spath.c_str(), "w");
                if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", spath.c_str()); return fail_exit(out_dir); }
                fprintf(f, "h map scc...\n");
                for (int k = 0; k < H; ++k)
                    for (int m = 0; m < Q; ++m) {
                        fprintf(f, "%d %d", hw[k], m + 1);
                        for (int q = 0; q < Q; ++q) fprintf(f, " %.17g", scc[((size_t)k * Q + m) * Q + q]);
                        fprintf(f, "\n");
                    }
                fclose(f);
                f = fopen(tpath.c_str(), "w");
                if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", tpath.c_str()); return fail_exit(out_dir); }
                fprintf(f, "h map_p map_q separation kept rho\n");
                for (int k = 0; k < H; ++k)
                    for (int p = 0, pr = 0; p < Q; ++p)
                        for (int q = p + 1; q < Q; ++q, ++pr)
                            for (int s = 0; s < S; ++s) {
                                const size_t at = ((size_t)k * P + pr) * S + s;
                                fprintf(f, "%d %d %d %d %lld %.17g\n", hw[k], p + 1, q + 1, lo + s, (long long)counts[at * 3], rho[at]);
                            }
                fclose(f);
            }
        }
        if (!balance_method.empty()) {
            // raw counts in, the balanced matrix over IF: everything below reads IF
            const int method = balance_method == "ice" ? C3D_BALANCE_ICE : balance_method == "vc" ? C3D_BALANCE_VC : C3D_BALANCE_SQRT_VC;
            std::vector<double> weights(n), balanced((size_t)n * n), report(C3D_BALANCE_REPORT);
            std::vector<int32_t> masked(n);
            CHECK(c3d_balance_matrix(ctx, IF, n, method, 0, balance_ignore_diags, balance_min_nnz, nullptr, nullptr, balance_tol, balance_iters, 1.0, weights.data(),
                                     masked.data(), balanced.data(), nullptr, report.data(), nullptr));
            memcpy(IF, balanced.data(), sizeof(double) * balanced.size());
            if (!quiet)
                printf("Balanced   : %s, %d rounds, %s, variance %.3g, %d of %d bins kept\n", balance_method.c_str(), (int)report[0],
                       report[1] != 0 ? "converged" : "not converged", report[2], (int)report[3], n);
            if (!balance_out.empty()) {
                const std::string wpath = balance_out + "_weights.txt", mpath = balance_out + "_matrix.txt";
                FILE* f = fopen(wpath.c_str(), "w");
                if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", wpath.c_str()); return fail_exit(out_dir); }
                fprintf(f, "bead weight masked\n");
                for (int i = 0; i < n; ++i) fprintf(f, "%d %.17g %d\n", i + 1, weights[i], masked[i]);
                fclose(f);
                f = fopen(mpath.c_str(), "w");
                if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", mpath.c_str()); return fail_exit(out_dir); }
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < n; ++j) fprintf(f, j + 1 < n ? "%.17g " : "%.17g\n", IF[(size_t)i * n + j]);
                fclose(f);
            }
        }
        CHECK(c3d_set_if_matrix(ctx, IF, n, alpha, K));
        std::vector<int32_t> d10((size_t)n * n);
        CHECK(c3d_get_dist10(ctx, d10.data()));
        CHECK(c3d_write_front_half(d10.data(), n, model.min_sep, (out_dir + "/" + id + ".dist").c_str(),
                                   (out_dir + "/" + id + ".rr").c_str(), (out_dir + "/contact.tbl").c_str(), &R));
        if (!quiet) printf("L          : %d\nRestraints : %d lines in tbl file\n", n, R);
    } else {
        int32_t *pi = nullptr, *pj = nullptr, *pt = nullptr;
        CHECK(c3d_read_tbl(tbl_path.c_str(), &pi, &pj, &pt, &R));
        ri.assign(pi, pi + R); rj.assign(pj, pj + R); rt.assign(pt, pt + R);
        c3d_free(pi); c3d_free(pj); c3d_free(pt);
        n = n_beads;
        for (int k = 0; k < R; ++k) { if (ri[k] > n) n = ri[k]; if (rj[k] > n) n = rj[k]; }
        if (n > C3D_MAX_BEADS_DEFAULT && n <= C3D_MAX_BEADS_LIMIT) CHECK(c3d_set_option(ctx, "max_beads", n));
        CHECK(c3d_set_restraints(ctx, n, R, ri.data(), rj.data(), rt.data()));
    }

    const double t_front = now_s();
    std::vector<c3d_stage> stages(c3d_default_schedule(nullptr, 0, min_steps));
    c3d_default_schedule(stages.data(), (int)stages.size(), min_steps);
    if (lbfgs) stages.back().kind = 8;
    c3d_fire_params fire;
    c3d_default_fire(&fire);
    CHECK(c3d_set_option(ctx, "final_minimiser", final_min));
    CHECK(c3d_set_schedule(ctx, stages.data(), (int)stages.size(), &fire, (float)gtol, 250));
    CHECK(c3d_set_option(ctx, "use_graph", use_graph));
    if (precision != 32) {
        if (lbfgs) CHECK(c3d_set_option(ctx, "f64_lbfgs", 1));        // --lbfgs beside --precision 64 is the consent to the fp64 L-BFGS stage
        CHECK(c3d_set_option(ctx, "precision", precision));
        // as with max_beads above: the matrix that was read is the user's consent to the fp64 target matrix it needs
        if (n > C3D_F64_MAX_BEADS_DEFAULT && n <= C3D_F64_MAX_BEADS_LIMIT) CHECK(c3d_set_option(ctx, "f64_max_beads", n));
    }
    CHECK(c3d_init_replicas(ctx, models, seed, first_rep));
    if (embed_max_beads) CHECK(c3d_set_option(ctx, "embed_max_beads", embed_max_beads));
    if (embed) CHECK(c3d_embed_replicas(ctx, 50));
    CHECK(c3d_run(ctx));
    const double t_run = now_s();

    std::vector<float> xyz((size_t)models * n * 3);
    std::vector<double> en((size_t)models * 3);
    CHECK(c3d_get_energies(ctx, en.data()));
    if (superpose || !rmsf_path.empty()) {
        // the best-ranked model (lowest int(E_noe), the lower index on a tie: c3d_rank's rule) is the frame and the hand of all.  Energies,
        // assessment and Spearman do not depend on either: they are not computed again.
        int best = 0;
        for (int r = 1; r < models; ++r) if ((long)en[3 * r] < (long)en[3 * best]) best = r;
        if (!rmsf_path.empty()) {
            std::vector<double> mean((size_t)n * 3), rmsf(n);
            std::vector<int32_t> mir(models);
            CHECK(c3d_superpose_replicas(ctx, best, nullptr, C3D_SUPERPOSE_MIRROR, 3, nullptr, mir.data(), mean.data(), rmsf.data()));
            int nm = 0;
            for (int r = 0; r < models; ++r) nm += mir[r];
            FILE* f = fopen(rmsf_path.c_str(), "w");
            if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", rmsf_path.c_str()); return fail_exit(out_dir); }
            fprintf(f, "# bead mean_x mean_y mean_z rmsf   (%d models superposed on %s_%u.pdb, 3 generalized-Procrustes iterations; %d mirrored)\n", models,
                    id.c_str(), first_rep + (unsigned)best + 1u, nm);
            for (int i = 0; i < n; ++i) fprintf(f, "%d %.3f %.3f %.3f %.3f\n", i + 1, mean[3 * (size_t)i], mean[3 * (size_t)i + 1], mean[3 * (size_t)i + 2], rmsf[i]);
            fclose(f);
        }
        if (superpose) CHECK(c3d_superpose_replicas(ctx, best, nullptr, C3D_SUPERPOSE_MIRROR | C3D_SUPERPOSE_APPLY, 0, nullptr, nullptr, nullptr, nullptr));
    }
    CHECK(c3d_get_coords(ctx, xyz.data()));
    for (int r = 0; r < models; ++r) {
        char name[64];
        snprintf(name, sizeof name, "%s_%u.pdb", id.c_str(), first_rep + (unsigned)r + 1u);
        CHECK(c3d_write_pdb((out_dir + "/" + name).c_str(), xyz.data() + (size_t)r * n * 3, n, en[3 * r], en[3 * r + 1],
                            en[3 * r + 2], name));
        if (accepted) {
            // the accepted twin: same coordinates, same REMARK rows (the reference's assess_dgsa then drops the trial file, :791-795).  CNS's
            // acceptance thresholds are defined on covalent geometry a bead model does not have: with --accepted every model is "accepted"
            snprintf(name, sizeof name, "%sa_%u.pdb", id.c_str(), first_rep + (unsigned)r + 1u);
            CHECK(c3d_write_pdb((out_dir + "/" + name).c_str(), xyz.data() + (size_t)r * n * 3, n, en[3 * r], en[3 * r + 1],
                                en[3 * r + 2], name));
        }
    }
    if (!similarity_path.empty()) {
        // which replicas share a fold: c3d_model_similarity for every ordered pair, from the resident coordinates
        std::vector<double> rho((size_t)models * models), rmsd((size_t)models * models);
        CHECK(c3d_compare_replicas(ctx, nullptr, 0, rho.data(), rmsd.data()));
        FILE* f = fopen(similarity_path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", similarity_path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# replica_a replica_b spearman rmsd   (pair distances of a scaled onto b's; replica r is %s_<r+1>.pdb)\n", id.c_str());
        for (int a = 0; a < models; ++a)
            for (int b = 0; b < models; ++b)
                if (a != b) fprintf(f, "%u %u %.5f %.5f\n", first_rep + (unsigned)a, first_rep + (unsigned)b, rho[(size_t)a * models + b], rmsd[(size_t)a * models + b]);
        fclose(f);
    }
    if (!ensemble_prefix.empty()) {
        // the models that count: all of them, or the best-ranked few in c3d_rank's order (which is then the summation order)
        std::vector<int32_t> order(models);
        CHECK(c3d_rank(ctx, order.data()));
        const int top = ensemble_top > 0 && ensemble_top < models ? ensemble_top : 0, Kp = top ? top : models;
        const double cutoff = ensemble_cutoff < 0 ? 2.0 * (double)model.b0 : ensemble_cutoff;
        const bool with_contact = cutoff > 0;
        const size_t nn = (size_t)n * n;
        std::vector<double> maps((with_contact ? 3 : 2) * nn);
        CHECK(c3d_ensemble_map(ctx, nullptr, 0, top ? order.data() : nullptr, top, cutoff, maps.data(), maps.data() + nn, with_contact ? maps.data() + 2 * nn : nullptr));
        const char* const names[3] = {"_mean.txt", "_sd.txt", "_contact.txt"};
        for (int k = 0; k < (with_contact ? 3 : 2); ++k) {
            const std::string path = ensemble_prefix + names[k];
            FILE* f = fopen(path.c_str(), "w");
            if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
            const double* M = maps.data() + (size_t)k * nn;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) fprintf(f, k == 2 ? "%.4f%s" : "%.3f%s", M[(size_t)i * n + j], j + 1 < n ? " " : "\n");
            fclose(f);
        }
        if (IF) {
            double rho_mean = 0, rho_contact = 0;
            CHECK(c3d_ensemble_score(ctx, IF, 3, nullptr, 0, top ? order.data() : nullptr, top, cutoff, &rho_mean, with_contact ? &rho_contact : nullptr));
            if (with_contact) printf("ensemble: %d models, Spearman(IF, mean d) = %.4f, Spearman(IF, contact) = %.4f\n", Kp, rho_mean, rho_contact);
            else printf("ensemble: %d models, Spearman(IF, mean d) = %.4f, Spearman(IF, contact) = none (no cutoff)\n", Kp, rho_mean);
        } else {
            printf("ensemble: %d models, maps written; no Spearman line: a run started from --tbl has no IF matrix to compare them with\n", Kp);
        }
    }
    if (!geometry_prefix.empty()) {
        std::vector<int32_t> order(models);
        CHECK(c3d_rank(ctx, order.data()));
        std::vector<int64_t> clashes(models);
        std::vector<double> nearest((size_t)models * n), chain((size_t)models * C3D_GEOMETRY_FIELDS);
        CHECK(c3d_geometry_replicas(ctx, nullptr, 0, clash_cutoff, clash_sep, clashes.data(), nullptr, nearest.data(), chain.data()));
        std::string path = geometry_prefix + "_geometry.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# rank model clashes nearest bond_mean bond_sd i2_mean i2_sd rg extent   (pairs |i-j| >= %d; clash: d <= %g A; model r is %s_<r>.pdb)\n", clash_sep,
                clash_cutoff, id.c_str());
        for (int k = 0; k < models; ++k) {
            const int r = order[k];
            double lo = nearest[(size_t)r * n];
            for (int i = 1; i < n; ++i) lo = nearest[(size_t)r * n + i] < lo ? nearest[(size_t)r * n + i] : lo;
            const double* c6 = chain.data() + (size_t)r * C3D_GEOMETRY_FIELDS;
            fprintf(f, "%d %u %lld %.3f %.3f %.3f %.3f %.3f %.3f %.3f\n", k + 1, first_rep + (unsigned)r + 1u, (long long)clashes[r], lo, c6[0], c6[1], c6[2], c6[3], c6[4], c6[5]);
        }
        fclose(f);
        // the profile over the models of --ensemble: all, or the best-ranked few in rank order
        const int top = ensemble_top > 0 && ensemble_top < models ? ensemble_top : 0;
        const double cutoff = ensemble_cutoff < 0 ? 2.0 * (double)model.b0 : ensemble_cutoff;
        const bool with_contact = cutoff > 0;
        std::vector<double> prof(3 * (size_t)n);
        CHECK(c3d_separation_profile(ctx, nullptr, 0, top ? order.data() : nullptr, top, cutoff, prof.data(), prof.data() + n, with_contact ? prof.data() + 2 * (size_t)n : nullptr));
        path = geometry_prefix + "_separation.txt";
        f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        if (with_contact) fprintf(f, "# s mean sd contact   (%d models; contact: d < %g A)\n", top ? top : models, cutoff);
        else fprintf(f, "# s mean sd   (%d models)\n", top ? top : models);
        for (int s = 0; s < n; ++s) {
            if (with_contact) fprintf(f, "%d %.3f %.3f %.6f\n", s, prof[s], prof[(size_t)n + s], prof[2 * (size_t)n + s]);
            else fprintf(f, "%d %.3f %.3f\n", s, prof[s], prof[(size_t)n + s]);
        }
        fclose(f);
    }
    if (!stratified_prefix.empty()) {
        std::vector<int32_t> order(models);
        CHECK(c3d_rank(ctx, order.data()));
        const int range = 3, hi = stratified_max_sep ? stratified_max_sep : n - 1;       // spearman_IF_pdb.pl's range
        std::vector<double> rho((size_t)models * n), scc(models);
        CHECK(c3d_stratified_score(ctx, IF, range, stratified_max_sep, nullptr, 0, rho.data(), scc.data(), nullptr));
        auto put = [](FILE* f, double v) { if (std::isnan(v)) fprintf(f, " nan"); else fprintf(f, " %.6f", v); };
        std::string path = stratified_prefix + "_scc.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# rank model scc   (separations %d..%d; model r is %s_<r>.pdb)\n", range, hi, id.c_str());
        for (int k = 0; k < models; ++k) {
            fprintf(f, "%d %u", k + 1, first_rep + (unsigned)order[k] + 1u);
            put(f, scc[order[k]]);
            fprintf(f, "\n");
        }
        fclose(f);
        path = stratified_prefix + "_strata.txt";
        f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# s N rho_1 ... rho_%d   (columns: the models in rank order)\n", models);
        for (int s = range; s <= hi; ++s) {
            fprintf(f, "%d %d", s, n - s);
            for (int k = 0; k < models; ++k) put(f, rho[(size_t)order[k] * n + s]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    if (!per_bead_prefix.empty()) {
        std::vector<int32_t> order(models);
        CHECK(c3d_rank(ctx, order.data()));
        const int range = 3;                                                              // spearman_IF_pdb.pl's range
        std::vector<double> rho((size_t)models * n);
        std::vector<int32_t> restrained(n), satisfied((size_t)models * n);
        std::vector<int64_t> dev((size_t)models * n);
        CHECK(c3d_bead_scores(ctx, IF, range, nullptr, 0, nullptr, 0, rho.data(), nullptr, restrained.data(), satisfied.data(), dev.data()));
        const std::string path = per_bead_prefix + "_beads.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# bead restrained rho_1 satisfied_1 dev_1 ... rho_%d satisfied_%d dev_%d   (columns: the models in rank order; model r is %s_<r>.pdb)\n", models, models,
                models, id.c_str());
        fprintf(f, "# models:");
        for (int k = 0; k < models; ++k) fprintf(f, " %u", first_rep + (unsigned)order[k] + 1u);
        fprintf(f, "\n# rho: Spearman(IF[i][j], d(i,j)) over |i-j| >= %d; satisfied: net count within 0.5 A; dev: summed deviation beyond 0.2 A, in A\n", range);
        for (int i = 0; i < n; ++i) {
            fprintf(f, "%d %d", i + 1, restrained[i]);
            for (int k = 0; k < models; ++k) {
                const size_t at = (size_t)order[k] * n + i;
                if (std::isnan(rho[at])) fprintf(f, " nan"); else fprintf(f, " %.6f", rho[at]);
                fprintf(f, " %d %.3f", satisfied[at], (double)dev[at] / 1000.0);
            }
            fprintf(f, "\n");
        }
        fclose(f);
    }
    if (!accessibility_prefix.empty()) {
        std::vector<int32_t> order(models);
        CHECK(c3d_rank(ctx, order.data()));
        const double radius = bead_radius < 0 ? 0.5 * (double)model.b0 : bead_radius, probe = probe_radius < 0 ? 0.5 * (double)model.b0 : probe_radius;
        const double R = radius + probe, sphere = 4.0 * 3.14159265358979323846 * R * R;
        std::vector<int32_t> exposed((size_t)models * n);
        CHECK(c3d_accessibility(ctx, nullptr, 0, radius, probe, nullptr, sphere_points, exposed.data(), nullptr));
        const std::string path = accessibility_prefix + "_accessibility.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# bead mean f_1 ... f_%d   (exposed share of a bead's sphere points; columns: the models in rank order; model r is %s_<r>.pdb)\n", models, id.c_str());
        fprintf(f, "# models:");
        for (int k = 0; k < models; ++k) fprintf(f, " %u", first_rep + (unsigned)order[k] + 1u);
        fprintf(f, "\n# R = %g A (bead radius %g + probe radius %g), P = %d points, accessible area of every model in A^2:", R, radius, probe, sphere_points);
        for (int k = 0; k < models; ++k) {
            long long open = 0;
            for (int i = 0; i < n; ++i) open += exposed[(size_t)order[k] * n + i];
            fprintf(f, " %.1f", sphere * (double)open / (double)sphere_points);
        }
        fprintf(f, "\n");
        for (int i = 0; i < n; ++i) {
            long long open = 0;
            for (int k = 0; k < models; ++k) open += exposed[(size_t)k * n + i];
            fprintf(f, "%d %.4f", i + 1, (double)open / ((double)sphere_points * models));
            for (int k = 0; k < models; ++k) fprintf(f, " %.4f", (double)exposed[(size_t)order[k] * n + i] / (double)sphere_points);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    if (!compartments_prefix.empty()) {
        std::vector<int32_t> order(models);
        CHECK(c3d_rank(ctx, order.data()));
        // the maps: IF, the models in rank order, their consensus
        const int nv = compartment_vectors, Q = models + 2;
        const size_t vec = (size_t)(nv > 0 ? nv : 1);
        std::vector<double> vectors((size_t)Q * vec * n), share((size_t)Q * vec), residual((size_t)Q * vec), agreement((size_t)(Q - 1) * vec * vec), side((size_t)(Q - 1) * vec);
        CHECK(c3d_compartments(ctx, IF, nullptr, 0, order.data(), models, C3D_COMPARTMENT_CONSENSUS, compartment_min_sep, nv, compartment_iters, nullptr, nullptr,
                               vectors.data(), share.data(), residual.data(), agreement.data(), side.data(), nullptr));
        const std::string path = compartments_prefix + "_compartments.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# bead IF consensus pc1_1 ... pc1_%d   (the first compartment eigenvector; columns: the models in rank order; model r is %s_<r>.pdb)\n", models, id.c_str());
        fprintf(f, "# models:");
        for (int k = 0; k < models; ++k) fprintf(f, " %u", first_rep + (unsigned)order[k] + 1u);
        fprintf(f, "\n# %d vector(s), %d rounds, min_sep %d; per vector: share residual agreement same_side\n", nv, compartment_iters, compartment_min_sep);
        for (int q = 0; q < Q; ++q) {
            if (q == 0) fprintf(f, "# IF:");
            else if (q == Q - 1) fprintf(f, "# consensus:");
            else fprintf(f, "# model %d:", q);
            for (int a = 0; a < nv; ++a) {
                fprintf(f, " %.6f %.3e", share[(size_t)q * nv + a], residual[(size_t)q * nv + a]);
                if (q > 0) fprintf(f, " %.6f %.6f", agreement[((size_t)(q - 1) * nv + a) * nv + a], side[(size_t)(q - 1) * nv + a]);
            }
            fprintf(f, "\n");
        }
        for (int i = 0; i < n; ++i) {
            fprintf(f, "%d %.6f %.6f", i + 1, vectors[(size_t)i], vectors[(size_t)(Q - 1) * nv * n + i]);
            for (int k = 1; k <= models; ++k) fprintf(f, " %.6f", vectors[(size_t)k * nv * n + i]);
            fprintf(f, "\n");
        }
        fclose(f);
    }
    if (!insulation_prefix.empty()) {
        std::vector<int32_t> order(models), win;
        CHECK(c3d_rank(ctx, order.data()));
        // the default windows are clipped to those that fit the chain; a list of the user's goes to the entry as it is
        for (const char* p = insulation_windows.c_str(); *p;) {
            char* end = nullptr;
            const long w = strtol(p, &end, 10);
            if (end == p) { fprintf(stderr, "c3d_solve: --insulation-windows takes a comma-separated list of integers\n"); return fail_exit(out_dir); }
            if (insulation_windows_given || 2 * w + 1 <= n) win.push_back((int32_t)w);
            p = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') { fprintf(stderr, "c3d_solve: --insulation-windows takes a comma-separated list of integers\n"); return fail_exit(out_dir); }
        }
        // the maps: IF, the models in rank order, their consensus
        const int Q = models + 2, nw = (int)win.size();
        const size_t rows = (size_t)Q * (nw > 0 ? nw : 1) * n, fits = (size_t)(Q - 1) * (nw > 0 ? nw : 1);
        const double min_strength = 0.1;
        std::vector<double> score(rows), strength(rows), fit_r(fits);
        std::vector<int32_t> boundary(rows), counts(4 * fits);
        CHECK(c3d_insulation(ctx, IF, nullptr, 0, order.data(), models, C3D_INSULATION_CONSENSUS | (insulation_contact != 0 ? C3D_INSULATION_CONTACT : 0), win.data(), nw,
                             insulation_contact, min_strength, insulation_tol, nullptr, score.data(), boundary.data(), strength.data(), fit_r.data(), counts.data(), nullptr));
        const std::string path = insulation_prefix + "_insulation.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# window bead IF consensus IF_boundary IF_strength consensus_boundary consensus_strength models   (insulation scores; models: how many of the %d models have a boundary of strength >= %.1f within %d beads; model r is %s_<r>.pdb)\n",
                models, min_strength, insulation_tol, id.c_str());
        fprintf(f, "# models:");
        for (int k = 0; k < models; ++k) fprintf(f, " %u", first_rep + (unsigned)order[k] + 1u);
        if (insulation_contact != 0) fprintf(f, "\n# contacts below %.3f A; per map and window: fit_r n_IF n_map IF_matched map_matched\n", insulation_contact);
        else fprintf(f, "\n# mean distance; per map and window: fit_r n_IF n_map IF_matched map_matched\n");
        for (int k = 0; k < nw; ++k)
            for (int q = 1; q < Q; ++q) {
                const size_t at = (size_t)(q - 1) * nw + k;
                if (q == Q - 1) fprintf(f, "# window %d consensus:", win[k]);
                else fprintf(f, "# window %d model %d:", win[k], q);
                fprintf(f, " %.6f %d %d %d %d\n", fit_r[at], counts[4 * at], counts[4 * at + 1], counts[4 * at + 2], counts[4 * at + 3]);
            }
        for (int k = 0; k < nw; ++k)
            for (int i = 0; i < n; ++i) {
                const size_t a_if = (size_t)k * n + i, a_co = ((size_t)(Q - 1) * nw + k) * n + i;
                int support = 0;
                for (int q = 1; q <= models; ++q) {
                    const size_t row = ((size_t)q * nw + k) * n;
                    bool near = false;
                    for (int j = i - std::min(insulation_tol, i); j <= i + std::min(insulation_tol, n - 1 - i); ++j)
                        near = near || (boundary[row + j] && strength[row + j] >= min_strength);
                    support += near;
                }
                fprintf(f, "%d %d %.6f %.6f %d %.6f %d %.6f %d\n", win[k], i + 1, score[a_if], score[a_co], boundary[a_if], strength[a_if], boundary[a_co], strength[a_co], support);
            }
        fclose(f);
    }
    if (!loops_prefix.empty()) {
        std::vector<int32_t> order(models), listed;
        CHECK(c3d_rank(ctx, order.data()));
        const int w = loop_window;
        int lo = 2 * w + 1, hi = std::min(n - 1, lo + C3D_LOOP_MAX_BAND - 1);
        if (!loop_sep.empty() && sscanf(loop_sep.c_str(), "%d:%d", &lo, &hi) != 2) { fprintf(stderr, "c3d_solve: --loop-sep takes MIN:MAX\n"); return fail_exit(out_dir); }
        double thr[4];
        if (sscanf(loop_thr.c_str(), "%lf,%lf,%lf,%lf", &thr[0], &thr[1], &thr[2], &thr[3]) != 4) { fprintf(stderr, "c3d_solve: --loop-thr takes four numbers a,b,c,d\n"); return fail_exit(out_dir); }
        if (!loop_list.empty()) {
            FILE* lf = fopen(loop_list.c_str(), "r");
            if (!lf) { fprintf(stderr, "c3d_solve: cannot read %s\n", loop_list.c_str()); return fail_exit(out_dir); }
            // a line is `i j` and whatever columns follow (a <prefix>_loops.txt can be fed back); blank lines and `#` lines are skipped
            char line[4096];
            int row = 0;
            while (fgets(line, sizeof line, lf)) {
                ++row;
                const char* q = line;
                while (*q == ' ' || *q == '\t') ++q;
                if (*q == '#' || *q == '\n' || *q == '\r' || *q == 0) continue;
                int a, b, used = 0;
                if (sscanf(q, "%d %d%n", &a, &b, &used) != 2 || (q[used] && !isspace((unsigned char)q[used])) || listed.size() / 2 >= (size_t)C3D_LOOP_MAX_LIST) {
                    fprintf(stderr, "c3d_solve: --loop-list %s, line %d: not a pair of bead numbers `i j`, or more than %d pairs\n", loop_list.c_str(), row, C3D_LOOP_MAX_LIST);
                    fclose(lf);
                    return fail_exit(out_dir);
                }
                listed.push_back(a - 1);
                listed.push_back(b - 1);
            }
            fclose(lf);
            if (listed.empty()) { fprintf(stderr, "c3d_solve: --loop-list %s holds no pair\n", loop_list.c_str()); return fail_exit(out_dir); }
        }
        // the maps: IF, the models in rank order, their consensus; the list: the file's pixels, else the peaks of IF
        const int Q = models + 2, max_peaks = 4096, merge = std::min(2, w), corner = std::min(3, w);
        const size_t Lmax = loop_list.empty() ? (size_t)max_peaks : listed.size() / 2;
        std::vector<double> at(6 * (size_t)Q * Lmax), p2ll(Q);               // Lmax >= 1: what the call can write
        std::vector<int32_t> peaks(2 * (size_t)max_peaks), closed(2 * (size_t)Q);
        int32_t report[C3D_LOOP_REPORT];
        CHECK(c3d_loops(ctx, IF, nullptr, 0, order.data(), models, C3D_LOOP_CONSENSUS, nullptr, loop_peak, w, lo, hi, thr, 0.0, merge, corner,
                        loop_list.empty() ? nullptr : listed.data(), (int)(listed.size() / 2), max_peaks, nullptr, nullptr, peaks.data(), report, at.data(), closed.data(),
                        nullptr, p2ll.data(), nullptr));
        const int L = loop_list.empty() ? report[2] : (int)(listed.size() / 2);
        const int32_t* px = loop_list.empty() ? peaks.data() : listed.data();
        const std::string path = loops_prefix + "_loops.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# i j IF r_donut r_ll r_h r_v consensus_d consensus_r_donut consensus_r_ll models_closed   (window %d, peak %d, separations %d..%d; %d candidates, %d peaks, %d listed; model r is %s_<r>.pdb)\n",
                w, loop_peak, lo, hi, report[0], report[1], L, id.c_str());
        fprintf(f, "# models:");
        for (int k = 0; k < models; ++k) fprintf(f, " %u", first_rep + (unsigned)order[k] + 1u);
        fprintf(f, "\n");
        for (int l = 0; l < L; ++l) {
            const double* a_if = at.data() + 6 * (size_t)l;
            const double* a_co = at.data() + 6 * ((size_t)(Q - 1) * L + l);
            int shut = 0;
            for (int q = 1; q <= models; ++q) {
                const double* a = at.data() + 6 * ((size_t)q * L + l);
                shut += a[2] < 1.0 && a[3] < 1.0;
            }
            fprintf(f, "%d %d %.6g %.4f %.4f %.4f %.4f %.3f %.4f %.4f %d\n", px[2 * l] + 1, px[2 * l + 1] + 1, a_if[0], a_if[2], a_if[3], a_if[4], a_if[5], a_co[0], a_co[2],
                    a_co[3], shut);
        }
        for (int q = 0; q < Q; ++q) {
            if (q == 0) fprintf(f, "# IF");
            else if (q == Q - 1) fprintf(f, "# consensus");
            else fprintf(f, "# model %d", q);
            fprintf(f, " %d %d %.4f\n", closed[2 * q], closed[2 * q + 1], p2ll[q]);
        }
        fclose(f);
    }
    if (!entanglement_prefix.empty()) {
        std::vector<int32_t> order(models), bounds;
        CHECK(c3d_rank(ctx, order.data()));
        const int S = n - 1;
        int lo = 2, hi = 0;
        if (!entangle_sep.empty() && sscanf(entangle_sep.c_str(), "%d:%d", &lo, &hi) != 2) { fprintf(stderr, "c3d_solve: --entangle-sep takes a:b\n"); return fail_exit(out_dir); }
        if (!entangle_bounds.empty()) {
            FILE* bf = fopen(entangle_bounds.c_str(), "r");
            if (!bf) { fprintf(stderr, "c3d_solve: cannot read %s\n", entangle_bounds.c_str()); return fail_exit(out_dir); }
            int v;
            while (fscanf(bf, "%d", &v) == 1 && bounds.size() <= (size_t)C3D_ENTANGLE_MAX_DOMAINS + 1) bounds.push_back(v);
            const bool whole = feof(bf) != 0;
            fclose(bf);
            if (!whole || bounds.size() < 2) { fprintf(stderr, "c3d_solve: --entangle-bounds %s: not a list of 2 to %d whole numbers\n", entangle_bounds.c_str(), C3D_ENTANGLE_MAX_DOMAINS + 1); return fail_exit(out_dir); }
        }
        const int D = bounds.empty() ? 0 : (int)bounds.size() - 1;
        std::vector<double> writhe(models), acn(models), seg_w((size_t)models * S), seg_a((size_t)models * S), link((size_t)models * D * D), link_abs((size_t)models * D * D);
        CHECK(c3d_entanglement(ctx, nullptr, 0, lo, hi, D ? bounds.data() : nullptr, D, writhe.data(), acn.data(), seg_w.data(), seg_a.data(), D ? link.data() : nullptr,
                               D ? link_abs.data() : nullptr, nullptr));
        double mean = 0, var = 0;
        for (int k = 0; k < models; ++k) mean += writhe[k];
        mean /= models;
        int agree = 0;
        for (int k = 0; k < models; ++k) { var += (writhe[k] - mean) * (writhe[k] - mean); agree += (writhe[k] > 0) == (mean > 0) && (writhe[k] < 0) == (mean < 0); }
        std::string path = entanglement_prefix + "_entanglement.txt";
        FILE* f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# rank model writhe acn acn_per_segment   (%d segments, separations %d..%d; writhe mean %.6f sd %.6f, sign agreement %.3f; model r is %s_<r>.pdb)\n", S, lo,
                hi ? hi : S - 1, mean, std::sqrt(var / models), (double)agree / models, id.c_str());
        for (int k = 0; k < models; ++k) {
            const int r = order[k];
            fprintf(f, "%d %u %.9f %.9f %.9f\n", k + 1, first_rep + (unsigned)r + 1u, writhe[r], acn[r], acn[r] / S);
        }
        fclose(f);
        path = entanglement_prefix + "_segments.txt";
        f = fopen(path.c_str(), "w");
        if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
        fprintf(f, "# model segment seg_writhe seg_acn   (models in rank order; segment s joins beads s and s+1)\n");
        for (int k = 0; k < models; ++k)
            for (int s = 0; s < S; ++s)
                fprintf(f, "%u %d %.9f %.9f\n", first_rep + (unsigned)order[k] + 1u, s + 1, seg_w[(size_t)order[k] * S + s], seg_a[(size_t)order[k] * S + s]);
        fclose(f);
        if (D) {
            path = entanglement_prefix + "_link.txt";
            f = fopen(path.c_str(), "w");
            if (!f) { fprintf(stderr, "c3d_solve: cannot write %s\n", path.c_str()); return fail_exit(out_dir); }
            fprintf(f, "# model p q link link_abs   (%d domains of segments, bounds", D);
            for (int v : bounds) fprintf(f, " %d", v);
            fprintf(f, "; p = q: the domain's own writhe)\n");
            for (int k = 0; k < models; ++k)
                for (int p = 0; p < D; ++p)
                    for (int q = p; q < D; ++q) {
                        const size_t o = ((size_t)order[k] * D + p) * D + q;
                        fprintf(f, "%u %d %d %.9f %.9f\n", first_rep + (unsigned)order[k] + 1u, p + 1, q + 1, link[o], link_abs[o]);
                    }
            fclose(f);
        }
    }
    double ms = 0;
    long steps = 0, launches = 0;
    c3d_last_timing(ctx, &ms, &steps, &launches);
    if (!quiet) {
        printf(accepted ? "trial and accepted structures written.\n" : "trial structures written.\n");
        printf("c3d_solve: %d beads, %d restraints, %d models, %ld SA steps/model in %.1f ms on device %d (%.3g replica-steps/s)\n",
               n, R, models, steps, ms, device, ms > 0 ? 1e3 * (double)steps * models / ms : 0.0);
        if (IF) {
            std::vector<double> rho(models);
            if (c3d_score_replicas(ctx, IF, 3, nullptr, nullptr, rho.data()) == C3D_OK)      // on the device, from the resident coordinates (K6)
                for (int r = 0; r < models; ++r)
                    printf("  model %2u  E_noe %14.2f  Spearman(IF,d) %.4f\n", first_rep + r + 1, en[3 * r], rho[r]);
            else fprintf(stderr, "c3d_solve: models not scored: %s\n", c3d_last_error());
        }
    }
    if (!quiet)
        printf("c3d_solve wall: device init %.3f s, parse + K1 + front-half files %.3f s, anneal (incl. graph build) %.3f s, "
               "read-back + PDB + scoring %.3f s, total %.3f s\n", t_ctx - t_start, t_front - t_ctx, t_run - t_front, now_s() - t_run,
               now_s() - t_start);
    if (IF) c3d_free(IF);
    c3d_destroy(ctx);
    remove((out_dir + "/iam.running").c_str());
    return 0;
}
