/*
 * c3d.h — C ABI of libc3d.so, the MI355X (gfx950) solver that replaces the
 * `cns_solve < dgsa.inp` process the reference shells out to.
 *
 * Reference boundary being replaced (file:line under the reference tree):
 *   chromosome3D.pl:87-89    IF2dist_new / dist2rr / carr2tbl  -> c3d_set_if_matrix,
 *                            c3d_get_dist10, c3d_write_front_half
 *   chromosome3D.pl:254-289  build_models: job.sh -> `cns_solve < dgsa.inp`, success iff
 *                            <ID>_<M>.pdb exists                -> c3d_run / c3d_write_models
 *   chromosome3D.pl:882-1846 the dgsa.inp deck (knobs :1093-1126, protocol :1574-1829)
 *                                                               -> c3d_model / c3d_stage
 *   chromosome3D.pl:769-829  assess_dgsa (rank by int(REMARK noe)) -> c3d_rank, c3d_assess
 *   spearman_IF_pdb.pl:26-70 scoring                            -> c3d_spearman_if_dist
 *
 * Conventions: plain C types only; every function returns C3D_OK (0) or a negative
 * c3d_status; c3d_last_error() gives a thread-local message.  The caller owns all host
 * buffers, the library owns all device memory.  Nothing here falls back to a CPU solver:
 * without a usable HIP device c3d_create fails with C3D_ERR_NO_DEVICE.
 */
#ifndef C3D_H_
#define C3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    C3D_OK = 0,
    C3D_ERR_INVALID = -1,    /* bad argument / call order */
    C3D_ERR_NO_DEVICE = -2,  /* no HIP device, or the gfx950 code object cannot load */
    C3D_ERR_HIP = -3,        /* a HIP runtime call failed */
    C3D_ERR_IO = -4,         /* file could not be read / written / parsed */
    C3D_ERR_NOMEM = -5,
    C3D_ERR_DIVERGED = -6    /* non-finite coordinates/forces after a run */
} c3d_status;

typedef struct c3d_ctx c3d_ctx;

/* Energy model of one bead chain (defaults: c3d_default_model).  Mirrors the deck:
 * con_wt chromosome3D.pl:66,1111,1120; mass/fbeta :1415-1416; SEPARATION :20. */
typedef struct {
    int32_t min_sep;   /* 5: restraints only for |i-j| >= min_sep                        */
    int32_t noe_pot;   /* 0 symmetric soft-square, 1 X-PLOR soft-square, 2 square,
                          3 CNS soft-square with a soft LOWER side too (mrswitch, masym, msoexp; default) */
    int32_t rep_sep;   /* repel acts on |i-j| >= rep_sep (1..3)                          */
    int32_t ang_mode;  /* (i,i+2) term: 0 lower bound only, 1 harmonic                   */
    float s_noe;       /* NOE scale = con_wt = 10                                        */
    float rswitch;     /* 0.5: the upper side is square up to d - t = rswitch            */
    float asym;        /* 2.0: slope of the upper tail in units of rswitch (tail slope = asym x rswitch x S = 10) */
    float k_bond, b0;  /* pseudo-bond (i,i+1)                                            */
    float k_ang, a0;   /* pseudo-angle (i,i+2)                                           */
    float r0_rep;      /* bead contact distance, scaled by stage `repel`                 */
    float k_rep;       /* bead-level repel multiplier                                    */
    float mass;        /* 100 amu                                                        */
    float fbeta;       /* 10 /ps                                                         */
    float masym;       /* noe_pot 3: asymptote slope of the lower side (CNS masymptote)  */
    float mrswitch;    /* noe_pot 3: the lower side is square up to t - d = mrswitch     */
    int32_t msoexp;    /* noe_pot 3: exponent of the lower side's soft form a + b / D^msoexp + masym D beyond mrswitch
                          (CNS msoexponent), 1 or 2; 0 = the default (2).  Shipped: mrswitch 10, masym 0, msoexp 2 — X-PLOR's own defaults
                          (rswitch 10, asymptote 0, soexponent 2), which the deck never overrides for the minus side:
                          the push on a pair far inside its target rises to 2 S mrswitch and then DECAYS as D^-3     */
} c3d_model;   /* ABI: no size / version member — every caller fills the struct through c3d_default_model of the library it links (the Perl
                  binding, c3d_solve, c3d_batch and the ctypes mirror do); `msoexp` was appended in round 4 ("ABI notes") */

/* One stage of the annealing schedule (defaults: c3d_default_schedule, which restates
 * chromosome3D.pl:1631-1700 hot stages, :1729-1782 slow cool, :1790-1803 minimisation). */
typedef struct {
    int32_t kind;      /* 0 MD + T-coupling, 1 MD + velocity rescale, 2 FIRE minimise,
                          5 minimise with two-point (Barzilai-Borwein) step sizes — one force evaluation a step, no energy, the length
                            of a move = the inverse of a one-number curvature estimate from the previous move and the change of the force
                            over it, taken one evaluation late (the replica sums of a step reach the next one) — for the first
                            `final_minimiser_steps` (1000) steps, then FIRE for what is left of nsteps: half the evaluations FIRE needs
                            to the same exit test, the same minima; the default schedule's final stage since round 5
                            (option final_minimiser = 0: a stage of kind 5 is a FIRE stage)
                          8 L-BFGS minimise (opt-in; the reference's method, deck :1790-1803): m = lbfgs_memory pairs (5), the compact
                            form from the projections of the current gradient, a fixed unit step, no energy, no line search, each bead's
                            move capped at fire.max_step, a pair kept only if its curvature is positive, the memory dropped when the
                            direction is not downhill — for the first `final_minimiser_steps` steps, then FIRE from a fresh state for what
                            is left of nsteps (option final_minimiser does not apply to it).  Per-step path only: two launches a step
                            (k_lbfgs_eval, k_lbfgs_move), whatever `resident` says; symmetric tiles do not apply to its steps.  On a
                            precision-64 context it runs in fp64 behind the option f64_lbfgs (k64_lbfgs_eval, k64_lbfgs_move: the same
                            method in doubles, the first length dt_start^2 kAccel / mass formed in fp64); without that option precision
                            64 and a stage of kind 8 refuse each other.  About half the force evaluations of kind 5 to the same exit test */
    int32_t nsteps;
    float dt;          /* ps (MD)                                                        */
    float w_all;       /* `weights * w`                                                  */
    float w_vdw;       /* vdw weight                                                     */
    float repel_s;     /* nbonds repel=                                                  */
    float t_bath;      /* K                                                              */
} c3d_stage;

typedef struct {
    float dt_start, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step;
    int32_t n_min;
} c3d_fire_params;

/* --- lifecycle ---------------------------------------------------------------------- */
const char* c3d_last_error(void);
const char* c3d_version(void);
int c3d_device_count(void);
int c3d_create(int device, c3d_ctx** out);
void c3d_destroy(c3d_ctx* ctx);

void c3d_default_model(c3d_model* m);
void c3d_default_fire(c3d_fire_params* f);
/* Fills up to `cap` stages; returns the number of stages of the default schedule
 * (1 pre-minimisation + 5 hot + 81 cool + 1 final minimisation of `min_steps`). */
int c3d_default_schedule(c3d_stage* stages, int cap, int min_steps);

/* --- problem set-up ----------------------------------------------------------------- */
/* K1 on device: D = K * mean(IF^alpha) / IF^alpha, quantised like "%.1f"; builds the n x n
 * target matrix (restraints for |i-j| >= min_sep, IF > 0).  IF is row-major n*n (host). */
int c3d_set_if_matrix(c3d_ctx* ctx, const double* IF, int n, double alpha, double K);
/* Alternative entry: restraint rows as in contact.tbl (1-based i, j; target in tenths of A).  A row with a target <= 0 carries no
 * restraint; of several rows of one pair the last with a positive target holds.  Pairs closer than min_sep carry no restraint, as in
 * the matrix — in every precision and every kernel form.  min_sep is the model's at this call and stays it: once targets are set
 * (here or by c3d_set_if_matrix) c3d_set_model refuses a model with another min_sep (C3D_ERR_INVALID). */
int c3d_set_restraints(c3d_ctx* ctx, int n, int R, const int32_t* ri, const int32_t* rj, const int32_t* rt10);
/* n*n int32, tenths of an Angstrom, -10 where IF == 0 (the <ID>.dist content). */
int c3d_get_dist10(c3d_ctx* ctx, int32_t* dist10);
int c3d_num_beads(const c3d_ctx* ctx);
/* The pairs that carry a restraint: i < j, j - i >= min_sep, target > 0 — counted once a pair, whichever entry set the targets (a list
 * with rows closer than min_sep, rows without a target or several rows of one pair reports fewer than its R). */
int c3d_num_restraints(const c3d_ctx* ctx);

int c3d_set_model(c3d_ctx* ctx, const c3d_model* m);
int c3d_set_schedule(c3d_ctx* ctx, const c3d_stage* stages, int n_stages, const c3d_fire_params* fire,
                     float gtol, int check_every);
/* Execution knobs.  The three launch forms (many steps per launch, one launch per step, symmetric tiles) and every setting
 * of the knobs below except `precision`, `symmetric` and `start` end in the same bits.
 *   resident        -1 (default) / 0 / 1: run step ranges as ONE multi-step launch of the cluster kernel (c3d_cluster.hip)
 *                   wherever a geometry exists / never / as -1, without the back-off after an abandoned launch
 *   resident_min_ops  4 (default): a range of fewer program steps than this runs step by step, not as a multi-step launch (values
 *                   below 1 count as 1; a fraction is dropped); measurement knob
 *   cluster         0: never use the cluster kernel (test knob)
 *   cluster_geometry  100 x compute waves + 10 x rows per wave + helper waves (e.g. 1244): force that geometry of the cluster
 *                   kernel instead of the planner's choice (measurement knob; 0 = planner); before c3d_init_replicas
 *   cluster_late_tiles  1 (default) / 0: how the per-tile sums of a step reach the wave that needs them in the cluster kernel —
 *                   1: where the planner finds the pair loop long enough, that wave fetches them after the next step has
 *                   started (off the critical path); 0: always gathered with the rows before it starts.  Same bits either way
 *                   (measurement knob); before c3d_init_replicas
 *   narrow_columns  1 (default) / 0: column layout of the pair loop — the lanes of the last 256-column block own 1..4 columns each and
 *                   up to 8 columns behind it are summed separately (N = 455: 7 column slots per row instead of 8); 0 = four
 *                   columns per lane everywhere (round 2's layout).  The two layouts sum in different orders: results agree to
 *                   rounding, not bit for bit; every launch form follows the layout in force.  Before c3d_init_replicas.
 *   cluster_static_placement  1 (default): a cluster launch numbers the workgroups of an XCD as blockIdx / 8 and every workgroup
 *                   checks its XCC id against blockIdx % 8; a mismatch abandons the launch and switches the context to 0 =
 *                   per-XCD atomic slot counters (2: test hook, the next launch's workgroup 0 reports a mismatch)
 *   cluster_xcd_count  8 (default) .. 1: the multi-step launches of this context live on that many XCDs (replica r on XCD cluster_xcd_base +
 *                   r % count; the planner fits the replicas of the fullest of THEM into its 32 CUs), workgroups elsewhere exit at once; before
 *                   c3d_init_replicas.  cluster_xcd_base (default 0) = the first of them, may change between launches.  Two contexts with
 *                   disjoint XCD sets anneal side by side without sharing a CU (c3d_batch pairs config 4's small chromosomes this way); the
 *                   same bits whatever the set (a replica's trajectory does not depend on where it runs)
 *   cluster_num_xcc, cluster_inject_incomplete, resident_inject_timeout   test hooks of the cluster kernel's safety net
 *                   (a device that does not expose 8 XCDs gets no cluster plan; a launch that ends without its completion
 *                   mark or with a time-out is re-run on the per-step path)
 *   precision       32 (default) or 64: the fp64 reference kernels (c3d_f64.hip); call before c3d_init_replicas.  A precision-64 context
 *                   keeps its state in doubles and has a boundary in doubles: c3d_get_coords_f64, c3d_get_velocities_f64 and
 *                   c3d_set_coords_f64 move that state bit for bit, c3d_eval_f64 evaluates forces and energies with the fp64 kernels at
 *                   the fp64 coordinates.  The float entries keep working on such a context through a float mirror of the state that every
 *                   range of steps (and c3d_set_coords_f64) refreshes: c3d_get_coords, c3d_get_velocities, c3d_eval, c3d_get_energies,
 *                   scoring and c3d_compare_replicas read the state ROUNDED to float, and c3d_set_coords sets it from floats.  The fp64 step takes
 *                   2560 beads by default and up to 16384 behind f64_max_beads (below; c3d_init_replicas returns C3D_ERR_INVALID beyond
 *                   the limit in force).  The fp32 path takes up to 5120 beads by default and up to 16384 behind max_beads (below);
 *                   c3d_set_if_matrix / c3d_set_restraints refuse more.  A precision-64 context takes its targets from the integer tenths
 *                   of c3d_set_if_matrix or from c3d_set_restraints' list.
 *                   64 and a schedule with a stage of kind 8 exclude each other unless f64_lbfgs is 1 (below): whichever call comes second
 *                   returns C3D_ERR_INVALID
 *   max_beads       5120 (default) .. 16384 (C3D_MAX_BEADS_DEFAULT .. C3D_MAX_BEADS_LIMIT): the largest matrix c3d_set_if_matrix and
 *                   c3d_set_restraints accept; set it before them (other values: C3D_ERR_INVALID).  Raising it is consent to the memory of a
 *                   large matrix: about 8 n npad bytes per context stay resident (targets and the pair targets; npad = n rounded up to
 *                   256): 0.55 GB at 8192 beads, 2.1 GB at 16384; c3d_set_if_matrix takes 21 n^2 bytes more while it runs (the matrix
 *                   and its powers in fp64, the integer tenths, flags: 5.6 GB at 16384) and the host keeps the n^2 integer tenths (1 GB).
 *                   Beyond 5120 beads the fp32 step kernels run in their chunked form (below).  Not beyond 5120: symmetric 1
 *                   (c3d_init_replicas refuses it).  precision 64 and c3d_embed_replicas have limits of their own (f64_max_beads,
 *                   embed_max_beads, next)
 *   f64_max_beads   2560 (default) .. 16384 (C3D_F64_MAX_BEADS_DEFAULT .. C3D_F64_MAX_BEADS_LIMIT), an integer (other values:
 *                   C3D_ERR_INVALID): the largest n c3d_init_replicas accepts under precision 64; set it before that call.  Up to 2560
 *                   beads the fp64 step stages a replica's coordinates in LDS (k64_step: exactly the kernels of earlier releases); beyond,
 *                   it streams the columns through two LDS buffers, 512 at a time (k64_step_chunked; same bits wherever both run).
 *                   Raising it is consent to the fp64 target matrix, 8 n np bytes (np = n rounded up to 128): 2.1 GB at 16384, on top of
 *                   the 1 GB of integer tenths on the device.  max_beads is needed as well beyond 5120
 *   f64_lbfgs       0 (default) or 1 (other values: C3D_ERR_INVALID): the caller's consent to stages of kind 8 on a precision-64 context.
 *                   At 0 c3d_set_schedule refuses a kind-8 stage under precision 64, and precision = 64 refuses a schedule that holds
 *                   one.  At 1 both are accepted, in either order, and the L-BFGS steps run in fp64 (k64_lbfgs_eval in k64_step's staged
 *                   or chunked form, then k64_lbfgs_move), up to f64_max_beads; lbfgs_memory, final_minimiser_steps, the stats lbfgs_steps /
 *                   lbfgs_resets and c3d_step_kernel_name work as in fp32.  Their history, 2 x 8 x 3 x np doubles a replica (6.3 MB at 16384
 *                   beads), is allocated when the first such step runs and freed with the replicas.  Setting it back to 0 is refused while
 *                   precision is 64 and the schedule holds a kind-8 stage.  Setting it releases nothing on the device
 *   f64_column_chunk 0 (default): the fp64 step's column source by size — staged up to 2560 beads, the chunked form with 512 columns a
 *                   pass beyond; 256, 512 or 1024 = the chunked form with that many columns a pass wherever n is larger than it.  Same
 *                   bits either way (test and measurement knob; other values: C3D_ERR_INVALID)
 *   embed_max_beads 4549 (default) .. 16384 (C3D_EMBED_MAX_BEADS_DEFAULT .. C3D_EMBED_MAX_BEADS_LIMIT), an integer (other values:
 *                   C3D_ERR_INVALID): the largest n c3d_embed_replicas accepts.  Up to 4549 beads the eigen stage of a replica runs in one
 *                   workgroup (9 n + 16 floats in the 160 KiB of LDS of a CU); beyond, in a tiled form with its vectors in global memory
 *                   (same bits wherever both run).  Raising it is consent to the memory of a large embedding, freed when the call
 *                   returns: 8 n^2 bytes for the smoothed bounds U and L, and 4 n^2 bytes of trial distances per replica of a batch —
 *                   replicas are embedded in batches whose trial distances fit C3D_EMBED_SCRATCH_BYTES (4 GiB), one replica at least.
 *                   At 16384 beads: 2 GiB + 1 GiB per replica, four replicas a batch, on top of the 2.1 GB such a context holds.
 *                   (max_beads is needed as well beyond 5120; a precision-64 context embeds with the same fp32 kernels, up to its f64_max_beads)
 *   embed_form      0 (default): the eigen stage of c3d_embed_replicas is k_dg_eig while n <= 4549 and the tiled form beyond; 1 = the
 *                   tiled form at every n.  Same bits either way (test and measurement knob; stat "embed_form")
 *   embed_batch     0 (default): replicas per batch of c3d_embed_replicas by the scratch budget; k > 0 = k at a time.  Trial distances
 *                   and start vectors are keyed by replica id: same bits whatever the batch (test knob; stat "embed_batches")
 *   column_chunk    0 (default): where the per-step kernels read a column's coordinates — 0 = the library's choice: the replica's whole
 *                   coordinate array staged in LDS while it fits (n <= 5120: exactly the kernels of earlier releases), beyond that the
 *                   chunked form, which streams 1024 columns at a time through two LDS buffers; 256, 1024 or 2048 = the chunked
 *                   form with that many columns a pass at every n > 1024 (smaller problems have a narrow last column block and stay
 *                   staged).  Same bits either way (test and measurement knob)
 *   symmetric       1: symmetric-tile kernels for large N (c3d_sym.hip; opt-in); call before c3d_init_replicas.  At most 5120 beads.  Not for
 *                   a general tail (k_step's general form runs; decided per step from the model in force), the L-BFGS steps of a kind-8 stage
 *                   (their own kernels), or a problem the multi-step kernel takes (at most 768 padded beads) unless resident is 0
 *   eval_rows_per_wave  4 (default) / 2 / -2: form of the forces hook (c3d_eval_forces) — four rows per wave with the scalar pair term; 2 = two
 *                   rows per wave, the step kernels' code (shipped potential: the packed pair term); -2 = two rows per wave, scalar pair
 *                   term.  2 and -2 return the same bits (a -m gpu test); test knob
 *   pair_targets    1 (default) / 0: beyond the multi-step kernel's reach (n > 1024) the per-step kernel of the shipped potential reads
 *                   resident pre-scaled targets of row pairs (built once per matrix and model) instead of forming the per-pair
 *                   constants from the target matrix in every step.  Same bits either way (measurement knob)
 *   wide_tiles      1 (default) / 0: beyond the multi-step kernel's reach (n > 1024) the per-step kernel of the shipped potential runs 16 rows
 *                   a workgroup and four a wave (two packed row pairs; needs pair_targets 1) instead of 8 and two: a wave's fixed work per
 *                   step is shared by twice the pair terms (N = 2500 x 8: 29.8 -> 26.2 us per step).  Through round 4 equal to the narrow form within rounding
 *                   only; since round 5 — a row's force is one explicit fma in every form — the same bits in every problem of tools/fuzz_wide.py
 *                   (measurement knob)
 *   prefetch_ranks  1 (default) / 0: c3d_set_if_matrix starts the IF side of the Spearman coefficient (average ranks of the matrix's ordered
 *                   pairs |i-j| >= 3, spearman_IF_pdb.pl:30-44: 5 ms of host time at N = 455) on a helper thread over a copy of the matrix;
 *                   c3d_score_replicas takes it when its IF argument holds the same numbers, else computes it as before.  Up to 2048 beads
 *                   only (the worker keeps 16 bytes per pair until the context goes: 67 MB there).  Same result either way
 *                   (measurement knob; stat "rank_prefetch_hits")
 *   device_ranks    0 (default) / 1 / -1 (other values: C3D_ERR_INVALID): who ranks the IF matrix for c3d_score_replicas.  0: the device
 *                   when n > 5120 (C3D_MAX_BEADS_DEFAULT), the matrix is symmetric over the ranked pairs and no prefetched result
 *                   covers it, the host otherwise — every n <= 5120 is ranked exactly as before.  1: the device whenever the matrix is
 *                   symmetric (a prefetched result is ignored and not counted).  -1: the host always.  An asymmetric matrix is ranked
 *                   on the host whatever this says.  The device's ranks are the host's bit for bit (half-integers below 2^29); the
 *                   Spearman coefficient differs by the summation order only.  Memory: see c3d_score_replicas (stat "device_rank_runs")
 *   final_minimiser 1 (default) / 0: what a stage of kind 5 (the default schedule's final stage) runs — two-point step sizes handing over to
 *                   FIRE after final_minimiser_steps, or FIRE throughout as in rounds 1-4.  Stages of kind 2 are FIRE whatever this says
 *   final_minimiser_steps   1000 (default): two-point steps of a kind-5 stage, L-BFGS steps of a kind-8 stage, before FIRE takes it over (>= 2)
 *   lbfgs_memory    1..8 (default 5): pairs (s, y) a stage of kind 8 keeps; takes effect at the next first step of such a stage
 *   start           0 (default) random coil, 1 extended strand (chromosome3D.pl:2413-2416)
 *   use_graph       != 0: per-step path replays hipGraphs (default 1)
 *   replica_groups  1..4 stream groups of the per-step path (default 2);  graph_chunk, rows_per_wave,
 *   stage_dma       tuning and test knobs of the per-step kernel
 *   event_timing    1 (default) / 0: HIP-event pair around c3d_run / c3d_run_steps (feeds c3d_last_timing)
 *   kernel_timing   1: start/stop events attached to every multi-step launch (stat "last_kernel_us")
 *   spin_wait_us    how long c3d_run_steps watches the completion mark a multi-step launch writes into host-mapped memory before it
 *                   falls back to hipStreamSynchronize (default 400; 0 = always synchronise).  Results are untouched by it. */
int c3d_set_option(c3d_ctx* ctx, const char* key, double value);
/* the option max_beads: its default and its largest value */
#define C3D_MAX_BEADS_DEFAULT 5120
#define C3D_MAX_BEADS_LIMIT 16384
/* the option embed_max_beads: its default and its largest value; the trial-distance scratch a batch of c3d_embed_replicas stays within */
#define C3D_F64_MAX_BEADS_DEFAULT 2560
#define C3D_F64_MAX_BEADS_LIMIT 16384
#define C3D_EMBED_MAX_BEADS_DEFAULT 4549
#define C3D_EMBED_MAX_BEADS_LIMIT 16384
#define C3D_EMBED_SCRATCH_BYTES (4ull << 30)
/* the two distance histograms of a replica batch stay within this when c3d_score_replicas re-runs a call whose models are wider than 262 A */
#define C3D_SCORE_SCRATCH_BYTES (1ull << 30)

/* Process-wide switches, to be set before the first c3d_create (no environment variable is read by the library):
 *   preload         which code objects c3d_create loads before it returns (the library never leaves a load to the runtime's first-launch
 *                   path and never loads beside another HIP call of the library: csrc/c3d_gate.cpp "code objects"):
 *                   1 (default)  what a default job launches from — K1 + per-step unit, both multi-step units of the shipped potential,
 *                                scoring — +13 ms on the first c3d_create, once per process and device;
 *                   2            all sixteen units, +24 ms (long-lived executors: nothing is ever loaded after the first c3d_create of a device);
 *                   0            none: each unit at the first entry that needs it (measurement knob).
 *                   Units beyond the default set (other potentials, fp64, symmetric tiles, embedding) load at the first entry that
 *                   needs them in every mode, while no other thread of the process is inside an entry.  Results are untouched. */
int c3d_set_process_option(const char* key, double value);

/* --- replicas ----------------------------------------------------------------------- */
/* n_replicas chains with ids first_replica .. first_replica+n_replicas-1; the RNG is
 * Philox4x32-10 keyed by (seed, replica id), so a replica's trajectory does not depend on
 * how replicas are spread over processes or GPUs (seed 82364: chromosome3D.pl:980). */
int c3d_init_replicas(c3d_ctx* ctx, int n_replicas, uint64_t seed, uint32_t first_replica);
/* A7 (deck chromosome3D.pl:1471-1525, bead-level restatement): replace the random-coil start of every
 * replica by a metric-matrix distance-geometry embedding — bounds from the restraints, triangle
 * smoothing, random trial distances (Philox, keyed by replica id), 3 leading eigenvectors found with
 * `iters` orthogonal iterations (50 is plenty).  Call between c3d_init_replicas and c3d_run.  At most 4549 beads by default (the eigen stage
 * keeps 9 n + 16 floats of a replica in the 160 KiB of LDS of one CU), up to 16384 after c3d_set_option("embed_max_beads", n), where the eigen
 * stage runs tiled over the device and the replicas are embedded in batches (memory: see the option); C3D_ERR_INVALID beyond, before any launch. */
int c3d_embed_replicas(c3d_ctx* ctx, int iters);
/* overwrite coordinates (n_replicas*n*3, xyz interleaved) — tests and restarts */
int c3d_set_coords(c3d_ctx* ctx, const float* xyz);
int c3d_get_coords(c3d_ctx* ctx, float* xyz);
/* (after a range that ended inside the two-point part of a final stage — kind 5, its first final_minimiser_steps steps — the velocity
 *  slot holds the previous evaluation's FORCE per bead, kcal/mol/A: that minimiser has no velocities and keeps its history there;
 *  after MD and FIRE steps it is the velocity in A/ps; the same holds inside the L-BFGS part of a stage of kind 8: the slot holds the force of
 *  the last evaluation) */
int c3d_get_velocities(c3d_ctx* ctx, float* v);
/* The same three in doubles, for a precision-64 context with replicas (any other context: C3D_ERR_INVALID, the message names what is
 * missing); layouts as above, n_replicas*n*3, xyz interleaved.
 * c3d_get_coords_f64: the fp64 coordinates of the current step parity, bit for bit.  c3d_get_velocities_f64: the fp64 velocity slot (the
 * remark at c3d_get_velocities applies: inside the two-point and L-BFGS parts it holds the last evaluation's force).
 * c3d_set_coords_f64: the fp64 state becomes exactly these doubles; everything else is what c3d_set_coords leaves on such a context —
 * velocities zero in both parities, sums, minimiser state and the position in the schedule untouched — and the float mirror is refreshed
 * (coordinates rounded to float, velocities zero), so c3d_get_coords, energies and scoring see the new structure.  A non-finite value
 * anywhere in xyz: C3D_ERR_INVALID before anything is copied. */
int c3d_get_coords_f64(c3d_ctx* ctx, double* xyz);
int c3d_get_velocities_f64(c3d_ctx* ctx, double* v);
int c3d_set_coords_f64(c3d_ctx* ctx, const double* xyz);

/* --- solve -------------------------------------------------------------------------- */
/* whole schedule, with the gtol exit of the final minimisation; centres the models. */
int c3d_run(c3d_ctx* ctx);
/* advance by at most nsteps SA steps of the schedule (no early exit); returns steps done
 * through *done.  Used by the benchmark and by tests that follow a trajectory. */
int c3d_run_steps(c3d_ctx* ctx, long nsteps, long* done);
long c3d_schedule_length(const c3d_ctx* ctx);   /* SA steps in the whole schedule */
long c3d_steps_done(const c3d_ctx* ctx);
int c3d_centre(c3d_ctx* ctx);
/* device time of the last c3d_run / c3d_run_steps, from HIP events on the solver's stream */
int c3d_last_timing(const c3d_ctx* ctx, double* ms_total, long* steps, long* launches);
/* Counters of the context since c3d_create, for benchmarks and tests (no reference counterpart: the reference's
 * only instrument is the wall clock around `./job.sh`, chromosome3D.pl:287).  Keys: "graph_captures" (hipGraphs
 * captured + instantiated), "graph_launches", "graphs_cached", "step_launches" (k_step dispatches), "resident_launches",
 * "cluster_launches", "resident_fallbacks" (multi-step launches abandoned for the per-step path), "cluster_incomplete"
 * (those of them that ended without every (replica, part) workgroup reporting), "cluster_static_placement",
 * "cluster_placement_mismatches", "cluster_xcd_count", "cluster_xcd_base", "cluster_ok" (1: a multi-step geometry exists for the replicas as initialised), "spin_completions" (multi-step launches whose end was seen on the completion mark), "num_xcc", "last_path"
 * (0 per-step, 2 k_cluster), "cluster_parts", "cluster_rows_per_wave", "cluster_late_tiles", "last_host_launch_us", "last_host_sync_us" (host time inside the launch / synchronise call of the last c3d_run_steps, cluster launches), "cluster_compute_waves",
 * "cluster_helper_waves", "cluster_wgs_per_cu" (the other two numbers of the multi-step geometry in force, 0 without one), "replica_groups",
 * "units_loaded" (code objects this process has loaded, all devices), "units_loaded_mask" (bit per unit, this context's device),
 * "k1_recomputed" (elements of the last c3d_set_if_matrix that sat within 1e-10 of a "%.1f" rounding tie and were redone
 * on the host in the reference's operation order), "k1_patched" (how many of those changed, since c3d_create),
 * "rms_force" (largest RMS force component over the replicas at the last minimiser step: the quantity c3d_run holds
 * against gtol, the stand-in for L-BFGS's convergence test of chromosome3D.pl:1800-1803), "lbfgs_steps" (L-BFGS steps run, kind 8),
 * "lbfgs_resets" (memory drops of the last kind-8 stage since its first step, summed over the replicas: read from the device),
 * "embed_form" (the eigen stage the last c3d_embed_replicas ran: 0 k_dg_eig, 1 tiled), "embed_batches" (replica batches of that call),
 * "device_rank_runs" (calls of c3d_score_replicas that ranked the IF matrix on the device), "score_wide_runs" (calls of it that were
 * re-run with a histogram sized to the models), "compare_runs" (completed calls of c3d_compare_replicas),
 * "f64_evals" (completed calls of c3d_eval_f64), "superpose_runs" / "rmsd_table_runs" (completed calls of c3d_superpose_replicas /
 * c3d_rmsd_table), "ensemble_map_runs" / "ensemble_score_runs" (completed calls of c3d_ensemble_map / c3d_ensemble_score),
 * "geometry_runs" / "separation_runs" (completed calls of c3d_geometry_replicas / c3d_separation_profile),
 * "stratified_runs" (completed calls of c3d_stratified_score), "stratified_if_ms" / "stratified_models_ms" (device time of the two passes
 * of the last completed one, from HIP events: measurement), "bead_runs" (completed calls of c3d_bead_scores), "bead_if_ms" /
 * "bead_models_ms" (device time of its two passes in the last completed call, the first 0 where no IF was ranked: measurement). */
int c3d_get_stat(const c3d_ctx* ctx, const char* key, double* value);
/* Test hook, no reference counterpart: the multi-step kernel's hand-off trusts a 16-byte unit once its tag word matches — i.e. that a
 * 16-byte aligned store is never observed half-written by a 16-byte load on gfx950.  This runs that exact store / load pair (one producer
 * workgroup, a consumer workgroup on every other CU, the context's stream) for `iterations` rewrites of 1024 units and returns the number
 * of unit reads, of TORN units (must be 0) and of reads that saw a new value. */
int c3d_debug_tear16(c3d_ctx* ctx, int iterations, unsigned long long* unit_reads, unsigned long long* torn, unsigned long long* fresh);
/* Test hook: the fp32 step controller as a table.  One step of `kind` (0 / 1 MD, 2 / 3 FIRE, 5 / 6 two-point step length; dt and t_bath as
 * a stage gives them) is decided for `rows` independent rows by the function every fp32 step kernel calls once per replica, with the
 * context's own model (mass, fbeta, bead count) and FIRE values.  Row r: psum[4 r ..] = the previous evaluation's four replica sums (MD:
 * sum v^2, sum vx, vy, vz; FIRE: v.F, F.F, v.v, -; two-point: s.y, F.F, y.y, s.s), state_in[2 r ..] = (dt, alpha), npos_in[r].  Returns
 * scalars[6 r ..] = (lambda, v_cm x, y, z, keep, mix) and the state the step leaves in state_out / npos_out.  Needs the bead count (targets set);
 * touches nothing of the solve. */
int c3d_debug_step_scalars(c3d_ctx* ctx, int kind, float dt, float t_bath, int rows, const float* psum, const float* state_in,
                           const int32_t* npos_in, float* scalars, float* state_out, int32_t* npos_out);
/* Test hooks: the fp64 step controller and the fp64 row update as tables (precision-64 contexts only; every value crosses in doubles, the
 * state's counter as int32_t).  The statements run are the two source texts every k64_step kernel includes, a thread a row, under the
 * context's own model and FIRE values as the fp64 path derives them (t_fac, 1 / n, dt 418.4 / mass, 418.4 / mass).
 * c3d_debug_step_scalars_f64: kinds and rows as c3d_debug_step_scalars — psum[4 r ..], state_in[2 r ..] = (dt, alpha), npos_in[r] ->
 * scalars[6 r ..] = (lambda, v_cm x, y, z, keep, mix), state_out[2 r ..], npos_out[r].
 * c3d_debug_row_finish_f64: one bead's update of a step of `kind` (0 / 1 MD with the stage's dt, 4 MD begin, 2 / 3 FIRE, 5 / 6 two-point).
 * Row r in: in[16 r ..] = x[3], v[3] (kinds 5: the force of the previous evaluation; 4: the Maxwell velocity), F[3], lambda, v_cm[3], keep,
 * mix, dt of the FIRE state — the scalars as c3d_debug_step_scalars_f64 returns them.  Row r out: out[10 r ..] = new x[3], new v[3], the
 * bead's terms of the four sums the next step reads.
 * Both refuse (C3D_ERR_INVALID) a context whose precision is not 64, other kinds, rows outside 1 .. 2^20; both need the bead count
 * (targets set) and touch nothing of the solve. */
#define C3D_ROW_FINISH_IN 16
#define C3D_ROW_FINISH_OUT 10
int c3d_debug_step_scalars_f64(c3d_ctx* ctx, int kind, double dt, double t_bath, int rows, const double* psum, const double* state_in,
                               const int32_t* npos_in, double* scalars, double* state_out, int32_t* npos_out);
int c3d_debug_row_finish_f64(c3d_ctx* ctx, int kind, double dt, int rows, const double* in, double* out);
/* Test hook: the fp32 row update as a table — finish_row, the function every fp32 step kernel (k_cluster, k_cluster_tp, k_step,
 * k_update_sym) calls once per row and step, a thread a row under the context's own model and FIRE values (418.4 / mass and max_step as
 * floats; the kernel forms dt 418.4 / mass itself).  Kinds and the row layout are c3d_debug_row_finish_f64's, in floats: in[16 r ..] =
 * x[3], v[3], F[3], lambda, v_cm[3], keep, mix, dt of the FIRE state -> out[10 r ..] = new x[3], new v[3], the bead's terms of the four
 * sums.  Domain: the capped move d (FIRE: dt v'; two-point: mix F, and lambda v of the previous move) with |d| < 2^63 in every
 * component, so that d.d is a finite float; beyond it the cap's 1 / sqrt(d.d) is 0 and the bead stays where it is (a component of d
 * that is itself infinite gives NaN), while v' and the sums are formed as everywhere.
 * Refuses (C3D_ERR_INVALID) other kinds and rows outside 1 .. 2^20; needs the bead count (targets set) and touches nothing of the solve. */
int c3d_debug_row_finish(c3d_ctx* ctx, int kind, float dt, int rows, const float* in, float* out);
/* Test hook: the serial section of an L-BFGS move (stage kind 8) as a table.  Between its two barriers one thread of every workgroup of
 * the move kernel decides the step from the replica's sums: the pair test s.y > 1e-12 sqrt(s.s y.y), the ring of lbfgs_memory slots,
 * gamma (s.y / y.y after a kept pair, doubled after a rejected one, clamped to [1e-7, 1e2]), the two triangular solves of the compact form
 * and the descent test F.d > 0.  This runs those very statements (one source text, shared with the kernels) for `rows` independent rows,
 * in the precision of the context: the fp32 kernels' section (coefficients rounded to float) or, on a precision-64 context, the fp64
 * kernels'; the first step's gamma is dt_start^2 * 418.4 / mass from the context's model and FIRE values, as that precision forms it.
 * Row r in: sums[36 r ..] = per ring slot j (F.s_j, F.y_j, s_j.y, y_j.y) at 4 j, then s.s, F.F, 0, 0 — (s, y) the pair this step completes,
 * F the force just evaluated; the state of the previous step as state_int_in[4 r ..] = (cnt pairs held, head = slot of the newest, mem =
 * ring size, resets) and state_dbl_in[129 r ..] = (gamma, S'Y [8][8], Y'Y [8][8], both indexed by slot); first[r] != 0: the stage's first
 * step (the state is then not read); mem0[r] = lbfgs_memory, 1 .. 8.  A state out of range is clamped first: mem to [1, 8], head to
 * [0, mem - 1], cnt to [0, mem].  Row r out: the state the step leaves, coef[17 r ..] = (gamma, a_j by slot, b_j by slot) of the direction
 * gamma F + sum a_j s_j + sum b_j y_j (0 for a slot outside it), mask_slot[2 r ..] = (bit j set: slot j is in the direction, the slot this
 * move's s goes to).  Needs the bead count (targets set); touches nothing of the solve. */
#define C3D_LBFGS_MAX_PAIRS 8
#define C3D_LBFGS_SUMS (4 * C3D_LBFGS_MAX_PAIRS + 4)
#define C3D_LBFGS_STATE_DOUBLES (1 + 2 * C3D_LBFGS_MAX_PAIRS * C3D_LBFGS_MAX_PAIRS)
#define C3D_LBFGS_COEFS (1 + 2 * C3D_LBFGS_MAX_PAIRS)
int c3d_debug_lbfgs_direction(c3d_ctx* ctx, int rows, const double* sums, const int32_t* state_int_in, const double* state_dbl_in,
                              const int32_t* first, const int32_t* mem0, int32_t* state_int_out, double* state_dbl_out, double* coef,
                              int32_t* mask_slot);
/* Test hook: the rows of an L-BFGS move as a table, in the context's precision (as c3d_debug_lbfgs_direction: floats, or doubles on a
 * precision-64 context).  After the serial section every bead of the move forms its direction gamma F + sum a_j s_j + sum b_j y_j over the
 * slots of the mask, caps it at max_step, moves, writes the move s into ring slot `slot` and forms its move.move; the statements run are
 * the one source text both move kernels include, a thread a row over a ring laid out as theirs.  coef[17] = (gamma, a_j, b_j by slot),
 * mask (bit j: slot j is in the direction) and slot are the call's, as they are a replica's in a move.
 * Row r in: in[54 r ..] = x[3], F[3], s_j[3] for j = 0 .. 7, y_j[3] for j = 0 .. 7 (narrowed to floats on an fp32 context: pass
 * float-exact values there).  Row r out: out[10 r ..] = new x[3], ring slot `slot` read back [3], ring slot (slot + 1) % 8 read back [3]
 * (untouched by the move), move.move.  A ring slot outside the mask is never read.
 * Domain of the fp32 cap: the direction d finite (d.d may be beyond a float: it is then rescaled before the square root).
 * Refuses (C3D_ERR_INVALID) slot outside 0 .. 7, mask outside 0 .. 255, rows outside 1 .. 2^16; touches nothing of the solve. */
#define C3D_LBFGS_MOVE_ROW_IN (6 + 6 * C3D_LBFGS_MAX_PAIRS)
#define C3D_LBFGS_MOVE_ROW_OUT 10
int c3d_debug_lbfgs_move_rows(c3d_ctx* ctx, int rows, const double* coef, int mask, int slot, const double* in, double* out);
/* Test hook of A7 (c3d_embed_replicas): U, L (n*n each, row-major) = the smoothed distance bounds the embedding draws its trial distances
 * from — b0 on |i-j| = 1, the target on restrained pairs, [r0_rep x the last stage's repel, 1e30] elsewhere, then all-pairs shortest
 * paths on U, the inverse triangle inequality on L, L <= U.  The same kernels and arguments as the embedding; no bead limit of its own.
 * Needs the targets (c3d_set_if_matrix / c3d_set_restraints), not the replicas. */
int c3d_dg_smoothed_bounds(c3d_ctx* ctx, float* U, float* L);
/* Test hook of c3d_score_replicas: the IF side of the Spearman coefficient as the DEVICE computes it, whatever the option device_ranks
 * says.  rank (n*n, row-major) = the average rank of IF(i,j) among the ordered pairs |i-j| >= range, 0 inside that band; *m = the number of
 * ordered pairs; *saa = sum (rank - (m+1)/2)^2 over them.  IF is n*n with the n of c3d_set_if_matrix / c3d_set_restraints and symmetric over
 * the ranked pairs (C3D_ERR_INVALID otherwise: c3d_score_replicas ranks such a matrix on the host). */
int c3d_debug_if_ranks(c3d_ctx* ctx, const double* IF, int range, double* rank, double* saa, size_t* m);
/* Name of the kernel the last op of the last range of c3d_run / c3d_run_steps ran on, as a profiler prints it (thread-local string): the
 * choice that op's launch was made from, also when the range was replayed from a captured graph.  After an L-BFGS step the force pass,
 * k_lbfgs_eval<...>; "" before the first range. */
const char* c3d_step_kernel_name(const c3d_ctx* ctx);

/* One evaluation through the production pair kernel at the replicas' current coordinates:
 * F (n_replicas*n*3) = total weighted force; e (n_replicas*3) = unweighted (noe, bond+angle,
 * repel) energies in fp64. Either may be NULL. */
int c3d_eval(c3d_ctx* ctx, float w_all, float w_vdw, float repel_s, float* F, double* e);
/* One evaluation by the fp64 kernels at the fp64 coordinates of a precision-64 context with replicas (any other context:
 * C3D_ERR_INVALID).  F (n_replicas*n*3) = the total weighted force, from k64_eval_forces / k64_eval_forces_chunked: the fp64 step's own
 * pair loop, sums and chain terms in the form (potential, tail, fold, column chunk) a stage with these weights steps in, so F has the bits
 * of the force that step integrates.  e (3*n_replicas) = the unweighted noe, bond+angle and repel energies with c3d_eval's meaning, from the
 * fp64 coordinates and the fp64 targets (k64_energy; one workgroup a replica, sums in a fixed order: two calls return the same bits).
 * Either may be NULL, not both.  Changes no state of the solve: coordinates, velocity slot, sums, minimiser state, step parity, the L-BFGS
 * history and c3d_step_kernel_name stay as they are.  The force buffer (n_replicas x 3 x np doubles, np = n rounded up to 128) is
 * allocated by the first call and freed with the replicas.  The stat "f64_evals" counts completed calls. */
int c3d_eval_f64(c3d_ctx* ctx, double w_all, double w_vdw, double repel_s, double* F, double* e);
/* per replica: e[3*r + {0,1,2}] = E_noe, E_bond(+angle), E_repel at the final weights */
int c3d_get_energies(c3d_ctx* ctx, double* e);
/* K6 on the device, for every replica at its current coordinates: the restraint-satisfaction count and
 * the sum of deviations of chromosome3D.pl:447-485 / :581-600 (relax 0.5 A, threshold 0.2 A) and, if IF
 * (the n*n matrix given to c3d_set_if_matrix) and rho are non-NULL, Spearman(IF, d) over |i-j| >= range
 * as spearman_IF_pdb.pl:42-70 defines it.  Any output pointer may be NULL.
 * Extent: distances are counted in a histogram of 0.001 A bins, 2^18 of them (262.144 A) in the first place; a call in which any pair of
 * any replica is further apart is scored again with a histogram sized to the bounding box of the widest replica, replicas in batches
 * whose two histograms fit C3D_SCORE_SCRATCH_BYTES (one replica at least; allocated for the call) — the same numbers for a replica
 * either way.  Beyond 50 000 A, the limit of c3d_spearman_if_dist_batch, C3D_ERR_INVALID: at once when the bounding box is wider than
 * that, else after the pass that finds such a pair (up to 400 MB of histograms per replica).
 * IF ranks: from the helper thread of c3d_set_if_matrix (up to 2048 beads), else computed by the call — on the host up to 5120 beads and
 * for asymmetric matrices, on the device beyond (option device_ranks): the matrix is uploaded into the context's scoring scratch, the keys
 * of its upper triangle are sorted there and every pair looks its rank up; nothing is cached between calls.  That scratch, kept until
 * the context goes, holds 8 n^2 bytes (matrix, then ranks) at every size, and with device ranks 8 bytes per sort slot — the ranked pairs
 * i < j, (n-range)(n-range+1)/2, rounded up to a power of two and to 4096 at least: 2 GiB + 1 GiB at 16384 beads, where the host path needs about 10 GB of host memory instead. */
int c3d_score_replicas(c3d_ctx* ctx, const double* IF, int range, int32_t* satisfied, double* sum_dev, double* rho);
/* The models of a run against one another, on the device (c3d_score_compare.inc k_cmp_*): the two numbers of the reference's output_models/similarity.txt
 * (c3d_model_similarity below) for every ordered pair of models, without reading coordinates back.
 * K = n_replicas + n_extra models of n beads: model k < n_replicas is replica k at its current coordinates (fp32, taken as doubles
 * unchanged); model n_replicas + e is extra_xyz + 3 n e (xyz interleaved, doubles; e.g. a bundled model).  spearman, rmsd: K x K row-major,
 * entry [a][b] = what c3d_model_similarity(a, b, n, ...) returns — rmsd[a][b] scales a's distances by mean(d_b)/mean(d_a), so that table
 * is not symmetric.  Either output may be NULL, not both.
 * The distances and their tie groups are the host's bit for bit (c3d_debug_distance_ranks); the sums are added in another order, fixed:
 * entries agree with the host to about m 2^-53 (m = n(n-1)/2), a model against a copy of itself gives exactly 1 and 0, and two calls on
 * the same coordinates return the same bits.  A model whose distances are all equal gives NaN as the host does.  No state of the solve changes.
 * C3D_ERR_INVALID: no replicas, n < 3, n_extra < 0, n_extra > 0 without coordinates, K > C3D_COMPARE_MAX_MODELS, both outputs NULL, extra
 * coordinates that c3d_model_similarity refuses (not finite, |x| >= 1e6).  C3D_ERR_NOMEM: no device memory for the scratch.
 * Scratch, allocated for the call and freed before it returns: 4 m bytes per model (the pairs' positions in the sorted order), 8 bytes per
 * sort slot (m rounded up to a power of two, 4096 at least; reused model after model), 24 n bytes per model (fp64 coordinates), 8 n per
 * model of row sums and at most 64 MB of per-workgroup sums: 10 GiB + 1 GiB at 16384 beads x 20 models, 8 MB + 1 MB at 455 x 20.
 * Stat "compare_runs" counts the calls that completed. */
#define C3D_COMPARE_MAX_MODELS 256
int c3d_compare_replicas(c3d_ctx* ctx, const double* extra_xyz, int n_extra, double* spearman, double* rmsd);
/* Test hook: rank (n(n-1)/2 doubles, pairs i<j in row order) = the average ranks of replica `replica`'s distances as the device computes them */
int c3d_debug_distance_ranks(c3d_ctx* ctx, int replica, double* rank);
/* The models of a run in one frame, on the device (c3d_score_superpose.inc k_sup_*): a run's replicas come out in arbitrary frames and, mirror images
 * having equal energy under distance restraints, in both hands.  c3d_superpose_replicas fits every replica onto one target:
 * replica `reference` (0..n_replicas-1) at its current coordinates, or, with reference = -1, ref_xyz (n x 3 doubles, xyz interleaved, e.g. a
 * bundled model; checked as the extra models of c3d_compare_replicas are).  The models are the replicas' state: on a precision-64 context the
 * fp64 state bit for bit, else the floats taken as doubles unchanged.
 * The fit: model and target are centred on their centroids; the model gets the least-squares rotation R onto the target (Horn's quaternion
 * matrix of the 3 x 3 covariance, its extreme eigenpairs by 10 cyclic Jacobi sweeps, a fixed count); with C3D_SUPERPOSE_MIRROR it is first
 * reflected through the origin if the reflected fit is strictly better.  mirrored[k] = 1 for a reflected model (always 0 without the flag),
 * rmsd[k] = sqrt(sum_i |R a_i - b_i|^2 / n) over the centred coordinates, summed directly (exactly 0 for the reference replica itself).
 * iters = 0 stops there.  iters > 0 (at most C3D_SUPERPOSE_MAX_ITERS) then repeats `iters` times: the mean of the fitted models becomes the
 * target and every model gets the rotation onto it (generalized Procrustes; rotations only, the handedness stays as the first pass settled
 * it); rmsd[k] is then sqrt(sum_i |x_k,i - mean_i|^2 / n) against the final mean.
 * mean_xyz (n x 3) = the mean of the fitted models, rmsf (n) = sqrt(mean_k |x_k,i - mean_i|^2), the per-bead spread.  The fitted models
 * are in the target's frame: at the target's centroid with iters = 0, at the origin otherwise.  Any output pointer may be NULL.
 * Without C3D_SUPERPOSE_APPLY no state of the solve changes (the guarantee of c3d_eval_f64 and c3d_compare_replicas).  With it the
 * replicas' coordinates become the fitted ones, as c3d_set_coords / c3d_set_coords_f64 would leave them: the current parity's floats
 * (each the fp64 result rounded once) or both fp64 buffers and the float mirror; velocities zero in both parities; pad beads, sums,
 * minimiser state, the position in the schedule and c3d_step_kernel_name untouched.
 * c3d_rmsd_table: rmsd[a][b], mirrored[a][b] (K x K row-major, K = n_replicas + n_extra models as in c3d_compare_replicas) = the fit of
 * model a onto model b for every ordered pair; flags: C3D_SUPERPOSE_MIRROR or 0.  The diagonal is exactly 0 and not mirrored, the table is
 * symmetric to rounding.  Either output may be NULL, not both.
 * All sums have a fixed order that follows from n alone (chunks of 64 beads added in chunk order, no atomics): two calls return the same
 * bits, and extra models leave the replicas' entries their bits.
 * C3D_ERR_INVALID, before any launch: no replicas, n < 3, reference outside -1..n_replicas-1 or -1 without ref_xyz, n_extra < 0 or extra
 * models without coordinates, K > C3D_COMPARE_MAX_MODELS, unknown flag bits (C3D_SUPERPOSE_APPLY is unknown to the table), iters < 0 or
 * > C3D_SUPERPOSE_MAX_ITERS, every output NULL (without C3D_SUPERPOSE_APPLY), coordinates given by the caller that are not finite or have
 * |x| >= 1e6.  C3D_ERR_NOMEM: no device memory for the scratch.
 * Scratch, allocated for the call and freed before it returns: 24 n bytes per model (48 n for a superposition: centred and fitted), 200
 * bytes per fitted pair (K pairs, K^2 for the table) and the per-chunk sums of one block of sixteen models, 22 528 ceil(n / 64) ceil(Kb / 16)
 * bytes (Kb = 1, or K for the table): 16 MB + 12 MB at 16384 beads x 20 models, 200 MB + 13 MB + 92 MB at 16384 x 256.
 * Stats "superpose_runs" and "rmsd_table_runs" count the calls that completed. */
#define C3D_SUPERPOSE_MIRROR 1   /* a model that fits better reflected is reflected */
#define C3D_SUPERPOSE_APPLY  2   /* the superposed coordinates become the replicas' state */
#define C3D_SUPERPOSE_MAX_ITERS 50
int c3d_superpose_replicas(c3d_ctx* ctx, int reference, const double* ref_xyz, int flags, int iters, double* rmsd, int32_t* mirrored,
                           double* mean_xyz, double* rmsf);
int c3d_rmsd_table(c3d_ctx* ctx, const double* extra_xyz, int n_extra, int flags, double* rmsd, int32_t* mirrored);
/* The ensemble itself, on the device (c3d_score_ensemble.inc k_ens_*): what the models say about every bead pair together.  A mean of superposed
 * coordinates shrinks wherever the models disagree; the quantity that stays meaningful for a population is the distance map.
 * Models: K = n_replicas + n_extra, numbered as in c3d_compare_replicas; the replicas are taken as c3d_superpose_replicas takes them (on a
 * precision-64 context the fp64 state bit for bit, else the floats taken as doubles unchanged); extra models are n x 3 doubles, xyz
 * interleaved, checked as there.  pick: n_pick model indices in 0..K-1 — the models that count, in the order they are summed; an index may
 * repeat and then counts twice; NULL with n_pick = 0 means all K in index order.  Kp is the length of that list (at most 4096).
 * The distance d_k(i,j) is the one of c3d_compare_replicas, sqrt(((ux ux) + uy uy) + uz uz) in fp64 with every operation rounded on its
 * own: it has the bits of the host's.
 * c3d_ensemble_map: mean, sd, contact — n x n row-major doubles, any of them NULL, not all three:
 *   mean(i,j)    = sum_k d_k / Kp, summed in list order;
 *   sd(i,j)      = sqrt(sum_k (d_k - mean)^2 / Kp), the population form, from the deviations in a second walk over the models (never as
 *                  sum d^2 - Kp mean^2, which loses about 1e-6 A where the models agree);
 *   contact(i,j) = #{k : d_k(i,j) < cutoff} / Kp: an exact count, divided once.
 * The diagonal is mean 0, sd 0, contact 1.  Every pair i < j is computed once and stored to both halves: the matrices equal their
 * transposes bit for bit.  No atomics and one fixed order: two calls on the same state return the same bits.  The matrices are copied
 * straight into the caller's buffers.
 * c3d_ensemble_score: how the ensemble's map — not one model's — follows the input: rho_mean = Spearman(IF, mean distance), rho_contact =
 * Spearman(IF, contact frequency), both over the ordered pairs |i-j| >= range with average ranks on ties, either NULL, not both.  A good
 * ensemble has rho_mean < 0 and rho_contact > 0; a constant map gives NaN as a host computation would.  The two maps are the ones
 * c3d_ensemble_map returns for the same arguments, bit for bit (the same kernel); they and IF (n x n with the context's n) are ranked on the
 * device by the kernels that rank IF for c3d_score_replicas.  IF must be symmetric over the ranked pairs: there is NO host ranking to fall
 * back on here, an asymmetric matrix is C3D_ERR_INVALID.
 * No state of the solve changes in either call (the guarantee of c3d_compare_replicas).
 * C3D_ERR_INVALID, before any launch: no replicas, n < 2, n_extra < 0 or extra models without coordinates, K > C3D_COMPARE_MAX_MODELS,
 * n_pick < 0, a list without a length or a length without a list, a pick index outside 0..K-1, more than 4096 picks, every output NULL,
 * extra coordinates that are not finite or have |x| >= 1e6, contact / rho_contact wanted with a cutoff that is not finite or <= 0,
 * range < 1 or a range that leaves no pairs, no IF.  C3D_ERR_NOMEM: no device memory for the scratch.
 * Scratch, one allocation per call, freed before it returns: 24 n bytes per model, 4 bytes per pick and 8 n^2 bytes for each matrix the
 * call needs — the map those that were asked for: 5 MB + 0.2 MB at 455 beads x 20 models, 6 GiB + 8 MB at 16384 x 20 with all three; the
 * score two at every size (IF's ranks, and one slot that holds the mean and then the contact map), and 8 bytes per sort slot (the ranked
 * pairs i < j rounded up to a power of two, 4096 at least): 3.3 MB + 1 MB + 0.2 MB at 455 x 20, 4 GiB + 1 GiB + 8 MB at 16384 x 20.
 * Stats "ensemble_map_runs" and "ensemble_score_runs" count the calls that completed. */
int c3d_ensemble_map(c3d_ctx* ctx, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, double cutoff,
                     double* mean, double* sd, double* contact);
int c3d_ensemble_score(c3d_ctx* ctx, const double* IF, int range, const double* extra_xyz, int n_extra,
                       const int32_t* pick, int n_pick, double cutoff, double* rho_mean, double* rho_contact);
/* A model's geometry and the distance against genomic separation, on the device (c3d_score_geometry.inc k_geo_*, k_sep_*): all-pairs reductions over
 * the models of the ensemble entries above — K = n_replicas + n_extra, numbered as in c3d_compare_replicas, the replicas taken as
 * c3d_superpose_replicas takes them (precision 64: the fp64 state bit for bit, else the floats taken as doubles unchanged), extra models n x 3
 * doubles checked as there; pick / n_pick with exactly the meaning and limits they have in c3d_ensemble_map.  The distance d(i,j) is
 * theirs too, sqrt(((ux ux) + uy uy) + uz uz) in fp64 with every operation rounded on its own: the host's bits, and those of the reference's
 * sqrt(($x1-$x2)**2+($y1-$y2)**2+($z1-$z2)**2).
 * c3d_geometry_replicas, per model k; any output may be NULL, not all four:
 *   clashes[k]          = #{i < j, j - i >= sep : d(i,j) <= cutoff}.  With sep = 1 this is the reference's clash_count(pdb, cutoff)
 *                         (chromosome3D.pl:693-714) exactly: bonded neighbours are included and the comparison is `<=`, as at :708 — the
 *                         "clash(<=3.5 A)" of BASELINE.md §3, by which a bead model under distance-only restraints is checked for
 *                         collapse.  Integers only: the count is exact.
 *   bead_clashes[k n+i] = the number of such partners of bead i, on both sides; their sum over i is exactly 2 clashes[k].
 *   nearest[k n+i]      = min over j, |i-j| >= sep, of d(i,j): a minimum has no summation order, so it has the host's bits.  +infinity
 *                         for a bead without such a partner (sep > max(i, n-1-i)).
 *   chain[6 k+f]        : f = 0, 1 mean and population sd of the n-1 bond lengths d(i,i+1); f = 2, 3 those of the n-2 distances d(i,i+2);
 *                         f = 4 the radius of gyration sqrt(mean_i |x_i - centroid|^2); f = 5 the model's extent, max over i < j of d(i,j),
 *                         which has exact bits.  Every sd is the two-pass form — the mean, then the squared deviations in a second walk —
 *                         never sum d^2 - n mean^2, for the reason given at c3d_ensemble_map.  (C3D_GEOMETRY_FIELDS = 6.)
 *   cutoff must be finite and > 0 when clashes or bead_clashes is asked for; 1 <= sep <= n-1; n >= 3.
 * c3d_separation_profile: mean, sd, contact — n doubles each, indexed by s = 0 .. n-1, any of them NULL, not all three.  For s >= 1, over
 * the (n-s) Kp values d_k(i, i+s), k in list order:
 *   mean[s]    = their mean: R(s), the polymer's distance against separation;
 *   sd[s]      = their population sd about that mean, from the deviations in a second walk over the same values;
 *   contact[s] = #{d < cutoff} / ((n-s) Kp): P(s); an exact 64-bit count, divided once.  The `<` is strict as in c3d_ensemble_map, so the
 *                profile is the diagonal average of that map — ON PURPOSE not the `<=` of the clash count above, which is the reference's.
 *   s = 0 gives mean 0, sd 0, contact 1, as the map's diagonal does.  cutoff is needed (finite, > 0) for contact only; n >= 2.
 * Both: no state of the solve changes (the guarantee of c3d_compare_replicas).  Floating-point sums take no atomics and their order follows
 * from n and the pick list alone (strided partial sums met in a fixed tree; per separation, bead chunks ascending and models in list
 * order): two calls on the same state return the same bits, and extra models leave the replicas' entries their bits.  Counts, minima
 * and maxima are order-free and exact.  The results agree with a host computation of the same definitions to about T 2^-53 relative,
 * T the number of terms of the sum (n, or (n-s) Kp).
 * C3D_ERR_INVALID, before any launch: no replicas, n < 3 (profile: n < 2), n_extra < 0 or extra models without coordinates, K >
 * C3D_COMPARE_MAX_MODELS, every output NULL, sep outside 1..n-1, a cutoff that is not finite or <= 0 where one is needed, the pick list's
 * refusals of c3d_ensemble_map, extra coordinates that are not finite or have |x| >= 1e6.  C3D_ERR_NOMEM: no device memory for the scratch.
 * Scratch, one allocation per call, freed before it returns.  Geometry: 44 n K + 56 K bytes (24 n a model of coordinates, 4 + 8 + 8 a bead
 * of counts, nearest and furthest partners, 8 + 48 a model of results): 0.4 MB at 455 beads x 20 models, 14.4 MB at 16384 x 20.  Profile:
 * 24 n K + 4 Kp + 24 n bytes: 0.23 MB at 455 x 20, 8.3 MB at 16384 x 20 — where the three n x n maps would be 6 GiB.
 * Stats "geometry_runs" and "separation_runs" count the calls that completed. */
#define C3D_GEOMETRY_FIELDS 6
int c3d_geometry_replicas(c3d_ctx* ctx, const double* extra_xyz, int n_extra, double cutoff, int sep,
                          int64_t* clashes, int32_t* bead_clashes, double* nearest, double* chain);
int c3d_separation_profile(c3d_ctx* ctx, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick,
                           double cutoff, double* mean, double* sd, double* contact);
/* IF against model distance per genomic separation, on the device (c3d_score_stratified.inc k_str_*).  The Spearman coefficient of
 * c3d_score_replicas runs over all pairs |i-j| >= range; IF falls and distance rises with |i-j| in every chain-like model, so the
 * distance-decay curve dominates it.  This entry correlates inside each stratum s = |i-j| and combines the strata with variance-stabilising
 * weights: HiCRep's stratum-adjusted correlation (Yang et al. 2017), with a rank correlation inside each stratum to match the reference's
 * metric.
 *
 * Models.  K = n_replicas + n_extra, numbered and taken as c3d_geometry_replicas takes them.  On a precision-64 context that is the fp64
 *   state bit for bit.  Otherwise the floats are taken as doubles.  Extra models are n x 3 doubles, checked as there.
 * Distance.  d_k(i,j) is the unit's cmp_dist, with the host's bits, rounded to integer thousandths of an A as the reference's
 *   sprintf "%.3f" does (round_milli_dev, spearman_IF_pdb.pl:47).
 * Stratum.  Stratum s is lo <= s <= hi, with lo = range >= 1 and hi = max_sep, or n-1 when max_sep is 0.
 *   - It holds the N = n - s pairs (i, i+s), i = 0 .. N-1.
 *   - It pairs IF[i][i+s] with that rounded distance.
 *   - IF must be symmetric over the strata asked for.  A stratum of the ordered pairs (both triangles, as the reference walks them) then
 *     has every observation twice.  That leaves a correlation of average ranks unchanged.
 *   - Zeros of IF count, as in the reference.
 *   - -0.0 equals 0.0 (rank_key).
 * Doubled ranks.
 *   - a_i = 2 x (average rank of IF[i][i+s] within the stratum).
 *   - b_i = 2 x (average rank of the rounded distance within the stratum).
 *   - Both are integers: #{smaller} + #{not larger} + 1.
 * Integer sums.
 *   - T = N(N+1).
 *   - C = N sum a_i b_i - T^2.
 *   - A = N sum a_i^2 - T^2.
 *   - B = N sum b_i^2 - T^2.
 *   - All are exact in int64.  The largest term is 4 N^4 < 2.9e17 at N = 16383.
 * Per-stratum coefficient.
 *   - rho[k][s] = (double)C / sqrt((double)A * (double)B) when A > 0 and B > 0.
 *   - Otherwise it is NaN.  That covers a constant stratum and N = 1.
 *   - It is also NaN for s outside [lo, hi].
 * Combined coefficient per model.
 *   - With cN = (double)N*(double)N*(double)N, num = sum_s (double)C / cN.
 *   - den = sum_s sqrt((double)A*(double)B) / cN.
 *   - Both sums run over the strata with A > 0 and B > 0, in ascending s, each sum one sequential chain.
 *   - scc[k] = num / den, or NaN when no stratum counts.
 *   - This is sum w_s rho_s / sum w_s with HiCRep's weights w_s = N_s sqrt(var(a/2N) var(b/2N)).
 *   - It is negative for a good model, as rho_mean of c3d_ensemble_score is.
 *
 * Outputs: rho is K x n, row-major; scc holds K values; sums is K x n x C3D_STRATUM_FIELDS and holds C, A, B per stratum, 0 outside
 * [lo, hi].  Any output may be NULL, not all three.  A caller can form a band-limited SCC from sums without another call.  rho and scc are
 * formed on the host from the integer sums read back, with exactly the expressions above; the integer sums are the device's work: one LDS
 * sort per stratum of IF (k_str_if) and per (stratum, model) of the distances (k_str_model), two binary searches an element, int64 sums.
 * Every quantity before the last division is an exact integer: the result has no summation order and takes no atomics.
 * No state of the solve changes (the guarantee of c3d_compare_replicas); two calls return the same bits; extra models leave the replicas'
 * entries their bits.
 * C3D_ERR_INVALID with the function's name, before any launch: no replicas, n < 2, no IF, range < 1, max_sep < 0, max_sep > n-1 or
 * 0 < max_sep < range, range > n-1, every output NULL, and the model-set refusals of c3d_geometry_replicas (n_extra < 0 or extra models
 * without coordinates, K > C3D_COMPARE_MAX_MODELS, extra coordinates that are not finite or have |x| >= 1e6).  C3D_ERR_INVALID after the pass
 * that finds it, with nothing written to the outputs: IF not symmetric over the strata asked for, a non-finite IF entry there, a pair of a
 * model further apart than 50 000 A (the limit of c3d_score_replicas and of the host twin).  C3D_ERR_NOMEM: no device memory for the scratch.
 * Memory: IF goes into the context's scoring scratch as c3d_score_replicas uploads it (8 n^2 bytes, kept: 1.7 MB at 455 beads, 2 GiB at
 * 16384).  Everything else is one allocation per call, freed before it returns: 48 n K bytes (24 n a model of coordinates, 24 n of sums)
 * + 4 bytes a pair of the strata (the IF ranks) + 8 bytes a stratum: 0.85 MB at 455 x 20 and range 3, 0.55 GB at 16384 x 20 (0.54 GB of it
 * the IF ranks of all 1.3e8 pairs).
 * Stat "stratified_runs" counts the calls that completed. */
#define C3D_STRATUM_FIELDS 3
int c3d_stratified_score(c3d_ctx* ctx, const double* IF, int range, int max_sep, const double* extra_xyz, int n_extra,
                         double* rho, double* scc, int64_t* sums);
/* A model's fit to the data bead by bead, on the device (c3d_score_bead.inc k_bead_*): which bins are placed badly.  Two tracks a bead,
 * both the reference's own metrics restricted to one first index: the Spearman coefficient of row i of IF against the distances of bead i
 * (spearman_IF_pdb.pl:42-70 with r1 = i), and the restraint tallies of bead i (count_satisfied_tbl_rows, sum_noe_dev;
 * chromosome3D.pl:447-485, 581-600).
 *
 * Models.  K = n_replicas + n_extra, numbered and taken exactly as c3d_stratified_score takes them: on a precision-64 context the fp64
 *   state bit for bit, otherwise the floats taken as doubles; extra models are n x 3 doubles, checked as there.
 * Beads.  beads = NULL with n_beads = 0 means every bead: B = n.  Otherwise beads holds n_beads indices in 0..n-1, strictly ascending, and
 *   B = n_beads.  Every output is indexed [k][b] in list order, b the position in the list.
 * Distance.  q_k(i,j) = the unit's cmp_dist, with the host's bits, rounded to integer thousandths of an A as the reference's "%.3f" does
 *   (round_milli_dev).  A pair (i, j), j != i, of an asked bead beyond 50 000 A (or not a number) refuses the call after the pass that
 *   finds it, as in c3d_stratified_score.
 * Row.  Row i is J(i) = { j : |i-j| >= range }, N_i = max(0, i-range+1) + max(0, n-i-range) members.  It pairs IF[i][j] with q_k(i,j).
 *   - IF is read from row i only: no symmetry is required.
 *   - Zeros of IF count, as in the reference.  -0.0 equals 0.0 (rank_key).
 *   - A value of a row asked for that is not finite refuses the call.
 * Doubled ranks and integer sums, exactly as in c3d_stratified_score.
 *   - a_j and b_j are #{smaller} + #{not larger} + 1 within the row: 2 x the average ranks, integers.
 *   - T = N(N+1), C = N sum a_j b_j - T^2, A = N sum a_j^2 - T^2, B = N sum b_j^2 - T^2.
 *   - All are exact in int64: 4 N^4 < 2.9e17 at N = 16383.
 *   - sums[(k*B + b)*C3D_BEAD_FIELDS + 0..2] holds C, A, B.  The three are 0 when N_i <= 1.
 * Coefficient.  rho[k*B + b] = (double)C / sqrt((double)A * (double)B) when A > 0 and B > 0, otherwise NaN; formed on the host from the
 *   integers that were read back.  An all-zero IF row (an unmappable bin) is therefore NaN, not an error.
 * Tallies.  A partner j of bead i counts iff the context's target matrix holds a target t10 > 0 (in tenths of an A) for (i,j) and
 *   |i-j| >= model.min_sep (the rule of c3d_score_replicas' kernel); partners on both sides of i.  With d = (double)q / 1000.0 and
 *   t = (double)t10 / 10.0 the comparisons are the reference's, in doubles:
 *   - satisfied: +1 if d < t + 0.5, -1 if d < t - 0.5.
 *   - dev_milli: + (q - 100 t10) if d > t + 0.2, + (100 t10 - q) if d < t - 0.2: an exact integer of thousandths.
 *   - restrained[b] is the number of such partners (it does not depend on the model), satisfied[k*B + b] the net count,
 *     dev_milli[k*B + b] the deviation.  Summed over all beads each is twice the whole model's figure (every pair has two ends).
 *   - The targets are read from the float matrix every context fills (t10 = lrintf(10 t), as c3d_score_replicas reads it); a precision-64
 *     context whose float matrix is not filled is read from the integer tenths it keeps: the same integers.
 *
 * Any output may be NULL, not all five.  IF may be NULL when neither rho nor sums is asked for (IF is not read then).
 * C3D_ERR_INVALID with the function's name, before any launch and with nothing written: no context or no replicas, n < 2, range < 1 or
 * range > n-1, rho or sums asked for without IF, every output NULL, a bead list that is out of range, not strictly ascending or given with
 * n_beads <= 0, beads = NULL with n_beads != 0, and the model-set refusals of c3d_geometry_replicas.  C3D_ERR_INVALID after the pass that
 * finds it, with nothing written: a non-finite IF value in a row asked for, a model too wide.  C3D_ERR_NOMEM: no device memory.
 * No state of the solve changes; two calls return the same bytes; extra models leave the replicas' entries their bits.  No atomics and no
 * floating-point sum on the device: k_bead_if sorts a row of IF in LDS, k_bead_model a row of distances a (bead, model) and, in the same
 * pass over j, tallies the bead's restrained partners; every sum is an int64 block reduction.
 * Memory: IF goes into the context's scoring scratch as c3d_stratified_score uploads it (8 n^2 bytes, kept; not where only tallies are
 * asked for).  Everything else is one allocation per call, freed before it returns: 24 n K (models) + 4 B n (IF ranks of the rows asked
 * for, where a coefficient is asked for) + 16 B (sums of squares, bead list, restrained) + (24 + 4 + 8) B K (sums, satisfied, dev_milli)
 * + flags: 1.2 MB at 455 x 20 with every bead, about 1 GiB of ranks at 16384 beads with every bead (a bead list cuts that to its rows).
 * Stat "bead_runs" counts the calls that completed; "bead_if_ms" / "bead_models_ms" are the device time of the two passes. */
#define C3D_BEAD_FIELDS 3
int c3d_bead_scores(c3d_ctx* ctx, const double* IF, int range, const int32_t* beads, int n_beads,
                    const double* extra_xyz, int n_extra,
                    double* rho, int64_t* sums, int32_t* restrained, int32_t* satisfied, int64_t* dev_milli);
/* Bead accessibility on the device (c3d_score_access.inc k_access): where a locus sits in the fold — buried in the interior, or on the
 * surface where a probe of a given size reaches it.  The Shrake-Rupley construction over uniform spheres: the track bead-model packages
 * call "accessibility" (TADbit), the quantity that relates a model to accessibility assays.  A neighbour count (bead_clashes, nearest of
 * c3d_geometry_replicas) does not say it: six partners on one side leave a bead half open, six around it close it.
 *
 * Models.  K = n_replicas + n_extra, numbered and taken exactly as c3d_geometry_replicas takes them: on a precision-64 context the fp64
 *   state bit for bit, otherwise the floats taken as doubles; extra models are n x 3 doubles, checked as there.
 * Points.  points = n_points x 3 doubles, unit vectors u_p, used as given; NULL asks for the lattice of c3d_sphere_points(n_points).
 *   P = n_points, 1 <= P <= C3D_ACCESS_MAX_POINTS.  A caller's point is refused unless it is finite and its squared norm
 *   (ux ux + uy uy) + uz uz lies within 1e-9 of 1.
 * Definition.  For model k, bead i and point p, in doubles, every product and every sum rounded on its own (no fma):
 *   - R = radius + probe, R2 = R * R.
 *   - c = x_i + R u_p, a component as one product and one sum.
 *   - point p of bead i is buried if some bead j != i of the same model has ((ex ex) + ey ey) + ez ez < R2 with e = c - x_j; the
 *     comparison is strict.  j = i is left out by index, not by distance: a second bead at the same coordinates does bury.
 *   - exposed[k n + i] = the number of points of bead i that are not buried, 0 .. P.
 *   The accessible area follows on the host as 4 pi R^2 exposed / P.  With uniform spheres `radius` and `probe` enter through their sum
 *   alone; they are two arguments because they are two physical quantities.
 * c3d_sphere_points, host only, no device needed: the Fibonacci lattice of n_points unit vectors into u (n_points x 3 doubles),
 *   z = 1 - (2k+1)/P, r = sqrt(1 - z z), phi = k pi (3 - sqrt 5), u_k = (r cos phi, r sin phi, z), k = 0 .. P-1.  C3D_ERR_INVALID for
 *   n_points outside 1..C3D_ACCESS_MAX_POINTS or u NULL.
 * exposed is K x n, row-major, required.  device_ms, optional: one double, the device time of the call's kernel from HIP events (there is
 * no stat key for it).
 * The result is a set of integers that depends on no summation order: no atomics on floating-point data, two calls return the same bytes,
 * extra models leave the replicas' entries their bytes, and the integers are those of a host loop over all j written with the operations
 * above.  The device does not test all j: only beads closer to bead i than 2 R can bury a point of i, so a workgroup first lists a bead's
 * neighbours — d(i,j)^2 <= 4 R2 (1 + 2^-20), a bound that is proved conservative under the limits below (c3d_score_access.inc) — and
 * tests points against the list.
 * No state of the solve changes (the guarantee of c3d_compare_replicas).
 * C3D_ERR_INVALID with the function's name, before any launch and with nothing written: no context or no replicas, n < 2, n_extra < 0 or
 * extra models without coordinates, K > C3D_COMPARE_MAX_MODELS, exposed NULL, n_points outside 1..C3D_ACCESS_MAX_POINTS, radius not finite
 * or <= 0, probe not finite or < 0, radius + probe outside [0.01, 1e5] A (the range in which the neighbour bound is proved for |x| < 1e6),
 * a bad point, extra coordinates that are not finite or have |x| >= 1e6.  C3D_ERR_INVALID after the pass that finds it, with nothing
 * written: a replica's coordinate that is not finite or has |x| >= 1e6 (a solve that has diverged; the bound's proof does not cover it).
 * C3D_ERR_NOMEM: no device memory for the scratch.
 * Scratch, one allocation per call, freed before it returns: 28 n K + 24 P bytes and a flag word (24 n a model of coordinates, 4 a bead of
 * counts, 24 a point): 0.26 MB at 455 beads x 20 models, 9.2 MB at 16384 x 20, both with 96 points. */
#define C3D_ACCESS_MAX_POINTS 1024
int c3d_sphere_points(int n_points, double* u);
int c3d_accessibility(c3d_ctx* ctx, const double* extra_xyz, int n_extra, double radius, double probe,
                      const double* points, int n_points, int32_t* exposed, double* device_ms);
/* Compartment eigenvectors on the device (c3d_score_compartment.inc k_cpt_*): do the models reproduce the A/B compartment pattern of the
 * data?  At 500 kb and 1 Mb compartments are the large-scale feature of a contact map; the standard read-out is the leading eigenvector of
 * the correlation matrix of the observed/expected (O/E) map, and the sign of PC1 is the compartment call.
 *
 * Maps, in order, Q in all: IF if non-NULL (n x n with the context's n; refused if asymmetric, not finite or holding a negative entry);
 *   then one map per picked model, its distance map (the distance of c3d_compare_replicas: ((ux ux) + uy uy) + uz uz, every operation
 *   rounded on its own, then sqrt); then, with C3D_COMPARTMENT_CONSENSUS in flags, the consensus: the pick list's mean distance map, summed
 *   in list order as c3d_ensemble_map defines `mean`.
 * Models.  K = n_replicas + n_extra, numbered and taken as in c3d_ensemble_map (the fp64 state bit for bit on a precision-64 context).
 *   pick = the models analysed, in order; NULL with 0 = all K; at most 256 entries.
 * Definitions, for a symmetric n x n map M:
 *   1. Expected.  For s = 1..n-1, E[s] = mean over i of M(i, i+s), i ascending.  E[0] = 0.
 *   2. O/E.  X(i,j) = M(i,j) / E[|i-j|] where |i-j| >= min_sep and E[|i-j|] != 0, and X(i,j) = 1 elsewhere (min_sep = 1: the diagonal is
 *      1).  Every pair i < j is computed once and stored to both halves: X equals its transpose bit for bit.
 *   3. Row statistics.  m_i = mean_j X(i,j); q_i = sqrt(mean_j (X(i,j) - m_i)^2), the two-pass form; D_i = 1/q_i, or 0 for a row without
 *      spread, which gets 0 in every vector.  live = the number of rows with q_i > 0.
 *   4. The operator.  C = Z Z^T / n with Z = D (X - m 1^T): the Pearson correlation of the rows of X.  It is never formed; X being
 *      symmetric, both passes are matrix-vector products with X:  w = X (D v) - (m^T D v) 1,  C v = D (X w - m (1^T w)) / n.
 *   5. Iteration.  V (n_vec x n) starts from `start`, or from c3d_compartment_start's vectors if start is NULL.  One round
 *      orthonormalises V by modified Gram-Schmidt in index order (v_a -= (v_b . v_a) v_b for b < a, then v_a /= |v_a|) and sets
 *      Y_a = C v_a.  After `iters` rounds (V <- Y), V is orthonormalised once more and Y computed once more; then lambda_a = v_a . y_a,
 *      share = lambda_a / live (0 where live is 0) and residual = |y_a - lambda_a v_a|_2.  A vector that projects to exactly 0 makes the
 *      call C3D_ERR_INVALID ("dependent start vectors"), with nothing written.
 *   6. Sign.  IF's vectors, and every map's vectors when no IF is given: the entry of largest magnitude is positive (lowest index on
 *      ties).  Vector a of a model or consensus map, when IF is given: its dot product with IF's vector a is made non-negative; an exact
 *      0 falls back to the first rule.
 *   7. Fit to the data (only with IF), per map other than IF: agreement[a][b] = |Pearson r| of the map's vector a against IF's vector b
 *      (a table, because PC1 of one map may be PC2 of the other; means first, then the centred sums); same_side[a] =
 *      #{i : v_map,a(i) v_IF,a(i) > 0} / n, an exact count divided once.
 * c3d_compartment_start, host only, exact in fp64: start[a n + i] = ((double)h + 0.5) / 2^32 - 0.5 with the 32-bit integer hash
 *   h = k + 0x9E3779B9; h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16 of k = 4 i + a: no libm, one division
 *   by a power of two.  C3D_ERR_INVALID for n < 3, n_vec outside 1..min(3, n-1) or start NULL.
 * Outputs, any may be NULL but not all of expected, vectors, share, agreement, same_side; agreement and same_side are refused without
 *   IF.  expected Q x n; vectors Q x n_vec x n; share, residual Q x n_vec; agreement (Q - 1) x n_vec x n_vec and same_side
 *   (Q - 1) x n_vec, the maps after IF; device_ms, optional: the HIP-event time of the call (there is no stat key for it).
 * Every floating-point sum has an order that follows from n, n_vec and the pick list alone, through the scoring unit's one block
 * reduction: no atomics, two calls return the same bytes, and a model's results are the same bytes whether it is analysed alone or among
 * others.  No state of the solve changes.
 * C3D_ERR_INVALID with the function's name, before any launch and with nothing written: no context or no replicas, n < 3, n_vec outside
 * 1..min(3, n-1), iters outside 0..C3D_COMPARTMENT_MAX_ITERS, min_sep outside 1..n-1, unknown flag bits, consensus with an empty list,
 * the pick and extra-model refusals of c3d_ensemble_map (and more than 256 picks), the outputs as above, start vectors that are not
 * finite.  After the pass that finds it, with nothing written: a bad IF, dependent start vectors.  C3D_ERR_NOMEM: no device memory for
 * the scratch.
 * Scratch, one allocation per call, freed before it returns: 8 n^2 bytes per map in flight (IF is uploaded and turned into X in place, a
 * model's X is written straight from coordinates) + (24 + 32 n_vec) n bytes of row statistics and vectors per map in flight + 24 n K of
 * coordinates + 16 n_vec n.  Maps run in batches whose X slots fit C3D_SCORE_SCRATCH_BYTES, at least one a batch: one 2 GiB slot at 16384
 * beads, and all 22 maps at once (36.4 MB of X) at 455 beads x 20 models with IF and the consensus. */
#define C3D_COMPARTMENT_MAX_VECTORS 3
#define C3D_COMPARTMENT_MAX_ITERS   10000
#define C3D_COMPARTMENT_CONSENSUS   1      /* flags: one more map after the models: the pick list's mean distance map */
int c3d_compartment_start(int n, int n_vec, double* start);   /* the library's start vectors, n_vec x n */
int c3d_compartments(c3d_ctx* ctx, const double* IF, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick,
                     int flags, int min_sep, int n_vec, int iters, const double* start,
                     double* expected, double* vectors, double* share, double* residual,
                     double* agreement, double* same_side, double* device_ms);
/* Insulation profiles and domain boundaries on the device (c3d_score_insulation.inc k_ins_*): do the models reproduce the domains (TADs) of
 * the data?  Compartments are the large-scale feature of a contact map, domain boundaries the local one; the standard read-out is the
 * insulation profile: for every bin the mean of the map over the square that straddles the bin.  Its minima on a contact map, or maxima on
 * a distance map, are the boundaries, and each boundary has a strength.
 *
 * Maps, in order, Q in all: IF if non-NULL (n x n with the context's n); then one map per picked model; then, with
 *   C3D_INSULATION_CONSENSUS in flags, the consensus of the pick list.  Models, pick, n_pick (at most 256), extra models and the fp64
 *   state of a precision-64 context are taken exactly as c3d_compartments takes them, and the pair distance d is the same:
 *   sqrt(((ux ux) + uy uy) + uz uz), every operation rounded on its own.
 * Windows.  `windows` holds n_win (1..C3D_INSULATION_MAX_WINDOWS) strictly ascending w with 1 <= w <= C3D_INSULATION_MAX_WINDOW and
 *   2w + 1 <= n.  w_max is the last of them.
 * Definitions, per map M, window w and bead i:
 *   1. Square.  Bead i is inside when w <= i <= n-1-w; its square is the w^2 cells (a, b) with a in [i-w, i-1] and b in [i+1, i+w].  Only
 *      the band 2 <= b-a <= 2 w_max of a map is ever read.
 *   2. mean[q][w][i] is NaN for a bead that is not inside.  For a bead that is inside, without C3D_INSULATION_CONTACT:
 *      IF: (sum M(a,b)) / w^2.  Model: (sum d(a,b)) / w^2.  Consensus: (sum c(a,b)) / w^2, c(a,b) the pick list's mean distance, summed
 *      in list order from 0 and divided once by Kp, as c3d_ensemble_map defines `mean`.
 *      With C3D_INSULATION_CONTACT: model: #{cells: d < cutoff} / w^2; consensus: #{(k, cell): d_k < cutoff} / (w^2 Kp); both exact
 *      integer counts (they are below 2^53 and are carried in doubles, where every count is exact), divided once; the < is strict, as in
 *      c3d_ensemble_map.  IF is unchanged.
 *   3. score[q][w][i] = log2(mean_i / mbar), mbar the mean of mean_i over the valid beads; a bead is valid when it is inside and
 *      mean_i > 0, every other bead gets NaN; if no bead is valid the whole row is NaN.
 *   4. Boundaries are a function of the score row alone, through exact operations only (comparisons, min/max, one subtraction).
 *      y = -score for IF and for contact maps, where boundaries are minima; y = +score for distance maps, where they are maxima.  Bead i
 *      is a boundary if i-1, i and i+1 are valid and y_i > y_{i-1} and y_i > y_{i+1}.  Its strength is the prominence as
 *      scipy.signal.peak_prominences defines it: walk left from i-1 while the bead is valid and y_j <= y_i, keeping the minimum; the same
 *      to the right; strength = y_i - max(left minimum, right minimum).  boundary is 0 or 1; strength is 0 where boundary is 0.
 *   5. Fit to IF (only with IF), for the Q - 1 maps after it, per window.  fit_r = Pearson r of the map's score against IF's score over
 *      the beads valid in both: the means first, then the centred sums, r = sxy / sqrt(sxx syy); NaN with fewer than 3 such beads or a
 *      constant side.  Its sign is left as it comes: a good distance map has r < 0, a good contact map r > 0, the convention of
 *      c3d_ensemble_score.  fit_counts[4] = {n_IF, n_map, IF_matched, map_matched}: the boundaries counted are those with strength >=
 *      min_strength, and one is matched when the other set has a counted boundary within tol beads.  Integers, exact given the boundary
 *      and strength arrays.
 * Outputs, any may be NULL but not all of them; fit_r and fit_counts are refused without IF.  mean, score, strength: Q x n_win x n
 *   doubles; boundary: Q x n_win x n int32; fit_r: (Q - 1) x n_win doubles; fit_counts: (Q - 1) x n_win x 4 int32; device_ms, optional:
 *   the HIP-event time of the call (there is no stat key for it).
 * How it runs.  No n x n map is formed for anything: the host packs IF's upper band (row a holds M(a, a+1 .. a + 2 w_max)) and uploads
 *   n x 2 w_max doubles, k_ins_band writes the consensus in the same layout, and a model's squares come straight from its coordinates.
 *   The squares of a bead are nested — the square of w is the union of the rings r = max(i-a, b-i) = 1..w — so every listed window comes
 *   out of one walk over the largest square a bead is inside.  A workgroup owns a map and 32 consecutive beads, their coordinates and a halo of w_max
 *   on either side in LDS, and every bead's walk computes its distances from them.  With C3D_INSULATION_STAGE, up to w_max = 40, the
 *   tile's distinct distances are computed once into LDS and the walks read them: the same values in the same order, the same bytes.
 *   Measured (profiles/r31_insulation.md) the staged form is not faster at any w_max it fits, so it is not the default.
 * Every floating-point sum is one of positive terms whose order follows from n, the window and the pick list alone, through the scoring
 * unit's one block reduction: no atomics on floating-point data, no prefix sums, two calls return the same bytes, a model's rows are
 * the same bytes whether it is analysed alone or among others, and a window's whether it is listed alone or with others.  No state of
 * the solve changes.
 * C3D_ERR_INVALID with the function's name, before any launch and with nothing written: the refusals of c3d_compartments for the context,
 * models, picks, extra coordinates and unknown flag bits; n < 3; n_win outside 1..C3D_INSULATION_MAX_WINDOWS or windows NULL; a window out
 * of range, not ascending or with 2w + 1 > n; consensus with an empty list; C3D_INSULATION_CONTACT with a cutoff that is not finite or
 * <= 0; min_strength not finite or < 0; tol < 0; the outputs as above; IF asymmetric, not finite or negative anywhere in the band that is
 * read (the host checks while it packs the band).  C3D_ERR_NOMEM: no device memory for the scratch.
 * Scratch, one allocation per call, freed before it returns: 24 n K of coordinates + 16 n w_max per band (IF, consensus) +
 * 28 Q n_win n of results: 1.4 MB at 455 beads x 20 models with IF, the consensus and windows {5, 10, 25}; 105 MB at 16384 x 20 with
 * windows {8, 32, 128} (7.9 MB of coordinates, 33.6 MB a band, 30.3 MB of results), where one n x n map alone is 2 GiB. */
#define C3D_INSULATION_MAX_WINDOW   128
#define C3D_INSULATION_MAX_WINDOWS  8
#define C3D_INSULATION_CONSENSUS    1   /* one more map after the models: the pick list's mean distance map / pooled contacts */
#define C3D_INSULATION_CONTACT      2   /* model and consensus maps: contacts (d < cutoff) in the square, not the mean distance */
#define C3D_INSULATION_STAGE        4   /* stage a tile's distances in LDS where w_max <= 40: the same bytes, measured no faster; for measurements */
int c3d_insulation(c3d_ctx* ctx, const double* IF, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick,
                   int flags, const int32_t* windows, int n_win, double cutoff, double min_strength, int tol,
                   double* mean, double* score, int32_t* boundary, double* strength,
                   double* fit_r, int32_t* fit_counts, double* device_ms);
/* Loop enrichment on the device (c3d_score_loop.inc k_loop_*): which pixels of IF are loops, and do the models close them?  Compartments
 * are the large-scale feature of a contact map and domain boundaries the local one; loops are the point feature: pixels (i, j) whose
 * contact frequency stands out against their own neighbourhood beyond what the distance decay explains.  The read-outs are the four
 * local-background ratios of HiCCUPS and aggregate peak analysis (APA).  A model closes a loop when the two anchors sit nearer than
 * the pixel's surroundings: the same ratios on its distance map, below 1.
 *
 * Maps, in order, Q in all: IF if non-NULL (n x n with the context's n); then one map per picked model, its distance map; then, with
 *   C3D_LOOP_CONSENSUS in flags, the consensus: the pick list's mean distance, summed in list order and divided once by Kp, as
 *   c3d_ensemble_map defines `mean`.  Models, pick, n_pick (at most 256), extra models and the fp64 state of a precision-64 context are
 *   taken exactly as c3d_insulation takes them (pick NULL and n_pick 0: all models), and the pair distance is the same:
 *   sqrt(((ux ux) + uy uy) + uz uz), every operation rounded on its own.  C3D_LOOP_IF_ONLY in flags leaves the models out (it refuses a
 *   pick list and the consensus).  A call needs at least one of: IF, a non-empty pick list.
 * Mask.  `mask` is optional and holds n int32 values; non-zero means an unmappable bin (c3d_balance_matrix's `masked` can be passed as
 *   it is).  A cell (a, b) is live when neither a nor b is masked.  The mask applies to every map alike.
 * Geometry.  0 <= p < w <= C3D_LOOP_MAX_WINDOW.  Separations s = j - i with min_sep <= s <= max_sep, min_sep >= 2w + 1, max_sep <= n - 1,
 *   B = max_sep - min_sep + 1 <= C3D_LOOP_MAX_BAND.  Only the separations s_lo = min_sep - 2w through s_hi = min(max_sep + 2w, n - 1) of
 *   any map are ever read, S = s_hi - s_lo + 1 of them; no window touches the diagonal.  A pixel (i, j = i + s) is inside when i >= w
 *   and j + w <= n - 1.
 * Definitions, per map M:
 *   1. Expected.  E[s] = (sum over i ascending, with (i, i+s) live, of M(i, i+s)) / (the number of such i), 0 when there is none.
 *      `expected` is Q x S.
 *   2. Neighbourhoods of a pixel, over cells (i + a, j + b) with a, b in [-w, w]; P = {|a| <= p and |b| <= p}.
 *      donut: not P, a != 0, b != 0.  lower-left: not P, a >= 1, b <= -1 (the quadrant towards the diagonal).
 *      horizontal: |a| <= 1, |b| > p.  vertical: |b| <= 1, |a| > p.
 *   3. Sums.  SM_x = the sum of M(cell) over the live cells of neighbourhood x, SE_x = the sum of E[separation of the cell] over the
 *      same cells.  Each of the eight sums is one accumulator that takes its cells in row-major order: a ascending, then b ascending.
 *      A pixel's numbers are therefore a function of the pixel alone: the same bytes from the dense scan and from the list pass, alone
 *      or among others, on any grid.
 *   4. Ratios.  r_x = M(i,j) / ((SM_x / SE_x) * E[s]), three roundings in that order.  NaN when the pixel is not inside, when i or j is
 *      masked, when E[s] == 0, or when SM_x == 0 or SE_x == 0.  The sign is left as it comes: a loop is r > 1 on IF and r < 1 on a
 *      distance map.
 *   5. Dense scan, IF only.  `ratio` is 4 x B x n doubles, [x][s - min_sep][i], x in the order donut, lower-left, horizontal,
 *      vertical; NaN wherever i + s > n - 1.
 *   6. Peaks, IF only.  thr[4] in the same order.  A pixel is a candidate when all four ratios are non-NaN, r_x >= thr[x] for each and
 *      M(i,j) >= min_obs.  A candidate is a peak unless another candidate within Chebyshev distance `merge` (0 <= merge <= w) has a
 *      larger M(i,j), or an equal one and a lexicographically smaller (i, j).  Exact comparisons of the ratio bytes and of input
 *      values.  `peaks`: max_peaks x 2 int32, the peaks in ascending (i, j) order; only the written ones are stored.
 *      report[C3D_LOOP_REPORT] = {candidates, peaks found, peaks written = min(found, max_peaks), inside pixels with a masked end}.
 *      Finding more than max_peaks is not an error.
 *   7. The list.  list_in non-NULL: L = n_list pairs (i, j) in the caller's order, at most C3D_LOOP_MAX_LIST, each with i < j,
 *      j - i in [min_sep, max_sep] and j <= n - 1; a pair may be not inside, its ratios are then NaN.  Otherwise the list is the written
 *      peaks of this call (this needs IF), L = report[2]: size `at` for max_peaks.  `at`: Q x L x 6 doubles
 *      {M(i,j), E[s], r_donut, r_ll, r_h, r_v}; on a model row M(i,j) is the pair distance; IF's rows hold the same bytes as `ratio`
 *      at those pixels.  `closed`: Q x 2 int32 {listed pixels whose r_donut and r_ll are both non-NaN, of those the number with both
 *      on the loop side}: > 1 for IF, < 1 for models and the consensus.
 *   8. APA.  For offsets (a, b) in [-w, w]^2, apa[q][a][b] is the mean of M(i+a, j+b) / E[separation of the cell] over the listed
 *      pixels that are inside and whose cell is live with E != 0: the quotient rounded first, the terms added in list order through the
 *      scoring unit's block reduction (thread t takes the pixels t, t + 256, ...) and divided once by their number; NaN when there are
 *      none.  `apa` is Q x (2w+1)^2 doubles.  p2ll[q] = apa[q][0][0] / (the mean of the corner x corner cells a in [w - corner + 1, w],
 *      b in [-w, -w + corner - 1], added row-major), 1 <= corner <= w; NaN if any term is NaN.
 * Outputs, any may be NULL but not all of them.  ratio, peaks and report are refused without IF; at, closed, apa and p2ll are refused
 *   when the list would be empty by construction: no list_in and no IF.  device_ms, optional: the HIP-event time of the device part
 *   (there is no stat key for it).
 * How it runs.  No n x n map is formed for anything: the host packs IF's band (row a holds M(a, a + s_lo .. a + s_hi), n x S doubles)
 *   and uploads it with the mask, k_loop_band writes the consensus in the same layout, a model's cells come from its coordinates.
 *   k_loop_expected: a workgroup a (separation, map).  k_loop_scan, the hot kernel: a workgroup owns a 32 x 32 tile of pixels, stages
 *   the (32 + 2w)^2 cells and their E values by separation in LDS (at most 72^2 doubles, 41 KiB) and gives every thread four pixels,
 *   each walking its (2w+1)^2 cells once.  k_loop_nms, k_loop_rows, k_loop_offsets, k_loop_write: the suppression and the ordered
 *   compaction, on integer counts and an integer scan.  k_loop_list: a thread a (listed pixel, map).  k_loop_apa: a workgroup a (cell
 *   offset, map).  With the list taken from the peaks the host reads the report once between the two parts.
 * Determinism.  No atomics on floating-point data and no floating-point prefix sums; two calls return the same bytes; a model's rows
 *   are the same bytes whether it is analysed alone or among others, and a listed pixel's whether it is listed alone or in a longer
 *   list (apa and p2ll are sums over the list and depend on it).  No state of the solve changes.
 * C3D_ERR_INVALID with the function's name, before any launch and with nothing written: the refusals of c3d_insulation for the context,
 * models, picks, extra coordinates and unknown flag bits; p, w, min_sep, max_sep, B, merge or corner out of the ranges above; thr NULL
 * when peaks are wanted (peaks, report, or a list taken from the peaks), or a threshold that is not finite or is <= 0; min_obs not
 * finite or < 0; max_peaks < 0 or above C3D_LOOP_MAX_LIST; a bad list entry or n_list; the consensus of no model (C3D_LOOP_IF_ONLY with C3D_LOOP_CONSENSUS); the output
 * rules above; IF asymmetric, not finite or negative anywhere in the band that is read (the host checks while it packs the band).
 * C3D_ERR_NOMEM: no device memory for the scratch.
 * Measured on an MI355X (profiles/r33_loops.md, tools/loops.py; the entry's device_ms): 455 x 20 with IF and the consensus, w = 5,
 * separations 11..200: 0.52 ms; 4096 x 20 with IF, w = 10, B = 512: 2.5 ms; 16384 x 20 without IF on a list of 4096 pixels: 6.4 ms; 16384
 * with IF alone, w = 20, B = 512: 19.6 ms, of which k_loop_scan and the suppression take 15.2 ms — 9.1e11 cells/s, 10 % of the LDS read
 * rate and 19 % of the fp64 addition rate: the walk is VALU-bound; the numpy restatement on the same host: about 10 minutes, scaled.
 * Scratch, one allocation per call, freed before it returns: 24 n K of coordinates + 8 n S per band (IF, consensus) + 8 Q S of
 * expected values + with IF 32 B n of ratios (when asked for) and 2 B n of flags + 48 Q L for the list: 9.1 MB at 455 beads x 20 models
 * with IF, the consensus, w = 5, separations 11..200, `ratio` and max_peaks = 4096; 12.3 MB at 16384 x 20 with w = 20, B = 512 and a
 * list of 4096 pixels (90.1 MB with the consensus band), where one n x n map alone is 2 GiB. */
#define C3D_LOOP_MAX_WINDOW  20
#define C3D_LOOP_MAX_BAND    1024
#define C3D_LOOP_MAX_LIST    65536
#define C3D_LOOP_CONSENSUS   1      /* one more map after the models: the pick list's mean distance map */
#define C3D_LOOP_IF_ONLY     2      /* no model maps: IF alone (refuses a pick list and the consensus) */
#define C3D_LOOP_REPORT      4
int c3d_loops(c3d_ctx* ctx, const double* IF, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick,
              int flags, const int32_t* mask, int p, int w, int min_sep, int max_sep,
              const double* thr, double min_obs, int merge, int corner,
              const int32_t* list_in, int n_list, int max_peaks,
              double* expected, double* ratio, int32_t* peaks, int32_t* report,
              double* at, int32_t* closed, double* apa, double* p2ll, double* device_ms);
/* Entanglement of the models on the device (c3d_score_entangle.inc k_ent_*): writhe, average crossing number and linking.  Every other
 * analysis entry measures a model through its distances, which are blind to handedness and to topology: a mirror pair has the same
 * distance map and opposite chirality at every scale, and the annealer, whose only repulsion is the soft k_rep term, passes beads through
 * one another at high temperature, so the replicas of a run are where the topology varies.  The measures are the Gauss double integrals
 * over the chain.  No state of the solve changes.
 * Models and segments.  The models are K = n_replicas + n_extra, numbered, taken and checked exactly as c3d_geometry_replicas takes them:
 * on a precision-64 context the fp64 state bit for bit, else the floats widened; extra models are n x 3 doubles.  A model of n beads has
 * S = n - 1 segments, segment s joins beads s and s+1; the entry needs n >= 4.
 * The pair term g(s,t) of segments s != t of one model with bead positions x:
 *     a = x[t]   - x[s]        c = x[t+1] - x[s]
 *     d = x[t]   - x[s+1]      b = x[t+1] - x[s+1]
 *     T(u,v,w) = 2 atan2( u.(v x w),  |u||v||w| + (u.v)|w| + (u.w)|v| + (v.w)|u| )
 *     g(s,t)   = ( T(a,b,c) + T(a,d,b) ) / (4 pi)
 * the Van Oosterom-Strackee signed solid angle of the planar parallelogram {p_t - p_s} spanned by the two segments, seen from the origin,
 * split into two triangles of the same orientation: exact for straight segments, equal to
 * (1/4 pi) of the double integral of (r_s - r_t).(dr_s x dr_t)/|r_s - r_t|^3, and with the integral's sign (a right-handed helix is
 * positive).  A triangle with numerator 0 and denominator 0 contributes 0 (coincident beads are one such case).  g(s,t) := 0 for
 * |s - t| <= 1: adjacent segments are coplanar.  The device forms the two numerators as c.(a x b) and -(d.(a x b)), the same triple
 * products turned, and divides a sum by 2 pi once at its end; a bead-to-bead length is sqrt(((ux ux) + uy uy) + uz uz).
 * Counted pairs.  (s,t) is counted iff min_sep <= |s-t| <= max_sep, 2 <= min_sep <= S-1; max_sep = 0 means S-1, otherwise
 * min_sep <= max_sep <= S-1.  A small max_sep gives the local writhe: chirality at that scale.
 * Outputs; any may be NULL, but not all of them.  C(s) is the set of t for which (s,t) is counted.
 *     seg_writhe[k S + s] = sum over t in C(s) of g_k(s,t)          seg_acn[k S + s] = the same sum of |g_k(s,t)|
 *     writhe[k] = sum over s of seg_writhe[k S + s], which is 2 sum_{s<t} g: the writhe of the open chain
 *     acn[k]    = the same sum over seg_acn: the average crossing number
 *     link[(k D + p) D + q] = sum over s in domain p, t in domain q, (s,t) counted, of g_k(s,t)       link_abs[...] = the same sum of |g|
 * Domains are D = n_domains consecutive runs of segments given by bounds[0..D], strictly increasing with bounds[0] = 0 and
 * bounds[D] = S; domain p is the segments bounds[p] .. bounds[p+1]-1; 1 <= D <= C3D_ENTANGLE_MAX_DOMAINS.  bounds == NULL is allowed
 * only if link and link_abs are NULL too.  Off the diagonal `link` is the Gauss linking integral of the two sub-chains (two closed,
 * once-linked rings joined into one chain give +-1 in their block), on the diagonal the domain's own writhe; the entries of a model's
 * table sum to writhe[k] up to rounding.  g(s,t) and g(t,s) agree to rounding only, so every entry is taken from the p <= q side — s in
 * domain p — and copied across: the table is symmetric bit for bit.  The natural bounds are the boundaries c3d_insulation reports.  The
 * table costs one more evaluation of every counted pair with p <= q, a workgroup a block: its time is set by the largest block.
 * `ms`, if not NULL, receives the device time of the call in milliseconds, as c3d_loops reports it.
 * Guarantees.  No floating-point atomics; every sum has an order that follows from n, min_sep, max_sep and bounds alone: a thread adds
 * its pairs in the order of its walk, the sixteen threads of a row segment meet in index order, a model's S row sums and a block's
 * partial sums meet in the fixed tree.  Two calls on the same state return the same bits; extra models leave the replicas' entries
 * their bits.  Mirroring a model (one coordinate negated) negates seg_writhe, writhe and link exactly and leaves the acn outputs' bits:
 * numerators negate, denominators keep their bits.
 * C3D_ERR_INVALID, before any launch: the refusals of c3d_geometry_replicas that apply (no context, no replicas, n_extra < 0 or extra
 * models without coordinates, K > C3D_COMPARE_MAX_MODELS, extra coordinates that are not finite or have |x| >= 1e6), n < 4, min_sep or
 * max_sep out of range, every output NULL, n_domains outside 1..C3D_ENTANGLE_MAX_DOMAINS when a table is asked for, bad bounds,
 * bounds == NULL with a table asked for.  C3D_ERR_NOMEM: no device memory for the scratch, one allocation per call, freed before it
 * returns: 24 n K of coordinates + 16 S K of row sums + 16 K + 16 D D K + 4 (D + 1) bytes.  The entry keeps no stat key.
 * Measured on an MI355X (profiles/r34_entanglement.md, tools/entanglement.py; the entry's ms): 455 x 20: 0.19 ms, with a 64-domain table
 * 0.42 ms; 16384 x 20: 58 ms for 5.4e9 ordered segment pairs, 9.2e10 pairs/s, bound by the two atan2 of a pair; with the table 97 ms;
 * the numpy restatement on the same host: 0.9 s and about 7 minutes (scaled). */
#define C3D_ENTANGLE_MAX_DOMAINS 256
int c3d_entanglement(c3d_ctx* ctx, const double* extra_xyz, int n_extra, int min_sep, int max_sep,
                     const int32_t* bounds, int n_domains,
                     double* writhe, double* acn, double* seg_writhe, double* seg_acn,
                     double* link, double* link_abs, double* ms);
/* Balancing a raw contact matrix on the device (c3d_score_balance.inc k_bal_*): the input side.  c3d_set_if_matrix expects a normalised
 * matrix; this entry turns raw contact counts into one by iterative correction (ICE), vanilla coverage (VC) or its square root (sqrt-VC).
 * It needs a context, but no targets and no replicas, and changes no state of the solve.  Bins that cannot be balanced get weight 0, so
 * their rows of the balanced matrix are 0: c3d_set_if_matrix reads IF == 0 as "no restraint" and the analyses read an all-zero row as an
 * unmappable bin, so masked bins need no special case anywhere.
 *
 * Input.  M is n x n row-major doubles, 2 <= n <= the context's max_beads in force (5120, or up to 16384 after
 *   c3d_set_option("max_beads", n), which is the consent to the memory).  Every value is finite and >= 0 and M(i,j) == M(j,i) exactly;
 *   anything else is C3D_ERR_INVALID, found on the device before any round (the check c3d_compartments makes of IF).
 * Definitions.
 *   1. The matrix the marginals see: A'(i,j) = M(i,j) if |i-j| >= ignore_diags, else 0.  ignore_diags >= 0; 0 keeps everything, 2 is
 *      the customary value.
 *   2. The mask.  nnz_i = #{ j : A'(i,j) > 0 } over all j, exact integers.
 *      U0 = { i : (mask_in == NULL or mask_in[i] == 0) and nnz_i >= max(min_nnz, 1) }.  Closure: repeat
 *      O = { i in U : A'(i,j) == 0 for every j in U }, U <- U \ O, until O is empty (a count of positive entries, so exact; usually one
 *      pass).  masked[i] is 0 for a kept bin, 1 for one listed in mask_in, 2 for too few non-zeros, 3 for one removed by the closure.
 *      |U| < 2 is C3D_ERR_INVALID.
 *   3. The start.  w_i = w0[i] on U if w0 is given (every such value finite and > 0, else C3D_ERR_INVALID; values at masked bins are not
 *      read), else w_i = 1 on U; w_i = 0 off U, always.
 *   4. Rounds t = 0, 1, ... with the exponent p = 1 for ICE and VC, p = 1/2 for sqrt-VC:
 *        s_i = w_i * sum_j A'(i,j) w_j for i in U;  mbar = (sum_{i in U} s_i) / |U|;  r_i = s_i / mbar;
 *        var_t = sum_{i in U} (r_i - 1)^2 / |U|, and history[t] = var_t;
 *        if var_t < tol: stop converged with T = t; else if t == max_iters: stop unconverged with T = max_iters;
 *        else w_i <- w_i / r_i^p (for p = 1/2: w_i / sqrt(r_i)).
 *      So there are at most max_iters updates and max_iters + 1 marginal passes; max_iters = 0 only evaluates w0.  VC and sqrt-VC are
 *      this loop with max_iters forced to 1 and tol forced to 0, and they refuse w0 != NULL.  For ICE 0 <= max_iters <=
 *      C3D_BALANCE_MAX_ITERS and tol >= 0.  A weight that stops being finite and positive is C3D_ERR_DIVERGED.
 *   5. The scale, with the mbar of the last pass: w_i <- w_i * sqrt(target / mbar), target > 0 and finite.  The mean row sum of the
 *      balanced A' over U is then target.  K1 is scale-invariant, so structures do not depend on target.
 *   6. Outputs, any may be NULL.  weights[n]: the final weights.  masked[n]: as in 2.  balanced (n x n) = fl(fl(w_i * w_j) * M(i,j))
 *      over ALL diagonals, the ignored ones included: the weights are multiplied first, so the result is symmetric bit for bit (device
 *      ranking and c3d_compartments refuse an asymmetric IF) and equals numpy's (w[:,None] * w[None,:]) * M bit for bit; two
 *      multiplications, never a fused form.  history: max_iters + 1 doubles, entries beyond T are not written.  report[C3D_BALANCE_REPORT]
 *      = { T, converged (1 / 0), var_T, |U|, #masked by 1, #masked by 2, #masked by 3, mbar of the last pass before scaling }.
 *      device_ms: the HIP-event time of the device part — from the first count of non-zeros, after the matrix is uploaded and checked,
 *      to the kernel that forms `balanced`; the read-backs are not in it.  There is no stat key for the call.
 * Determinism.  Every sum is a fixed tree (the scoring unit's block_reduce), no atomics.  A row's s_i is the sum of the products of the
 *   column pairs 2t + 512k a thread t takes, low column first, closed by one block_reduce of a workgroup that owns 4 consecutive rows,
 *   times w_i: it depends on n, ignore_diags, the row's values and w only — not on the grid, the method, the other outputs asked for or
 *   how often the host looks.  mbar and var_t are two passes over s in that order, the mean first, then the centred sum, thread t the
 *   bins t + 256k.  Two calls return the same bytes.
 * Stopping without a host round-trip per round.  The update kernel writes the round record (var_t, mbar, t and a stop word) on the
 *   device, and every later kernel of the call reads the stop word and returns at once.  The host enqueues rounds in batches of 16 and
 *   reads the record between them; with C3D_BALANCE_CHECK_EVERY_ROUND in flags it reads it after every round.  Both ways return the same
 *   bytes and the same T as the definition.
 * C3D_ERR_INVALID with the function's name and with nothing written: no context, no matrix, n < 2 or above max_beads, an unknown method
 * or flag bit, ignore_diags < 0, target not finite or <= 0, tol < 0 or max_iters out of range (ICE), w0 with VC or sqrt-VC — all before
 * any launch; a bad matrix, |U| < 2 (ignore_diags >= n ends there) and a bad w0 on U after the pass that finds them.  C3D_ERR_DIVERGED and
 * C3D_ERR_NOMEM (no device memory for the scratch) write nothing either.
 * Measured on an MI355X (profiles/r32_balance.md, tools/balance.py): a round — one streaming pass over the matrix and the update — takes
 * 10 us at 455 beads, 19 us at 2048, 69 us at 5792, 134 us at 8192 and 461 us at 16384, where the 2 GiB are read at 4.65 TB/s, 74 % of
 * the 6.3 TB/s a streaming read achieves; one round of the numpy restatement on the same host: 20 ms at 16384.
 * Scratch, one allocation per call, freed before it returns: 8 n np bytes for the call's copy of the matrix — np = n rounded up to even,
 * so that every row starts 16-byte aligned, the pad column 0; `balanced` is formed in place over that copy after the last round and read
 * back from there — plus 8 np + 16 n + 8 (max_iters + 1) bytes of weights, marginals, mask codes, counts and history: 1.67 MB at 455
 * beads, 2 GiB + 0.4 MB at 16384 beads. */
#define C3D_BALANCE_ICE      0
#define C3D_BALANCE_VC       1
#define C3D_BALANCE_SQRT_VC  2
#define C3D_BALANCE_CHECK_EVERY_ROUND 1      /* flags: the host reads the round record after every round (test and measurement knob) */
#define C3D_BALANCE_MAX_ITERS 10000
#define C3D_BALANCE_REPORT 8
int c3d_balance_matrix(c3d_ctx* ctx, const double* M, int n, int method, int flags, int ignore_diags, int min_nnz,
                       const int32_t* mask_in, const double* w0, double tol, int max_iters, double target,
                       double* weights, int32_t* masked, double* balanced, double* history, double* report, double* device_ms);
/* Reproducibility of contact maps: HiCRep's stratum-adjusted correlation coefficient (SCC) of every pair of n_maps maps, on the device.
 * Do the replicates agree, does the balanced map still agree with the raw one, how far is condition A from condition B: each map is
 * smoothed with a (2h+1) x (2h+1) box mean, the two maps are correlated inside every genomic separation, pairs that are empty in both maps
 * are dropped and the strata are combined with rank-variance weights.  Any symmetric non-negative map will do — IF, c3d_balance_matrix's
 * `balanced`, the contact-frequency map of c3d_ensemble_map.  The entry needs a context, no targets and no replicas; it changes no state
 * of the solve and keeps no stat key and no option key.
 *
 * Input.  maps is n_maps matrices of n x n row-major doubles, 2 <= n_maps <= C3D_MAPSIM_MAX_MAPS, 3 <= n <= the max_beads in force.  Every
 *   value is finite and >= 0 and M(i,j) == M(j,i) exactly; anything else is C3D_ERR_INVALID with the map's index in the message, found on
 *   the device before any other kernel (the check c3d_compartments makes of IF, once a map).  h holds n_h half-widths, 1 <= n_h <=
 *   C3D_MAPSIM_MAX_WIDTHS, each in 0..C3D_MAPSIM_MAX_H, strictly ascending.  0 <= min_sep <= max_sep <= n - 1; max_sep == 0 means n - 1.
 *   lo = min_sep, hi = the resolved max_sep, S = hi - lo + 1.  flags: 0 or C3D_MAPSIM_KEEP_ZEROS.
 * Definitions.
 *   1. Smoothing.  For a map M and a half-width h, the row window of (i,j) is r in [max(0,i-h), min(n-1,i+h)] and the column window
 *      c in [max(0,j-h), min(n-1,j+h)].  t(r) = M(r,c0) + M(r,c0+1) + ... over the column window in ascending c, starting from the first
 *      term; X(i,j) = (t(r0) + t(r0+1) + ...) / (double)(rows x cols) over the row window in ascending r, with one IEEE division.  A row
 *      sum depends only on (r, column window), so forming the row sums once and adding them down the columns gives the bits of the direct
 *      double loop.  Only additions and one division occur.  h = 0 is the map itself.
 *   2. A stratum.  Stratum s of a pair of maps (p, q), p < q, holds the pairs (i, i+s), i = 0..n-s-1, with x_i = X_p(i,i+s) and
 *      y_i = X_q(i,i+s).  Pair i is kept unless x_i == 0 and y_i == 0; with C3D_MAPSIM_KEEP_ZEROS all pairs are kept.  N is the number of
 *      kept pairs.
 *   3. Moments, over the kept pairs.  mx = (sum x) / N and my likewise (both 0 if N == 0); Cxy = sum (x - mx)(y - my), Cxx = sum (x - mx)^2,
 *      Cyy = sum (y - my)^2, every product rounded on its own.  Every sum goes through the scoring unit's block_reduce: thread t brings the
 *      pairs i = t + 256k in ascending k, and an unkept pair brings 0.  A stratum's bytes therefore depend on the two maps, h and s only.
 *   4. Ranks.  Inside the kept pairs, a_i and b_i are the doubled average ranks of x and y, each on its own: #{smaller} + #{not larger} + 1,
 *      the definition c3d_stratified_score uses; -0.0 ranks as 0.0.  A = N sum a^2 - T^2, B = N sum b^2 - T^2, T = N(N+1), exact in int64
 *      (4 N^4 < 2.9e17 at N = 16384).  Only the two sums of squares are needed, so neither sort keeps an index; unkept pairs take the pad
 *      key and sort behind the kept ones.
 *   5. Per stratum, on the host, in doubles.  rho_s = Cxy / sqrt(Cxx * Cyy).  w_s = sqrt((double)A * (double)B) / (4 N^3), with
 *      4 N^3 = ((4.0 * N) * N) * N: N times the square root of the product of the variances of rank/N, which are HiCRep's weights.  The
 *      stratum counts if N >= 3, A > 0, B > 0, Cxx > 0 and Cyy > 0.  Otherwise rho_s is NaN and w_s is 0.
 *   6. SCC.  scc(p,q) = (sum w_s rho_s) / (sum w_s), the two sums sequential over ascending counted s; NaN if no stratum counts.
 *      scc(q,p) = scc(p,q).  scc(p,p) = 1.0, written by the host.
 * Outputs, any may be NULL.  P = n_maps (n_maps - 1) / 2 pairs, in the order (0,1), (0,2), ..., (1,2), ...
 *   scc [n_h][n_maps][n_maps] the combined coefficient;  rho [n_h][P][S] rho_s;  moments [n_h][P][S][3] { Cxy, Cxx, Cyy };
 *   counts [n_h][P][S][3], int64 { N, A, B };  smoothed [n_h][n_maps][S][n]: row s - lo holds X(i, i+s) for i < n - s, then zeros;
 *   device_ms: one double, the HIP-event time from after the upload and check to the last kernel (the sum over the half-widths; the
 *   read-backs between them are not in it).
 * Determinism.  There are no atomics.  Two calls return the same bytes.  A pair's results do not depend on n_maps, on the other
 *   half-widths or on which outputs are asked for.  Passing the maps in another order permutes the outputs and changes no bit of them:
 *   every product and every sum under a square root is commutative in the two maps.
 * C3D_ERR_INVALID with the function's name and with nothing written, before any launch: no context or no maps; n_maps, n, n_h, a
 * half-width, the order of the half-widths, min_sep or max_sep out of range; unknown flag bits.  A bad matrix after the check pass, before
 * any other kernel.  C3D_ERR_NOMEM when the scratch does not fit, with nothing written.
 * Measured on an MI355X (profiles/r35_map_similarity.md, tools/map_similarity.py): 455 x 2 maps, h = 0..5, all strata: 0.74 ms; 4096 x 4,
 * separations 1..500, h = 3: 0.86 ms; 16384 x 2, separations 1..2000, h = 5: 6.9 ms, against about 51 s of the numpy restatement (scaled).
 * Scratch, one allocation per call, freed before it returns: 8 n_maps n^2 bytes for the call's copy of the maps, 8 n_maps S n bytes for
 * one half-width's smoothed bands at a time in diagonal-major storage (the stratum kernel reads contiguously; there is no second n x n
 * array per map), and 48 P S bytes of moments and counts: 3.3 MB + 3.3 MB at 455 x 2 with all strata, 4 GiB + 0.5 GiB at 16384 x 2 with
 * 2000 strata.
 * Out of scope: HiCRep's depth down-sampling, its variance estimate, and sparse input. */
#define C3D_MAPSIM_KEEP_ZEROS 1      /* flags: pairs that are 0 in both maps stay in their stratum */
#define C3D_MAPSIM_MAX_MAPS  16
#define C3D_MAPSIM_MAX_H     20
#define C3D_MAPSIM_MAX_WIDTHS 8
int c3d_map_similarity(c3d_ctx* ctx, const double* maps, int n_maps, int n, const int32_t* h, int n_h, int min_sep, int max_sep, int flags,
                       double* scc, double* rho, double* moments, int64_t* counts, double* smoothed, double* device_ms);
/* rank[k] = replica index with the k-th lowest int(E_noe) (chromosome3D.pl:796-802,822-828);
 * ties broken by replica id. */
int c3d_rank(c3d_ctx* ctx, int32_t* rank);

/* --- host helpers (formats of the reference; no device needed) ------------------------ */
/* chromosome3D.pl:116-129,164-179: whitespace-separated numbers, N = fields on line 1.
 * *IF is malloc'ed (free with c3d_free). */
int c3d_parse_if_file(const char* path, double** IF, int* n);
void c3d_free(void* p);
/* <ID>.dist, <ID>.rr, contact.tbl exactly as chromosome3D.pl:156-161, 203-205, 360 write them */
int c3d_write_front_half(const int32_t* dist10, int n, int min_sep, const char* dist_path,
                         const char* rr_path, const char* tbl_path, int* n_restraints);
/* contact.tbl reader (format chromosome3D.pl:360; parse rules :497-520) */
int c3d_read_tbl(const char* path, int32_t** ri, int32_t** rj, int32_t** rt10, int* R);
/* CA-only model in the layout assess_dgsa leaves (chromosome3D.pl:853-857, 208-215) preceded
 * by REMARK lines carrying the energies (`REMARK noe = ...`, :611-614). resname from the
 * bundled output_models (MET). */
int c3d_write_pdb(const char* path, const float* xyz, int n, double e_noe, double e_bond, double e_rep,
                  const char* title);
/* Residue names of the models c3d_write_pdb writes.  The reference names residue i after letter i of a fixed 663-letter
 * pseudo-protein (`$REFSEQUENCE`, chromosome3D.pl:93-98; 3-letter codes through %AA1TO3, :78) — the chemistry CNS needs and a
 * bead model does not; its bundled output_models were re-exported with every residue MET, which is the default here.  seq1 =
 * one-letter amino-acid codes, one per bead (chromosome3d_amd/data/refsequence.fasta holds the reference's); beads beyond its
 * end, and letters outside the 20 standard ones, are MET.  NULL or "" restores all-MET.  Process-wide; call before writing. */
int c3d_set_residue_sequence(const char* seq1);
int c3d_read_pdb_ca(const char* path, float** xyz, int* n);
/* A16, what assess_dgsa does to every solver-output PDB before it ranks them (chromosome3D.pl:813-820): filter_nonCA
 * :864-880 (REMARK rows go to `log_path`, appended after a line with the input path; ATOM rows containing "CA" stay),
 * reindex_chain :831-862 (atoms and residues renumbered from 1, chain id blanked), `sed -i "s/END//g"` :818 (the END row
 * becomes an empty line), add_connect_rows :208-215 (CONECT i i+1, END).  `out_path` may equal `in_path`; `log_path` may
 * be NULL.  The result is byte-identical to the file the reference leaves behind (tests/golden/output_side). */
int c3d_shape_pdb(const char* in_path, const char* out_path, const char* log_path);
/* chromosome3D.pl:447-485, 581-600 on coordinates rounded to 3 decimals as a PDB holds them */
int c3d_assess(const float* xyz, int n, int R, const int32_t* ri, const int32_t* rj, const int32_t* rt10,
               double relax, int* satisfied, double* sum_dev);
/* The same two numbers and, appended to `path`, the violation table count_satisfied_tbl_rows leaves behind (chromosome3D.pl:475-483): two
 * '#' lines naming pdb_label and tbl_label, then one row per restraint in the reference's format, violated rows first. */
int c3d_write_violations(const float* xyz, int n, int R, const int32_t* ri, const int32_t* rj, const int32_t* rt10, double relax,
                         const char* pdb_label, const char* tbl_label, const char* path, int* satisfied, double* sum_dev);
/* spearman_IF_pdb.pl:42-70 */
int c3d_spearman_if_dist(const double* IF, const float* xyz, int n, int range, double* rho);
/* the same for n_models models (n_models*n*3 coordinates) of one matrix: IF is ranked once */
int c3d_spearman_if_dist_batch(const double* IF, const float* xyz, int n, int n_models, int range, double* rho);

/* Cross-resolution check of the reference's output_models/similarity.txt (data only; the definitions
 * were recovered from the bundled models and reproduce its numbers to 1e-12):
 *   c3d_reduce_model      mean of consecutive bead pairs (an odd last bead is kept): out has (n+1)/2 beads
 *   c3d_model_similarity  two models of n beads: Spearman of the i<j distances, and the RMS difference of
 *                         those distances after scaling a's by mean(d_b)/mean(d_a) ("RMSD" in that file) */
int c3d_reduce_model(const double* xyz, int n, double* out);
int c3d_model_similarity(const double* a, const double* b, int n, double* spearman, double* rmsd);

#ifdef __cplusplus
}
#endif
#endif /* C3D_H_ */
