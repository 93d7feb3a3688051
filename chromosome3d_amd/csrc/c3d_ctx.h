// c3d_ctx.h — private to the host units of libc3d.so (c3d_api.cpp, c3d_config.cpp, c3d_gate.cpp, c3d_run.cpp, c3d_debug.cpp, c3d_analysis.cpp): the
// context, the error macros, the gate's entry object and the helpers that one unit defines and another calls (namespace c3d::host).  What
// a single unit uses stays in that unit's anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/c3d.h"
#include "c3d_host.h"
#include "c3d_internal.h"

// a launcher of c3d_internal.h, or the hipError_t a chain of them ended with: C3D_ERR_HIP with "<what>: <the runtime's text>"
#define LAUNCH_TRY(what, expr)                                                                 \
    do {                                                                                       \
        if (const hipError_t e__ = (expr); e__ != hipSuccess)                                  \
            return c3d::fail(C3D_ERR_HIP, std::string(what ": ") + hipGetErrorString(e__));    \
    } while (0)
// a call of the HIP runtime: its own text is the <what>
#define HIP_TRY(expr) LAUNCH_TRY(#expr, expr)

namespace c3d::host {
using c3d::fail;
// frees a temporary device allocation on every exit path
template <class T>
struct DevTmp {
    T* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
};

struct Op {
    c3d::DevStep p;
    int stage;
    bool counted;   // a force evaluation = one SA step
};

// What the last op of the last range ran: the kernel family and its form, as chosen for the launch (c3d_step_kernel_name formats it)
struct KernelRecord {
    enum Family { NONE, STEP, LBFGS_EVAL, PAIRS_SYM, STEP64, LBFGS_EVAL64, CLUSTER } family = NONE;
    c3d::StepForm step{};                        // STEP, LBFGS_EVAL
    c3d::Form64 f64{};                           // STEP64, LBFGS_EVAL64
    int pot = 0, rpw = 0, nb = 0, wl = 0;        // PAIRS_SYM (pot), CLUSTER
    bool rs1 = false, late = false, tp = false;  // PAIRS_SYM (rs1), CLUSTER
};

// hipFree of a context's buffer; a failure (only possible after a device fault) is kept in the error string, the pointer is dropped either way
template <class T>
void dev_free(T*& p) {
    if (!p) return;
    const hipError_t e = hipFree(p);
    if (e != hipSuccess) (void)fail(C3D_ERR_HIP, std::string("hipFree: ") + hipGetErrorString(e));
    p = nullptr;
}

// ---- c3d_config.cpp: the context's configuration as the kernels take it; the keys of its option and stat tables (row k, nullptr past the last)
c3d::DevModel dev_model(const c3d_ctx* c);
c3d::DevStep dev_step(const c3d_ctx* c, int kind, float dt, float w_all, float w_vdw, float repel_s, float t_bath);
c3d::DevFire dev_fire(const c3d_ctx* c);
const char* option_key(int k);
const char* stat_key(int k);

// ---- c3d_api.cpp: the replica state and the fp64 targets (a change of configuration drops / rebuilds them), the pinned stage of the read-backs
void free_replica_buffers(c3d_ctx* c);
int build_targets64(c3d_ctx* c);
int ensure_stage(c3d_ctx* c, size_t bytes);
int read_back(c3d_ctx* c, const void* dev, size_t bytes);        // device -> c->h_stage, synchronised

// ---- c3d_gate.cpp: code objects and the gate every HIP call of a context runs under ("code objects" there)
enum Unit : unsigned {
    UNIT_DEVICE = 0, UNIT_SCORE, UNIT_CLUSTER_BASE, UNIT_EMBED, UNIT_F64, UNIT_SYM,
    UNIT_CLUSTER_P0, UNIT_CLUSTER_TP0 = UNIT_CLUSTER_P0 + 5, UNIT_COUNT = UNIT_CLUSTER_TP0 + 5
};
constexpr unsigned unit_bit(unsigned u) { return 1u << u; }
// A public entry: current device, units present (launching entries only), shared side of the gate — in that order.  Every HIP call of a
// context runs inside one; only the device queries of c3d_create (count, properties, attributes) come before it.
struct Entry {
    int rc = C3D_OK;
    bool locked = false;
    Entry(const c3d_ctx* c, unsigned extra, bool launches);
    ~Entry();
    Entry(const Entry&) = delete;
    Entry& operator=(const Entry&) = delete;
};
int preload_units(int device);             // c3d_create: what the process option "preload" names, before the context's first HIP resource
long units_loaded();                       // stat "units_loaded": code objects this process has loaded (all devices)
unsigned units_loaded_mask(int device);    // stat "units_loaded_mask": bit per unit

// ---- c3d_run.cpp: the launch program and its executor
void build_program(c3d_ctx* c);
void drop_graphs(c3d_ctx* c);
int plan_cluster(c3d_ctx* c);
int active_groups(const c3d_ctx* c);
int max_rms_force(c3d_ctx* c, double* out);
}  // namespace c3d::host

struct c3d_ctx {
    // ---- what the caller configured: model, schedule, and every option with its default (c3d_config.cpp holds the table of their keys)
    c3d_model model;
    std::vector<c3d_stage> stages;
    c3d_fire_params fire;
    float gtol = 0.0f;
    int check_every = 250;
    bool use_graph = true;                 // "use_graph"
    int rpw = 2, stage_dma = 1, graph_chunk = 256;   // "rows_per_wave", "stage_dma", "graph_chunk"
    static constexpr int kMaxGroups = 4;
    int ngroups = 2;                       // "replica_groups": groups stepped on separate streams (overlap latency phases)
    int event_timing = 1;                  // "event_timing" 0: no event pair around c3d_run_steps / c3d_run (c3d_last_timing then reports 0 ms)
    int kernel_timing = 0;                 // "kernel_timing": the multi-step kernel's own start / end events (kev0, kev1)
    int precision = 32;                    // "precision" 64: the fp64 reference step (c3d_f64.hip) instead of the fp32 kernels
    int f64_max_beads = C3D_F64_MAX_BEADS_DEFAULT;   // "f64_max_beads": the largest n a precision-64 context initialises (2560..16384)
    bool f64_lbfgs = false;                // "f64_lbfgs": the caller's consent to kind-8 stages on a precision-64 context (k64_lbfgs_eval + k64_lbfgs_move)
    int f64_column_chunk = 0;              // "f64_column_chunk": 0 = by size, else k64_step_chunked's CHUNK wherever n > chunk (c3d::column_chunk64_for)
    int sym = 0;                           // "symmetric": symmetric-tile step kernels (c3d_sym.hip): 1 on, 0 off (measured slower: DESIGN 7)
    int start_mode = 0;                    // "start": initial structure: 0 random coil, 1 extended strand (reference :2413-2416)
    bool narrow_columns = true;            // "narrow_columns" 0: every block 4 columns per lane (round 2's layout; measurements)
    int resident = -1;                     // "resident": multi-step cluster kernel (c3d_cluster.hip): -1 where it applies, 0 off, 1 as -1 without the back-off
    int resident_min_ops = 4;              // "resident_min_ops": shorter ranges go step by step (at least 1)
    double spin_wait_us = 400.0;           // "spin_wait_us": a cluster launch is waited for on its completion mark for this long before hipStreamSynchronize (0: never)
    int cluster = -1;                      // "cluster": 1 / -1: use the cluster kernel where it applies, 0: never
    int cluster_late = -1;                 // "cluster_late_tiles": measurement knob: 0 = the tile sums always travel with the rows; -1 = planner's choice
    int cluster_geom = 0;                  // "cluster_geometry": measurement knob: 100 CW + 10 RPW + helpers forces that cluster geometry (0 = planner's choice)
    int xcd_base = 0, xcd_count = 8;       // "cluster_xcd_base" / "cluster_xcd_count": the XCDs a multi-step launch of this context lives on
    bool static_place = true;              // "cluster_static_placement": cluster launches number the workgroups of an XCD as blockIdx / 8 (verified in the kernel)
    int eval_rpw = 4;                      // "eval_rows_per_wave": 4 = scalar pair term in the forces hook, 2 = the packed one, -2 = scalar at two rows per wave
    bool pair_targets = true;              // "pair_targets": the per-step kernel's resident row-pair constants (measurement knob)
    bool wide_tiles = true;                // "wide_tiles": beyond the multi-step kernel's reach, 16 rows a workgroup and 4 a wave (measurement knob)
    int column_chunk = 0;                  // "column_chunk": 0 = the library's choice, else the chunked form's CHUNK (c3d::column_chunk_for)
    int max_beads = C3D_MAX_BEADS_DEFAULT; // "max_beads": the largest matrix c3d_set_if_matrix / c3d_set_restraints accept (5120..16384)
    int embed_max_beads = C3D_EMBED_MAX_BEADS_DEFAULT;   // "embed_max_beads": the largest n c3d_embed_replicas accepts (4549..16384)
    int embed_form = 0;                    // "embed_form": 0 = k_dg_eig while it fits, the tiled eigen stage beyond; 1 = tiled at every n
    int embed_batch = 0;                   // "embed_batch": 0 = replicas per batch from C3D_EMBED_SCRATCH_BYTES, else that many
    int bb_steps = 1000;                   // "final_minimiser_steps": two-point / L-BFGS steps before FIRE takes the stage over
    bool final_bb = true;                  // "final_minimiser": 1 = stages of kind 5 start with the two-point step-size minimiser, 0 = they are FIRE stages
    int lbfgs_mem = 5;                     // "lbfgs_memory": pairs an L-BFGS stage keeps (1..8), fixed at the stage's first step
    int prefetch_ranks = 1;                // "prefetch_ranks" 0: no helper thread (measurement knob)
    int device_ranks = 0;                  // "device_ranks": who ranks the IF matrix for c3d_score_replicas (c3d.h)
    // ---- test hooks
    bool inject_timeout = false;           // "resident_inject_timeout": pretend the next resident launch timed out
    bool inject_misplaced = false;         // "cluster_static_placement" 2: workgroup 0 of the next cluster launch reports a wrong XCD
    bool inject_incomplete = false;        // "cluster_inject_incomplete": the next cluster launch expects one workgroup more than will ever report
    // ---- what the device reported (c3d_create)
    int device = 0, num_cus = 0, num_xcc = 0;   // (test hook "cluster_num_xcc" overwrites the last: pretend a partitioned device)
    // ---- targets and replica state
    int n = 0, npad = 0, ntiles = 0, nrep = 0, R = 0;
    size_t rep_floats = 0;                 // 3*npad per replica
    bool have_targets = false, have_replicas = false;
    uint64_t seed = 82364;
    uint32_t first_rep = 0;
    std::vector<int32_t> h_dist10;         // n*n, from K1 (empty when restraints came from a tbl)
    std::vector<int32_t> r_i, r_j, r_t10;  // c3d_set_restraints' list (0-based, i < j, one entry a pair): what a precision-64 context builds its tenths from
    c3d::DevBuffers buf{};
    c3d::Buffers64 b64;                    // fp64 state (c3d_f64.hip), double buffered by step parity like the fp32 buffers
    float *d_feval = nullptr, *d_sym_scratch = nullptr;
    int2* d_sym_tiles = nullptr;
    c3d::LbfgsBuffers lb{};                // the L-BFGS history, tile sums and state (ensure_lbfgs), freed with the replica buffers
    c3d::LbfgsBuffers64 lb64{};            // their history, tile sums and state in doubles (ensure_lbfgs), freed with the replica buffers
    int lbfgs_parity = -1;                 // parity the last L-BFGS step left its state in (stat "lbfgs_resets")
    int parity = 0;
    // The IF side of the Spearman coefficient (average ranks of the matrix's ordered pairs: a radix sort of up to 2 x 10^5 records, 5 ms at
    // N = 455) depends on the INPUT alone: c3d_set_if_matrix starts it on a helper thread over a copy of the matrix, and c3d_score_replicas
    // — which comes after the anneal — takes the result when its IF argument holds the same numbers (memcmp), else computes as before.
    struct IfRanks {
        std::thread worker;
        std::vector<double> matrix, rank;  // the copy the worker reads; rank_matrix of if_pair_ranks
        size_t m = 0;
        double mean = 0, saa = 0;
        int n = 0, range = 0;
        bool valid = false;
        void join() { if (worker.joinable()) worker.join(); }
        void release() {                   // the worker's copies go with the matrix they belong to
            join();
            valid = false;
            std::vector<double>().swap(matrix);
            std::vector<double>().swap(rank);
        }
    } ifr;
    // ---- program and graphs, the streams and events they run on
    std::vector<c3d::host::Op> program;
    size_t pc = 0;
    long steps_done = 0;
    bool zero_weight = false;              // some stage has w_all = 0: ITS steps take the general kernels (run_ops splits the range there)
    bool has_two_point = false;            // the program holds two-point minimiser steps (run_ops splits ranges at their borders)
    bool has_lbfgs = false;                // the program holds L-BFGS steps (kinds 8 / 9: run_ops splits ranges at their borders, per-step path only)
    std::map<std::tuple<long, int, int, int>, hipGraphExec_t> graphs;
    hipStream_t stream = nullptr;          // group 0 / everything that is not a step launch
    hipStream_t gstream[kMaxGroups] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t gev[kMaxGroups] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr, ev0 = nullptr, ev1 = nullptr;
    hipEvent_t kev0 = nullptr, kev1 = nullptr;     // kernel_timing: the multi-step kernel's own start / end
    bool ev1_recorded = false;             // the closing event of the timed range already sits behind the last launch
    c3d::host::KernelRecord ran;           // the kernel the last op of the last range ran (c3d_step_kernel_name)
    // ---- cluster kernel state (c3d_cluster.hip): plan, run-length coded program on the device, op -> (run, offset), hand-off records, slot counters, give-up word
    bool cl_ok = false;
    c3d::ClusterPlan cl_plan{};
    void* d_crec = nullptr;
    size_t crec_bytes = 0;
    static constexpr unsigned kClaimSets = 4096;
    static constexpr unsigned kClaimWords = 16;   // per launch: [0..7] slot counters of the XCDs, [8] completion counter
    unsigned* d_claim = nullptr;           // [kClaimSets][kClaimWords]
    unsigned cl_seq = 0;
    c3d::StepRun* d_prog = nullptr;
    size_t prog_cap = 0;
    bool prog_dirty = true;
    std::vector<int> op_run, op_skip;
    std::vector<c3d::StepRun> prog_runs;
    unsigned *h_tmo = nullptr, *h_tmo_dev = nullptr;   // hipHostMalloc'ed, mapped; its device address
    int resident_skip = 0;                 // ranges left to run step by step before a multi-step launch is tried again
    int resident_backoff = 0;              // doubles with every abandoned launch, back to 0 after a good one
    // ---- scratch and staging
    void* h_stage = nullptr;               // pinned host staging of the read-backs (ensure_stage)
    size_t h_stage_bytes = 0;
    void* d_score = nullptr;               // c3d_score_replicas' device scratch (ranks, rounded coordinates, sums, histograms), grown on demand
    size_t d_score_bytes = 0;
    // ---- the stats (c3d_get_stat, c3d_last_timing)
    double last_ms = 0, last_kernel_ms = 0;
    long last_steps = 0, last_launches = 0;
    double last_host_launch_us = 0, last_host_sync_us = 0;   // host time inside the launch call / the synchronise call of the last c3d_run_steps (cluster launches)
    int last_path = 0;                     // 0 per-step, 2 k_cluster, 3 fp64 reference (what the last run_ops used)
    long graph_captures = 0, graph_launches = 0, step_launches = 0, resident_launches = 0, cluster_launches = 0;
    long spin_completions = 0, lbfgs_steps = 0;   // (L-BFGS steps run)
    int resident_fallbacks = 0;            // resident launches abandoned for the per-step path (see run_resident)
    int cluster_incomplete = 0, placement_mismatches = 0;   // cluster launches that ended without the completion mark (and were re-run step by step)
    long k1_recomputed = 0, k1_patched = 0;   // K1: near-tie elements redone on the host in the reference's order / changed by it
    int last_embed_form = 0, last_embed_batches = 0;   // "embed_form", "embed_batches": what the last c3d_embed_replicas ran
    long rank_prefetch_hits = 0, device_rank_runs = 0, score_wide_runs = 0;   // c3d_score_replicas: prefetched ranks taken / ranked on the device / the sized-histogram re-run
    long compare_runs = 0, f64_evals = 0;  // completed calls of c3d_compare_replicas / c3d_eval_f64
    long superpose_runs = 0, rmsd_table_runs = 0;   // completed calls of c3d_superpose_replicas / c3d_rmsd_table
    long ensemble_map_runs = 0, ensemble_score_runs = 0;   // completed calls of c3d_ensemble_map / c3d_ensemble_score
    long geometry_runs = 0, separation_runs = 0;   // completed calls of c3d_geometry_replicas / c3d_separation_profile
    long stratified_runs = 0, bead_runs = 0;       // completed calls of c3d_stratified_score / c3d_bead_scores
    double stratified_if_ms = 0, stratified_models_ms = 0;   // device time of the last completed call's two passes (HIP events)
    double bead_if_ms = 0, bead_models_ms = 0;     // device time of the last completed call's two passes (the first 0 where no IF was ranked)
};

// entries that launch kernels, copy or fill: they load what the context's configuration (and `extra`) can launch from
#define C3D_ENTRY(c, extra)                       \
    c3d::host::Entry entry__((c), (extra), true); \
    if (entry__.rc != C3D_OK) return entry__.rc
// entries that only allocate, free, create, destroy or synchronise: they load nothing
#define C3D_GATE(c)                           \
    c3d::host::Entry entry__((c), 0u, false); \
    if (entry__.rc != C3D_OK) return entry__.rc
