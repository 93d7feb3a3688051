// c3d_api.cpp — C-ABI host of libc3d.so: context, device buffers, schedule -> launch program,
// hipGraph replay, resident launches, timing.  Compiled with hipcc (-x hip) for the HIP runtime API only;
// the kernels live in c3d_device.hip (per-step), c3d_cluster.hip (multi-step), c3d_embed.hip, c3d_score.hip.
//
// Reference boundary: chromosome3D.pl:254-289 (build_models: `cns_solve < dgsa.inp`) and the
// deck it writes (:882-1846).  What CNS does per model (deck :1574-1829) becomes a flat
// "program" of SA steps; a range of it runs as ONE cluster launch (run_cluster, c3d_cluster.hip) where the
// replicas fit the chip's XCDs, else as one launch per step (two replica groups on two streams, replayed
// from hipGraphs).  Every copy and memset is ordered on the context's own stream: contexts of different
// host threads never meet on the legacy stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/c3d.h"
#include "c3d_host.h"
#include "c3d_internal.h"

using c3d::fail;

namespace {

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess)                                                                 \
            return fail(C3D_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

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

// ---- Philox4x32-10 (Salmon et al. SC'11): initial coordinates / velocities ------------------
inline void philox4x32(const uint32_t ctr_in[4], const uint32_t key_in[2], uint32_t out[4]) {
    uint32_t c[4] = {ctr_in[0], ctr_in[1], ctr_in[2], ctr_in[3]};
    uint32_t k[2] = {key_in[0], key_in[1]};
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0];
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1];
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k[0] += 0x9E3779B9u;
        k[1] += 0xBB67AE85u;
    }
    memcpy(out, c, sizeof(c));
}
inline double u01(uint32_t u) { return ((double)u + 0.5) * (1.0 / 4294967296.0); }
void normals4(uint64_t seed, uint32_t replica, uint32_t bead, uint32_t purpose, double g[4]) {
    const uint32_t ctr[4] = {bead, purpose, 0u, 0u};
    const uint32_t key[2] = {(uint32_t)(seed & 0xFFFFFFFFu) ^ (replica * 0x9E3779B9u), (uint32_t)(seed >> 32) + replica};
    uint32_t r[4];
    philox4x32(ctr, key, r);
    const double two_pi = 6.283185307179586476925286766559;
    double a = sqrt(-2.0 * log(u01(r[0]))), b = two_pi * u01(r[1]);
    g[0] = a * cos(b); g[1] = a * sin(b);
    a = sqrt(-2.0 * log(u01(r[2]))); b = two_pi * u01(r[3]);
    g[2] = a * cos(b); g[3] = a * sin(b);
}

}  // namespace

struct c3d_ctx {
    int device = 0;
    hipStream_t stream = nullptr;          // group 0 / everything that is not a step launch
    static constexpr int kMaxGroups = 4;
    int ngroups = 2;                       // replica groups stepped on separate streams (overlap latency phases)
    hipStream_t gstream[kMaxGroups] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t gev[kMaxGroups] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t kev0 = nullptr, kev1 = nullptr;     // kernel_timing: the multi-step kernel's own start / end
    int kernel_timing = 0;
    double last_kernel_ms = 0;
    double last_host_launch_us = 0, last_host_sync_us = 0;   // host time inside the launch call / the synchronise call of the last c3d_run_steps (cluster launches)
    int event_timing = 1;                          // 0: no event pair around c3d_run_steps / c3d_run (c3d_last_timing then reports 0 ms)
    bool ev1_recorded = false;                     // the closing event of the timed range already sits behind the last launch

    int n = 0, npad = 0, ntiles = 0, nrep = 0, R = 0;
    c3d_model model;
    std::vector<c3d_stage> stages;
    c3d_fire_params fire;
    float gtol = 0.0f;
    int check_every = 250;
    bool narrow_columns = true;            // option "narrow_columns" 0: every block 4 columns per lane (round 2's layout; measurements)
    bool zero_weight = false;              // some stage has w_all = 0: ITS steps take the general kernels (run_ops splits the range there)
    bool use_graph = true;
    int rpw = 2;
    int stage_dma = 1;
    int graph_chunk = 256;
    int precision = 32;                    // 64: the fp64 reference step (c3d_f64.hip) instead of the fp32 kernels
    c3d::Buffers64 b64;                    // fp64 state (c3d_f64.hip), double buffered by step parity like the fp32 buffers
    int sym = 0;                           // symmetric-tile step kernels (c3d_sym.hip): 1 on, 0 off (measured slower: DESIGN 7)
    float* d_sym_scratch = nullptr;
    int2* d_sym_tiles = nullptr;
    int start_mode = 0;                    // initial structure: 0 random coil, 1 extended strand (reference :2413-2416)
    int resident = -1;                     // multi-step cluster kernel (c3d_cluster.hip): 1 forced, 0 off, -1 where it applies
    int resident_min_ops = 4;              // shorter ranges go step by step
    double spin_wait_us = 400.0;           // a cluster launch is waited for on its completion mark for this long before hipStreamSynchronize (0: never)
    long spin_completions = 0;

    std::vector<int32_t> h_dist10;   // n*n, from K1 (empty when restraints came from a tbl)
    c3d::DevBuffers buf{};
    int eval_rpw = 4;                      // option "eval_rows_per_wave": 4 = scalar pair term in the forces hook, 2 = the packed one, -2 = scalar at two rows per wave
    bool pair_targets = true;              // option "pair_targets": the per-step kernel's resident row-pair constants (measurement knob)
    bool wide_tiles = true;                // option "wide_tiles": beyond the multi-step kernel's reach, 16 rows a workgroup and 4 a wave (measurement knob)
    int max_beads = 5120;                  // option "max_beads": the largest matrix c3d_set_if_matrix / c3d_set_restraints accept (5120..16384)
    int embed_max_beads = C3D_EMBED_MAX_BEADS_DEFAULT;   // option "embed_max_beads": the largest n c3d_embed_replicas accepts (4549..16384)
    int embed_form = 0;                    // option "embed_form": 0 = k_dg_eig while it fits, the tiled eigen stage beyond; 1 = tiled at every n
    int embed_batch = 0;                   // option "embed_batch": 0 = replicas per batch from C3D_EMBED_SCRATCH_BYTES, else that many
    int last_embed_form = 0, last_embed_batches = 0;   // stats "embed_form", "embed_batches": what the last c3d_embed_replicas ran
    int f64_max_beads = C3D_F64_MAX_BEADS_DEFAULT;   // option "f64_max_beads": the largest n a precision-64 context initialises (2560..16384)
    int f64_column_chunk = 0;              // option "f64_column_chunk": 0 = by size, else k64_step_chunked's CHUNK wherever n > chunk (c3d::column_chunk64_for)
    std::vector<int32_t> r_i, r_j, r_t10;  // c3d_set_restraints' list (0-based, i < j, one entry a pair): what a precision-64 context builds its tenths from
    int column_chunk = 0;                  // option "column_chunk": 0 = the library's choice, else the chunked form's CHUNK (c3d::column_chunk_for)
    float* d_feval = nullptr;
    size_t rep_floats = 0;           // 3*npad per replica
    bool have_targets = false, have_replicas = false;

    std::vector<Op> program;
    size_t pc = 0;
    int parity = 0;
    long steps_done = 0;
    std::map<std::tuple<long, int, int, int>, hipGraphExec_t> graphs;

    bool inject_timeout = false;           // test hook: pretend the next resident launch timed out
    int resident_fallbacks = 0;            // resident launches abandoned for the per-step path (see run_resident)
    int resident_skip = 0;                 // ranges left to run step by step before a multi-step launch is tried again
    int resident_backoff = 0;              // doubles with every abandoned launch, back to 0 after a good one
    int num_cus = 0, num_xcc = 0;
    int cluster_late = -1;                 // measurement knob: 0 = the tile sums always travel with the rows; -1 = planner's choice
    int cluster_geom = 0;                  // measurement knob: 100 CW + 10 RPW + helpers forces that cluster geometry (0 = planner's choice)
    int xcd_base = 0, xcd_count = 8;       // the XCDs a multi-step launch of this context lives on (options cluster_xcd_base / cluster_xcd_count)
    bool inject_misplaced = false;         // test hook: workgroup 0 of the next cluster launch reports a wrong XCD
    bool static_place = true;              // cluster launches number the workgroups of an XCD as blockIdx / 8 (verified in the kernel)
    int placement_mismatches = 0;
    bool inject_incomplete = false;        // test hook: the next cluster launch expects one workgroup more than will ever report
    int cluster_incomplete = 0;            // cluster launches that ended without the completion mark (and were re-run step by step)

    // cluster kernel state (c3d_cluster.hip): the run-length coded program on the device, op -> (run, offset),
    // hand-off records, per-launch slot counters, the host-mapped word a workgroup that gives up writes
    int cluster = -1;                      // 1 / -1: use it where it applies, 0: never
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
    unsigned* h_tmo = nullptr;             // hipHostMalloc'ed, mapped
    void* h_stage = nullptr;               // pinned host staging of the read-backs (ensure_stage)
    void* d_score = nullptr;               // c3d_score_replicas' device scratch (ranks, rounded coordinates, sums, histograms), grown on demand
    size_t d_score_bytes = 0;
    size_t h_stage_bytes = 0;
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
    int bb_steps = 1000;                   // option final_minimiser_steps: two-point steps before FIRE takes the stage over
    bool final_bb = true;                  // option final_minimiser: 1 = stages of kind 5 start with the two-point step-size minimiser, 0 = they are FIRE stages
    int prefetch_ranks = 1;                // option prefetch_ranks: 0 = no helper thread (measurement knob)
    unsigned* h_tmo_dev = nullptr;         // its device address

    long rank_prefetch_hits = 0;
    int device_ranks = 0;                  // option device_ranks: who ranks the IF matrix for c3d_score_replicas (c3d.h)
    long device_rank_runs = 0, score_wide_runs = 0;   // stats: calls that ranked on the device / that took the sized-histogram re-run
    long compare_runs = 0;                 // stat: completed calls of c3d_compare_replicas
    long f64_evals = 0;                    // stat: completed calls of c3d_eval_f64
    long superpose_runs = 0, rmsd_table_runs = 0;   // stats: completed calls of c3d_superpose_replicas / c3d_rmsd_table
    long k1_recomputed = 0, k1_patched = 0;   // K1: near-tie elements redone on the host in the reference's order / changed by it
    long graph_captures = 0, graph_launches = 0, step_launches = 0, resident_launches = 0, cluster_launches = 0;
    bool has_two_point = false;            // the program holds two-point minimiser steps (run_ops splits ranges at their borders)
    bool has_lbfgs = false;                // the program holds L-BFGS steps (kinds 8 / 9: run_ops splits ranges at their borders, per-step path only)
    int lbfgs_mem = 5;                     // option lbfgs_memory: pairs an L-BFGS stage keeps (1..8), fixed at the stage's first step
    c3d::LbfgsBuffers lb{};                // the L-BFGS history, tile sums and state (ensure_lbfgs), freed with the replica buffers
    bool f64_lbfgs = false;                // option "f64_lbfgs": the caller's consent to kind-8 stages on a precision-64 context (k64_lbfgs_eval + k64_lbfgs_move)
    c3d::LbfgsBuffers64 lb64{};            // their history, tile sums and state in doubles (ensure_lbfgs64), freed with the replica buffers
    long lbfgs_steps = 0;                  // L-BFGS steps run (stat "lbfgs_steps")
    int lbfgs_parity = -1;                 // parity the last L-BFGS step left its state in (stat "lbfgs_resets")
    int last_path = 0;                     // 0 per-step, 2 k_cluster, 3 fp64 reference (what the last run_ops used)
    KernelRecord ran;                      // the kernel the last op of the last range ran (c3d_step_kernel_name)

    double last_ms = 0;
    long last_steps = 0, last_launches = 0;
    uint64_t seed = 82364;
    uint32_t first_rep = 0;
};

namespace {

// hipFree of a context's buffer; a failure (only possible after a device fault) is kept in the error string, the
// pointer is dropped either way
template <class T>
void dev_free(T*& p) {
    if (!p) return;
    const hipError_t e = hipFree(p);
    if (e != hipSuccess) (void)fail(C3D_ERR_HIP, std::string("hipFree: ") + hipGetErrorString(e));
    p = nullptr;
}

void free_replica_buffers(c3d_ctx* c) {
    for (int k = 0; k < 2; ++k) {
        dev_free(c->buf.X[k]); dev_free(c->buf.V[k]); dev_free(c->buf.P[k]); dev_free(c->buf.S[k]);
    }
    dev_free(c->d_crec);
    c->crec_bytes = 0; c->cl_ok = false;
    dev_free(c->buf.Vinit); dev_free(c->buf.E); dev_free(c->d_feval);
    dev_free(c->d_sym_scratch); dev_free(c->d_sym_tiles);
    dev_free(c->lb.hist); dev_free(c->lb.part); dev_free(c->lb.S[0]); dev_free(c->lb.S[1]);
    dev_free(c->lb64.hist); dev_free(c->lb64.part); dev_free(c->lb64.S[0]); dev_free(c->lb64.S[1]);
    c->lbfgs_parity = -1;
    dev_free(c->b64.T); dev_free(c->b64.t10); dev_free(c->b64.Vinit); dev_free(c->b64.F);
    for (int k = 0; k < 2; ++k) { dev_free(c->b64.X[k]); dev_free(c->b64.V[k]); dev_free(c->b64.P[k]); dev_free(c->b64.S[k]); }
    c->have_replicas = false;
}
void drop_graphs(c3d_ctx* c) {
    for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second);
    c->graphs.clear();
}
// Everything else a context holds, once its streams have drained: graphs, replica state, targets, the program, claim sets, staging, score
// scratch, events, streams.  c3d_destroy's alone; the caller holds the gate.
void release_context(c3d_ctx* c) {
    for (hipStream_t s : c->gstream) if (s) (void)hipStreamSynchronize(s);
    drop_graphs(c);
    free_replica_buffers(c);
    dev_free(c->buf.tgt); dev_free(c->buf.tgs2);
    dev_free(c->d_prog); dev_free(c->d_claim); dev_free(c->d_score);
    if (c->h_tmo) (void)hipHostFree(c->h_tmo);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (hipEvent_t e : {c->ev0, c->ev1, c->kev0, c->kev1, c->fork_ev}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->gev) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : c->gstream) if (s && s != c->stream) (void)hipStreamDestroy(s);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

c3d::DevModel dev_model(const c3d_ctx* c) {
    c3d::DevModel m{};
    const c3d_model& h = c->model;
    m.n = c->n; m.npad = c->npad; m.ntiles = c->ntiles; m.nrep = c->nrep;
    m.rep_base = 0; m.nrep_g = c->nrep;
    m.rpw = c->rpw;
    m.stage_dma = c->stage_dma;
    m.noe_pot = h.noe_pot; m.ang_mode = h.ang_mode; m.rep_sep = h.rep_sep;
    m.mexp = h.msoexp == 2 ? 2 : 1;
    m.rs = h.rswitch;
    m.tail_c = h.asym * h.rswitch;
    m.tail_b = (m.tail_c - 2.0f * h.rswitch) * h.rswitch * h.rswitch;
    m.mrs = h.mrswitch; m.nmrs = -h.mrswitch;
    m.inv_rs = 1.0f / h.rswitch; m.nm_rs = -h.mrswitch / h.rswitch;
    // the shipped lower side (square up to mrswitch, then soft with exponent 2 and no asymptote) has a fast form of its own in
    // the clamp-form kernels: device potential 4 (pair_term); it needs the upper tail in clamp form too (slope 2 rswitch)
    if (h.noe_pot == 3 && h.msoexp == 2 && h.masym == 0.0f && m.tail_b == 0.0f && m.tail_c == 2.0f * m.rs) {
        m.noe_pot = 4;
        // its pair term works on (d - t) / MRS (pair_term): the per-pair constants are t / mrs and 1 / mrs, the third run constant is
        // the upper bound rs / mrs, and the factor applied once per row is W mrs (dev_step: clamp_scale)
        m.inv_rs = 1.0f / h.mrswitch; m.nm_rs = h.rswitch / h.mrswitch;
    }
    // column layout of the pair loop (c3d_internal.h): lanes of the last 256-column block own wl consecutive columns, up to 8
    // columns behind it are left over; both follow from n alone, so every launch form sums the same terms in the same order
    {
        const int cols_last = c->n - (c->npad - 256);
        int wl = cols_last / 64, nleft = cols_last - 64 * wl;
        if (wl == 0 || nleft > 8) { wl = std::min(4, wl + 1); nleft = 0; }
        // beyond the cluster kernel's reach (npad > 1024: the per-step kernel streams the targets) one column slot in 40 is not worth
        // the narrow block's scalar loads and the left-over pass: 28.0 against 27.0 us per step at N = 2500
        if (!c->narrow_columns || c->npad > 1024) { wl = 4; nleft = 0; }
        m.wl = wl; m.nleft = nleft; m.jl0 = c->npad - 256 + 64 * wl;
    }
    m.mtail_c = h.masym;
    // lower side beyond mrswitch: dE/dD = mtail_c - mtail_b / D^(mexp + 1), continuous with 2 D at D = mrswitch
    m.mtail_b = (m.mtail_c - 2.0f * h.mrswitch) * h.mrswitch * h.mrswitch * (m.mexp == 2 ? h.mrswitch : 1.0f);
    m.k_bond2 = 2.0f * h.k_bond; m.b0 = h.b0;
    m.k_ang2 = 2.0f * h.k_ang; m.a0 = h.a0;
    m.acc = c3d::kAccel / h.mass;
    const int ndf = std::max(3 * c->n - 3, 1);
    m.t_fac = h.mass / c3d::kAccel / ((float)ndf * c3d::kBoltz);
    m.fbeta = h.fbeta;
    m.inv_n = 1.0f / (float)c->n;
    return m;
}
c3d::DevFire dev_fire(const c3d_ctx* c) {
    c3d::DevFire f;
    f.dt_start = c->fire.dt_start; f.dt_max = c->fire.dt_max; f.f_inc = c->fire.f_inc; f.f_dec = c->fire.f_dec;
    f.alpha_start = c->fire.alpha_start; f.f_alpha = c->fire.f_alpha; f.max_step = c->fire.max_step;
    f.n_min = c->fire.n_min;
    return f;
}
// the length the clamp form divides (d - t) by: rswitch, or mrswitch for device potential 4 (1 / DevModel::inv_rs in either case)
float clamp_scale(const c3d_ctx* c) { return dev_model(c).noe_pot == 4 ? c->model.mrswitch : c->model.rswitch; }
c3d::DevStep dev_step(const c3d_ctx* c, int kind, float dt, float w_all, float w_vdw, float repel_s, float t_bath) {
    c3d::DevStep p;
    p.kind = kind; p.dt = dt; p.w_all = w_all;
    p.w_noe2n = -2.0f * w_all * c->model.s_noe;
    p.w_rep4 = 4.0f * w_vdw * c->model.k_rep;
    const float rr = repel_s * c->model.r0_rep;
    p.rep_r2 = rr * rr;
    p.inv_rep_r2 = rr > 0.0f ? 1.0f / p.rep_r2 : 0.0f;
    p.w_rep4r2 = p.w_rep4 * p.rep_r2;
    // clamp form (c3d_step_core.h pair_term): the NOE weight times rswitch is applied once per row, the repel weight rides
    // relative to it.  A stage without restraint weight (w_all = 0) cannot be written that way: general kernels (zero_weight).
    p.w_rs = p.w_noe2n * clamp_scale(c);
    p.kq = p.w_rs != 0.0f ? p.w_rep4r2 / p.w_rs : 0.0f;
    p.t_bath = t_bath;
    return p;
}

bool is_two_point(int kind) { return kind == 5 || kind == 6; }
bool is_lbfgs(int kind) { return kind == 8 || kind == 9; }

void build_program(c3d_ctx* c) {
    c->program.clear();
    int prev_kind = -1;
    for (size_t s = 0; s < c->stages.size(); ++s) {
        const c3d_stage& st = c->stages[s];
        if (st.kind == 2 || st.kind == 5 || st.kind == 8) {
            // kind 3 / 6 = first step of a minimiser's run (fresh state).  A stage of kind 5 starts with the two-point step-size minimiser
            // (kinds 6 / 5) and hands over to FIRE (3 / 2) after bb_steps of them if the exit test has not ended the stage by then: the
            // two-point method has no descent guarantee — one replica in a few hundred ends in a cycle of long moves instead of a minimum —
            // and FIRE finishes what it leaves (the CPU restatement does the same: c3o_run_schedule).  Option final_minimiser = 0: kind 5 runs as FIRE throughout.
            // A stage of kind 8 runs L-BFGS (kinds 9 / 8) for its first final_minimiser_steps steps and hands over to FIRE the same way;
            // option final_minimiser does not apply to it.
            const bool lbfgs = st.kind == 8;
            const int nbb = (st.kind == 5 && c->final_bb) || lbfgs ? std::min(st.nsteps, c->bb_steps) : 0;
            for (int k = 0; k < st.nsteps; ++k) {
                const int kind = k < nbb ? (k == 0 ? (lbfgs ? 9 : 6) : (lbfgs ? 8 : 5)) : (k == nbb ? 3 : 2);
                c->program.push_back({dev_step(c, kind, 0.0f, st.w_all, st.w_vdw, st.repel_s, 0.0f), (int)s, true});
            }
        } else {
            if (prev_kind == 2 || prev_kind == 5 || prev_kind == 8 || prev_kind == -1)
                c->program.push_back({dev_step(c, 4, 0.0f, st.w_all, st.w_vdw, st.repel_s, st.t_bath), (int)s, false});
            for (int k = 0; k < st.nsteps; ++k)
                c->program.push_back({dev_step(c, st.kind, st.dt, st.w_all, st.w_vdw, st.repel_s, st.t_bath), (int)s, true});
        }
        prev_kind = st.kind;
    }
    c->pc = 0;
    c->zero_weight = false;
    for (const Op& op : c->program) c->zero_weight = c->zero_weight || op.p.w_rs == 0.0f;
    c->has_two_point = false;
    for (const Op& op : c->program) c->has_two_point = c->has_two_point || is_two_point(op.p.kind);
    c->has_lbfgs = false;
    for (const Op& op : c->program) c->has_lbfgs = c->has_lbfgs || is_lbfgs(op.p.kind);
    drop_graphs(c);
    // run-length code of the whole program (a FIRE stage is 2 runs, the cool ramp 81) for the cluster kernel
    c->prog_runs.clear();
    c->op_run.assign(c->program.size(), 0);
    c->op_skip.assign(c->program.size(), 0);
    for (size_t k = 0; k < c->program.size(); ++k) {
        const c3d::DevStep& p = c->program[k].p;
        if (!c->prog_runs.empty() && memcmp(&c->prog_runs.back().p, &p, sizeof(p)) == 0) ++c->prog_runs.back().count;
        else c->prog_runs.push_back({p, 1});
        c->op_run[k] = (int)c->prog_runs.size() - 1;
        c->op_skip[k] = c->prog_runs.back().count - 1;
    }
    c->prog_dirty = true;
}

// What a change of configuration (c3d_set_model / c3d_set_schedule / c3d_set_option) makes stale
enum Stale : unsigned { STALE_REPLICAS = 1, STALE_GRAPHS = 2, STALE_PAIR_TARGETS = 4, STALE_PROGRAM = 8 };
// the caller holds the gate when this releases anything device-side (drop_stale_gated)
void drop_stale(c3d_ctx* c, unsigned stale) {
    if (stale & STALE_REPLICAS) free_replica_buffers(c);
    if (stale & STALE_PAIR_TARGETS) dev_free(c->buf.tgs2);
    if (stale & STALE_PROGRAM) build_program(c);       // drops the graphs
    else if (stale & STALE_GRAPHS) drop_graphs(c);
}

int upload_targets(c3d_ctx* c, const std::vector<float>& enc) {
    dev_free(c->buf.tgt); dev_free(c->buf.tgs2);
    HIP_TRY(hipMalloc(&c->buf.tgt, sizeof(float) * enc.size()));
    HIP_TRY(hipMemcpyAsync(c->buf.tgt, enc.data(), sizeof(float) * enc.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

void set_dims(c3d_ctx* c, int n) {
    c->n = n;
    c->npad = (n + 255) / 256 * 256;   // one column block of the pair kernel = 256 columns
    c->ntiles = (n + c3d::kTileRows - 1) / c3d::kTileRows;
    c->rep_floats = (size_t)3 * c->npad;
}

// AoS host (nrep*n*3) -> SoA padded device layout
void pack(const c3d_ctx* c, const float* aos, std::vector<float>& soa, bool pad_far) {
    soa.assign(c->rep_floats * c->nrep, 0.0f);
    for (int r = 0; r < c->nrep; ++r) {
        float* base = soa.data() + c->rep_floats * r;
        for (int comp = 0; comp < 3; ++comp) {
            for (int i = 0; i < c->n; ++i) base[(size_t)comp * c->npad + i] = aos[((size_t)r * c->n + i) * 3 + comp];
            if (pad_far)
                for (int i = c->n; i < c->npad; ++i) base[(size_t)comp * c->npad + i] = c3d::kPadCoord * (float)(comp + 1) + 16.0f * (float)(i - c->n);
        }
    }
}
void unpack(const c3d_ctx* c, const float* soa, float* aos) {
    for (int r = 0; r < c->nrep; ++r) {
        const float* base = soa + c->rep_floats * r;
        for (int comp = 0; comp < 3; ++comp)
            for (int i = 0; i < c->n; ++i) aos[((size_t)r * c->n + i) * 3 + comp] = base[(size_t)comp * c->npad + i];
    }
}

void group_range(const c3d_ctx* c, int g, int& base, int& count) {
    const int G = std::min(c->ngroups, std::max(c->nrep, 1));
    const int q = c->nrep / G, r = c->nrep % G;
    base = g * q + std::min(g, r);
    count = q + (g < r ? 1 : 0);
}
int active_groups(const c3d_ctx* c) { return std::min(c->ngroups, std::max(c->nrep, 1)); }

// ---- code objects ---------------------------------------------------------------------------------------------------------------
// The HIP runtime loads a code object (one per translation unit with kernels: sixteen in this library) at the first use of one of its
// kernels.  Round 5 left that to the runtime and to helper threads, and eight contexts of one process starting together — c3d_batch
// --devices 4 --lanes 2 --map-devices-to 0 — ended in a DEVICE exception once (rc -13: the runtime's GPU-core-dump helper does not
// exist on the box, the process died on its pipe before the runtime could say which exception; DESIGN.md section 6 "code objects").
// That a load beside other HIP calls of the process caused it is a hypothesis: the record does not name the exception.  The rule that
// follows from it — no code object loads while any thread of the process is inside the HIP runtime for this library:
//   * a unit is loaded by ensure_units() alone — the calling thread, one unit at a time, g_units.rw held EXCLUSIVELY;
//   * every HIP call of a context runs inside a public entry that holds g_units.rw SHARED for its whole duration (struct Entry): kernels,
//     copies and fills (C3D_ENTRY, which first loads the units the context's configuration can launch from), and allocation, release,
//     stream / event / graph creation and destruction, synchronisation (C3D_GATE, which loads nothing).  The only calls outside are the
//     device queries of c3d_create and c3d_device_count (hipGetDeviceCount, hipGetDeviceProperties, hipDeviceGetAttribute) and
//     hipSetDevice, which precede the gate;
//   * c3d_create loads what a default job runs (per-step + K1 unit, both multi-step units of the shipped potential, scoring) before it
//     makes its first stream — +13 ms once per process and device, +24 ms for all sixteen: profiles/r06_create_with_code_objects.txt
//     (c3d_set_process_option "preload": 2 = all sixteen, 0 = each at the first entry that needs it); the multi-step and embedding units
//     also get their dynamic-LDS allowance there (hipFuncSetAttribute per instantiation: state of the runtime, so it belongs under the
//     same lock), and a launch changes no runtime state afterwards;
//   * a load that fails is reported (C3D_ERR_HIP) and not remembered as done.
// No helper thread of the library touches the HIP runtime (the IF-rank worker is host arithmetic only).  tools/sanitize/hip_stub.cpp
// checks the rule on the CPU: every HIP function it fakes but those queries counts as device work, and a load beside any of them fails.
enum Unit : unsigned {
    UNIT_DEVICE = 0, UNIT_SCORE, UNIT_CLUSTER_BASE, UNIT_EMBED, UNIT_F64, UNIT_SYM,
    UNIT_CLUSTER_P0, UNIT_CLUSTER_TP0 = UNIT_CLUSTER_P0 + 5, UNIT_COUNT = UNIT_CLUSTER_TP0 + 5
};
constexpr unsigned unit_bit(unsigned u) { return 1u << u; }
constexpr unsigned kUnitsDefault = unit_bit(UNIT_DEVICE) | unit_bit(UNIT_SCORE) | unit_bit(UNIT_CLUSTER_P0 + 4) | unit_bit(UNIT_CLUSTER_TP0 + 4);
constexpr unsigned kUnitsAll = (1u << UNIT_COUNT) - 1u;
constexpr int kMaxDevices = 64;
// launches share it, loads own it; a waiting load goes first (std::shared_mutex on glibc prefers readers: with three lanes of a device
// overlapping their entries, the first c3d_create of the NEXT device could wait for a gap that never comes)
class LaunchGate {
    std::mutex mu;
    std::condition_variable cv;
    int launching = 0, loads_waiting = 0;
    bool loading = false;
public:
    void lock_shared() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !loading && loads_waiting == 0; });
        ++launching;
    }
    void unlock_shared() {
        std::lock_guard<std::mutex> lk(mu);
        if (--launching == 0) cv.notify_all();
    }
    void lock() {
        std::unique_lock<std::mutex> lk(mu);
        ++loads_waiting;
        cv.wait(lk, [&] { return !loading && launching == 0; });
        --loads_waiting;
        loading = true;
    }
    void unlock() {
        std::lock_guard<std::mutex> lk(mu);
        loading = false;
        cv.notify_all();
    }
};
struct Units {
    LaunchGate rw;
    std::atomic<unsigned> loaded[kMaxDevices];     // bit u: unit u is loaded (and prepared) on that device
    std::atomic<long> loads{0};                    // units loaded by this process (stat "units_loaded": a test reads it)
    Units() { for (auto& a : loaded) a.store(0); }
};
Units g_units;
thread_local int t_entry_depth = 0;                // public entries call one another (c3d_rank -> c3d_get_energies -> c3d_eval): the outermost one locks

const char* unit_name(unsigned u) {
    static const char* const names[] = {"per-step + K1", "scoring", "multi-step planner", "embedding", "fp64", "symmetric tiles"};
    if (u < UNIT_CLUSTER_P0) return names[u];
    return u < UNIT_CLUSTER_TP0 ? "multi-step (k_cluster)" : "multi-step (k_cluster_tp)";
}
hipError_t load_one_unit(unsigned u) {
    switch (u) {
        case UNIT_DEVICE: return c3d::preload_device_unit();
        case UNIT_SCORE: return c3d::preload_score_unit();
        case UNIT_CLUSTER_BASE: return c3d::preload_cluster_base_unit();
        case UNIT_EMBED: return c3d::preload_embed_unit();
        case UNIT_F64: return c3d::preload_f64_unit();
        case UNIT_SYM: return c3d::preload_sym_unit();
        default: break;
    }
    if (u >= UNIT_CLUSTER_TP0 && u < UNIT_COUNT) return c3d::preload_cluster_unit((int)(u - UNIT_CLUSTER_TP0), true);
    if (u >= UNIT_CLUSTER_P0 && u < UNIT_CLUSTER_TP0) return c3d::preload_cluster_unit((int)(u - UNIT_CLUSTER_P0), false);
    return hipErrorInvalidValue;
}
// Loads the units of `mask` that `device` does not hold yet.  Must be called WITHOUT g_units.rw held by this thread (Entry does so
// before it takes the shared side; a nested entry finds its units loaded by the outermost one or reports the programming error).
int ensure_units(int device, unsigned mask) {
    if (device < 0 || device >= kMaxDevices) return fail(C3D_ERR_INVALID, "device index beyond the 64 this build keeps code-object state for");
    mask &= kUnitsAll;
    if ((g_units.loaded[device].load(std::memory_order_acquire) & mask) == mask) return C3D_OK;
    if (t_entry_depth > 0) return fail(C3D_ERR_HIP, "internal: a code object is wanted inside an entry that did not name it");
    std::lock_guard<LaunchGate> lk(g_units.rw);
    HIP_TRY(hipSetDevice(device));
    for (unsigned u = 0; u < UNIT_COUNT; ++u) {
        if (!(mask & unit_bit(u)) || (g_units.loaded[device].load(std::memory_order_relaxed) & unit_bit(u))) continue;
        const hipError_t e = load_one_unit(u);
        if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("loading the code object of the ") + unit_name(u) + " kernels: " + hipGetErrorString(e));
        g_units.loaded[device].fetch_or(unit_bit(u), std::memory_order_release);
        g_units.loads.fetch_add(1);
    }
    return C3D_OK;
}
// the units the context's current configuration can launch from (the configuration changes through public entries only)
unsigned units_wanted(const c3d_ctx* c) {
    unsigned m = unit_bit(UNIT_DEVICE) | unit_bit(UNIT_SCORE);
    const int pot = std::min(std::max(dev_model(c).noe_pot, 0), 4);
    if (c->cluster != 0 && c->resident != 0 && c->precision != 64)          // fp64 never takes the multi-step path (run_ops_segment)
        m |= unit_bit(UNIT_CLUSTER_P0 + (unsigned)pot) | unit_bit(UNIT_CLUSTER_TP0 + (unsigned)pot);
    if (c->precision == 64) m |= unit_bit(UNIT_F64);
    if (c->sym > 0) m |= unit_bit(UNIT_SYM);
    return m;
}
// A public entry: current device, units present (launching entries only), shared side of the gate — in that order.  Every HIP call of a
// context runs inside one; only the device queries of c3d_create (count, properties, attributes) come before it.
struct Entry {
    int rc = C3D_OK;
    bool locked = false;
    Entry(const c3d_ctx* c, unsigned extra, bool launches) {
        if (hipSetDevice(c->device) != hipSuccess) { rc = fail(C3D_ERR_HIP, "hipSetDevice failed"); return; }
        if (launches) rc = ensure_units(c->device, units_wanted(c) | extra);
        if (rc != C3D_OK) return;
        if (t_entry_depth++ == 0) { g_units.rw.lock_shared(); locked = true; }
    }
    ~Entry() {
        if (rc != C3D_OK) return;
        --t_entry_depth;
        if (locked) g_units.rw.unlock_shared();
    }
    Entry(const Entry&) = delete;
    Entry& operator=(const Entry&) = delete;
};
// entries that launch kernels, copy or fill: they load what the context's configuration (and `extra`) can launch from
#define C3D_ENTRY(c, extra)                 \
    Entry entry__((c), (extra), true);      \
    if (entry__.rc != C3D_OK) return entry__.rc
// entries that only allocate, free, create, destroy or synchronise: they load nothing
#define C3D_GATE(c)                         \
    Entry entry__((c), 0u, false);          \
    if (entry__.rc != C3D_OK) return entry__.rc

// c3d_set_schedule / c3d_set_option: drops what a change made stale, inside the gate when that releases anything device-side (the replica
// state is allocated from X[0] and t10 on: c3d_init_replicas)
int drop_stale_gated(c3d_ctx* c, unsigned stale) {
    const bool device_side = ((stale & STALE_REPLICAS) && (c->buf.X[0] || c->b64.t10)) || ((stale & STALE_PAIR_TARGETS) && c->buf.tgs2) ||
                             ((stale & (STALE_GRAPHS | STALE_PROGRAM)) && !c->graphs.empty());
    if (!device_side) { drop_stale(c, stale); return C3D_OK; }
    C3D_GATE(c);
    drop_stale(c, stale);
    return C3D_OK;
}

// The symmetric-tile kernels evaluate the clamp form only (k_pairs_sym reads rs and mrs, not the tails): decided per op from the model in
// force, which c3d_set_model may change on a live context; a general tail runs k_step's general form.  The tile list and slabs exist
// whenever `symmetric` is on (c3d_init_replicas).
bool use_sym(const c3d_ctx* c) {
    return c->sym > 0 && c->d_sym_scratch && !c3d::general_tail(dev_model(c));
}

void model_host64(const c3d_ctx* c, double (&mh)[15]) {
    const c3d_model& h = c->model;
    const double v[15] = {h.s_noe, h.rswitch, h.asym, h.masym, h.mrswitch, h.k_bond, h.b0, h.k_ang, h.a0, h.r0_rep, h.k_rep, h.mass, h.fbeta,
                          (double)h.min_sep, (double)h.msoexp};
    for (int k = 0; k < 15; ++k) mh[k] = v[k];
}
// fp64 target matrix from the resident integer tenths, in the encoding the current model's kernel expects (c3d_f64.hip pair64)
int build_targets64(c3d_ctx* c) {
    double mh[15];
    model_host64(c, mh);
    hipError_t e = c3d::launch_targets64(dev_model(c), mh, c->model.min_sep, c->b64.t10, c->b64.T, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 targets: ") + hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

// Per-step kernel beyond the cluster kernel's reach (no narrow column block: every n > 1024), device potential 4: the resident per-pair
// constants of row pairs (DevModel::tgs2), built on first use after the targets or the model changed

// The L-BFGS history (2 x 8 pairs x 3 x npad floats a replica: sized for the largest memory, so that lbfgs_memory never reallocates), the
// tile sums and the state, zeroed; allocated outside any stream capture (run_ops_segment), freed with the replica buffers
int ensure_lbfgs(c3d_ctx* c) {
    if (c->lb.hist) return C3D_OK;
    const size_t hist = c3d::lbfgs_hist_floats(c->npad) * c->nrep, part = (size_t)c->nrep * c->ntiles * c3d::kLbfgsQ;
    HIP_TRY(hipMalloc(&c->lb.hist, sizeof(float) * hist));
    HIP_TRY(hipMalloc(&c->lb.part, sizeof(float) * part));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMalloc(&c->lb.S[k], sizeof(c3d::LbfgsState) * c->nrep));
    HIP_TRY(hipMemsetAsync(c->lb.hist, 0, sizeof(float) * hist, c->stream));
    HIP_TRY(hipMemsetAsync(c->lb.part, 0, sizeof(float) * part, c->stream));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(c->lb.S[k], 0, sizeof(c3d::LbfgsState) * c->nrep, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // the step launches run on the group streams
    return C3D_OK;
}

// The same for a precision-64 context: doubles, np columns (6.3 MB a replica at 16384 beads)
int ensure_lbfgs64(c3d_ctx* c) {
    if (c->lb64.hist) return C3D_OK;
    const size_t hist = c3d::lbfgs_hist_floats(c3d::cols64(c->n)) * c->nrep, part = (size_t)c->nrep * c->ntiles * c3d::kLbfgsQ;
    HIP_TRY(hipMalloc(&c->lb64.hist, sizeof(double) * hist));
    HIP_TRY(hipMalloc(&c->lb64.part, sizeof(double) * part));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMalloc(&c->lb64.S[k], sizeof(c3d::LbfgsState) * c->nrep));
    HIP_TRY(hipMemsetAsync(c->lb64.hist, 0, sizeof(double) * hist, c->stream));
    HIP_TRY(hipMemsetAsync(c->lb64.part, 0, sizeof(double) * part, c->stream));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(c->lb64.S[k], 0, sizeof(c3d::LbfgsState) * c->nrep, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // the step launches run on the group streams
    return C3D_OK;
}

int ensure_pair_targets(c3d_ctx* c, const c3d::DevModel& m) {
    if (c->buf.tgs2 || !c->pair_targets || !c3d::pair_targets_fit(m) || c->npad <= 1024 || !c->buf.tgt) return C3D_OK;
    HIP_TRY(hipMalloc(&c->buf.tgs2, sizeof(float) * c3d::pair_targets_floats(c->n, c->npad)));
    hipError_t e = c3d::launch_pair_targets(m, c->buf.tgt, c->buf.tgs2, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("pair targets: ") + hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(c->stream));          // the step launches run on the group streams
    return C3D_OK;
}
// The kernel an op runs on the per-step path and its form: launch_op launches what this says, run_ops_segment records it for the range's
// last op (a graph replay does not pass through launch_op)
KernelRecord op_kernel(const c3d_ctx* c, const c3d::DevModel& m, const Op& op) {
    KernelRecord k;
    if (c->precision == 64) {              // launch_step64 makes the same choice from the same doubles
        double mh[15];
        model_host64(c, mh);
        k.family = is_lbfgs(op.p.kind) ? KernelRecord::LBFGS_EVAL64 : KernelRecord::STEP64;
        k.f64 = c3d::form64(m.noe_pot, mh, c->stages[op.stage].w_all, c->n, c->f64_column_chunk);
    } else if (!is_lbfgs(op.p.kind) && use_sym(c)) {      // (symmetric tiles do not apply to L-BFGS steps)
        k.family = KernelRecord::PAIRS_SYM;
        k.pot = c3d::device_pot(m.noe_pot);
        k.rs1 = c3d::sym_rs1(m);
    } else {
        k.family = is_lbfgs(op.p.kind) ? KernelRecord::LBFGS_EVAL : KernelRecord::STEP;
        k.step = c3d::step_form(m, op.p, c->wide_tiles, c->pair_targets, c->buf.tgs2 != nullptr, c->column_chunk);
    }
    return k;
}
// one SA-step launch for replica group g, reading parity `par`
int launch_op(c3d_ctx* c, const Op& op, int g, int par) {
    c3d::DevModel m = dev_model(c);
    group_range(c, g, m.rep_base, m.nrep_g);
    if (c->precision == 64) {              // the stage's own doubles, not the floats of DevStep
        const c3d_stage& st = c->stages[op.stage];
        double mh[15];
        model_host64(c, mh);
        const double fh[7] = {c->fire.dt_start, c->fire.dt_max, c->fire.f_inc, c->fire.f_dec, c->fire.alpha_start, c->fire.f_alpha, c->fire.max_step};
        const double sh[6] = {(double)op.p.kind, st.dt, st.w_all, st.w_vdw, st.repel_s, st.t_bath};
        if (is_lbfgs(op.p.kind)) {         // two launches, as in fp32: forces + tile sums, then sums + direction + move
            hipError_t e = c3d::launch_lbfgs_eval64(m, mh, sh, c->b64, c->lb64, par, c->lbfgs_mem, c->f64_column_chunk, c->gstream[g]);
            if (e == hipSuccess) e = c3d::launch_lbfgs_move64(m, mh, sh, fh, c->fire.n_min, c->b64, c->lb64, par, c->lbfgs_mem, c->gstream[g]);
            if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 L-BFGS step launch: ") + hipGetErrorString(e));
            return C3D_OK;
        }
        hipError_t e64 = c3d::launch_step64(m, mh, sh, fh, c->fire.n_min, c->b64, par, c->f64_column_chunk, c->gstream[g]);
        if (e64 != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 step launch: ") + hipGetErrorString(e64));
        return C3D_OK;
    }
    const KernelRecord k = op_kernel(c, m, op);
    if (k.family == KernelRecord::LBFGS_EVAL) {       // two launches: forces + tile sums, then sums + direction + move
        hipError_t e = c3d::launch_lbfgs_eval(m, op.p, c->buf, c->lb, par, c->lbfgs_mem, k.step, c->gstream[g]);
        if (e == hipSuccess) e = c3d::launch_lbfgs_move(m, op.p, dev_fire(c), c->buf, c->lb, par, c->lbfgs_mem, c->gstream[g]);
        if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("L-BFGS step launch: ") + hipGetErrorString(e));
        return C3D_OK;
    }
    hipError_t e = k.family == KernelRecord::PAIRS_SYM
                       ? c3d::launch_step_sym(m, op.p, dev_fire(c), c->buf, par, c->d_sym_tiles, c->d_sym_scratch, c->gstream[g])
                       : c3d::launch_step(m, op.p, dev_fire(c), c->buf, par, k.step, c->gstream[g]);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("step launch: ") + hipGetErrorString(e));
    return C3D_OK;
}

// The multi-step kernel's geometry for the context's beads, replicas, XCD set AND model (the device potential decides which column
// layouts and geometries exist: cluster_plan), and the record buffer it needs.  c3d_init_replicas plans when it allocates; c3d_set_model
// plans again when replicas exist (round 6: a model with another potential installed between two c3d_init_replicas calls of the same
// replica count used to keep the old potential's plan — "cluster launch: invalid argument" at the next c3d_run_steps).
int plan_cluster(c3d_ctx* c) {
    c3d::DevModel m = dev_model(c);
    m.nrep = c->nrep; m.nrep_g = c->nrep; m.rep_base = 0;
    c->cl_ok = false;                          // until the records fit: a failure below leaves the per-step path, not a stale plan
    if (!c3d::cluster_plan(m, c->num_cus, c->num_xcc, c->cluster_geom, c->cluster_late, c->xcd_count, &c->cl_plan)) return C3D_OK;
    c->cl_plan.device = c->device;
    const size_t bytes = c3d::cluster_record_bytes(m, c->cl_plan);
    if (!c->d_crec || bytes > c->crec_bytes) {
        if (c->d_crec) { HIP_TRY(hipStreamSynchronize(c->stream)); dev_free(c->d_crec); }
        c->crec_bytes = 0;
        HIP_TRY(hipMalloc(&c->d_crec, bytes));
        c->crec_bytes = bytes;
    }
    c->cl_seq = 0;                             // the next launch wipes the records and the slot counters
    c->cl_ok = true;
    return C3D_OK;
}

// Can the ops run as one k_cluster launch (a replica on a few 1024-thread workgroups of one XCD)?
bool cluster_ok(c3d_ctx* c) {
    if (!c->resident || !c->cluster || !c->cl_ok || !c->d_crec) return false;
    return !c3d::general_tail(dev_model(c));        // (ops without restraint weight never get here: run_ops splits the range at them)
}

// after a multi-step launch: did a workgroup give up (or was that injected)?  The launch reads parity p and writes
// parity p^1 only in its last step, so its inputs are intact whatever happened: if a workgroup gave up waiting (its
// replica's workgroups were not all resident, e.g. another process fills the GPU) the caller runs the same ops on
// the per-step path; the next `resident_backoff` ranges go there too before a multi-step launch is tried again.
bool launch_was_abandoned(c3d_ctx* c, unsigned done_mark) {
    // a workgroup found itself on another XCD than blockIdx % 8: from now on this context claims slots from per-XCD counters
    if (c->h_tmo[2]) { c->h_tmo[2] = 0; c->static_place = false; ++c->placement_mismatches; }
    // complete = the last of the launch's replicas x parts workgroups wrote the mark (c3d_cluster.hip); a launch that
    // neither timed out nor completed left some (replica, part) unclaimed: same treatment, counted separately
    const bool complete = c->h_tmo[1] == done_mark;
    if (!*c->h_tmo && complete) { c->resident_backoff = 0; return false; }
    if (!*c->h_tmo) ++c->cluster_incomplete;
    *c->h_tmo = 0;
    c->resident_backoff = std::min(4096, std::max(4, 2 * c->resident_backoff));
    c->resident_skip = c->resident_backoff;
    ++c->resident_fallbacks;
    return true;
}
void account_ops(c3d_ctx* c, size_t nops) {
    c->parity ^= 1;
    for (size_t k = 0; k < nops; ++k)
        if (c->program[c->pc + k].counted) { ++c->steps_done; ++c->last_steps; }
    c->last_launches += 1;
    c->pc += nops;
}


int run_cluster(c3d_ctx* c, size_t nops, bool* ran) {
    if (c->prog_dirty) {
        if (c->prog_runs.size() > c->prog_cap) {
            if (c->d_prog) { HIP_TRY(hipStreamSynchronize(c->stream)); dev_free(c->d_prog); }
            c->prog_cap = std::max<size_t>(c->prog_runs.size(), 256);
            HIP_TRY(hipMalloc(&c->d_prog, sizeof(c3d::StepRun) * c->prog_cap));
        }
        HIP_TRY(hipMemcpyAsync(c->d_prog, c->prog_runs.data(), sizeof(c3d::StepRun) * c->prog_runs.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->prog_dirty = false;
    }
    // tags of a launch carry its sequence number; records and slot counters are wiped when the number wraps
    const unsigned seq = c->cl_seq % c3d_ctx::kClaimSets;
    if (seq == 0) {
        HIP_TRY(hipMemsetAsync(c->d_crec, 0, c->crec_bytes, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_claim, 0, sizeof(unsigned) * c3d_ctx::kClaimWords * c3d_ctx::kClaimSets, c->stream));
    }
    ++c->cl_seq;
    if (c->inject_timeout) { *c->h_tmo = 1; c->inject_timeout = false; }
    c->h_tmo[1] = 0;
    const c3d::DevModel m = dev_model(c);
    c3d::ClusterPlan pl = c->cl_plan;
    if (c->inject_incomplete) { ++pl.expected; c->inject_incomplete = false; }
    if (c->kernel_timing) { pl.t0 = c->kev0; pl.t1 = c->kev1; }
    pl.static_place = c->static_place ? (c->inject_misplaced ? 2 : 1) : 0;
    pl.xcd_base = c->xcd_base;
    pl.two_point = false;
    for (size_t k = 0; k < nops && !pl.two_point; ++k) pl.two_point = is_two_point(c->program[c->pc + k].p.kind);
    c->inject_misplaced = false;
    c->h_tmo[2] = 0;
    const auto h0 = std::chrono::steady_clock::now();
    hipError_t e = c3d::launch_cluster(m, dev_fire(c), pl, c3d::anneal_io(c->buf, c->parity), c->buf.tgt, c->d_crec, c->d_prog,
                                       c->op_run[c->pc], c->op_skip[c->pc], (int)nops, seq << 20, c->h_tmo_dev,
                                       c->d_claim + c3d_ctx::kClaimWords * seq, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("cluster launch: ") + hipGetErrorString(e));
    if (c->event_timing) HIP_TRY(hipEventRecord(c->ev1, c->stream));    // closes the timed range unless more work follows (end_timing)
    const auto h1 = std::chrono::steady_clock::now();
    // The launch's last workgroup writes its completion mark into host-mapped memory (timeout[1], c3d_cluster.hip): a short launch is
    // waited for by watching that word — hipStreamSynchronize returns ~6 us after the kernel has ended (profiles/r04_launch_overhead.txt) —
    // for at most `spin_wait_us`; a longer launch, a time-out or a misplacement goes through the synchronise call as before.  Everything
    // that touches the results afterwards is ordered on the stream (next launch, copies), so nothing needs the kernel's formal end here.
    bool marked = false;
    if (c->spin_wait_us > 0 && !c->kernel_timing) {
        const unsigned mark = (seq << 20) | 1u;
        for (;;) {
            if (__atomic_load_n(&c->h_tmo[1], __ATOMIC_ACQUIRE) == mark) { marked = true; break; }
            if (__atomic_load_n(&c->h_tmo[0], __ATOMIC_RELAXED) || __atomic_load_n(&c->h_tmo[2], __ATOMIC_RELAXED)) break;
            if (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - h1).count() > c->spin_wait_us) break;
            __builtin_ia32_pause();
        }
    }
    if (!marked) HIP_TRY(hipStreamSynchronize(c->stream));
    else ++c->spin_completions;
    const auto h2 = std::chrono::steady_clock::now();
    c->last_host_launch_us += std::chrono::duration<double, std::micro>(h1 - h0).count();
    c->last_host_sync_us += std::chrono::duration<double, std::micro>(h2 - h1).count();
    c->ev1_recorded = true;
    ++c->cluster_launches;
    if (c->kernel_timing) {
        float kms = 0;
        HIP_TRY(hipEventElapsedTime(&kms, c->kev0, c->kev1));
        c->last_kernel_ms += kms;
    }
    if (launch_was_abandoned(c, (seq << 20) | 1u)) { *ran = false; c->ev1_recorded = false; return C3D_OK; }
    *ran = true;
    c->last_path = 2;
    KernelRecord& k = c->ran;
    k = KernelRecord();
    k.family = KernelRecord::CLUSTER;
    k.pot = c3d::device_pot(m.noe_pot); k.rpw = pl.rpw; k.nb = m.npad / 256; k.wl = m.wl; k.late = pl.late_tiles != 0; k.tp = pl.two_point;
    account_ops(c, nops);
    return C3D_OK;
}

// run program ops [pc, pc + nops): eager or via cached graphs; every replica group advances on its
// own stream (fork from / join into stream 0 around the call)
int run_ops_segment(c3d_ctx* c, size_t nops, bool zero_w, bool lbfgs = false);

// A stage without restraint weight (w_all = 0: the clamp form divides by it) takes the general kernels; the ops around it keep the
// multi-step launches: the range is split where the weight changes between zero and non-zero.
// The range is also split where two-point minimiser steps (kinds 5 / 6) begin or end: a multi-step launch that holds any of them runs
// k_cluster_tp, 2.5 % slower per step than k_cluster (c3d_cluster.hip) — the MD stages before a final stage of kind 5 keep their kernel
// also when a caller asks for the whole schedule in one c3d_run_steps.  And where L-BFGS steps (kinds 9 / 8) begin or end: they run on the
// per-step path only (k_lbfgs_eval + k_lbfgs_move), the MD stages and the FIRE hand-over around them keep the multi-step kernel.
int run_ops(c3d_ctx* c, size_t nops) {
    // A precision-64 range (one kernel, k64_step, for every other kind) is split at the L-BFGS borders only.
    const bool p64 = c->precision == 64;
    if (p64 ? !c->has_lbfgs : (!c->zero_weight && !c->has_two_point && !c->has_lbfgs)) return run_ops_segment(c, nops, false);
    const size_t end = c->pc + nops;
    while (c->pc < end) {
        const c3d::DevStep& p0 = c->program[c->pc].p;
        const bool z = !p64 && p0.w_rs == 0.0f, tp = !p64 && is_two_point(p0.kind), lb = is_lbfgs(p0.kind);
        size_t k = 1;
        while (c->pc + k < end) {
            const c3d::DevStep& p = c->program[c->pc + k].p;
            if ((!p64 && p.w_rs == 0.0f) != z || (!p64 && is_two_point(p.kind)) != tp || is_lbfgs(p.kind) != lb) break;
            ++k;
        }
        const int rc = run_ops_segment(c, k, z, lb);
        if (rc) return rc;
    }
    return C3D_OK;
}

// A stream costs 8.5 ms to make (tools/microbench/hip_init_phases.cpp: the first one of a process 21-160 ms) and the multi-step kernel runs on
// the context's main stream alone: the streams of replica groups 1.. are made when the per-step path first runs with that many groups.
int ensure_group_streams(c3d_ctx* c, int G) {
    for (int g = 1; g < G && g < c3d_ctx::kMaxGroups; ++g) {
        if (c->gstream[g]) continue;
        HIP_TRY(hipStreamCreateWithFlags(&c->gstream[g], hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->gev[g], hipEventDisableTiming));
    }
    return C3D_OK;
}

int run_ops_segment(c3d_ctx* c, size_t nops, bool zero_w, bool lbfgs) {
    if (nops == 0) return C3D_OK;
    if (c->precision == 64 || zero_w || lbfgs) { }          // fp64 (k64_step) and L-BFGS steps: the per-step path below, never the cluster kernel
    else if (c->resident_skip > 0 && c->resident < 1) --c->resident_skip;     // cooling off after an abandoned launch
    else if (nops >= (size_t)c->resident_min_ops && nops < ((size_t)1 << 20)) {
        bool ran = false;
        int rc = C3D_OK;
        if (cluster_ok(c)) rc = run_cluster(c, nops, &ran);
        if (rc != C3D_OK || ran) return rc;
    }
    c->last_path = 0;
    c->ev1_recorded = false;
    if (c->precision != 64 && (!use_sym(c) || lbfgs)) {          // (before any stream capture begins: it allocates and synchronises)
        if (int rc = ensure_pair_targets(c, dev_model(c))) return rc;
    }
    if (lbfgs)
        if (int rc = c->precision == 64 ? ensure_lbfgs64(c) : ensure_lbfgs(c)) return rc;
    const int G = active_groups(c);
    if (int rc = ensure_group_streams(c, G)) return rc;
    // every replica group advances on its own stream (fork from / join into stream 0 around the range): while one
    // group sits in its launch boundary the other computes
    if (G > 1) {
        HIP_TRY(hipEventRecord(c->fork_ev, c->stream));
        for (int g = 1; g < G; ++g) HIP_TRY(hipStreamWaitEvent(c->gstream[g], c->fork_ev, 0));
    }
    size_t done = 0;
    while (done < nops) {
        const size_t chunk = std::min<size_t>(nops - done, c->use_graph ? (size_t)c->graph_chunk : nops - done);
        if (!c->use_graph || chunk < 4) {
            for (int g = 0; g < G; ++g) {
                int par = c->parity;
                for (size_t k = 0; k < chunk; ++k) {
                    int rc = launch_op(c, c->program[c->pc + k], g, par);
                    if (rc) return rc;
                    par ^= 1;
                }
            }
        } else {
            // one graph per (range, parity, group); homogeneous minimiser ranges (same stage, all kind 2, all 5 or all 8) share a graph
            // regardless of pc (kind 8 keeps its ring head and counts on the device)
            const Op& first = c->program[c->pc];
            const Op& last = c->program[c->pc + chunk - 1];
            long sig = (long)c->pc;
            if ((first.p.kind == 2 || first.p.kind == 5 || first.p.kind == 8) && last.p.kind == first.p.kind && first.stage == last.stage)
                sig = -(long)(first.stage + 1) - (first.p.kind == 5 ? 1000000L : first.p.kind == 8 ? 2000000L : 0L);     // (a stage of kind 5 or 8 has a minimiser part and a FIRE part)
            if (c->graphs.size() >= 2048) {                        // bounded: a caller with ever new ranges starts over
                for (int g = 0; g < G; ++g) HIP_TRY(hipStreamSynchronize(c->gstream[g]));
                drop_graphs(c);
            }
            for (int g = 0; g < G; ++g) {
                const auto key = std::make_tuple(sig, (int)chunk, c->parity, g);
                auto it = c->graphs.find(key);
                if (it == c->graphs.end()) {
                    hipGraph_t gr = nullptr;
                    HIP_TRY(hipStreamBeginCapture(c->gstream[g], hipStreamCaptureModeThreadLocal));
                    int par = c->parity;
                    int rc = C3D_OK;
                    for (size_t k = 0; k < chunk && rc == C3D_OK; ++k) { rc = launch_op(c, c->program[c->pc + k], g, par); par ^= 1; }
                    hipError_t ce = hipStreamEndCapture(c->gstream[g], &gr);
                    if (rc) { if (gr) (void)hipGraphDestroy(gr); return rc; }
                    if (ce != hipSuccess) return fail(C3D_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
                    hipGraphExec_t ge = nullptr;
                    hipError_t ie = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
                    (void)hipGraphDestroy(gr);
                    if (ie != hipSuccess) return fail(C3D_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
                    it = c->graphs.emplace(key, ge).first;
                    ++c->graph_captures;
                }
                HIP_TRY(hipGraphLaunch(it->second, c->gstream[g]));
                ++c->graph_launches;
            }
        }
        c->step_launches += (long)chunk * G;
        if (lbfgs) { c->lbfgs_steps += (long)chunk; c->lbfgs_parity = c->parity ^ (int)(chunk & 1); }
        if (chunk & 1) c->parity ^= 1;
        for (size_t k = 0; k < chunk; ++k)
            if (c->program[c->pc + k].counted) { ++c->steps_done; ++c->last_steps; }
        c->last_launches += (long)chunk;
        c->pc += chunk;
        done += chunk;
    }
    for (int g = 1; g < G; ++g) {
        HIP_TRY(hipEventRecord(c->gev[g], c->gstream[g]));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->gev[g], 0));
    }
    if (c->precision == 64) {
        // the fp32 buffers of the current parity receive a copy of the state (read-back, energies, scoring, the minimiser's exit test)
        hipError_t e = c3d::launch_export64(dev_model(c), c->b64, c->parity, c->buf.X[c->parity], c->buf.V[c->parity], c->buf.P[c->parity], c->stream);
        if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 export: ") + hipGetErrorString(e));
        c->last_path = 3;
    }
    c->ran = op_kernel(c, dev_model(c), c->program[c->pc - 1]);
    return C3D_OK;
}

int begin_timing(c3d_ctx* c) {
    c->last_ms = 0; c->last_kernel_ms = 0; c->last_steps = 0; c->last_launches = 0; c->last_host_launch_us = 0; c->last_host_sync_us = 0;
    c->ev1_recorded = false;
    if (c->event_timing) HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return C3D_OK;
}
int end_timing(c3d_ctx* c) {
    if (!c->ev1_recorded) {                        // a multi-step launch has recorded it behind itself and synchronised already
        if (c->event_timing) HIP_TRY(hipEventRecord(c->ev1, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (!c->event_timing) return C3D_OK;
    HIP_TRY(hipEventSynchronize(c->ev1));          // (a launch waited for on its completion mark may not have retired its event yet)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->last_ms = ms;
    return C3D_OK;
}

// Read-backs (exit test of the minimiser, coordinates, energies, scoring sums) land in a pinned buffer the context owns: the runtime does not
// have to pin a pageable destination for every copy, and what a copy costs does not depend on where the allocator put the destination.
int ensure_stage(c3d_ctx* c, size_t bytes) {
    if (bytes <= c->h_stage_bytes) return C3D_OK;
    if (c->h_stage) { HIP_TRY(hipStreamSynchronize(c->stream)); (void)hipHostFree(c->h_stage); c->h_stage = nullptr; c->h_stage_bytes = 0; }
    const size_t cap = std::max<size_t>(bytes, (size_t)64 << 10);
    HIP_TRY(hipHostMalloc(&c->h_stage, cap, hipHostMallocDefault));
    c->h_stage_bytes = cap;
    return C3D_OK;
}
// device -> pinned staging, synchronised; the caller reads c->h_stage
int read_back(c3d_ctx* c, const void* dev, size_t bytes) {
    if (int rc = ensure_stage(c, bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(c->h_stage, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

// max over replicas of the RMS force from the FIRE partial sums of the current parity
int max_rms_force(c3d_ctx* c, double* out) {
    const int nparts = c->ntiles;
    if (int rc = read_back(c, c->buf.P[c->parity], sizeof(float) * (size_t)c->nrep * nparts * 4)) return rc;
    const float* h = static_cast<const float*>(c->h_stage);
    double worst = 0;
    for (int r = 0; r < c->nrep; ++r) {
        double ff = 0;
        for (int t = 0; t < nparts; ++t) ff += h[((size_t)r * nparts + t) * 4 + 1];
        const double rms = sqrt(ff / (3.0 * c->n));
        if (!(rms <= worst)) worst = rms;   // NaN propagates
    }
    *out = worst;
    return C3D_OK;
}

// are the last step's per-tile sums (functions of every velocity / force component) all finite?
int partials_finite(c3d_ctx* c, bool* ok) {
    const size_t cnt = (size_t)c->nrep * c->ntiles * 4;
    if (int rc = read_back(c, c->buf.P[c->parity], sizeof(float) * cnt)) return rc;
    const float* h = static_cast<const float*>(c->h_stage);
    *ok = true;
    for (size_t k = 0; k < cnt; ++k) if (!std::isfinite(h[k])) { *ok = false; break; }
    return C3D_OK;
}

// fp64 state <- the fp32 coordinates of the current parity (start structures, c3d_set_coords, the DG embedding); velocities zero
int import64(c3d_ctx* c) {
    hipError_t e = c3d::launch_import64(dev_model(c), c->buf.X[c->parity], c->b64, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 import: ") + hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

}  // namespace

// =============================================================================================
extern "C" int c3d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" void c3d_default_model(c3d_model* m) {
    if (!m) return;
    // Round 3: every number below comes from the reference's 45 bundled models, in two independent steps:
    // (1) inverse force matching (tools/calib/force_match.py, profiles/r03_force_matching.txt): which restraint potential
    //     leaves every bead of a bundled model force-free.  Answer, the same at 1 Mb and at 500 kb: the soft-square switches
    //     to its linear tail 0.5 A above the target with slope 2 S 0.5 = 10 (CNS terms: rswitch 0.5, asymptote 1.0 — half of
    //     round 2's 1.0 / 2.0), the lower side is square for a few Angstrom and saturates, pseudo-bonds ~300-400 kcal/mol/A^2
    //     around 3.95 A, (i,i+2) ~45 around 6 A, repel contact ~4.6 A with k ~2-4;
    // (2) refit on the 23 one-megabase matrices against the structure-level metrics of the parity table (Rg ratio,
    //     distance-matrix similarity, bond and (i,i+2) statistics, Spearman), the 22 matrices at 500 kb held out
    //     (tools/calib/fit_structure.py, profiles/r03_structure_fit.txt): a plateau around the values below.
    m->min_sep = 5; m->noe_pot = 3; m->rep_sep = 2; m->ang_mode = 1;
    m->s_noe = 10.0f; m->rswitch = 0.5f; m->asym = 2.0f;   // tail slope = asym x rswitch x S = 10
    m->k_bond = 500.0f; m->b0 = 3.93f;
    m->k_ang = 15.0f; m->a0 = 5.55f;
    m->r0_rep = 5.25f; m->k_rep = 4.0f;
    m->mass = 100.0f; m->fbeta = 10.0f;
    // lower side of the NOE term (round 4): square up to mrswitch inside the target, then the soft form with exponent 2 and no
    // asymptote — the push on a pair far inside its target DECAYS as D^-3 beyond 10 A.  These are X-PLOR's own defaults for the soft
    // potential (rswitch 10, asymptote 0, soexponent 2), which CNS keeps for the minus side because the deck's modules only set the
    // plus side [CNS-UNVERIFIED]; the relaxation fit finds mrswitch = 9.9-10.0 on its own (profiles/r04_relax_fit.txt)
    m->mrswitch = 10.0f; m->masym = 0.0f; m->msoexp = 2;
}
extern "C" void c3d_default_fire(c3d_fire_params* f) {
    if (!f) return;
    f->dt_start = 0.002f; f->dt_max = 0.02f; f->f_inc = 1.1f; f->f_dec = 0.5f;
    f->alpha_start = 0.1f; f->f_alpha = 0.99f; f->max_step = 0.5f; f->n_min = 5;
}
extern "C" int c3d_default_schedule(c3d_stage* st, int cap, int min_steps) {
    std::vector<c3d_stage> v;
    // regularisation (deck :1631-1645: 100 + 100 minimiser steps, weights * 1, vdw 20, repel 0.5)
    v.push_back({2, 200, 0.0f, 1.0f, 20.0f, 0.5f, 0.0f});
    // hot stages (deck :1649-1700): 1000 steps at 2000 K, dt 0.003
    const float hot_t = 2000.0f, hot_dt = 0.003f;
    const int hot_n[5] = {125, 125, 125, 500, 125};
    const float hot_w[5] = {0.1f, 0.2f, 0.2f, 0.4f, 1.0f};
    const float hot_v[5] = {20.0f, 20.0f, 0.01f, 0.003f, 0.003f};
    const float hot_r[5] = {0.5f, 0.5f, 0.9f, 0.9f, 0.9f};
    for (int k = 0; k < 5; ++k) v.push_back({0, hot_n[k], hot_dt, hot_w[k], hot_v[k], hot_r[k], hot_t});
    // slow cool (deck :1740-1782): ncycle = 80, 81 passes of int(1000/80) = 12 steps, dt 0.005
    const int ncycle = (int)(hot_t / 25.0f);
    const int nstep = 1000 / ncycle;
    const double vdw_step = pow(4.0 / 0.003, 1.0 / ncycle);
    const double rad_step = (1.0 - 0.85) / ncycle;
    double radius = 1.0, kv = 0.003, bath = hot_t;
    for (int i = 0; i <= ncycle; ++i) {
        v.push_back({1, nstep, 0.005f, 1.0f, (float)kv, (float)radius, (float)bath});
        radius = std::max(0.85, radius - rad_step);
        kv = std::min(4.0, kv * vdw_step);
        bath -= 25.0;
    }
    // final minimisation (deck :1790-1803): weights * 1; kind 5 = two-point step-size minimiser, FIRE after final_minimiser_steps (round 5)
    v.push_back({5, min_steps, 0.0f, 1.0f, 1.0f, 0.85f, 0.0f});
    if (st) for (int k = 0; k < (int)v.size() && k < cap; ++k) st[k] = v[k];
    return (int)v.size();
}

static std::atomic<int> g_preload{1};

extern "C" int c3d_set_process_option(const char* key, double value) {
    if (!key) return fail(C3D_ERR_INVALID, "c3d_set_process_option: null key");
    if (!strcmp(key, "preload")) {
        if (value != 0 && value != 1 && value != 2) return fail(C3D_ERR_INVALID, "c3d_set_process_option: preload is 0, 1 or 2");
        g_preload.store((int)value);
        return C3D_OK;
    }
    return fail(C3D_ERR_INVALID, std::string("c3d_set_process_option: unknown key ") + key);
}

extern "C" int c3d_create(int device, c3d_ctx** out) {
    if (!out) return fail(C3D_ERR_INVALID, "c3d_create: null out");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(C3D_ERR_NO_DEVICE, "no HIP device visible: libc3d has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(C3D_ERR_INVALID, "c3d_create: device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(C3D_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", libc3d is built for gfx950 only");
    int num_xcc = 0;
    if (hipDeviceGetAttribute(&num_xcc, hipDeviceAttributeNumberOfXccs, device) != hipSuccess) num_xcc = 0;   // unknown: no cluster kernel
    // Code objects ("code objects" above): what a default job launches from is loaded HERE, on this thread, before the context makes its first
    // HIP resource — not by a helper thread beside the caller's first launches, as in rounds 4-5 (that saved the first job of a process ~13 ms
    // and is where the one device exception of round 5 was met).  Later contexts of the device find the units loaded (one atomic load).
    if (const int pre = g_preload.load())
        if (const int rc = ensure_units(device, pre >= 2 ? kUnitsAll : kUnitsDefault)) return rc;
    c3d_ctx* c = new c3d_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount;
    c->num_xcc = num_xcc;
    c3d_default_model(&c->model);
    c3d_default_fire(&c->fire);
    c->stages.resize(c3d_default_schedule(nullptr, 0, 3000));
    c3d_default_schedule(c->stages.data(), (int)c->stages.size(), 3000);
    Entry gate(c, 0u, false);
    if (gate.rc != C3D_OK) { delete c; return gate.rc; }
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
              hipEventCreate(&c->kev0) == hipSuccess && hipEventCreate(&c->kev1) == hipSuccess &&
              hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) == hipSuccess;
    c->gstream[0] = c->stream;       // the other replica groups' streams: ensure_group_streams, when the per-step path first wants them
    // the word a multi-step launch sets when a workgroup gives up: host memory, read after the stream has drained
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->h_tmo), 64, hipHostMallocMapped) == hipSuccess;
    if (ok) {
        *c->h_tmo = 0;
        ok = hipHostGetDevicePointer(reinterpret_cast<void**>(&c->h_tmo_dev), c->h_tmo, 0) == hipSuccess &&
             hipMalloc(&c->d_claim, sizeof(unsigned) * c3d_ctx::kClaimWords * c3d_ctx::kClaimSets) == hipSuccess;
        c->h_tmo[1] = 0;
    }
    if (!ok) {
        c3d_destroy(c);                // a nested entry: the gate is this one
        return fail(C3D_ERR_HIP, "cannot create HIP stream/events");
    }
    *out = c;
    return C3D_OK;
}

extern "C" void c3d_destroy(c3d_ctx* c) {
    if (!c) return;
    c->ifr.release();                  // host arithmetic only: joined before the gate is taken
    {
        Entry gate(c, 0u, false);      // hipSetDevice cannot fail for a device c3d_create accepted; the context goes either way
        release_context(c);
    }
    delete c;
}

extern "C" int c3d_set_model(c3d_ctx* c, const c3d_model* m) {
    if (!c || !m) return fail(C3D_ERR_INVALID, "c3d_set_model: null argument");
    // msoexp (the struct's last member, added in round 4) = 0 means "the default, 2": a caller that zero-initialises the struct and
    // fills in what it knows keeps working ("ABI notes")
    const int msoexp = m->msoexp == 0 ? 2 : m->msoexp;
    if (m->mass <= 0 || m->rswitch <= 0 || m->min_sep < 1 || m->rep_sep < 1 || m->rep_sep > 3 || m->noe_pot < 0 || m->noe_pot > 3 || m->mrswitch <= 0 || (msoexp != 1 && msoexp != 2))
        return fail(C3D_ERR_INVALID, "c3d_set_model: parameter out of range");
    if (c->have_targets && m->min_sep != c->model.min_sep)
        return fail(C3D_ERR_INVALID, "c3d_set_model: min_sep must be set before the targets are built");
    // the fp64 target matrix encodes "no restraint" per potential: rebuilt by a launch (fp64 contexts load no potential-specific unit)
    const bool targets64 = c->precision == 64 && c->b64.T;
    Entry entry(c, 0u, targets64);
    if (entry.rc != C3D_OK) return entry.rc;
    c->model = *m;
    c->model.msoexp = msoexp;
    drop_stale(c, STALE_PAIR_TARGETS | STALE_PROGRAM);   // the pre-scaled pair targets of the per-step kernel carry 1 / mrs: rebuilt on demand
    if (c->have_replicas)                  // the multi-step kernel's plan depends on the potential
        if (int rc = plan_cluster(c)) return rc;
    return targets64 ? build_targets64(c) : C3D_OK;
}

extern "C" int c3d_set_schedule(c3d_ctx* c, const c3d_stage* st, int n_stages, const c3d_fire_params* fire, float gtol,
                                int check_every) {
    if (!c || !st || n_stages < 1) return fail(C3D_ERR_INVALID, "c3d_set_schedule: bad arguments");
    for (int k = 0; k < n_stages; ++k) {
        if (st[k].kind < 0 || (st[k].kind > 2 && st[k].kind != 5 && st[k].kind != 8) || st[k].nsteps < 0) return fail(C3D_ERR_INVALID, "c3d_set_schedule: bad stage");
        if (st[k].kind == 8 && c->precision == 64 && !c->f64_lbfgs)
            return fail(C3D_ERR_INVALID, "c3d_set_schedule: a stage of kind 8 (L-BFGS) has no fp64 form; set precision 32 first");
    }
    c->stages.assign(st, st + n_stages);
    if (fire) c->fire = *fire;
    c->gtol = gtol;
    if (check_every > 0) c->check_every = check_every;
    return drop_stale_gated(c, STALE_PROGRAM);
}

extern "C" int c3d_set_option(c3d_ctx* c, const char* key, double value) {
    if (!c || !key) return fail(C3D_ERR_INVALID, "c3d_set_option: null argument");
    unsigned stale = 0;                    // what the new value invalidates: dropped below, in one place
    if (!strcmp(key, "use_graph")) c->use_graph = value != 0;
    else if (!strcmp(key, "rows_per_wave")) {
        if (value != 1 && value != 2 && value != 4) return fail(C3D_ERR_INVALID, "rows_per_wave must be 1, 2 or 4");
        c->rpw = (int)value;
        stale = STALE_GRAPHS;
    } else if (!strcmp(key, "replica_groups")) {   // groups stepped concurrently on separate streams
        if (value < 1 || value > c3d_ctx::kMaxGroups) return fail(C3D_ERR_INVALID, "replica_groups must be 1..4");
        c->ngroups = (int)value;
        stale = STALE_GRAPHS;
    } else if (!strcmp(key, "event_timing")) c->event_timing = value != 0;
    else if (!strcmp(key, "kernel_timing")) c->kernel_timing = value != 0;
    else if (!strcmp(key, "resident")) { c->resident = value < 0 ? -1 : (value != 0); c->resident_skip = 0; }
    else if (!strcmp(key, "precision")) {  // 32 (the product kernels) or 64 (the fp64 reference step); call before c3d_init_replicas
        if (value != 32 && value != 64) return fail(C3D_ERR_INVALID, "precision must be 32 or 64");
        if (value == 64 && !c->f64_lbfgs)
            for (const c3d_stage& st : c->stages)
                if (st.kind == 8) return fail(C3D_ERR_INVALID, "precision 64: the schedule holds a stage of kind 8 (L-BFGS), which has no fp64 form");
        c->precision = (int)value;
        stale = STALE_REPLICAS | STALE_GRAPHS;
    } else if (!strcmp(key, "eval_rows_per_wave")) {
        if (value != 2 && value != 4 && value != -2) return fail(C3D_ERR_INVALID, "eval_rows_per_wave must be 4, 2 (packed pair term) or -2 (two rows per wave, scalar pair term)");
        c->eval_rpw = (int)value;
    } else if (!strcmp(key, "pair_targets")) { c->pair_targets = value != 0; stale = STALE_PAIR_TARGETS | STALE_GRAPHS; }
    else if (!strcmp(key, "wide_tiles")) { c->wide_tiles = value != 0; stale = STALE_GRAPHS; }
    else if (!strcmp(key, "symmetric")) { c->sym = value > 0; stale = STALE_REPLICAS | STALE_GRAPHS; }   // takes effect at the next c3d_init_replicas with a new replica count / matrix
    else if (!strcmp(key, "start")) {      // A5: 0 = Philox random coil, 1 = extended strand as extn.inp lays it out (:2413-2416)
        if (value != 0 && value != 1) return fail(C3D_ERR_INVALID, "start must be 0 (random coil) or 1 (extended strand)");
        c->start_mode = (int)value;
    } else if (!strcmp(key, "cluster")) c->cluster = value < 0 ? -1 : (value != 0);
    else if (!strcmp(key, "resident_inject_timeout")) c->inject_timeout = value != 0;   // test hook
    else if (!strcmp(key, "narrow_columns")) { c->narrow_columns = value != 0; stale = STALE_REPLICAS | STALE_GRAPHS; }
    else if (!strcmp(key, "cluster_static_placement")) { c->static_place = value != 0; c->inject_misplaced = value == 2; }   // 0: per-XCD atomic slot counters; 2: test hook
    else if (!strcmp(key, "cluster_inject_incomplete")) c->inject_incomplete = value != 0;   // test hook
    else if (!strcmp(key, "cluster_num_xcc")) { c->num_xcc = (int)value; stale = STALE_REPLICAS; }   // test hook: pretend a partitioned device
    else if (!strcmp(key, "prefetch_ranks")) c->prefetch_ranks = value != 0;
    else if (!strcmp(key, "device_ranks")) {       // who ranks the IF matrix for c3d_score_replicas
        if (value != -1 && value != 0 && value != 1)
            return fail(C3D_ERR_INVALID, "device_ranks is 0 (the device beyond 5120 beads), 1 (the device for every symmetric matrix) or -1 (the host)");
        c->device_ranks = (int)value;
    }
    else if (!strcmp(key, "final_minimiser_steps")) {
        if (value < 2) return fail(C3D_ERR_INVALID, "c3d_set_option: final_minimiser_steps >= 2");
        c->bb_steps = (int)value;
        stale = STALE_PROGRAM;
    } else if (!strcmp(key, "final_minimiser")) {  // what a stage of kind 5 runs: 1 (default) two-point step size then FIRE, 0 FIRE throughout
        if (value != 0 && value != 1) return fail(C3D_ERR_INVALID, "c3d_set_option: final_minimiser is 0 (FIRE) or 1 (two-point step size)");
        c->final_bb = value != 0;
        stale = STALE_PROGRAM;
    } else if (!strcmp(key, "lbfgs_memory")) {     // pairs a kind-8 stage keeps; takes effect at the next stage's first step
        if (value != (int)value || value < 1 || value > c3d::kLbfgsMaxPairs) return fail(C3D_ERR_INVALID, "c3d_set_option: lbfgs_memory is 1..8");
        c->lbfgs_mem = (int)value;
        stale = STALE_GRAPHS;
    } else if (!strcmp(key, "cluster_xcd_count")) {   // 1..8 XCDs for this context's multi-step launches; re-plans: before c3d_init_replicas
        const int v = (int)value;
        if (v < 1 || v > 8 || c->xcd_base + v > 8) return fail(C3D_ERR_INVALID, "cluster_xcd_count: 1..8, and cluster_xcd_base + cluster_xcd_count <= 8");
        c->xcd_count = v;
        stale = STALE_REPLICAS;
    } else if (!strcmp(key, "cluster_xcd_base")) {    // first XCD of the set; may change between launches (the plan depends on the count only)
        const int v = (int)value;
        if (v < 0 || v + c->xcd_count > 8) return fail(C3D_ERR_INVALID, "cluster_xcd_base: 0 .. 8 - cluster_xcd_count");
        c->xcd_base = v;
    } else if (!strcmp(key, "cluster_late_tiles")) { c->cluster_late = value != 0 ? -1 : 0; stale = STALE_REPLICAS; }   // measurement knob: 0 = never; before c3d_init_replicas
    else if (!strcmp(key, "cluster_geometry")) {   // measurement knob: 100 CW + 10 RPW + helpers (0 = planner); before c3d_init_replicas
        if (value < 0 || value > 1699) return fail(C3D_ERR_INVALID, "cluster_geometry = 100 compute waves + 10 rows per wave + helper waves");
        c->cluster_geom = (int)value;
        stale = STALE_REPLICAS;
    } else if (!strcmp(key, "spin_wait_us")) c->spin_wait_us = value < 0 ? 0 : value;
    else if (!strcmp(key, "resident_min_ops")) c->resident_min_ops = value < 1 ? 1 : (int)value;
    else if (!strcmp(key, "stage_dma")) { c->stage_dma = value != 0; stale = STALE_GRAPHS; }
    else if (!strcmp(key, "max_beads")) {          // the caller's consent to the memory of a large matrix (c3d.h); before c3d_set_if_matrix
        if (value != (int)value || value < C3D_MAX_BEADS_DEFAULT || value > C3D_MAX_BEADS_LIMIT)
            return fail(C3D_ERR_INVALID, "max_beads must be an integer from 5120 to 16384");
        c->max_beads = (int)value;
    } else if (!strcmp(key, "embed_max_beads")) {  // the caller's consent to the memory of a large embedding (c3d.h)
        if (value != (int)value || value < C3D_EMBED_MAX_BEADS_DEFAULT || value > C3D_EMBED_MAX_BEADS_LIMIT)
            return fail(C3D_ERR_INVALID, "embed_max_beads must be an integer from 4549 to 16384");
        c->embed_max_beads = (int)value;
    } else if (!strcmp(key, "f64_max_beads")) {    // the caller's consent to the fp64 target matrix, 8 n np bytes (c3d.h); before c3d_init_replicas
        if (value != (int)value || value < C3D_F64_MAX_BEADS_DEFAULT || value > C3D_F64_MAX_BEADS_LIMIT)
            return fail(C3D_ERR_INVALID, "f64_max_beads must be an integer from 2560 to 16384");
        c->f64_max_beads = (int)value;
    } else if (!strcmp(key, "f64_lbfgs")) {        // the caller's consent to kind-8 stages in fp64 (c3d.h); releases nothing on the device
        if (value != 0 && value != 1) return fail(C3D_ERR_INVALID, "f64_lbfgs must be 0 or 1");
        if (value == 0 && c->precision == 64)
            for (const c3d_stage& st : c->stages)
                if (st.kind == 8) return fail(C3D_ERR_INVALID, "f64_lbfgs: precision is 64 and the schedule holds a stage of kind 8 (L-BFGS); change one of them first");
        c->f64_lbfgs = value != 0;
    } else if (!strcmp(key, "f64_column_chunk")) { // test and measurement knob: the fp64 step kernel's column source (same bits either way)
        if (value != (int)value || (value != 0 && !c3d::column_chunk64_valid((int)value)))
            return fail(C3D_ERR_INVALID, "f64_column_chunk must be 0 (by size), 256, 512 or 1024");
        c->f64_column_chunk = (int)value;
        stale = STALE_GRAPHS;
    } else if (!strcmp(key, "embed_form")) {       // test and measurement knob: the eigen stage's form (same bits either way)
        if (value != 0 && value != 1) return fail(C3D_ERR_INVALID, "embed_form is 0 (k_dg_eig while it fits, tiled beyond) or 1 (tiled)");
        c->embed_form = (int)value;
    } else if (!strcmp(key, "embed_batch")) {      // test knob: replicas embedded at a time (same bits whatever it is)
        if (value != (int)value || value < 0) return fail(C3D_ERR_INVALID, "embed_batch is 0 (by the scratch budget) or a number of replicas");
        c->embed_batch = (int)value;
    } else if (!strcmp(key, "column_chunk")) {     // test and measurement knob: the per-step kernels' column source (same bits either way)
        if (value != (int)value || (value != 0 && !c3d::column_chunk_valid((int)value)))
            return fail(C3D_ERR_INVALID, "column_chunk must be 0 (the library's choice), 256, 1024 or 2048");
        c->column_chunk = (int)value;
        stale = STALE_GRAPHS;
    }
    else if (!strcmp(key, "graph_chunk")) {
        if (value < 8) return fail(C3D_ERR_INVALID, "graph_chunk must be >= 8");
        c->graph_chunk = (int)value & ~1;   // even: a chunk returns to the starting parity
        stale = STALE_GRAPHS;
    } else return fail(C3D_ERR_INVALID, std::string("unknown option ") + key);
    return drop_stale_gated(c, stale);
}

// The largest matrix a context accepts: kDefaultMaxBeads unless the option max_beads raises it, up to kMaxBeadsLimit.  Up to
// c3d::kMaxStagedCols the per-step kernels stage a replica's coordinates in LDS; beyond, they run in the chunked form (ColsChunked, c3d_step_core.h).
// The default stays where the staged form ends: a larger matrix needs ~8 n npad bytes per context (targets and pair targets) and K1's
// transient copies of the matrix, which the caller agrees to by raising the limit.
static constexpr int kDefaultMaxBeads = C3D_MAX_BEADS_DEFAULT;
static constexpr int kMaxBeadsLimit = C3D_MAX_BEADS_LIMIT;
static_assert(kDefaultMaxBeads == c3d::kMaxStagedCols, "the default limit is the staged form's");
static int too_many_beads(const c3d_ctx* c, const char* fn, int n) {
    char b[192];
    if (c->max_beads == kDefaultMaxBeads)
        snprintf(b, sizeof b, "%s: %d beads: more than %d are accepted only after c3d_set_option(\"max_beads\", n) (up to %d)", fn, n,
                 kDefaultMaxBeads, kMaxBeadsLimit);
    else
        snprintf(b, sizeof b, "%s: %d beads: more than max_beads = %d (the option goes up to %d)", fn, n, c->max_beads, kMaxBeadsLimit);
    return fail(C3D_ERR_INVALID, b);
}
// c3d_set_if_matrix computes the Spearman's IF ranks ahead of c3d_score_replicas up to this many beads (memory: see there)
static constexpr int kRankPrefetchBeads = 2048;

extern "C" int c3d_set_if_matrix(c3d_ctx* c, const double* IF, int n, double alpha, double K) {
    if (!c || !IF || n < 2) return fail(C3D_ERR_INVALID, "c3d_set_if_matrix: bad arguments");
    if (n > c->max_beads) return too_many_beads(c, "c3d_set_if_matrix", n);
    C3D_ENTRY(c, 0u);
    free_replica_buffers(c);
    set_dims(c, n);
    const size_t nn = (size_t)n * n;
    // The Spearman's IF ranks (range 3: spearman_IF_pdb.pl:14, the only range a driver asks for) on a helper thread, beside K1 and the
    // anneal — host arithmetic only, no HIP call.  Only up to kRankPrefetchBeads: the worker keeps a copy of the matrix and the rank matrix,
    // 16 bytes per pair, until the context goes (67 MB at 2048 beads; at the 5120 the library accepts it would be 420 MB per context and
    // ~1 GB while it sorts).  It starts HERE, before K1's allocations and copies, and the vectors keep their capacity from matrix to
    // matrix: started after the allocations (so that an early error return wastes no work: round 6 tried it) the worker's first
    // milliseconds — page faults of 3 MB of fresh vectors — coincide with K1's upload from pageable memory, and config 4 took 0.39-0.40 s
    // instead of 0.175 (same box, A/B, profiles/r06_rank_prefetch_start_ab.txt); without the worker at all 0.27-0.33 s.
    c->ifr.join();
    c->ifr.valid = false;
    if (c->prefetch_ranks && n <= kRankPrefetchBeads) {
        try {
            c->ifr.matrix.assign(IF, IF + nn);
            c->ifr.n = n; c->ifr.range = 3;
            c3d_ctx::IfRanks* const w = &c->ifr;
            c->ifr.worker = std::thread([w] {
                try { c3d::if_pair_ranks(w->matrix.data(), w->n, w->range, w->rank, w->m, w->mean, w->saa); w->valid = true; }
                catch (...) { w->valid = false; }
            });
        } catch (...) { c->ifr.release(); }               // no memory or no thread: c3d_score_replicas computes the ranks itself
    } else {
        c->ifr.release();                                  // a matrix beyond the limit: the copies of the previous one go
    }
    DevTmp<double> dIF, dP, dpart;
    DevTmp<int32_t> ddist;
    DevTmp<unsigned char> dflags;
    DevTmp<unsigned> dnflag;
    const int npartial = 64;
    dev_free(c->buf.tgt); dev_free(c->buf.tgs2);
    c->have_targets = false;
    HIP_TRY(hipMalloc(&dIF.p, sizeof(double) * nn));
    HIP_TRY(hipMalloc(&dP.p, sizeof(double) * nn));
    HIP_TRY(hipMalloc(&dpart.p, sizeof(double) * npartial));
    HIP_TRY(hipMalloc(&ddist.p, sizeof(int32_t) * nn));
    HIP_TRY(hipMalloc(&dflags.p, nn));
    HIP_TRY(hipMalloc(&dnflag.p, sizeof(unsigned)));
    HIP_TRY(hipMalloc(&c->buf.tgt, sizeof(float) * (size_t)n * c->npad));
    HIP_TRY(hipMemcpyAsync(dIF.p, IF, sizeof(double) * nn, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dnflag.p, 0, sizeof(unsigned), c->stream));
    HIP_TRY(hipMemsetAsync(dflags.p, 0, nn, c->stream));
    hipError_t e = c3d::launch_if_to_target(dIF.p, n, c->npad, alpha, K, c->model.min_sep, c->model.rep_sep, dP.p, dpart.p,
                                            npartial, ddist.p, c->buf.tgt, dflags.p, dnflag.p, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("K1 launch: ") + hipGetErrorString(e));
    c->h_dist10.resize(nn);
    c->r_i.clear(); c->r_j.clear(); c->r_t10.clear();
    unsigned nflag = 0;
    HIP_TRY(hipMemcpyAsync(c->h_dist10.data(), ddist.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&nflag, dnflag.p, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->k1_recomputed = 0;
    if (nflag) {
        // Near-tie elements: redo them exactly as the reference does (:132-161) — libm pow, the running sum over all N*N
        // elements in row-major order, P / mean, K / that, "%.1f" — and patch the device copy where the tenth changed.
        std::vector<unsigned char> flags(nn);
        HIP_TRY(hipMemcpyAsync(flags.data(), dflags.p, nn, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        double sum = 0.0;
        for (size_t k = 0; k < nn; ++k) sum += pow(IF[k], alpha);
        const double mean = sum / ((double)n * (double)n);
        for (size_t k = 0; k < nn; ++k) {
            if (!flags[k]) continue;
            double v = pow(IF[k], alpha) / mean;
            if (v == 0) continue;
            v = K / v;
            char b[64];
            snprintf(b, sizeof b, "%.1f", v);
            char* dot = strchr(b, '.');
            long long t = atoll(b) * 10 + (dot ? dot[1] - '0' : 0);
            if (t > 2000000000LL) t = 2000000000LL;
            ++c->k1_recomputed;
            if ((int32_t)t == c->h_dist10[k]) continue;
            c->h_dist10[k] = (int32_t)t;
            const int i = (int)(k / n), j = (int)(k % n);
            const int sep = i > j ? i - j : j - i;
            const float enc = (sep >= c->model.min_sep && t > 0) ? (float)((double)t / 10.0) : 0.0f;
            HIP_TRY(hipMemcpyAsync(c->buf.tgt + (size_t)i * c->npad + j, &enc, sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            dev_free(c->buf.tgs2);
            ++c->k1_patched;
        }
    }
    int R = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (j - i >= c->model.min_sep && c->h_dist10[(size_t)i * n + j] > 0) ++R;
    c->R = R;
    c->have_targets = true;
    build_program(c);
    return C3D_OK;
}

extern "C" int c3d_set_restraints(c3d_ctx* c, int n, int R, const int32_t* ri, const int32_t* rj, const int32_t* rt10) {
    if (!c || n < 2 || R < 0 || (R > 0 && (!ri || !rj || !rt10))) return fail(C3D_ERR_INVALID, "c3d_set_restraints: bad arguments");
    if (n > c->max_beads) return too_many_beads(c, "c3d_set_restraints", n);
    C3D_ENTRY(c, 0u);
    free_replica_buffers(c);
    c->ifr.release();
    set_dims(c, n);
    std::vector<float> enc((size_t)n * c->npad);
    std::fill(enc.begin(), enc.end(), 0.0f);
    for (int k = 0; k < R; ++k) {
        const int i = ri[k] - 1, j = rj[k] - 1;
        if (i < 0 || j < 0 || i >= n || j >= n || i == j) return fail(C3D_ERR_INVALID, "c3d_set_restraints: index out of range");
        if (rt10[k] <= 0) continue;
        const float t = (float)((double)rt10[k] / 10.0);
        enc[(size_t)i * c->npad + j] = c3d::encode_target_host(t);
        enc[(size_t)j * c->npad + i] = c3d::encode_target_host(t);
    }
    int rc = upload_targets(c, enc);
    if (rc) return rc;
    c->h_dist10.clear();
    // the list itself, for a precision-64 context (c3d_init_replicas): 0-based, i < j, the last entry of a pair as in `enc` above
    {
        std::vector<std::pair<uint64_t, int>> key;
        key.reserve(R);
        for (int k = 0; k < R; ++k) {
            const int i = std::min(ri[k], rj[k]) - 1, j = std::max(ri[k], rj[k]) - 1;
            key.emplace_back((uint64_t)i * n + j, k);
        }
        std::sort(key.begin(), key.end());
        c->r_i.clear(); c->r_j.clear(); c->r_t10.clear();
        int32_t last = 0;                           // the pair's value in `enc`: the last entry with a positive target
        for (size_t q = 0; q < key.size(); ++q) {
            if (rt10[key[q].second] > 0) last = rt10[key[q].second];
            if (q + 1 < key.size() && key[q + 1].first == key[q].first) continue;
            if (last > 0) { c->r_i.push_back((int32_t)(key[q].first / n)); c->r_j.push_back((int32_t)(key[q].first % n)); c->r_t10.push_back(last); }
            last = 0;
        }
    }
    c->R = R;
    c->have_targets = true;
    build_program(c);
    return C3D_OK;
}

extern "C" int c3d_get_dist10(c3d_ctx* c, int32_t* out) {
    if (!c || !out) return fail(C3D_ERR_INVALID, "c3d_get_dist10: null argument");
    if (c->h_dist10.empty()) return fail(C3D_ERR_INVALID, "c3d_get_dist10: targets were not built from an IF matrix");
    memcpy(out, c->h_dist10.data(), sizeof(int32_t) * c->h_dist10.size());
    return C3D_OK;
}
extern "C" int c3d_num_beads(const c3d_ctx* c) { return c ? c->n : 0; }
extern "C" int c3d_num_restraints(const c3d_ctx* c) { return c ? c->R : 0; }

extern "C" int c3d_init_replicas(c3d_ctx* c, int nrep, uint64_t seed, uint32_t first_replica) {
    if (!c || nrep < 1) return fail(C3D_ERR_INVALID, "c3d_init_replicas: bad arguments");
    if (!c->have_targets) return fail(C3D_ERR_INVALID, "c3d_init_replicas: set the IF matrix / restraints first");
    if (c->sym > 0 && c->npad > c3d::kMaxStagedCols && c->precision != 64)
        return fail(C3D_ERR_INVALID, "c3d_init_replicas: symmetric tiles stage a replica in LDS and take at most 5120 beads; set symmetric 0");
    if (c->precision == 64) {              // on the host, before anything is allocated or launched
        if (c->h_dist10.empty() && c->r_t10.empty())
            return fail(C3D_ERR_INVALID, "precision 64 needs targets built from an IF matrix (integer tenths)");
        if (c->n > c->f64_max_beads) {
            if (c->f64_max_beads == C3D_F64_MAX_BEADS_DEFAULT)
                return fail(C3D_ERR_INVALID, "precision 64: more than 2560 beads are accepted only after c3d_set_option(\"f64_max_beads\", n) (up to " +
                                                 std::to_string(C3D_F64_MAX_BEADS_LIMIT) + ")");
            return fail(C3D_ERR_INVALID, "precision 64: " + std::to_string(c->n) + " beads: more than f64_max_beads = " +
                                             std::to_string(c->f64_max_beads) + " (the option goes up to " + std::to_string(C3D_F64_MAX_BEADS_LIMIT) + ")");
        }
    }
    C3D_ENTRY(c, 0u);
    if (c->have_replicas && nrep != c->nrep) free_replica_buffers(c);
    c->nrep = nrep; c->seed = seed; c->first_rep = first_replica;
    const size_t nf = c->rep_floats * nrep;
    if (!c->have_replicas) {
        drop_graphs(c);
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipMalloc(&c->buf.X[k], sizeof(float) * nf));
            HIP_TRY(hipMalloc(&c->buf.V[k], sizeof(float) * nf));
            HIP_TRY(hipMalloc(&c->buf.P[k], sizeof(float) * 4 * (size_t)nrep * c->ntiles * c3d::kTileRows));
            HIP_TRY(hipMalloc(&c->buf.S[k], sizeof(c3d::FireState) * nrep));
        }
        HIP_TRY(hipMalloc(&c->buf.Vinit, sizeof(float) * nf));
        HIP_TRY(hipMalloc(&c->buf.E, sizeof(double) * 4 * nrep));
        HIP_TRY(hipMalloc(&c->d_feval, sizeof(float) * nf));
        // cluster kernel: the two pointer blocks (one per step parity), geometry for this (n, replicas), records
        {
            c3d::DevModel m = dev_model(c);
            m.nrep = nrep; m.nrep_g = nrep; m.rep_base = 0;
            // symmetric-tile kernels (large N): tile list and the partial-force slabs, whatever the model in force (use_sym)
            if (c->sym > 0) {
                int Q, G, od, dg;
                c3d::sym_geometry(m, &Q, &G, &od, &dg);
                std::vector<int2> tl((size_t)od + dg);
                c3d::sym_tile_list(m, tl.data());
                HIP_TRY(hipMalloc(&c->d_sym_tiles, sizeof(int2) * tl.size()));
                HIP_TRY(hipMemcpyAsync(c->d_sym_tiles, tl.data(), sizeof(int2) * tl.size(), hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipStreamSynchronize(c->stream));
                HIP_TRY(hipMalloc(&c->d_sym_scratch, sizeof(float) * c3d::sym_scratch_floats(m)));
            }
            if (int rc = plan_cluster(c)) return rc;
        }
        c->have_replicas = true;
    }
    // random coil (step b0) and Maxwell(0.5 K) velocities (deck :1646-1648), Philox keyed (seed, replica)
    const int n = c->n;
    std::vector<float> x((size_t)nrep * n * 3), v((size_t)nrep * n * 3);
    std::vector<double> v64(c->precision == 64 ? (size_t)nrep * n * 3 : 0);
    const double sigma = sqrt((double)c3d::kBoltz * 0.5 * (double)c3d::kAccel / (double)c->model.mass);
    for (int r = 0; r < nrep; ++r) {
        const uint32_t rid = first_replica + (uint32_t)r;
        std::vector<double> xd((size_t)3 * n);
        double px = 0, py = 0, pz = 0;
        for (int i = 0; i < n; ++i) {
            if (c->start_mode == 1) {
                // extended strand: the reference's template runs along x with small random y, z (`do (x=x/5.)`,
                // `do (y=random(0.5))`, `do (z=random(0.5))`, :2413-2416) and is regularised to chain geometry; for
                // beads: b0 apart along x, y and z uniform in [0, 0.5), keyed by (seed, replica, bead)
                const uint32_t ctr[4] = {(uint32_t)i, 2u, 0u, 0u};
                const uint32_t key[2] = {(uint32_t)(seed & 0xFFFFFFFFu) ^ (rid * 0x9E3779B9u), (uint32_t)(seed >> 32) + rid};
                uint32_t u[4];
                philox4x32(ctr, key, u);
                xd[3 * i] = (double)c->model.b0 * i; xd[3 * i + 1] = 0.5 * u01(u[0]); xd[3 * i + 2] = 0.5 * u01(u[1]);
                continue;
            }
            if (i > 0) {
                double g[4];
                normals4(seed, rid, (uint32_t)i, 0u, g);
                double nrm = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                if (nrm < 1e-12) { g[0] = 1; g[1] = g[2] = 0; nrm = 1; }
                px += (double)c->model.b0 * g[0] / nrm; py += (double)c->model.b0 * g[1] / nrm; pz += (double)c->model.b0 * g[2] / nrm;
            }
            xd[3 * i] = px; xd[3 * i + 1] = py; xd[3 * i + 2] = pz;
        }
        double cx = 0, cy = 0, cz = 0;
        for (int i = 0; i < n; ++i) { cx += xd[3 * i]; cy += xd[3 * i + 1]; cz += xd[3 * i + 2]; }
        cx /= n; cy /= n; cz /= n;
        for (int i = 0; i < n; ++i) {
            x[((size_t)r * n + i) * 3 + 0] = (float)(xd[3 * i] - cx);
            x[((size_t)r * n + i) * 3 + 1] = (float)(xd[3 * i + 1] - cy);
            x[((size_t)r * n + i) * 3 + 2] = (float)(xd[3 * i + 2] - cz);
            double g[4];
            normals4(seed, rid, (uint32_t)i, 1u, g);
            v[((size_t)r * n + i) * 3 + 0] = (float)(sigma * g[0]);
            v[((size_t)r * n + i) * 3 + 1] = (float)(sigma * g[1]);
            v[((size_t)r * n + i) * 3 + 2] = (float)(sigma * g[2]);
            if (!v64.empty()) for (int k = 0; k < 3; ++k) v64[((size_t)r * n + i) * 3 + k] = sigma * g[k];
        }
    }
    std::vector<float> soa;
    pack(c, x.data(), soa, true);
    HIP_TRY(hipMemcpyAsync(c->buf.X[0], soa.data(), sizeof(float) * nf, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpyAsync(c->buf.X[1], soa.data(), sizeof(float) * nf, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    pack(c, v.data(), soa, false);
    HIP_TRY(hipMemcpyAsync(c->buf.Vinit, soa.data(), sizeof(float) * nf, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipMemsetAsync(c->buf.V[k], 0, sizeof(float) * nf, c->stream));
        HIP_TRY(hipMemsetAsync(c->buf.P[k], 0, sizeof(float) * 4 * (size_t)nrep * c->ntiles * c3d::kTileRows, c->stream));
        HIP_TRY(hipMemsetAsync(c->buf.S[k], 0, sizeof(c3d::FireState) * nrep, c->stream));
    }
    HIP_TRY(hipMemsetAsync(c->d_feval, 0, sizeof(float) * nf, c->stream));
    // The seven fills above are waited for here.  Left in flight behind the call, they made the first synchronisation after the first multi-step
    // launch of a process — the minimiser's first exit test — take 8 ms instead of 0.02 (first anneal 21 against 12.7 ms; measured with
    // tools/host_phase_times.py, profiles/r04_first_job_latency.txt; the mechanism inside the runtime was not pursued).
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->pc = 0; c->parity = 0; c->steps_done = 0;
    if (c->precision == 64) {
        const int np = c3d::cols64(n);
        const size_t n3 = (size_t)nrep * 3 * np, nP = (size_t)nrep * c->ntiles * 4;
        if (!c->b64.T) {
            HIP_TRY(hipMalloc(&c->b64.t10, sizeof(int32_t) * (size_t)n * n));
            if (!c->h_dist10.empty())
                HIP_TRY(hipMemcpyAsync(c->b64.t10, c->h_dist10.data(), sizeof(int32_t) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
            else {                                  // c3d_set_restraints' list, scattered on the device (no n x n matrix on the host)
                const size_t R = c->r_t10.size();
                DevTmp<int32_t> dl;
                HIP_TRY(hipMalloc(&dl.p, sizeof(int32_t) * 3 * R));
                HIP_TRY(hipMemcpyAsync(dl.p, c->r_i.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipMemcpyAsync(dl.p + R, c->r_j.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipMemcpyAsync(dl.p + 2 * R, c->r_t10.data(), sizeof(int32_t) * R, hipMemcpyHostToDevice, c->stream));
                HIP_TRY(hipMemsetAsync(c->b64.t10, 0, sizeof(int32_t) * (size_t)n * n, c->stream));
                hipError_t e = c3d::launch_tenths64(n, (int)R, dl.p, dl.p + R, dl.p + 2 * R, c->b64.t10, c->stream);
                if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 tenths: ") + hipGetErrorString(e));
                HIP_TRY(hipStreamSynchronize(c->stream));
            }
            HIP_TRY(hipMalloc(&c->b64.T, sizeof(double) * (size_t)n * np));
            HIP_TRY(hipMalloc(&c->b64.Vinit, sizeof(double) * n3));
            for (int k = 0; k < 2; ++k) {
                HIP_TRY(hipMalloc(&c->b64.X[k], sizeof(double) * n3));
                HIP_TRY(hipMalloc(&c->b64.V[k], sizeof(double) * n3));
                HIP_TRY(hipMalloc(&c->b64.P[k], sizeof(double) * nP));
                HIP_TRY(hipMalloc(&c->b64.S[k], c3d::fire_state64_bytes() * nrep));
            }
        }
        std::vector<double> vs(n3, 0.0);       // Maxwell velocities in the SoA layout [nrep][3][np]
        for (int r = 0; r < nrep; ++r)
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < 3; ++k) vs[((size_t)r * 3 + k) * np + i] = v64[((size_t)r * n + i) * 3 + k];
        HIP_TRY(hipMemcpyAsync(c->b64.Vinit, vs.data(), sizeof(double) * n3, hipMemcpyHostToDevice, c->stream));
        for (int k = 0; k < 2; ++k) {
            HIP_TRY(hipMemsetAsync(c->b64.P[k], 0, sizeof(double) * nP, c->stream));
            HIP_TRY(hipMemsetAsync(c->b64.S[k], 0, c3d::fire_state64_bytes() * nrep, c->stream));
        }
        int rc = build_targets64(c);                // every time: the model may have changed since the last call
        if (rc) return rc;
        rc = import64(c);
        if (rc) return rc;
    }
    return C3D_OK;
}

// A7: the lower bound of pairs without a restraint, the last stage's repel contact distance (formed in float)
static float dg_lower(const c3d_ctx* c) {
    float repel_s = 0.85f;
    if (!c->stages.empty()) repel_s = c->stages.back().repel_s;
    return repel_s * c->model.r0_rep;
}

// A7: replace the replicas' starting coordinates by a metric-matrix distance-geometry embedding
// (deck :1471-1525 restated for beads; one embed per model, trial distances keyed by replica id)
extern "C" int c3d_embed_replicas(c3d_ctx* c, int iters) {
    if (!c || iters < 1) return fail(C3D_ERR_INVALID, "c3d_embed_replicas: bad arguments");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_embed_replicas: call c3d_init_replicas first");
    static_assert(c3d::kDgEigMaxBeads == C3D_EMBED_MAX_BEADS_DEFAULT, "the default limit is k_dg_eig's");
    if (c->n > c->embed_max_beads) {               // on the host, before any launch
        if (c->embed_max_beads == C3D_EMBED_MAX_BEADS_DEFAULT)
            return fail(C3D_ERR_INVALID, "c3d_embed_replicas: " + std::to_string(c->n) + " beads; at most " +
                                             std::to_string(C3D_EMBED_MAX_BEADS_DEFAULT) + " (k_dg_eig keeps 9 n + 16 floats in 160 KiB of LDS)" +
                                             " unless c3d_set_option(\"embed_max_beads\", n) allows the tiled eigen stage more (up to " +
                                             std::to_string(C3D_EMBED_MAX_BEADS_LIMIT) + ")");
        return fail(C3D_ERR_INVALID, "c3d_embed_replicas: " + std::to_string(c->n) + " beads: more than embed_max_beads = " +
                                         std::to_string(c->embed_max_beads) + " (the option goes up to " +
                                         std::to_string(C3D_EMBED_MAX_BEADS_LIMIT) + ")");
    }
    C3D_ENTRY(c, unit_bit(UNIT_EMBED));
    const int n = c->n, nrep = c->nrep;
    const size_t nn = (size_t)n * n;
    const bool tiled = c->embed_form == 1 || n > c3d::kDgEigMaxBeads;
    // replicas per batch: as many trial-distance matrices as C3D_EMBED_SCRATCH_BYTES hold, one at least (65535: a grid's y extent)
    size_t fit = (size_t)C3D_EMBED_SCRATCH_BYTES / (sizeof(float) * nn);
    if (c->embed_batch > 0) fit = (size_t)c->embed_batch;
    const int batch = (int)std::min<size_t>(std::max<size_t>(fit, 1), (size_t)std::min(nrep, 65535));
    DevTmp<float> U, L, D2, v0, wt;
    HIP_TRY(hipMalloc(&U.p, sizeof(float) * nn));
    HIP_TRY(hipMalloc(&L.p, sizeof(float) * nn));
    HIP_TRY(hipMalloc(&D2.p, sizeof(float) * nn * batch));
    HIP_TRY(hipMalloc(&v0.p, sizeof(float) * 3 * n * nrep));
    if (tiled) HIP_TRY(hipMalloc(&wt.p, sizeof(float) * 2 * 3 * n * batch));
    std::vector<float> hv((size_t)3 * n * nrep);
    for (int r = 0; r < nrep; ++r)
        for (int i = 0; i < n; ++i) {
            double g[4];
            normals4(c->seed, c->first_rep + (uint32_t)r, (uint32_t)i, 3u, g);
            for (int k = 0; k < 3; ++k) hv[((size_t)r * 3 + k) * n + i] = (float)g[k];
        }
    HIP_TRY(hipMemcpyAsync(v0.p, hv.data(), sizeof(float) * hv.size(), hipMemcpyHostToDevice, c->stream));
    hipError_t e = c3d::launch_dg_smooth(c->buf.tgt, n, c->npad, c->model.b0, dg_lower(c), U.p, L.p, c->stream);
    if (e == hipSuccess)
        e = c3d::launch_dg_embed(U.p, L.p, n, c->npad, nrep, c->seed, c->first_rep, iters, v0.p, D2.p, wt.p, c->buf.X[0], c->buf.X[1],
                                 tiled, batch, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("embed launch: ") + hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_embed_form = tiled ? 1 : 0;
    c->last_embed_batches = (nrep + batch - 1) / batch;
    if (c->precision == 64) return import64(c);
    return C3D_OK;
}

// test hook: the smoothed bounds c3d_embed_replicas embeds from (no LDS limit: the smoothing keeps 32 x 32 tiles)
extern "C" int c3d_dg_smoothed_bounds(c3d_ctx* c, float* U_out, float* L_out) {
    if (!c || !U_out || !L_out) return fail(C3D_ERR_INVALID, "c3d_dg_smoothed_bounds: null argument");
    if (!c->have_targets) return fail(C3D_ERR_INVALID, "c3d_dg_smoothed_bounds: set the IF matrix / restraints first");
    C3D_ENTRY(c, unit_bit(UNIT_EMBED));
    const int n = c->n;
    const size_t nn = (size_t)n * n;
    DevTmp<float> U, L;
    HIP_TRY(hipMalloc(&U.p, sizeof(float) * nn));
    HIP_TRY(hipMalloc(&L.p, sizeof(float) * nn));
    hipError_t e = c3d::launch_dg_smooth(c->buf.tgt, n, c->npad, c->model.b0, dg_lower(c), U.p, L.p, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("smoothing launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(U_out, U.p, sizeof(float) * nn, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(L_out, L.p, sizeof(float) * nn, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

extern "C" int c3d_set_coords(c3d_ctx* c, const float* xyz) {
    if (!c || !xyz) return fail(C3D_ERR_INVALID, "c3d_set_coords: null argument");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_set_coords: call c3d_init_replicas first");
    C3D_ENTRY(c, 0u);
    std::vector<float> soa;
    pack(c, xyz, soa, true);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpyAsync(c->buf.X[c->parity], soa.data(), sizeof(float) * soa.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->precision == 64) return import64(c);
    return C3D_OK;
}
static int get_soa(c3d_ctx* c, const float* dev, float* aos) {
    if (int rc = read_back(c, dev, sizeof(float) * c->rep_floats * c->nrep)) return rc;
    unpack(c, static_cast<const float*>(c->h_stage), aos);
    return C3D_OK;
}
extern "C" int c3d_get_coords(c3d_ctx* c, float* xyz) {
    if (!c || !xyz || !c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_get_coords: bad state");
    C3D_ENTRY(c, 0u);
    return get_soa(c, c->buf.X[c->parity], xyz);
}
extern "C" int c3d_get_velocities(c3d_ctx* c, float* v) {
    if (!c || !v || !c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_get_velocities: bad state");
    C3D_ENTRY(c, 0u);
    return get_soa(c, c->buf.V[c->parity], v);
}

// ---- the boundary of a precision-64 context in doubles ----
// what its four entries need: the fp64 state, which exists from c3d_init_replicas on a precision-64 context until the replicas are dropped
static int need_f64_state(const c3d_ctx* c, const char* fn) {
    if (!c) return fail(C3D_ERR_INVALID, std::string(fn) + ": null context");
    if (c->precision != 64)
        return fail(C3D_ERR_INVALID, std::string(fn) + ": the context holds no fp64 state: its precision is 32 (set precision 64 before c3d_init_replicas)");
    if (!c->have_replicas || !c->b64.X[0])
        return fail(C3D_ERR_INVALID, std::string(fn) + ": the context holds no fp64 state yet: call c3d_init_replicas first");
    return C3D_OK;
}
// SoA doubles [nrep][3][np] on the device -> [nrep][n][3] of the caller, through the pinned stage: every value as it is
static int get_soa64(c3d_ctx* c, const double* dev, double* aos) {
    const int n = c->n, np = c3d::cols64(n);
    if (int rc = read_back(c, dev, sizeof(double) * (size_t)c->nrep * 3 * np)) return rc;
    const double* h = static_cast<const double*>(c->h_stage);
    for (int r = 0; r < c->nrep; ++r)
        for (int comp = 0; comp < 3; ++comp) {
            const double* src = h + ((size_t)r * 3 + comp) * np;
            for (int i = 0; i < n; ++i) aos[((size_t)r * n + i) * 3 + comp] = src[i];
        }
    return C3D_OK;
}
extern "C" int c3d_get_coords_f64(c3d_ctx* c, double* xyz) {
    if (int rc = need_f64_state(c, "c3d_get_coords_f64")) return rc;
    if (!xyz) return fail(C3D_ERR_INVALID, "c3d_get_coords_f64: null buffer");
    C3D_ENTRY(c, unit_bit(UNIT_F64));
    return get_soa64(c, c->b64.X[c->parity], xyz);
}
extern "C" int c3d_get_velocities_f64(c3d_ctx* c, double* v) {
    if (int rc = need_f64_state(c, "c3d_get_velocities_f64")) return rc;
    if (!v) return fail(C3D_ERR_INVALID, "c3d_get_velocities_f64: null buffer");
    C3D_ENTRY(c, unit_bit(UNIT_F64));
    return get_soa64(c, c->b64.V[c->parity], v);
}
// c3d_set_coords + import64 without the pass through floats: both parities of X = these doubles (padding beads as k64_import places them),
// both parities of V zero, then the float mirror of the current parity through the existing export
extern "C" int c3d_set_coords_f64(c3d_ctx* c, const double* xyz) {
    if (int rc = need_f64_state(c, "c3d_set_coords_f64")) return rc;
    if (!xyz) return fail(C3D_ERR_INVALID, "c3d_set_coords_f64: null buffer");
    const int n = c->n, np = c3d::cols64(n);
    const size_t cnt = (size_t)c->nrep * n * 3, n3 = (size_t)c->nrep * 3 * np;
    for (size_t k = 0; k < cnt; ++k)
        if (!std::isfinite(xyz[k])) return fail(C3D_ERR_INVALID, "c3d_set_coords_f64: non-finite coordinate; nothing was copied");
    C3D_ENTRY(c, unit_bit(UNIT_F64));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = ensure_stage(c, sizeof(double) * n3)) return rc;
    double* h = static_cast<double*>(c->h_stage);
    for (int r = 0; r < c->nrep; ++r)
        for (int comp = 0; comp < 3; ++comp) {
            double* dst = h + ((size_t)r * 3 + comp) * np;
            for (int i = 0; i < n; ++i) dst[i] = xyz[((size_t)r * n + i) * 3 + comp];
            for (int i = n; i < np; ++i) dst[i] = (double)c3d::kPadCoord * (comp + 1) + 16.0 * (i - n);
        }
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipMemcpyAsync(c->b64.X[k], h, sizeof(double) * n3, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->b64.V[k], 0, sizeof(double) * n3, c->stream));
    }
    hipError_t e = c3d::launch_export64(dev_model(c), c->b64, c->parity, c->buf.X[c->parity], c->buf.V[c->parity], c->buf.P[c->parity], c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 export: ") + hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

extern "C" long c3d_schedule_length(const c3d_ctx* c) {
    if (!c) return 0;
    long n = 0;
    for (const Op& op : c->program) n += op.counted;
    return n;
}
extern "C" long c3d_steps_done(const c3d_ctx* c) { return c ? c->steps_done : 0; }

extern "C" int c3d_run_steps(c3d_ctx* c, long nsteps, long* done) {
    if (!c || nsteps < 0) return fail(C3D_ERR_INVALID, "c3d_run_steps: bad arguments");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_run_steps: call c3d_init_replicas first");
    C3D_ENTRY(c, 0u);
    // number of program ops that contain exactly nsteps counted steps (or the rest of the program)
    size_t nops = 0;
    long counted = 0;
    while (c->pc + nops < c->program.size() && counted < nsteps) {
        counted += c->program[c->pc + nops].counted;
        ++nops;
    }
    int rc = begin_timing(c);
    if (rc) return rc;
    rc = run_ops(c, nops);
    if (rc) return rc;
    rc = end_timing(c);
    if (rc) return rc;
    if (done) *done = counted;
    return C3D_OK;
}

extern "C" int c3d_centre(c3d_ctx* c) {
    if (!c || !c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_centre: bad state");
    C3D_ENTRY(c, 0u);
    hipError_t e = c3d::launch_centre(dev_model(c), c->buf, c->parity, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("centre launch: ") + hipGetErrorString(e));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

extern "C" int c3d_run(c3d_ctx* c) {
    if (!c) return fail(C3D_ERR_INVALID, "c3d_run: null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_run: call c3d_init_replicas first");
    C3D_ENTRY(c, 0u);
    int rc = begin_timing(c);
    if (rc) return rc;
    const int last_stage = (int)c->stages.size() - 1;
    const bool early = c->gtol > 0.0f && last_stage >= 0 && (c->stages[last_stage].kind == 2 || c->stages[last_stage].kind == 5 || c->stages[last_stage].kind == 8);
    // everything before the final minimisation
    size_t nfixed = c->program.size() - c->pc;
    if (early) {
        nfixed = 0;
        while (c->pc + nfixed < c->program.size() && c->program[c->pc + nfixed].stage != last_stage) ++nfixed;
    }
    rc = run_ops(c, nfixed);
    if (rc) return rc;
    if (early) {
        // chunks of check_every steps until every replica's RMS force < gtol
        while (c->pc < c->program.size()) {
            const size_t chunk = std::min<size_t>((size_t)(c->check_every & ~1), c->program.size() - c->pc);
            rc = run_ops(c, chunk);
            if (rc) return rc;
            double rms = 0;
            rc = max_rms_force(c, &rms);
            if (rc) return rc;
            if (rms < c->gtol) break;
        }
        c->pc = c->program.size();
    }
    hipError_t e = c3d::launch_centre(dev_model(c), c->buf, c->parity, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("centre launch: ") + hipGetErrorString(e));
    c->ev1_recorded = false;                       // work was queued behind the last multi-step launch
    rc = end_timing(c);
    if (rc) return rc;
    // a blown-up trajectory (NaN/Inf) must not reach the caller as a "model"
    bool finite = true;
    rc = partials_finite(c, &finite);
    if (rc) return rc;
    if (!finite) return fail(C3D_ERR_DIVERGED, "c3d_run: the trajectory diverged (non-finite forces); reduce the time step or stiffness");
    return C3D_OK;
}

extern "C" int c3d_last_timing(const c3d_ctx* c, double* ms_total, long* steps, long* launches) {
    if (!c) return fail(C3D_ERR_INVALID, "c3d_last_timing: null context");
    if (ms_total) *ms_total = c->last_ms;
    if (steps) *steps = c->last_steps;
    if (launches) *launches = c->last_launches;
    return C3D_OK;
}

extern "C" int c3d_get_stat(const c3d_ctx* c, const char* key, double* value) {
    if (!c || !key || !value) return fail(C3D_ERR_INVALID, "c3d_get_stat: null argument");
    if (!strcmp(key, "graph_captures")) *value = (double)c->graph_captures;
    else if (!strcmp(key, "last_kernel_us")) *value = 1e3 * c->last_kernel_ms;
    else if (!strcmp(key, "last_host_launch_us")) *value = c->last_host_launch_us;
    else if (!strcmp(key, "last_host_sync_us")) *value = c->last_host_sync_us;
    else if (!strcmp(key, "graph_launches")) *value = (double)c->graph_launches;
    else if (!strcmp(key, "graphs_cached")) *value = (double)c->graphs.size();
    else if (!strcmp(key, "step_launches")) *value = (double)c->step_launches;
    else if (!strcmp(key, "resident_launches")) *value = (double)c->resident_launches;
    else if (!strcmp(key, "cluster_launches")) *value = (double)c->cluster_launches;
    else if (!strcmp(key, "resident_fallbacks")) *value = (double)c->resident_fallbacks;
    else if (!strcmp(key, "cluster_incomplete")) *value = (double)c->cluster_incomplete;
    else if (!strcmp(key, "spin_completions")) *value = (double)c->spin_completions;
    else if (!strcmp(key, "cluster_static_placement")) *value = c->static_place ? 1.0 : 0.0;
    else if (!strcmp(key, "cluster_placement_mismatches")) *value = (double)c->placement_mismatches;
    else if (!strcmp(key, "num_xcc")) *value = (double)c->num_xcc;
    else if (!strcmp(key, "rms_force")) {
        // max over the replicas of the RMS force component at the last minimiser evaluation (what c3d_run compares with
        // gtol); meaningful after a FIRE step only
        double rms = 0;
        if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_get_stat: rms_force needs replicas");
        C3D_ENTRY(c, 0u);
        const int rc = max_rms_force(const_cast<c3d_ctx*>(c), &rms);
        if (rc) return rc;
        *value = rms;
    }
    else if (!strcmp(key, "lbfgs_steps")) *value = (double)c->lbfgs_steps;
    else if (!strcmp(key, "lbfgs_resets")) {
        // memory drops of the last L-BFGS stage, summed over the replicas (device state of the parity its last step wrote)
        *value = 0;
        const c3d::LbfgsState* dev = c->lbfgs_parity < 0 ? nullptr : c->precision == 64 ? c->lb64.S[c->lbfgs_parity] : c->lb.S[c->lbfgs_parity];
        if (dev) {
            C3D_ENTRY(c, 0u);
            if (int rc = read_back(const_cast<c3d_ctx*>(c), dev, sizeof(c3d::LbfgsState) * c->nrep)) return rc;
            const c3d::LbfgsState* h = static_cast<const c3d::LbfgsState*>(c->h_stage);
            long r = 0;
            for (int k = 0; k < c->nrep; ++k) r += h[k].resets;
            *value = (double)r;
        }
    }
    else if (!strcmp(key, "k1_recomputed")) *value = (double)c->k1_recomputed;
    else if (!strcmp(key, "k1_patched")) *value = (double)c->k1_patched;
    else if (!strcmp(key, "last_path")) *value = (double)c->last_path;
    else if (!strcmp(key, "rank_prefetch_hits")) *value = (double)c->rank_prefetch_hits;
    else if (!strcmp(key, "device_rank_runs")) *value = (double)c->device_rank_runs;
    else if (!strcmp(key, "score_wide_runs")) *value = (double)c->score_wide_runs;
    else if (!strcmp(key, "compare_runs")) *value = (double)c->compare_runs;
    else if (!strcmp(key, "f64_evals")) *value = (double)c->f64_evals;
    else if (!strcmp(key, "superpose_runs")) *value = (double)c->superpose_runs;
    else if (!strcmp(key, "rmsd_table_runs")) *value = (double)c->rmsd_table_runs;
    else if (!strcmp(key, "cluster_xcd_count")) *value = (double)c->xcd_count;
    else if (!strcmp(key, "cluster_xcd_base")) *value = (double)c->xcd_base;
    else if (!strcmp(key, "cluster_ok")) *value = c->cl_ok ? 1.0 : 0.0;
    else if (!strcmp(key, "cluster_parts")) *value = c->cl_ok ? (double)c->cl_plan.parts : 0.0;
    else if (!strcmp(key, "cluster_rows_per_wave")) *value = c->cl_ok ? (double)c->cl_plan.rpw : 0.0;
    else if (!strcmp(key, "cluster_late_tiles")) *value = c->cl_ok ? (double)c->cl_plan.late_tiles : 0.0;
    else if (!strcmp(key, "cluster_compute_waves")) *value = c->cl_ok ? (double)c->cl_plan.cw : 0.0;
    else if (!strcmp(key, "cluster_helper_waves")) *value = c->cl_ok ? (double)c->cl_plan.helpers : 0.0;
    else if (!strcmp(key, "cluster_wgs_per_cu")) *value = c->cl_ok ? (double)c->cl_plan.wgs_per_cu : 0.0;
    else if (!strcmp(key, "replica_groups")) *value = (double)active_groups(c);
    else if (!strcmp(key, "embed_form")) *value = (double)c->last_embed_form;
    else if (!strcmp(key, "embed_batches")) *value = (double)c->last_embed_batches;
    else if (!strcmp(key, "units_loaded")) *value = (double)g_units.loads.load();                       // code objects this PROCESS has loaded (all devices)
    else if (!strcmp(key, "units_loaded_mask")) *value = (double)g_units.loaded[c->device & (kMaxDevices - 1)].load();   // bit per unit, this context's device
    else return fail(C3D_ERR_INVALID, std::string("c3d_get_stat: unknown key ") + key);
    return C3D_OK;
}

// name of the kernel the last op of the last range ran on, as rocprofv3 prints it (without the argument list): the record its launch was made from
extern "C" const char* c3d_step_kernel_name(const c3d_ctx* c) {
    static thread_local char buf[96];
    if (!c) return "";
    const KernelRecord& k = c->ran;
    auto tf = [](bool b) { return b ? "true" : "false"; };
    switch (k.family) {
        case KernelRecord::CLUSTER:
            snprintf(buf, sizeof(buf), "c3d::k_cluster%s<%d, %d, %d, %d, %s>", k.tp ? "_tp" : "", k.pot, k.rpw, k.nb, k.wl, tf(k.late));
            break;
        case KernelRecord::STEP64:
        case KernelRecord::LBFGS_EVAL64: {    // (after an fp64 L-BFGS step: its force pass, k64_lbfgs_move follows it)
            const char* kernel = k.family == KernelRecord::STEP64 ? "k64_step" : "k64_lbfgs_eval";
            if (k.f64.chunk) snprintf(buf, sizeof(buf), "c3d::%s_chunked<%d, %s, %s, %d>", kernel, k.f64.pot, tf(k.f64.gen), tf(k.f64.fold), k.f64.chunk);
            else snprintf(buf, sizeof(buf), "c3d::%s<%d, %s, %s>", kernel, k.f64.pot, tf(k.f64.gen), tf(k.f64.fold));
            break;
        }
        case KernelRecord::PAIRS_SYM: snprintf(buf, sizeof(buf), "c3d::k_pairs_sym<%d, %s, false>", k.pot, tf(k.rs1)); break;
        case KernelRecord::STEP:
        case KernelRecord::LBFGS_EVAL: {      // (after an L-BFGS step: its force pass, k_lbfgs_move follows it)
            const char* kernel = k.family == KernelRecord::STEP ? "k_step" : "k_lbfgs_eval";
            if (k.step.chunk) {               // k_*_chunked<pot, gen, rpw, tile rows, wide, CHUNK>
                if (k.step.wide) snprintf(buf, sizeof(buf), "c3d::%s_chunked<4, false, 4, 16, true, %d>", kernel, k.step.chunk);
                else snprintf(buf, sizeof(buf), "c3d::%s_chunked<%d, %s, %d, 8, false, %d>", kernel, k.step.pot, tf(k.step.gen), k.step.rpw, k.step.chunk);
            } else if (k.step.wide) snprintf(buf, sizeof(buf), "c3d::%s<4, false, 4, false, 16, true>", kernel);
            else snprintf(buf, sizeof(buf), "c3d::%s<%d, %s, %d, %s, 8, false>", kernel, k.step.pot, tf(k.step.gen), k.step.rpw, tf(k.step.nc));
            break;
        }
        default: return "";
    }
    return buf;
}

extern "C" int c3d_eval(c3d_ctx* c, float w_all, float w_vdw, float repel_s, float* F, double* e) {
    if (!c || !c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_eval: bad state");
    C3D_ENTRY(c, 0u);
    const c3d::DevModel m = dev_model(c);
    const c3d::DevStep p = dev_step(c, 3, 0.0f, w_all, w_vdw, repel_s, 0.0f);
    if (F) {
        hipError_t err = c3d::launch_eval_forces(m, p, c->buf, c->parity, c->d_feval, c3d::general_step(m, p), c->eval_rpw,
                                                 c3d::column_chunk_for(m, c->column_chunk), c->stream);
        if (err != hipSuccess) return fail(C3D_ERR_HIP, std::string("eval launch: ") + hipGetErrorString(err));
        int rc = get_soa(c, c->d_feval, F);
        if (rc) return rc;
    }
    if (e) {
        const double rr = (double)repel_s * (double)c->model.r0_rep;
        hipError_t err = c3d::launch_energy(m, p, c->buf, c->parity, c->model.s_noe, c->model.k_rep, rr * rr, c->stream);
        if (err != hipSuccess) return fail(C3D_ERR_HIP, std::string("energy launch: ") + hipGetErrorString(err));
        if (int rc = read_back(c, c->buf.E, sizeof(double) * 4 * (size_t)c->nrep)) return rc;
        const double* h = static_cast<const double*>(c->h_stage);
        for (int r = 0; r < c->nrep; ++r) for (int k = 0; k < 3; ++k) e[3 * r + k] = h[4 * r + k];
    }
    return C3D_OK;
}

// c3d_eval on the fp64 side: the fp64 kernels at the fp64 coordinates, into a buffer of the context's own; reads X[parity] and T, writes b64.F
extern "C" int c3d_eval_f64(c3d_ctx* c, double w_all, double w_vdw, double repel_s, double* F, double* e) {
    if (int rc = need_f64_state(c, "c3d_eval_f64")) return rc;
    if (!F && !e) return fail(C3D_ERR_INVALID, "c3d_eval_f64: F and e are both NULL");
    C3D_ENTRY(c, unit_bit(UNIT_F64));
    const size_t n3 = (size_t)c->nrep * 3 * c3d::cols64(c->n);
    if (!c->b64.F) HIP_TRY(hipMalloc(&c->b64.F, sizeof(double) * (n3 + 4 * (size_t)c->nrep)));
    const c3d::DevModel m = dev_model(c);
    double mh[15];
    model_host64(c, mh);
    if (F) {
        const double sh[6] = {3.0, 0.0, w_all, w_vdw, repel_s, 0.0};
        hipError_t err = c3d::launch_eval_forces64(m, mh, sh, c->b64, c->parity, c->f64_column_chunk, c->b64.F, c->stream);
        if (err != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 eval launch: ") + hipGetErrorString(err));
        if (int rc = get_soa64(c, c->b64.F, F)) return rc;
    }
    if (e) {
        const double rr = repel_s * (double)c->model.r0_rep;
        hipError_t err = c3d::launch_energy64(m, mh, rr * rr, c->b64, c->parity, c->b64.F + n3, c->stream);
        if (err != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 energy launch: ") + hipGetErrorString(err));
        if (int rc = read_back(c, c->b64.F + n3, sizeof(double) * 4 * (size_t)c->nrep)) return rc;
        const double* h = static_cast<const double*>(c->h_stage);
        for (int r = 0; r < c->nrep; ++r) for (int k = 0; k < 3; ++k) e[3 * r + k] = h[4 * r + k];
    }
    ++c->f64_evals;
    return C3D_OK;
}

extern "C" int c3d_get_energies(c3d_ctx* c, double* e) {
    if (!c || !e) return fail(C3D_ERR_INVALID, "c3d_get_energies: null argument");
    float repel_s = 0.85f;
    if (!c->stages.empty()) repel_s = c->stages.back().repel_s;
    return c3d_eval(c, 1.0f, 1.0f, repel_s, nullptr, e);
}

// c3d_score_replicas' scratch inside d_score (byte offsets): the rank matrix (which first holds the matrix itself when the device ranks it),
// rounded coordinates, per-row sums, the two fixed histograms, the overflow flag, the replicas' bounding boxes (read by the re-run of a
// wide call only) and, when the device ranks, the sort keys, the per-row sums of squares and the asymmetry flag
struct ScoreScratch {
    size_t rank = 0, xr = 0, part = 0, hist = 0, below = 0, ovf = 0, box = 0, keys = 0, saa = 0, asym = 0, total = 0;
};
static ScoreScratch score_layout(int n, int nrep, unsigned nbins, size_t key_slots) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_rank = up(sizeof(double) * (size_t)n * n), b_xr = up(sizeof(double) * 3 * (size_t)n * nrep), b_part = up(sizeof(double) * 4 * (size_t)n * nrep),
                 b_hist = up(sizeof(unsigned) * (size_t)nbins * nrep);
    ScoreScratch L;
    L.xr = b_rank; L.part = L.xr + b_xr; L.hist = L.part + b_part; L.below = L.hist + b_hist; L.ovf = L.below + b_hist;
    L.box = L.ovf + 256;
    L.total = L.box + up(sizeof(double) * 6 * (size_t)nrep);
    if (key_slots) {
        L.keys = L.total; L.saa = L.keys + up(sizeof(unsigned long long) * key_slots); L.asym = L.saa + up(sizeof(double) * (size_t)n);
        L.total = L.asym + 256;
    }
    return L;
}
// one scratch allocation the context keeps (a hipMalloc / hipFree pair of the two 21 MB histograms alone cost about a millisecond per call)
static int score_scratch(c3d_ctx* c, size_t need) {
    if (need <= c->d_score_bytes) return C3D_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    dev_free(c->d_score);
    c->d_score_bytes = 0;
    HIP_TRY(hipMalloc(&c->d_score, need));
    c->d_score_bytes = need;
    return C3D_OK;
}
// pairs i < j, j - i >= range, of an n x n matrix: half the ranked multiset
static size_t rank_half_pairs(int n, int range) {
    const size_t w = n > range ? (size_t)(n - range) : 0;
    return w * (w + 1) / 2;
}

// The IF ranks on the device (c3d_score.hip k_rank_*): the matrix goes into the rank slot of the scratch and is ranked there.  *symmetric =
// false (and nothing else) when M(i,j) != M(j,i) for a ranked pair: the caller ranks on the host.  saa = the n row sums added in index order.
static int device_if_ranks(c3d_ctx* c, const double* IF, int range, const ScoreScratch& L, size_t mh, size_t slots, double* saa, bool* symmetric) {
    const int n = c->n;
    char* const base = static_cast<char*>(c->d_score);
    double* const d_rank = reinterpret_cast<double*>(base + L.rank);
    unsigned long long* const d_keys = reinterpret_cast<unsigned long long*>(base + L.keys);
    HIP_TRY(hipMemcpyAsync(d_rank, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
    hipError_t e = c3d::launch_if_rank_keys(d_rank, n, range, d_keys, mh, slots, reinterpret_cast<int*>(base + L.asym), c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("rank key launch: ") + hipGetErrorString(e));
    if (int rc = read_back(c, base + L.asym, sizeof(int))) return rc;
    *symmetric = *static_cast<const int*>(c->h_stage) == 0;
    if (!*symmetric) return C3D_OK;
    const double ma = 0.5 * (2.0 * (double)mh + 1.0);
    e = c3d::launch_if_rank_sort(d_rank, n, range, d_keys, mh, slots, ma, reinterpret_cast<double*>(base + L.saa), c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("rank sort launch: ") + hipGetErrorString(e));
    if (int rc = read_back(c, base + L.saa, sizeof(double) * (size_t)n)) return rc;
    const double* const rows = static_cast<const double*>(c->h_stage);
    double sum = 0;
    for (int i = 0; i < n; ++i) sum += rows[i];      // fixed order: deterministic
    *saa = sum;
    return C3D_OK;
}

// test hook: the rank matrix, m and saa as the device computes them for c3d_score_replicas (whatever the option device_ranks says)
extern "C" int c3d_debug_if_ranks(c3d_ctx* c, const double* IF, int range, double* rank, double* saa, size_t* m) {
    if (!c || !IF || !rank || !saa || !m || range < 1) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: bad arguments");
    if (!c->have_targets) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: set the IF matrix / restraints first");
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int n = c->n;
    const size_t mh = rank_half_pairs(n, range), slots = c3d::if_rank_key_slots(mh);
    if (mh < 1) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: range leaves no pairs");
    const ScoreScratch L = score_layout(n, c->have_replicas ? c->nrep : 0, 1u << 18, slots);
    if (int rc = score_scratch(c, L.total)) return rc;
    bool symmetric = false;
    if (int rc = device_if_ranks(c, IF, range, L, mh, slots, saa, &symmetric)) return rc;
    if (!symmetric) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: the matrix is not symmetric over the ranked pairs (the host ranks such a matrix)");
    HIP_TRY(hipMemcpyAsync(rank, static_cast<char*>(c->d_score) + L.rank, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *m = 2 * mh;
    return C3D_OK;
}

// K6 on the device: count_satisfied_tbl_rows / sum_noe_dev (:447-485, :581-600) and, when IF is given,
// spearman_IF_pdb.pl's coefficient for every replica, from the coordinates resident on the GPU.
// Distances are histogrammed in 2^18 bins of 0.001 A; a call in which a pair is further apart is scored again with a histogram sized to
// the models (below).  The IF ranks come from the helper thread of c3d_set_if_matrix, from c3d::if_pair_ranks or from the device (option
// device_ranks; c3d.h).
extern "C" int c3d_score_replicas(c3d_ctx* c, const double* IF, int range, int32_t* satisfied, double* sum_dev, double* rho) {
    if (!c || range < 1) return fail(C3D_ERR_INVALID, "c3d_score_replicas: bad arguments");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_score_replicas: call c3d_init_replicas first");
    if (rho && !IF) return fail(C3D_ERR_INVALID, "c3d_score_replicas: the Spearman coefficient needs the IF matrix");
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int n = c->n, nrep = c->nrep;
    const unsigned nbins = 1u << 18;      // distances up to 262 A in thousandths
    std::vector<double> rankA;
    size_t m = 0;
    double ma = 0, saa = 0;
    const bool spearman = IF && rho;
    // the ranks c3d_set_if_matrix started on its helper thread, if this is the same matrix (same numbers: memcmp) and range
    bool prefetched = false;
    if (spearman) {
        c->ifr.join();
        prefetched = c->ifr.valid && c->ifr.n == n && c->ifr.range == range && c->ifr.matrix.size() == (size_t)n * n &&
                     memcmp(c->ifr.matrix.data(), IF, sizeof(double) * (size_t)n * n) == 0;
    }
    // device_ranks: 1 = the device ranks every symmetric matrix, 0 = those beyond the default bead limit that no prefetch covers, -1 = none
    const bool try_device = spearman && (c->device_ranks > 0 || (c->device_ranks == 0 && n > C3D_MAX_BEADS_DEFAULT && !prefetched));
    const size_t mh = rank_half_pairs(n, range), slots = try_device ? c3d::if_rank_key_slots(mh) : 0;
    const ScoreScratch L = score_layout(n, nrep, nbins, slots);
    if (int rc = score_scratch(c, L.total)) return rc;
    char* const base = static_cast<char*>(c->d_score);
    struct { double* p; } d_rank{reinterpret_cast<double*>(base + L.rank)}, d_xr{reinterpret_cast<double*>(base + L.xr)}, d_part{reinterpret_cast<double*>(base + L.part)};
    struct { unsigned* p; } d_hist{reinterpret_cast<unsigned*>(base + L.hist)}, d_below{reinterpret_cast<unsigned*>(base + L.below)};
    struct { int* p; } d_ovf{reinterpret_cast<int*>(base + L.ovf)};
    if (spearman) {
        bool ranked = false;
        if (try_device) {
            if (2 * mh < 2) return fail(C3D_ERR_INVALID, "c3d_score_replicas: range leaves no pairs");
            if (int rc = device_if_ranks(c, IF, range, L, mh, slots, &saa, &ranked)) return rc;
            if (ranked) { m = 2 * mh; ma = 0.5 * ((double)m + 1.0); ++c->device_rank_runs; }
        }
        if (!ranked) {
            const std::vector<double>* ranks = &rankA;
            if (prefetched && c->device_ranks <= 0) {
                ranks = &c->ifr.rank; m = c->ifr.m; ma = c->ifr.mean; saa = c->ifr.saa;
                ++c->rank_prefetch_hits;
            } else {
                c3d::if_pair_ranks(IF, n, range, rankA, m, ma, saa);
            }
            if (m < 2) return fail(C3D_ERR_INVALID, "c3d_score_replicas: range leaves no pairs");
            HIP_TRY(hipMemcpyAsync(d_rank.p, ranks->data(), sizeof(double) * ranks->size(), hipMemcpyHostToDevice, c->stream));
        }
    }
    else d_rank.p = nullptr;
    const double mb = 0.5 * ((double)m + 1.0);     // mean of the ranks 1..m, ties or not
    hipError_t e = c3d::launch_score(c->buf.X[c->parity], c->buf.tgt, d_rank.p, n, c->npad, nrep, range, c->model.min_sep, nbins, ma,
                                     mb, 0.5, d_xr.p, d_hist.p, d_below.p, d_part.p, d_ovf.p, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("score launch: ") + hipGetErrorString(e));
    const size_t part_bytes = sizeof(double) * 4 * (size_t)n * nrep;
    if (int rc = ensure_stage(c, part_bytes + 64)) return rc;
    char* stage = static_cast<char*>(c->h_stage);
    HIP_TRY(hipMemcpyAsync(stage, d_part.p, part_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stage + part_bytes, d_ovf.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (*reinterpret_cast<const int*>(stage + part_bytes)) {
        // A pair lies beyond the fixed histogram: the same kernels again with a histogram that holds the bounding box of the widest
        // replica's rounded coordinates (the diagonal bounds every pair distance), replicas in batches whose two histograms fit
        // C3D_SCORE_SCRATCH_BYTES.  Replicas are independent and the histogram is integer: same numbers whatever the batch, and for a
        // replica that fitted the fixed histogram the numbers of the first pass.  Up to 50 000 A, the limit of c3d_spearman_if_dist_batch:
        // a box wider than that along one axis holds such a pair for certain (the two beads at its ends) and is refused at once; a box whose
        // diagonal alone is longer may hold none (the host accepts such a model), so it gets the largest histogram and the pass decides.
        constexpr unsigned kMaxBins = 50000001u;             // distances 0 .. 50 000.000 A in thousandths
        const char* const too_far = "c3d_score_replicas: a pair distance exceeds 50000 A (the limit of device and host scoring)";
        double* const d_box = reinterpret_cast<double*>(base + L.box);
        e = c3d::launch_score_bbox(d_xr.p, n, nrep, d_box, c->stream);
        if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("score launch: ") + hipGetErrorString(e));
        if (int rc = read_back(c, d_box, sizeof(double) * 6 * (size_t)nrep)) return rc;
        const double* const hb = static_cast<const double*>(c->h_stage);
        double widest = 0;
        for (int r = 0; r < nrep; ++r) {
            double d2 = 0;
            for (int k = 0; k < 3; ++k) {
                const double w = hb[6 * r + 2 * k + 1] - hb[6 * r + 2 * k];
                if (!(w <= 50000.001)) return fail(C3D_ERR_INVALID, too_far);      // also an infinite coordinate
                d2 += w * w;
            }
            widest = std::max(widest, sqrt(d2));
        }
        const double want = ceil(1000.0 * widest) + 2.0;
        const unsigned wbins = want <= (double)kMaxBins ? (unsigned)want : kMaxBins;
        const size_t per_rep = 2 * sizeof(unsigned) * (size_t)wbins;
        const int batch = (int)std::min<size_t>((size_t)nrep, std::max<size_t>(1, (size_t)C3D_SCORE_SCRATCH_BYTES / per_rep));
        DevTmp<unsigned> wide;
        HIP_TRY(hipMalloc(&wide.p, per_rep * batch));
        HIP_TRY(hipMemsetAsync(d_ovf.p, 0, sizeof(int), c->stream));
        for (int r0 = 0; r0 < nrep; r0 += batch) {
            const int nb = std::min(batch, nrep - r0);
            e = c3d::launch_score_wide(d_xr.p + (size_t)r0 * 3 * n, c->buf.tgt, d_rank.p, n, c->npad, nb, range, c->model.min_sep, wbins, ma, mb, 0.5,
                                       wide.p, wide.p + (size_t)wbins * batch, d_part.p + (size_t)r0 * n * 4, d_ovf.p, c->stream);
            if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("score launch: ") + hipGetErrorString(e));
        }
        if (int rc = ensure_stage(c, part_bytes + 64)) return rc;
        stage = static_cast<char*>(c->h_stage);
        HIP_TRY(hipMemcpyAsync(stage, d_part.p, part_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(stage + part_bytes, d_ovf.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (*reinterpret_cast<const int*>(stage + part_bytes)) return fail(C3D_ERR_INVALID, too_far);
        ++c->score_wide_runs;
    }
    const double* const part = reinterpret_cast<const double*>(stage);
    for (int r = 0; r < nrep; ++r) {
        double sab = 0, sbb = 0, sat = 0, dev = 0;
        for (int i = 0; i < n; ++i) {    // fixed order: deterministic
            const double* q = part + ((size_t)r * n + i) * 4;
            sab += q[0]; sbb += q[1]; sat += q[2]; dev += q[3];
        }
        if (satisfied) satisfied[r] = (int32_t)llround(sat);
        if (sum_dev) sum_dev[r] = dev;
        if (rho) rho[r] = sab / sqrt(saa * sbb);
    }
    return C3D_OK;
}

// c3d_compare_replicas' scratch (byte offsets into one allocation of the call): the models' fp64 coordinates, k + e of every pair and model,
// the sort keys of one model, the row sums of the distances, their totals, the table pass's per-chunk sums and the two tables
struct CompareScratch {
    size_t xyz = 0, ke = 0, keys = 0, rowsum = 0, sums = 0, partial = 0, table = 0, total = 0;
};
static CompareScratch compare_layout(int n, int K, size_t m, size_t slots) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nb = (size_t)(K + c3d::kCmpModels - 1) / c3d::kCmpModels;
    CompareScratch L;
    L.ke = up(sizeof(double) * 3 * (size_t)n * K);
    L.keys = L.ke + up(sizeof(unsigned) * m * K);
    L.rowsum = L.keys + up(sizeof(unsigned long long) * slots);
    L.sums = L.rowsum + up(sizeof(double) * (size_t)n * K);
    L.partial = L.sums + up(sizeof(double) * (size_t)K);
    L.table = L.partial + up(sizeof(double) * 512 * nb * nb * (size_t)c3d::compare_table_chunks(m, K));
    L.total = L.table + up(sizeof(double) * 2 * (size_t)K * K);
    return L;
}
// the call's scratch: freed when `tmp` goes, whatever the exit path
static int compare_alloc(DevTmp<char>& tmp, size_t bytes, const char* who) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&tmp.p), bytes);
    if (e == hipSuccess) return C3D_OK;
    tmp.p = nullptr;
    (void)hipGetLastError();
    char msg[160];
    snprintf(msg, sizeof msg, "%s: no device memory for %zu bytes of scratch (%s)", who, bytes, hipGetErrorString(e));
    return fail(e == hipErrorOutOfMemory ? C3D_ERR_NOMEM : C3D_ERR_HIP, msg);
}

// The replicas (and n_extra models given by the caller) against one another: c3d_model_similarity for every ordered pair, on the device
// (c3d_score.hip k_cmp_*).  Reads X[parity] only.
extern "C" int c3d_compare_replicas(c3d_ctx* c, const double* extra_xyz, int n_extra, double* spearman, double* rmsd) {
    if (!c) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: call c3d_init_replicas first");
    if (c->n < 3) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: models of fewer than 3 beads have no distances to rank");
    if (n_extra < 0 || (n_extra > 0 && !extra_xyz)) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: n_extra < 0, or extra models without coordinates");
    if ((long)c->nrep + n_extra > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: more than C3D_COMPARE_MAX_MODELS models");
    if (!spearman && !rmsd) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: both outputs are NULL");
    const int n = c->n, nrep = c->nrep, K = nrep + n_extra;
    if (n_extra > 0)
        if (int rc = c3d::check_model_coords(extra_xyz, (size_t)3 * n * n_extra, "c3d_compare_replicas")) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const size_t m = (size_t)n * (n - 1) / 2, slots = c3d::if_rank_key_slots(m);
    const CompareScratch L = compare_layout(n, K, m, slots);
    DevTmp<char> tmp;
    if (int rc = compare_alloc(tmp, L.total, "c3d_compare_replicas")) return rc;
    double* const d_xyz = reinterpret_cast<double*>(tmp.p + L.xyz);
    unsigned* const d_ke = reinterpret_cast<unsigned*>(tmp.p + L.ke);
    double* const d_rowsum = reinterpret_cast<double*>(tmp.p + L.rowsum);
    double* const d_table = reinterpret_cast<double*>(tmp.p + L.table);
    hipError_t e = c3d::launch_compare_coords(c->buf.X[c->parity], n, c->npad, nrep, d_xyz, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("compare launch: ") + hipGetErrorString(e));
    if (n_extra > 0)
        HIP_TRY(hipMemcpyAsync(d_xyz + (size_t)3 * n * nrep, extra_xyz, sizeof(double) * 3 * (size_t)n * n_extra, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < K; ++k) {
        e = c3d::launch_compare_ranks(d_xyz + (size_t)3 * n * k, n, reinterpret_cast<unsigned long long*>(tmp.p + L.keys), m, slots, d_ke + m * k,
                                      d_rowsum + (size_t)n * k, c->stream);
        if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("compare launch: ") + hipGetErrorString(e));
    }
    e = c3d::launch_compare_table(d_xyz, d_ke, d_rowsum, n, K, m, reinterpret_cast<double*>(tmp.p + L.sums),
                                  reinterpret_cast<double*>(tmp.p + L.partial), d_table, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("compare launch: ") + hipGetErrorString(e));
    if (int rc = read_back(c, d_table, sizeof(double) * 2 * (size_t)K * K)) return rc;
    // the centred ranks' sum of squares of a model is its own diagonal entry, summed in the order of every other entry: a model against a
    // copy of itself gives exactly 1
    const double* const t = static_cast<const double*>(c->h_stage);
    for (int a = 0; a < K; ++a)
        for (int b = 0; b < K; ++b) {
            const size_t q = (size_t)a * K + b;
            if (spearman) spearman[q] = t[2 * q] / sqrt(t[2 * ((size_t)a * K + a)] * t[2 * ((size_t)b * K + b)]);
            if (rmsd) rmsd[q] = sqrt(t[2 * q + 1] / (double)m);
        }
    ++c->compare_runs;
    return C3D_OK;
}

// test hook: the average ranks of one replica's distances as c3d_compare_replicas' kernels compute them
extern "C" int c3d_debug_distance_ranks(c3d_ctx* c, int replica, double* rank) {
    if (!c || !rank) return fail(C3D_ERR_INVALID, "c3d_debug_distance_ranks: null argument");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_debug_distance_ranks: call c3d_init_replicas first");
    if (c->n < 3) return fail(C3D_ERR_INVALID, "c3d_debug_distance_ranks: models of fewer than 3 beads have no distances to rank");
    if (replica < 0 || replica >= c->nrep) return fail(C3D_ERR_INVALID, "c3d_debug_distance_ranks: replica index out of range");
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int n = c->n;
    const size_t m = (size_t)n * (n - 1) / 2, slots = c3d::if_rank_key_slots(m);
    const CompareScratch L = compare_layout(n, 1, m, slots);
    DevTmp<char> tmp;
    if (int rc = compare_alloc(tmp, L.total, "c3d_debug_distance_ranks")) return rc;
    double* const d_xyz = reinterpret_cast<double*>(tmp.p + L.xyz);
    hipError_t e = c3d::launch_compare_coords(c->buf.X[c->parity] + (size_t)replica * c->rep_floats, n, c->npad, 1, d_xyz, c->stream);
    if (e == hipSuccess)
        e = c3d::launch_compare_ranks(d_xyz, n, reinterpret_cast<unsigned long long*>(tmp.p + L.keys), m, slots, reinterpret_cast<unsigned*>(tmp.p + L.ke),
                                      reinterpret_cast<double*>(tmp.p + L.rowsum), c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("compare launch: ") + hipGetErrorString(e));
    if (int rc = read_back(c, tmp.p + L.ke, sizeof(unsigned) * m)) return rc;
    const unsigned* const ke = static_cast<const unsigned*>(c->h_stage);
    for (size_t q = 0; q < m; ++q) rank[q] = 0.5 * (double)ke[q] + 1.0;
    return C3D_OK;
}

// ---- the models of a run in one frame (c3d_score.hip k_sup_*) ----
// the K models of a call as n x 3 doubles each on the device: the replicas' state (the fp64 state itself on a precision-64 context, else the
// floats widened), then n_extra models of the caller
static int superpose_models(c3d_ctx* c, double* d_xyz, const double* extra_xyz, int n_extra) {
    const int n = c->n, nrep = c->nrep;
    const hipError_t e = c->precision == 64 ? c3d::launch_superpose_gather64(c->b64.X[c->parity], n, c3d::cols64(n), nrep, d_xyz, c->stream)
                                            : c3d::launch_compare_coords(c->buf.X[c->parity], n, c->npad, nrep, d_xyz, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("superpose launch: ") + hipGetErrorString(e));
    if (n_extra > 0)
        HIP_TRY(hipMemcpyAsync(d_xyz + (size_t)3 * n * nrep, extra_xyz, sizeof(double) * 3 * (size_t)n * n_extra, hipMemcpyHostToDevice, c->stream));
    return C3D_OK;
}
// byte offsets into the one allocation of a call: models (the target of a superposition is model K), centroids, per-chunk sums, the pairs'
// sums, fits and residuals, two sets of mirror bits, then (superposition only) the fitted models and the block read back in one copy
struct SuperposeScratch {
    size_t xyz = 0, cent = 0, partial = 0, cov = 0, fit = 0, res = 0, mir = 0, mir2 = 0, fitted = 0, out = 0, total = 0;
};
static SuperposeScratch superpose_layout(int n, int models, int KB, size_t pairs, bool fitted, size_t out_bytes) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    SuperposeScratch L;
    L.cent = up(sizeof(double) * 3 * (size_t)n * models);
    L.partial = L.cent + up(sizeof(double) * 3 * (size_t)models);
    L.cov = L.partial + up(sizeof(double) * c3d::superpose_partial_doubles(n, KB));
    L.fit = L.cov + up(sizeof(double) * c3d::kSupCov * pairs);
    L.res = L.fit + up(sizeof(double) * c3d::kSupFit * pairs);
    L.mir = L.res + up(sizeof(double) * pairs);
    L.mir2 = L.mir + up(sizeof(int) * pairs);
    L.fitted = L.mir2 + up(sizeof(int) * pairs);
    L.out = L.fitted + (fitted ? up(sizeof(double) * 3 * (size_t)n * models) : 0);
    L.total = L.out + up(out_bytes);
    return L;
}

extern "C" int c3d_superpose_replicas(c3d_ctx* c, int reference, const double* ref_xyz, int flags, int iters, double* rmsd, int32_t* mirrored,
                                      double* mean_xyz, double* rmsf) {
    if (!c) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: call c3d_init_replicas first");
    if (c->n < 3) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: models of fewer than 3 beads have no orientation to fit");
    if (reference < -1 || reference >= c->nrep) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: reference is neither a replica index nor -1");
    if (reference == -1 && !ref_xyz) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: reference -1 without ref_xyz");
    if (flags & ~(C3D_SUPERPOSE_MIRROR | C3D_SUPERPOSE_APPLY)) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: unknown flag bits");
    if (iters < 0 || iters > C3D_SUPERPOSE_MAX_ITERS) return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: iters outside 0..C3D_SUPERPOSE_MAX_ITERS");
    const bool apply = (flags & C3D_SUPERPOSE_APPLY) != 0;
    if (!apply && !rmsd && !mirrored && !mean_xyz && !rmsf)
        return fail(C3D_ERR_INVALID, "c3d_superpose_replicas: every output is NULL and C3D_SUPERPOSE_APPLY is not set");
    const int n = c->n, K = c->nrep;
    if (reference == -1)
        if (int rc = c3d::check_model_coords(ref_xyz, (size_t)3 * n, "c3d_superpose_replicas")) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    // read back in one copy: sum of squares per model (K), mean (3 n), rmsf (n), mirror bits (K ints)
    const size_t out_doubles = (size_t)K + 4 * (size_t)n, out_bytes = sizeof(double) * out_doubles + sizeof(int) * (size_t)K;
    const SuperposeScratch L = superpose_layout(n, K + 1, 1, (size_t)K, true, out_bytes);
    DevTmp<char> tmp;
    if (int rc = compare_alloc(tmp, L.total, "c3d_superpose_replicas")) return rc;
    auto dbl = [&](size_t off) { return reinterpret_cast<double*>(tmp.p + off); };
    double* const d_xyz = dbl(L.xyz);
    double* const d_target = d_xyz + (size_t)3 * n * K;
    double* const d_cent = dbl(L.cent);
    double* const d_fitted = dbl(L.fitted);
    double* const d_out = dbl(L.out);
    double* const d_mean = d_out + K;
    double* const d_rmsf = d_mean + 3 * (size_t)n;
    int* const d_mir = reinterpret_cast<int*>(d_out + out_doubles);      // the first pass's bits: what the caller gets
    int* const d_mir2 = reinterpret_cast<int*>(tmp.p + L.mir2);
    if (int rc = superpose_models(c, d_xyz, ref_xyz, reference == -1 ? 1 : 0)) return rc;
    if (reference >= 0)
        HIP_TRY(hipMemcpyAsync(d_target, d_xyz + (size_t)3 * n * reference, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    hipError_t e = c3d::launch_superpose_centre(d_xyz, n, K + 1, d_cent, c->stream);
    if (e == hipSuccess)
        e = c3d::launch_superpose_fit(d_xyz, K, d_target, 1, n, reference >= 0 ? reference : c3d::kSupNoIdent, (flags & C3D_SUPERPOSE_MIRROR) != 0, nullptr,
                                      dbl(L.partial), dbl(L.cov), dbl(L.fit), d_mir, d_out, c->stream);
    if (e == hipSuccess) e = c3d::launch_superpose_apply(d_xyz, K, n, dbl(L.fit), iters == 0 ? d_cent + 3 * (size_t)K : nullptr, d_fitted, c->stream);
    for (int it = 0; it < iters && e == hipSuccess; ++it) {
        // the mean of the fitted models is the next target; every model gets a rotation onto it, its handedness as the first pass left it
        e = c3d::launch_superpose_mean(d_fitted, K, n, d_mean, d_rmsf, nullptr, c->stream);
        if (e != hipSuccess) break;
        HIP_TRY(hipMemcpyAsync(d_target, d_mean, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        e = c3d::launch_superpose_centre(d_target, n, 1, d_cent + 3 * (size_t)K, c->stream);
        if (e == hipSuccess)
            e = c3d::launch_superpose_fit(d_xyz, K, d_target, 1, n, c3d::kSupNoIdent, false, d_mir, dbl(L.partial), dbl(L.cov), dbl(L.fit), d_mir2,
                                          nullptr, c->stream);
        if (e == hipSuccess) e = c3d::launch_superpose_apply(d_xyz, K, n, dbl(L.fit), nullptr, d_fitted, c->stream);
    }
    // iters = 0: d_out[k] keeps the fit's residual against the target; else it becomes the squared distance from the final mean
    if (e == hipSuccess) e = c3d::launch_superpose_mean(d_fitted, K, n, d_mean, d_rmsf, iters > 0 ? d_out : nullptr, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("superpose launch: ") + hipGetErrorString(e));
    if (int rc = read_back(c, d_out, out_bytes)) return rc;
    if (apply) {
        if (c->precision == 64) {
            const size_t n3 = (size_t)K * 3 * c3d::cols64(n);
            e = c3d::launch_superpose_store64(d_fitted, n, c3d::cols64(n), K, c->b64.X[0], c->b64.X[1], c->stream);
            if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("superpose launch: ") + hipGetErrorString(e));
            for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(c->b64.V[k], 0, sizeof(double) * n3, c->stream));
            e = c3d::launch_export64(dev_model(c), c->b64, c->parity, c->buf.X[c->parity], c->buf.V[c->parity], c->buf.P[c->parity], c->stream);
            if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("fp64 export: ") + hipGetErrorString(e));
        } else {
            e = c3d::launch_superpose_store32(d_fitted, n, c->npad, K, c->buf.X[c->parity], c->stream);
            if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("superpose launch: ") + hipGetErrorString(e));
            for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(c->buf.V[k], 0, sizeof(float) * c->rep_floats * K, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const double* const h = static_cast<const double*>(c->h_stage);
    const int* const hm = reinterpret_cast<const int*>(h + out_doubles);
    for (int k = 0; k < K; ++k) {
        if (rmsd) rmsd[k] = sqrt(h[k] / (double)n);
        if (mirrored) mirrored[k] = hm[k];
    }
    if (mean_xyz) memcpy(mean_xyz, h + K, sizeof(double) * 3 * (size_t)n);
    if (rmsf) memcpy(rmsf, h + K + 3 * (size_t)n, sizeof(double) * (size_t)n);
    ++c->superpose_runs;
    return C3D_OK;
}

extern "C" int c3d_rmsd_table(c3d_ctx* c, const double* extra_xyz, int n_extra, int flags, double* rmsd, int32_t* mirrored) {
    if (!c) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: call c3d_init_replicas first");
    if (c->n < 3) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: models of fewer than 3 beads have no orientation to fit");
    if (n_extra < 0 || (n_extra > 0 && !extra_xyz)) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: n_extra < 0, or extra models without coordinates");
    if ((long)c->nrep + n_extra > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: more than C3D_COMPARE_MAX_MODELS models");
    if (flags & ~C3D_SUPERPOSE_MIRROR) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: unknown flag bits (the table moves nothing: C3D_SUPERPOSE_MIRROR alone)");
    if (!rmsd && !mirrored) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: both outputs are NULL");
    const int n = c->n, K = c->nrep + n_extra;
    if (n_extra > 0)
        if (int rc = c3d::check_model_coords(extra_xyz, (size_t)3 * n * n_extra, "c3d_rmsd_table")) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const size_t pairs = (size_t)K * K;
    const SuperposeScratch L = superpose_layout(n, K, K, pairs, false, 0);
    DevTmp<char> tmp;
    if (int rc = compare_alloc(tmp, L.total, "c3d_rmsd_table")) return rc;
    auto dbl = [&](size_t off) { return reinterpret_cast<double*>(tmp.p + off); };
    double* const d_xyz = dbl(L.xyz);
    if (int rc = superpose_models(c, d_xyz, extra_xyz, n_extra)) return rc;
    hipError_t e = c3d::launch_superpose_centre(d_xyz, n, K, dbl(L.cent), c->stream);
    if (e == hipSuccess)
        e = c3d::launch_superpose_fit(d_xyz, K, d_xyz, K, n, 0, (flags & C3D_SUPERPOSE_MIRROR) != 0, nullptr, dbl(L.partial), dbl(L.cov), dbl(L.fit),
                                      reinterpret_cast<int*>(tmp.p + L.mir), dbl(L.res), c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("superpose launch: ") + hipGetErrorString(e));
    // res and the mirror bits are neighbours in the allocation: one copy
    if (int rc = read_back(c, tmp.p + L.res, (L.mir - L.res) + sizeof(int) * pairs)) return rc;
    const double* const h = static_cast<const double*>(c->h_stage);
    const int* const hm = reinterpret_cast<const int*>(static_cast<const char*>(c->h_stage) + (L.mir - L.res));
    for (size_t q = 0; q < pairs; ++q) {
        if (rmsd) rmsd[q] = sqrt(h[q] / (double)n);
        if (mirrored) mirrored[q] = hm[q];
    }
    ++c->rmsd_table_runs;
    return C3D_OK;
}

extern "C" int c3d_rank(c3d_ctx* c, int32_t* rank) {
    if (!c || !rank) return fail(C3D_ERR_INVALID, "c3d_rank: null argument");
    std::vector<double> e((size_t)3 * std::max(c->nrep, 1));
    int rc = c3d_get_energies(c, e.data());
    if (rc) return rc;
    std::vector<int32_t> idx(c->nrep);
    for (int r = 0; r < c->nrep; ++r) idx[r] = r;
    // ascending int(E_noe) (get_cns_energy :617 truncates), ties by replica id
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return (long long)e[3 * a] < (long long)e[3 * b]; });
    for (int r = 0; r < c->nrep; ++r) rank[r] = idx[r];
    return C3D_OK;
}

// Test hook for the one hardware property the cluster kernel's hand-off leans on (c3d_cluster.hip): a 16-byte aligned plain store is never
// seen half-written by a 16-byte sc1 load of another workgroup.  Runs the producer / consumer pattern of tools/microbench/tear16.hip with the
// kernel's own store and load on THIS context's stream, all CUs (consumers on the producer's XCD and on every other one).
extern "C" int c3d_debug_tear16(c3d_ctx* c, int iterations, unsigned long long* unit_reads, unsigned long long* torn, unsigned long long* fresh) {
    if (!c || iterations < 1 || iterations > (1 << 24)) return fail(C3D_ERR_INVALID, "c3d_debug_tear16: bad arguments");
    C3D_ENTRY(c, unit_bit(UNIT_CLUSTER_BASE));
    DevTmp<unsigned char> buf;
    DevTmp<unsigned> stop;
    DevTmp<unsigned long long> stats;
    HIP_TRY(hipMalloc(&buf.p, 1024 * 16));
    HIP_TRY(hipMalloc(&stop.p, sizeof(unsigned)));
    HIP_TRY(hipMalloc(&stats.p, 3 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(buf.p, 0, 1024 * 16, c->stream));
    HIP_TRY(hipMemsetAsync(stop.p, 0, sizeof(unsigned), c->stream));
    HIP_TRY(hipMemsetAsync(stats.p, 0, 3 * sizeof(unsigned long long), c->stream));
    hipError_t e = c3d::launch_tear16(c->num_cus, buf.p, stop.p, stats.p, iterations, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string("tear16 launch: ") + hipGetErrorString(e));
    unsigned long long h[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(h, stats.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (unit_reads) *unit_reads = h[0];
    if (torn) *torn = h[1];
    if (fresh) *fresh = h[2];
    return C3D_OK;
}

#ifdef C3D_STAMPS
namespace c3d { hipError_t read_stamps(unsigned long long* out); hipError_t read_cluster_stamps(unsigned long long* out); hipError_t read_cluster_pstamps(unsigned long long* out); }
extern "C" int c3d_debug_cluster_pstamps(unsigned long long* out) {
    hipError_t e = c3d::read_cluster_pstamps(out);
    return e == hipSuccess ? C3D_OK : C3D_ERR_HIP;
}
extern "C" int c3d_debug_cluster_stamps(unsigned long long* out) {
    hipError_t e = c3d::read_cluster_stamps(out);
    return e == hipSuccess ? C3D_OK : C3D_ERR_HIP;
}
extern "C" int c3d_debug_stamps(unsigned long long* out) {
    hipError_t e = c3d::read_stamps(out);
    return e == hipSuccess ? C3D_OK : C3D_ERR_HIP;
}
#endif
