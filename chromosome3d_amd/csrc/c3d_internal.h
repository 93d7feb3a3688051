// c3d_internal.h — shared between the HIP kernels (c3d_device.hip) and the C-ABI host (c3d_api.cpp and the other host units: c3d_ctx.h).
// Not part of the public boundary (that is include/c3d.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "../../include/c3d.h"
#include "c3d_step_kinds.h"
#include "c3d_superpose.h"

namespace c3d {

constexpr float kBoltz = 0.0019872f;  // kcal/mol/K (X-PLOR/CNS AKMA)
constexpr float kAccel = 418.4f;      // kcal/mol/A/amu -> A/ps^2

// rows of the pair matrix owned by one workgroup of the step kernel (waves per workgroup = kTileRows / rpw)
constexpr int kTileRows = 8;
// the forces-only test hook runs the same tile with 4 rows per wave
constexpr int kEvalRowsPerWave = 4;
constexpr int kEvalBlock = 64 * kTileRows / kEvalRowsPerWave;

// far-away coordinates for the padding beads j in [n, npad): no NOE (target 0), repel term vanishes
constexpr float kPadCoord = 1.0e4f;

struct DevModel {
    int n, npad, ntiles, nrep;
    int rep_base, nrep_g;          // replica group of this launch: [rep_base, rep_base + nrep_g)
    int stage_dma;                 // 1: coordinates staged with global_load_lds (async), 0: through registers
    int rpw;                       // rows per wave of the step kernel (1, 2 or 4); waves/WG = kTileRows/rpw
    int noe_pot, ang_mode, rep_sep; // noe_pot: the c3d_model's 0..3, or 4 = 3 with the lower side's fast soft form (msoexp 2, masym 0)
    int mexp;                      // noe_pot 3 / 4, lower side: exponent of the soft form (c3d_model::msoexp, 1 or 2)
    float rs, tail_c, tail_b;      // soft tail: dE/dD = tail_c - tail_b / D^2  (D > rs)
    float mrs, mtail_c, mtail_b;   // noe_pot 3, lower side: dE/dD = mtail_c - mtail_b / D^(mexp + 1)  (D = t - d > mrs)
    float nmrs;                    // -mrs
    float inv_rs, nm_rs;           // 1 / rs, -mrs / rs: the clamp form works on (d - t) / (rs d), see pair_term (device potential 4: 1 / mrs, rs / mrs)
    // Column layout of the pair loop (c3d_step_core.h): blocks of 256 columns, lane l owns 4 consecutive ones — except in the LAST
    // block, where it owns wl (1..4) consecutive ones: column 256 (nb - 1) + wl l + c.  Up to 8 columns beyond the last block
    // (jl0 .. jl0 + nleft - 1 = n - 1) are "left over": their pair terms are evaluated eight to a row in a separate short pass
    // and summed in their own fixed tree.  n = 455: 256 + 64 x 3 + 7 -> 7 column slots per row instead of 8.
    int wl, nleft, jl0;
    float k_bond2, b0;             // 2*k_bond
    float k_ang2, a0;              // 2*k_ang
    float acc;                     // kAccel / mass
    float t_fac;                   // T = t_fac * sum(v^2):  mass / kAccel / (ndf * kBoltz)
    float fbeta;
    float inv_n;
    // Per-step kernel, device potential 4, no narrow column block (every n > 1024): the per-pair constant t / mrs of ROW PAIRS, resident
    // (Buffers::tgs2, built once per matrix and model by launch_pair_targets): [row pair q][column block jb][lane][column c][row & 1] —
    // the wave's two rows against its four columns of a block are 32 consecutive bytes, two register-pair-aligned float4 loads — with
    // "no restraint" encoded as 1e30 (such a pair feels exactly nothing under the decaying lower bound: pair_term2); nullptr = not in use
    const float* tgs2;
};

struct DevStep {
    int kind;        // a StepKind (c3d_step_kinds.h): 0 MD T-coupling, 1 MD velocity rescale, 2 FIRE step, 3 first FIRE step of a stage, 4 MD begin,
                     // 5 two-point step-size (Barzilai-Borwein) minimiser step, 6 its first step of a stage,
                     // 8 L-BFGS step, 9 its first step of a stage (k_lbfgs_eval + k_lbfgs_move only: never k_step / k_cluster)
    float dt;
    float w_all;     // weights * w
    float w_noe2n;   // -2 * w_all * s_noe
    float w_rep4;    // 4 * w_vdw * k_rep
    float rep_r2;    // (repel_s * r0_rep)^2
    float inv_rep_r2;// 1 / rep_r2
    float w_rep4r2;  // w_rep4 * rep_r2
    float w_rs;      // w_noe2n * rs (device potential 4: w_noe2n * mrs): the factor the clamp form leaves out of every pair term and applies once per row
    float kq;        // w_rep4r2 / w_rs: the repel weight relative to it (w_noe2n != 0; else the general kernels run)
    float t_bath;
};

struct DevFire {
    float dt_start, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step;
    int n_min;
};

struct FireState {   // per replica, double buffered
    float dt, alpha;
    int npos, pad;
};

// All device pointers of one context.  Layouts (npad = n rounded up to 256, one column block):
//   tgt   [n][npad]            encoded restraint target (see encode_target)
//   X,V   [2][nrep][3][npad]   SoA coordinates / velocities, double buffered by step parity
//   Vinit [nrep][3][npad]
//   P     [2][nrep][ntiles][4] per-tile partial sums
//   S     [2][nrep]            FIRE state
struct DevBuffers {
    float* tgt;
    float* tgs2;    // see DevModel::tgs2 (nullptr unless built)
    float* X[2];
    float* V[2];
    float* Vinit;
    float* P[2];
    FireState* S[2];
    double* E;      // [nrep][4]
};

// Runtime choices -> template arguments: f is called with std::integral_constant arguments (a generic lambda)
template <int V> using int_c = std::integral_constant<int, V>;
template <bool V> using bool_c = std::integral_constant<bool, V>;
inline int device_pot(int noe_pot) { return noe_pot == 0 || noe_pot == 1 || noe_pot == 3 || noe_pot == 4 ? noe_pot : 2; }   // anything else runs as 2
template <class F> hipError_t with_pot(int pot, F&& f) {
    switch (device_pot(pot)) {
        case 0: return f(int_c<0>{});
        case 1: return f(int_c<1>{});
        case 3: return f(int_c<3>{});
        case 4: return f(int_c<4>{});
        default: return f(int_c<2>{});
    }
}
template <class F> hipError_t with_rpw(int rpw, F&& f) { return rpw == 1 ? f(int_c<1>{}) : rpw == 2 ? f(int_c<2>{}) : f(int_c<4>{}); }
template <class F> hipError_t with_bool(bool b, F&& f) { return b ? f(bool_c<true>{}) : f(bool_c<false>{}); }

// default tails: the force stays at its value at the switch distance (slope 2 rs above, 2 mrs below for noe_pot 3)
inline bool general_tail(const DevModel& m) {
    if (!(m.tail_b == 0.0f && m.tail_c == 2.0f * m.rs)) return true;
    return m.noe_pot == 3 && !(m.mtail_b == 0.0f && m.mtail_c == 2.0f * m.mrs);      // (device potential 4 is a fast form by construction)
}
// the kernels of the general form also serve a step whose restraint weight is zero (the clamp form divides by it)
inline bool general_step(const DevModel& m, const DevStep& p) { return general_tail(m) || p.w_rs == 0.0f; }
// DevModel::tgs2 serves device potential 4 at two rows per wave without a narrow last block (ensure_pair_targets builds it beyond n = 1024)
inline bool pair_targets_fit(const DevModel& m) { return device_pot(m.noe_pot) == 4 && m.rpw == 2 && m.wl == 4 && m.nleft == 0; }

// The form of a per-step kernel (k_step, k_lbfgs_eval): k<pot, gen, rpw, nc>, or the wide k<4, false, 4, false, 16, true> — 16 rows a
// workgroup, four a wave, resident pair targets: problems beyond the multi-step kernel's reach.  Decided once per op: the launch and
// c3d_step_kernel_name both read it.  Switches: the context's options wide_tiles and pair_targets, and whether tgs2 is built.
//
// The column source (chunk): 0 = the replica's whole coordinate array staged in LDS (k_step, k_lbfgs_eval, k_eval_forces), else the
// chunked form with that many columns per pass (k_step_chunked, ...: ColsChunked, c3d_step_core.h) — column_chunk_for decides it.
struct StepForm {
    int pot;
    bool gen;
    int rpw;
    bool nc, pairs, wide;            // pairs: DevModel::tgs2 passed to the kernel
    int chunk;
};
// The staged kernels put 3 npad floats of coordinates in LDS: up to the 64 KB a launch gets without opting in (n <= 5120, 61 440 B plus
// the tile's own few hundred bytes).  Beyond that the chunked form runs, kDefaultColumnChunk columns a pass: the fastest CHUNK at every
// size measured, 4096 .. 16384 beads (24 KB of buffers, LDS no limit on the workgroups of a CU; profiles/r08_large_maps.md).
constexpr int kMaxStagedCols = 5120;
constexpr int kDefaultColumnChunk = 1024;
inline bool column_chunk_valid(int chunk) { return chunk == 256 || chunk == 1024 || chunk == 2048; }   // the instantiated set
// option = the context's column_chunk: 0 = the library's choice, else that CHUNK wherever a chunked form exists.  Layouts with a narrow
// last block (n <= 1024, whose coordinates always fit) have none.
inline int column_chunk_for(const DevModel& m, int option) {
    if (!(m.wl == 4 && m.nleft == 0)) return 0;
    if (option > 0) return option;
    return m.npad <= kMaxStagedCols ? 0 : kDefaultColumnChunk;
}
inline StepForm step_form(const DevModel& m, const DevStep& p, bool wide_tiles, bool pair_targets, bool tgs2_built, int column_chunk) {
    StepForm f;
    f.pot = device_pot(m.noe_pot);
    f.rpw = m.rpw == 1 || m.rpw == 2 ? m.rpw : 4;
    f.gen = general_step(m, p);
    f.nc = !(m.wl == 4 && m.nleft == 0);
    f.pairs = !f.gen && pair_targets_fit(m) && tgs2_built;
    f.wide = wide_tiles && pair_targets && f.pairs && m.npad > 1024;
    f.chunk = column_chunk_for(m, column_chunk);
    return f;
}
// the symmetric-tile kernel's RS1 (k_pairs_sym: c3d_sym.hip)
inline bool sym_rs1(const DevModel& m) { return m.rs == 1.0f; }

// host-callable launchers (defined in c3d_device.hip)
hipError_t launch_step(const DevModel& m, const DevStep& p, const DevFire& fp, const DevBuffers& b, int parity, const StepForm& f, hipStream_t s);
hipError_t launch_eval_forces(const DevModel& m, const DevStep& p, const DevBuffers& b, int parity, float* Fout,
                              bool general_tail, int rows_per_wave, int chunk, hipStream_t s);   // chunk: column_chunk_for
hipError_t launch_energy(const DevModel& m, const DevStep& p, const DevBuffers& b, int parity, float s_noe,
                         float k_rep, double rep_r2, hipStream_t s);
hipError_t launch_centre(const DevModel& m, const DevBuffers& b, int parity, hipStream_t s);
// L-BFGS stage (kinds 8 / 9, per-step path only): two launches a step.  k_lbfgs_eval = the step kernel's forces (same tile_forces<> and
// template choices as launch_step) and per-tile sums of the dot products the compact form (Byrd-Nocedal-Schnabel) needs; k_lbfgs_move =
// the replica sums in fp64, the 2m x 2m algebra (redundantly in every workgroup of a replica) and the move.  Layouts:
//   hist  [nrep][2: s, y][kLbfgsMaxPairs slots][3][npad]   the pairs, a ring of `mem` slots (a workgroup touches its own rows only)
//   part  [nrep][ntiles][kLbfgsQ]                             per tile: slot j: (F.s_j, F.y_j, s_j.y, y_j.y) at 4j, then s.s, F.F
//         (F = this evaluation's force, (s, y) = the pair this evaluation completes: s in slot nxt, y = F_prev - F written there)
//   S     [2][nrep] LbfgsState, double buffered by step parity; V[parity^1] = the force of the evaluation, P[parity^1] = (move.move, F.F, 0, 0)
constexpr int kLbfgsMaxPairs = 8;
constexpr int kLbfgsQ = 4 * kLbfgsMaxPairs + 4;
struct LbfgsState {
    int cnt, head, mem, resets;      // pairs held, slot of the newest, ring size m (fixed at the stage's first step), memory drops
    double gamma;                    // H0 = gamma I
    double SY[kLbfgsMaxPairs][kLbfgsMaxPairs];   // s_slot(i) . y_slot(j) (the upper triangle in age order is read)
    double YY[kLbfgsMaxPairs][kLbfgsMaxPairs];
};
struct LbfgsBuffers {
    float* hist;
    float* part;
    LbfgsState* S[2];
};
__host__ __device__ inline size_t lbfgs_hist_floats(int npad) { return (size_t)2 * kLbfgsMaxPairs * 3 * npad; }   // per replica
hipError_t launch_lbfgs_eval(const DevModel& m, const DevStep& p, const DevBuffers& b, const LbfgsBuffers& lb, int parity, int mem,
                             const StepForm& f, hipStream_t s);
hipError_t launch_lbfgs_move(const DevModel& m, const DevStep& p, const DevFire& fp, const DevBuffers& b, const LbfgsBuffers& lb, int parity,
                             int mem, hipStream_t s);
// c3d_lbfgs_move_row.inc (the rows of k_lbfgs_move) on `rows` rows, a thread a row (k_lbfgs_move_rows; c3d_debug_lbfgs_move_rows): device
// buffers in the move's layouts with np columns (rows padded to 256): xin, xout, fcur [3][np], hist lbfgs_hist_floats(np), d2 [np];
// coef[1 + 2 kLbfgsMaxPairs], the slot mask and the slot of s are uniform over the call
hipError_t launch_lbfgs_move_rows(const DevFire& fp, int rows, int np, const float* coef, int mask, int slot, const float* xin, float* xout,
                                  const float* fcur, float* hist, float* d2, hipStream_t s);
// c3d_lbfgs_serial.inc (the serial section of k_lbfgs_move) on `rows` rows of (sums[kLbfgsQ], LbfgsState, flags = (first, mem0)), a thread a
// row (c3d_debug_lbfgs_direction): out = the state left, coef[1 + 2 kLbfgsMaxPairs] widened to doubles, shi[2] = (slot mask, slot of s)
hipError_t launch_lbfgs_direction(const DevModel& m, const DevFire& fp, int rows, const double* sums, const LbfgsState* in, const int* flags,
                                  LbfgsState* out, double* coef, int* shi, hipStream_t s);
size_t pair_targets_floats(int n, int npad);           // size of DevBuffers::tgs2
hipError_t launch_pair_targets(const DevModel& m, const float* tgt, float* tgs2, hipStream_t s);
struct StepRun {    // `count` consecutive steps with the same parameters
    DevStep p;
    int count;
};
struct AnnealIO {   // state buffers of one multi-step launch (io = anneal_io(buffers, parity)), passed by value in the kernel arguments
    const float *pin, *xin, *vin, *vinit;
    const FireState* sin;
    float *xout, *vout, *pout;
    FireState* sout;
};
AnnealIO anneal_io(const DevBuffers& b, int parity);
// cluster kernel (c3d_cluster.hip): many SA steps of the replica group [m.rep_base, m.rep_base + m.nrep_g) in ONE launch;
// reads parity `parity` (through io), writes parity^1 once at the end.  A replica runs on `parts` workgroups of `threads`
// threads (`cw` compute waves x `rpw` rows + `helpers` helper waves) of ONE XCD, `wgs_per_cu` workgroups per CU, grid =
// wgs_per_cu x number of CUs.
// `runs` is the run-length coded step list of the WHOLE program (uploaded once); the launch starts `skip0` steps into
// run `run0` and makes `nsteps` steps.  `tag_base` (launch sequence number << 20) keeps the tags of different launches
// apart, `claim` points at 16 zeroed words that no other launch has used ([0..7] slot counters per XCD, [8] completion
// counter), timeout[0] = 0 (set by a workgroup that gives up), timeout[1] = 0 (set to tag_base | 1 by the workgroup that
// completes the launch's pl.expected).
struct ClusterPlan {
    int rpw, cw, helpers, wgs_per_cu, parts, per_xcd, grid, threads, units, device;
    int static_place = 1;                         // slot = blockIdx / 8, checked against the XCC id (0: per-XCD atomic counters)
    int xcd_base = 0, xcd_count = 8;              // the launch lives on XCDs xcd_base .. xcd_base + xcd_count - 1 (replica r on XCD xcd_base + r % xcd_count): two
    bool two_point = false;        // the launch's range holds two-point minimiser steps (kinds 5 / 6): k_cluster_tp
                                                  // contexts with disjoint sets anneal side by side (c3d_set_option "cluster_xcd_count" / "cluster_xcd_base")
    int late_tiles = 0;                           // tile sums fetched by H0 after the step has started instead of gating it (c3d_cluster.hip)
    unsigned expected = 0;                        // workgroups that must report completion: replicas x parts (the host may raise it: test hook)
    size_t lds;
    hipEvent_t t0 = nullptr, t1 = nullptr;        // when set: the launch stamps them with the kernel's own start and end
};
bool cluster_plan(const DevModel& m, int num_cus, int num_xcc, int forced_geom, int forced_late, int xcd_count, ClusterPlan* plan);
size_t cluster_record_bytes(const DevModel& m, const ClusterPlan& pl);
hipError_t launch_cluster(const DevModel& m, const DevFire& fp, const ClusterPlan& pl, const AnnealIO& io, const float* tgt, void* rec,
                          const StepRun* runs, int run0, int skip0, int nsteps, unsigned tag_base, unsigned* timeout,
                          unsigned* claim, hipStream_t s);
// Code objects.  The runtime loads a code object at the first use of one of its kernels; libc3d does not leave that to chance: every
// translation unit that holds kernels exports a function that loads its code object on the current device (and, for the multi-step
// units, gives every instantiation its dynamic-LDS allowance), and the loader of c3d_gate.cpp ("code objects") calls them one at a time,
// under a lock that every entry of the library holds shared around its HIP calls — no code object is loaded beside any of them.
hipError_t preload_device_unit();
hipError_t preload_cluster_base_unit();
hipError_t preload_cluster_unit(int pot, bool two_point);
hipError_t preload_score_unit();
hipError_t preload_embed_unit();
hipError_t preload_f64_unit();
hipError_t preload_sym_unit();
// the hand-off's 16-byte atomicity, watched: one producer workgroup, one consumer workgroup on every other CU (c3d_cluster.hip k_tear16)
hipError_t launch_tear16(int num_cus, void* buf, unsigned* stop, unsigned long long* stats, int iters, hipStream_t s);
// symmetric-tile step for large N (c3d_sym.hip): every pair once.  tiles = sym_tile_list() uploaded, scratch =
// sym_scratch_floats() floats of device memory (row-side and column-side partial forces of one step).
void sym_geometry(const DevModel& m, int* Q, int* G, int* ntiles_offdiag, int* ntiles_diag);
size_t sym_scratch_floats(const DevModel& m);
void sym_tile_list(const DevModel& m, int2* out);
hipError_t launch_step_sym(const DevModel& m, const DevStep& p, const DevFire& fp, const DevBuffers& b, int parity, const void* tiles,
                           float* scratch, hipStream_t s);
// step_scalars<true> on `rows` rows of (psum[4], FireState), a thread a row (c3d_sym.hip k_step_scalars; c3d_debug_step_scalars):
// scalars [rows][6] = lam, cmx, cmy, cmz, keep, mix; out = the state it leaves
hipError_t launch_step_scalars(const DevModel& m, const DevStep& p, const DevFire& fp, int rows, const float* psum, const FireState* in,
                               float* scalars, FireState* out, hipStream_t s);
// finish_row on `rows` rows, a thread a row (c3d_sym.hip k_row_finish; c3d_debug_row_finish): in [rows][16] = x0[3], v0[3], F[3], lam,
// cmx, cmy, cmz, keep, mix, dt of the state; out [rows][10] = xn[3], vn[3], the row's terms q of the four sums
constexpr int kRowFinishIn = C3D_ROW_FINISH_IN, kRowFinishOut = C3D_ROW_FINISH_OUT;
hipError_t launch_row_finish(const DevModel& m, const DevStep& p, const DevFire& fp, int rows, const float* in, float* out, hipStream_t s);
// fp64 step (c3d_f64.hip, option "precision" = 64): the CPU restatement's algorithm in its precision on the GPU, one launch per SA
// step of a replica group (k64_step, k64_step_chunked beyond 2560 beads), double buffered by step parity like the fp32 per-step path.
// Layouts (np = cols64(n): n rounded up to 128): T [n][np] targets in Angstrom (0.1 * t10, 0 = none); X, V [2][nrep][3][np] SoA;
// Vinit [nrep][3][np]; P [2][nrep][ntiles][4] per-tile sums; S [2][nrep] x fire_state64_bytes().
struct Buffers64 {
    int32_t* t10 = nullptr;        // the integer tenths T is (re)built from whenever the model changes
    double* T = nullptr;
    double* X[2] = {nullptr, nullptr};
    double* V[2] = {nullptr, nullptr};
    double* Vinit = nullptr;
    double* P[2] = {nullptr, nullptr};
    void* S[2] = {nullptr, nullptr};
    double* F = nullptr;           // c3d_eval_f64's force [nrep][3][np], then its energies [nrep][4]; allocated at first use
};
int cols64(int n);
// The staged kernel (k64_step) puts 3 * 8 * np bytes of coordinates in LDS: up to the 64 KB a launch gets without opt-in (n <= 2560,
// 61 760 B with the tile's own).  Beyond that the chunked form runs (k64_step_chunked), kDefaultColumnChunk64 columns a pass; the option
// f64_column_chunk forces a chunk wherever n is larger than it, so that both forms can run the same problem.
constexpr int kMaxStagedBeads64 = 2560;
constexpr int kDefaultColumnChunk64 = 512;       // the fastest CHUNK at every size measured, 2560 .. 16384 beads (profiles/r14_f64_large_maps.md)
inline bool column_chunk64_valid(int chunk) { return chunk == 256 || chunk == 512 || chunk == 1024; }   // the instantiated set
inline int column_chunk64_for(int n, int option) {
    if (option > 0) return n > option ? option : 0;
    return n <= kMaxStagedBeads64 ? 0 : kDefaultColumnChunk64;
}
// The kernel arguments of the fp64 path, built once per op by the host units (launch_op, c3d_eval_f64, build_targets64) and passed on as they
// are.  The builders are defined in c3d_f64.hip, the unit compiled with -ffp-contract=off: every derived double (the tails, nmrs4, t_fac; a
// step's R2, wr4, nws4, wq, acc, kb4, ka4, ...) is formed there, in one expression order.  d carries the geometry and the device potential.
struct Model64 {
    int n, np, ntiles, min_sep, noe_pot, rep_sep, ang_mode, mexp;      // noe_pot as DevModel's (4 = the fast soft lower side)
    double s_noe, rs, tail_c, tail_b, mrs, mtail_c, mtail_b;
    double k_bond, b0, k_ang, a0, r0_rep, k_rep, mass, fbeta;
    double nmrs4;                                  // -mrs^4 (the fast soft lower side's bound is nmrs4 / D^3)
    double t_fac, inv_n;                           // T = t_fac * sum v^2; 1 / n
};
struct Step64 {
    int kind;
    double dt, w_all, w_vdw, repel_s, t_bath;
    // uniform factors of a step, formed on the host (fp64 has no scalar ALU: formed in the kernel they are vector registers every wave
    // holds through its pair loop): R2 = (repel_s r0_rep)^2, wr4 = 4 w_vdw k_rep, nws4 = -4 w_all S, wq = wr4 / nws4 (0 where nws4 = 0)
    double R2, wr4, nws4, wq;
    double acc;        // MD: dt kAccel / mass (the kernel's own division was ~30 fp64 operations on every wave's path after its pair loop)
    double kb4, ka4;   // chain terms: -4 w_all k_bond, -4 w_all k_ang
    double kacc;       // kAccel / mass (FIRE: times the step's dt)
    double a0sq;       // a0^2
};
struct Fire64 {
    double dt_start, dt_max, f_inc, f_dec, alpha_start, f_alpha, max_step;
    int n_min;
};
Model64 model64(const DevModel& d, const c3d_model& h);
Step64 step64(const Model64& m, int kind, double dt, double w_all, double w_vdw, double repel_s, double t_bath);   // a stage's values, as doubles
Fire64 fire64(const c3d_fire_params& f);
// k64_step<pot, gen, fold>'s / k64_step_chunked<pot, gen, fold, chunk>'s form, decided once per op from the built Model64 (op_kernel,
// c3d_eval_f64, build_targets64): the launch, the target encoding and c3d_step_kernel_name all read this one value.  pot = the model's
// device potential, gen = a general tail, fold = the fast soft lower side (potential 4) at a restraint weight w_all != 0, chunk =
// column_chunk64_for(n, the context's f64_column_chunk) (0 = staged)
struct Form64 {
    int pot;
    bool gen, fold;
    int chunk;
};
inline Form64 form64(const Model64& m, double w_all, int column_chunk) {
    Form64 f;
    f.pot = m.noe_pot;
    f.gen = !(m.tail_b == 0.0 && m.tail_c == 2.0 * m.rs) || (f.pot == 3 && !(m.mtail_b == 0.0 && m.mtail_c == 2.0 * m.mrs));     // (potential 4 has a fast form of its own)
    f.fold = f.pot == 4 && !f.gen && w_all != 0.0;
    f.chunk = column_chunk64_for(m.n, column_chunk);
    return f;
}
hipError_t launch_step64(const DevModel& d, const Model64& m, const Step64& p, const Fire64& fp, const Form64& f, const Buffers64& b, int parity,
                         hipStream_t s);
// The L-BFGS stage in fp64 (option f64_lbfgs on a precision-64 context): k64_lbfgs_eval[_chunked] + k64_lbfgs_move, the layouts of the
// fp32 stage above in doubles with np columns: hist [nrep][2: s, y][kLbfgsMaxPairs][3][np] (lbfgs_hist_floats(np) doubles a replica),
// part [nrep][ntiles][kLbfgsQ], S [2][nrep] LbfgsState; V[parity^1] = the force of the evaluation, P[parity^1] = (move.move, F.F, 0, 0).
// The first step's gamma (kind 9) is dt_start^2 kAccel / mass formed in fp64: kind 6's first length in k64_step.
struct LbfgsBuffers64 {
    double* hist = nullptr;
    double* part = nullptr;
    LbfgsState* S[2] = {nullptr, nullptr};
};
hipError_t launch_lbfgs_eval64(const DevModel& d, const Model64& m, const Step64& p, const Form64& f, const Buffers64& b, const LbfgsBuffers64& lb,
                               int parity, int mem, hipStream_t s);
hipError_t launch_lbfgs_move64(const DevModel& d, const Model64& m, const Step64& p, const Fire64& fp, const Buffers64& b, const LbfgsBuffers64& lb,
                               int parity, int mem, hipStream_t s);
hipError_t launch_lbfgs_direction64(const Step64& p, const Fire64& fp, int rows, const double* sums, const LbfgsState* in, const int* flags,
                                    LbfgsState* out, double* coef, int* shi, hipStream_t s);      // the same of k64_lbfgs_move
hipError_t launch_lbfgs_move_rows64(const Fire64& fp, int rows, int np, const double* coef, int mask, int slot, const double* xin, double* xout,
                                    const double* fcur, double* hist, double* d2, hipStream_t s);      // k_lbfgs_move_rows in doubles
hipError_t launch_targets64(const Model64& m, const Form64& f, const int32_t* t10, double* T, hipStream_t s);   // in the encoding f's kernel expects
// the integer tenths of a restraint list (R pairs, 0-based, every pair once) into the zeroed n x n matrix t10, both triangles
hipError_t launch_tenths64(int n, int R, const int32_t* ri, const int32_t* rj, const int32_t* rt10, int32_t* t10, hipStream_t s);
hipError_t launch_import64(const DevModel& d, const float* Xf, const Buffers64& b, hipStream_t s);
hipError_t launch_export64(const DevModel& d, const Buffers64& b, int parity, float* Xf, float* Vf, float* Pf, hipStream_t s);
// The forces-and-energies hook of a precision-64 context (c3d_eval_f64).  launch_eval_forces64: k64_eval_forces[_chunked] in the form f (a
// stage's weights select the instantiation family of the stage's step), the total weighted force of X[parity] into Fout [nrep][3][np]: a
// buffer of the context's own (Buffers64::F), never the velocity slot; p of kind 3 (dt and t_bath unused).  launch_energy64: k64_energy,
// Eout [nrep][4] = unweighted noe, bond + angle, repel, 0.
hipError_t launch_eval_forces64(const DevModel& d, const Model64& m, const Step64& p, const Form64& f, const Buffers64& b, int parity, double* Fout,
                                hipStream_t s);
hipError_t launch_energy64(const DevModel& d, const Model64& m, double rep_r2, const Buffers64& b, int parity, double* Eout, hipStream_t s);
size_t fire_state64_bytes();
// The fp64 controller and row update as tables, a thread a row (k64_step_scalars / k64_row_finish run the two texts k64_step includes,
// c3d_f64_scalars.inc and c3d_f64_row_finish.inc; c3d_debug_step_scalars_f64 / c3d_debug_row_finish_f64).  State rows in / out are
// fire_state64_bytes() each: (double dt, double alpha, int32 npos, int32 pad).  scalars [rows][6] = lam, cm0 .. cm2, keep, mix.
// Row finish: in [rows][16] = x0[3], v0[3], F[3], lam, cm0 .. cm2, keep, mix, dt of the state; out [rows][10] = xn[3], vn[3], q0 .. q3.
constexpr int kRowFinish64In = 16, kRowFinish64Out = 10;
hipError_t launch_step_scalars64(const Model64& m, const Step64& p, const Fire64& fp, int rows, const double* psum, const void* in, double* scalars,
                                 void* out, hipStream_t s);
hipError_t launch_row_finish64(const Step64& p, const Fire64& fp, int rows, const double* in, double* out, hipStream_t s);
// K1: IF (n*n fp64, device) -> dist10 (n*n int32, device) and encoded targets (n*npad, device)
hipError_t launch_if_to_target(const double* IF, int n, int npad, double alpha, double K, int min_sep, int rep_sep,
                               double* scratchP, double* partial, int npartial, int32_t* dist10, float* tgt,
                               unsigned char* flags, unsigned* nflag, hipStream_t s);

// A7 (c3d_embed.hip): bead-level metric-matrix distance geometry for every replica, in two halves —
// launch_dg_smooth: bounds from the targets, triangle smoothing of U and L (n*n each), L <= U;
// launch_dg_embed: trial distances from the smoothed U, L and the 3 leading eigenvectors, into both parity buffers, `batch` replicas at a
// time; the eigen stage as k_dg_eig (one workgroup per replica, 9 n + 16 floats of LDS: n <= kDgEigMaxBeads) or tiled (any n; same bits)
constexpr int kDgEigMaxBeads = (int)((160 * 1024 / sizeof(float) - 16) / 9);   // 4549
hipError_t launch_dg_smooth(const float* tgt, int n, int npad, float b0, float lower, float* U, float* L, hipStream_t s);
hipError_t launch_dg_embed(const float* U, const float* L, int n, int npad, int nrep, uint64_t seed, uint32_t first_replica, int iters,
                           float* v, float* D2, float* wt, float* x0, float* x1, bool tiled, int batch, hipStream_t s);

// K6 (c3d_score.hip): satisfied / sum-of-deviations / Spearman partial sums for every replica
hipError_t launch_score(const float* xin, const float* tgt, const double* rankA, int n, int npad, int nrep, int range, int min_sep,
                        unsigned nbins, double ma, double mb, double relax, double* xr, unsigned* hist, unsigned* below,
                        double* partial, int* overflow, hipStream_t s);
// the same histogram, prefix and sums with any `nbins`, for the `nrep` replicas xr and partial start at (c3d_score_replicas runs it in
// batches when launch_score reported overflow); launch_score_bbox: box[rep][comp][0..1] = min, max of the rounded coordinates
hipError_t launch_score_bbox(const double* xr, int n, int nrep, double* box, hipStream_t s);
hipError_t launch_score_wide(const double* xr, const float* tgt, const double* rankA, int n, int npad, int nrep, int range, int min_sep,
                             unsigned nbins, double ma, double mb, double relax, unsigned* hist, unsigned* below, double* partial,
                             int* overflow, hipStream_t s);
// IF ranks of a symmetric matrix on the device.  M (n*n fp64, device) holds the matrix; mh = (n-range)(n-range+1)/2 upper-triangle pairs
// |i-j| >= range; keys = if_rank_key_slots(mh) 64-bit slots.  launch_if_rank_keys fills the keys and raises *asym if M(i,j) != M(j,i) for
// one of those pairs; launch_if_rank_sort sorts them, overwrites M with the rank matrix of c3d::if_pair_ranks (0 inside the band) and
// leaves saa_rows[i] = sum_j (rank(i,j) - ma)^2.
constexpr int kRankTile = 4096;
inline size_t if_rank_key_slots(size_t mh) {
    size_t slots = kRankTile;
    while (slots < mh) slots <<= 1;
    return slots;
}
hipError_t launch_if_rank_keys(const double* M, int n, int range, unsigned long long* keys, size_t mh, size_t slots, int* asym, hipStream_t s);
hipError_t launch_if_rank_sort(double* M, int n, int range, unsigned long long* keys, size_t mh, size_t slots, double ma, double* saa_rows,
                               hipStream_t s);
// The models of a run against one another (c3d_compare_replicas).  A model is n x 3 doubles, xyz interleaved; m = n(n-1)/2 pairs i < j in
// row order.  launch_compare_coords widens the replicas' floats into `nrep` such models; launch_compare_ranks does one model: keys of its
// distances (if_rank_key_slots(m) slots), the sort, then ke[pair] = first + last sorted position of the pair's tie group (average rank =
// ke / 2 + 1) and rowsum[i] = sum_j>i d_ij; launch_compare_table, over K models' ke (K x m) and rowsum (K x n): sums[k] = sum of model k's
// distances, table[a][b] = { sum (ra - mean)(rb - mean), sum (sums[b] / sums[a] d_a - d_b)^2 } through `partial`, which holds
// compare_table_chunks(m, K) x nb x nb x 512 doubles, nb = model_blocks(K): per-chunk sums, added in chunk order.
constexpr int kCmpModels = 16;
// Model blocks: a workgroup of 256 threads takes kCmpModels models a and kCmpModels models b, thread t the pair of a's model pair_row(t)
// and b's model pair_col(t) (k_cmp_table, k_sup_cov, k_sup_residual); K models are model_blocks(K) blocks a side.
constexpr int model_blocks(int K) { return (K + kCmpModels - 1) / kCmpModels; }
static_assert(kCmpModels == 16, "pair_row shifts by log2(kCmpModels), and a block of pairs is one 256-thread workgroup");
constexpr int pair_row(int tid) { return tid >> 4; }
constexpr int pair_col(int tid) { return tid & (kCmpModels - 1); }
inline size_t compare_chunk_pairs(size_t m, int K) {       // a multiple of the 64-pair tile; about 2048 workgroups, 64 chunks at least
    const size_t nb = (size_t)model_blocks(K), want = 2048 / (nb * nb) > 64 ? 2048 / (nb * nb) : 64;
    return ((m + want - 1) / want + 63) / 64 * 64;
}
inline int compare_table_chunks(size_t m, int K) {
    const size_t per = compare_chunk_pairs(m, K);
    return (int)((m + per - 1) / per);
}
hipError_t launch_compare_coords(const float* xin, int n, int npad, int nrep, double* xyz, hipStream_t s);
hipError_t launch_compare_ranks(const double* x, int n, unsigned long long* keys, size_t m, size_t slots, unsigned* ke, double* rowsum,
                                hipStream_t s);
hipError_t launch_compare_table(const double* xyz, const unsigned* ke, const double* rowsum, int n, int K, size_t m, double* sums,
                                double* partial, double* table, hipStream_t s);
// The models of a run in one frame (c3d_superpose_replicas, c3d_rmsd_table; k_sup_*).  A model is n x 3 doubles, xyz interleaved.
// launch_superpose_gather64: the fp64 state X [nrep][3][np] as such models, every value as it is (fp32 state: launch_compare_coords; both
// are k_models_gather, and the two stores below k_models_scatter: c3d_score_core.h).
// launch_superpose_centre: cent[k] = the centroid of model k, the model centred on it in place (K models).
// launch_superpose_fit: every model of A (KA) onto every model of B (KB), both centred: cov[a][b][kSupCov] (c3d_superpose.h), then
// fit[a][b][kSupFit] = Q, mirror bit, eigenvalue and mirrored[a][b]; res[a][b] = sum |Q a_i - b_i|^2 unless res is null.  ident: the pair
// a == b + ident gets the identity (kSupNoIdent: no pair).  mirror: the reflected candidate takes part; fixed (KA ints, or null): model a's
// handedness is given and only rotations are fitted.  partial holds superpose_partial_doubles(n, KB) doubles: per-chunk sums of one row
// block of sixteen models a, added in chunk order; a chunk is 64 beads at every n and K.
// launch_superpose_apply: fitted[k] = Q_k a_k + shift (3 doubles on the device, or null), fit holding one entry a model (KB = 1).
// launch_superpose_mean: mean (n x 3), rmsf (n) over the K fitted models, k in order; dev[k] = sum_i |x_k,i - mean_i|^2 unless null.
// launch_superpose_store32 / 64: the fitted models into beads 0..n-1 of X [nrep][3][npad] floats / of X0 and X1 [nrep][3][np] doubles.
constexpr int kSupNoIdent = -(1 << 30);
inline int superpose_chunks(int n) { return (n + 63) / 64; }
inline size_t superpose_partial_doubles(int n, int KB) {
    return (size_t)superpose_chunks(n) * (size_t)model_blocks(KB) * 256 * kSupCov;
}
hipError_t launch_superpose_gather64(const double* X, int n, int np, int nrep, double* xyz, hipStream_t s);
hipError_t launch_superpose_centre(double* xyz, int n, int K, double* cent, hipStream_t s);
hipError_t launch_superpose_fit(const double* A, int KA, const double* B, int KB, int n, int ident, bool mirror, const int* fixed, double* partial,
                                double* cov, double* fit, int* mirrored, double* res, hipStream_t s);
hipError_t launch_superpose_apply(const double* A, int K, int n, const double* fit, const double* shift, double* fitted, hipStream_t s);
hipError_t launch_superpose_mean(const double* fitted, int K, int n, double* mean, double* rmsf, double* dev, hipStream_t s);
hipError_t launch_superpose_store32(const double* fitted, int n, int npad, int nrep, float* X, hipStream_t s);
hipError_t launch_superpose_store64(const double* fitted, int n, int np, int nrep, double* X0, double* X1, hipStream_t s);
// The ensemble's distance map (c3d_ensemble_map, c3d_ensemble_score; k_ens_*).  xyz holds K models of n x 3 doubles, xyz interleaved; pick
// (device) lists Kp model indices in 0..K-1, the summation order.  launch_ensemble_map: mean, sd, contact (n x n row-major doubles on the
// device, any of them null) = per pair the mean of d_k, sqrt(sum (d_k - mean)^2 / Kp) and #{d_k < cutoff} / Kp, both triangles from one
// value; one workgroup a 64 x 64 tile of the upper triangle, the picked models staged in blocks of kEnsModels.
// launch_ensemble_corr: rows[i] = sum over j, |i-j| >= range, of (A(i,j) - ma)(B(i,j) - ma) for two rank matrices launch_if_rank_sort left.
constexpr int kEnsModels = 16;
constexpr int kEnsMaxPicks = 4096;
inline int ensemble_tiles(int n) { return (n + 63) / 64; }
hipError_t launch_ensemble_map(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact,
                               hipStream_t s);
hipError_t launch_ensemble_corr(const double* A, const double* B, int n, int range, double ma, double* rows, hipStream_t s);
// A model's geometry and the distance against separation (c3d_geometry_replicas, c3d_separation_profile; k_geo_*, k_sep_*).  xyz as above.
// launch_geometry, for each of the K models: bead_clashes, nearest, furthest (K x n on the device) = per bead the number of partners j,
// |i-j| >= sep, with d <= cutoff, the smallest such d (+inf without a partner) and the largest d over all j; clashes (K) = half the sum of
// a model's bead_clashes, chain (K x C3D_GEOMETRY_FIELDS) = bond mean / sd, (i,i+2) mean / sd, radius of gyration, extent.  A cutoff < 0
// counts nothing.  launch_separation_profile: mean, sd, contact (n doubles on the device, indexed by s; mean is always written, sd and
// contact may be null) over the Kp picked models' d(i, i+s); the sd is a second launch that reads the finished mean.
hipError_t launch_geometry(const double* xyz, int n, int K, double cutoff, int sep, int* bead_clashes, double* nearest, double* furthest,
                           long long* clashes, double* chain, hipStream_t s);
hipError_t launch_separation_profile(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact,
                                     hipStream_t s);
// IF against model distance per genomic separation (c3d_stratified_score; k_str_*).  Strata lo <= s <= hi, stratum s the n - s pairs (i, i + s).
// launch_stratified_if: a = the doubled average ranks of IF inside every stratum, packed diagonal-major from stratum lo (stratified_pairs
// values), saa[s - lo] = their sum of squares; flags (kStrFlags ints on the device, cleared here): [0] IF(i, j) != IF(j, i) in a stratum,
// [1] a value there that is not finite, [3] a stratum whose ranks do not add up to N (N + 1): an internal error.  launch_stratified_models: sums (K x n x C3D_STRATUM_FIELDS, cleared here) = C, A, B of every
// stratum and model from the models' "%.3f" distances ranked the same way; flags[2]: a pair further apart than 50 000 A (or not a number).
constexpr int kStrFlags = 4;
inline size_t stratified_pairs(int n, int lo, int hi) { return (size_t)(hi - lo + 1) * (size_t)n - ((size_t)hi * (hi + 1) / 2 - (size_t)lo * (lo - 1) / 2); }
hipError_t launch_stratified_if(const double* IF, int n, int lo, int hi, unsigned* a, long long* saa, int* flags, hipStream_t s);
hipError_t launch_stratified_models(const double* xyz, int n, int K, int lo, int hi, const unsigned* a, const long long* saa, long long* sums, int* flags,
                                    hipStream_t s);
// A model's fit to the data bead by bead (c3d_bead_scores; k_bead_*).  beads (device): nb ascending bead indices, or null for every bead
// (nb = n); row b is bead i = beads[b], its partners J(i) = { j : |i-j| >= range }.  flags: the kStrFlags ints above, cleared by the caller.
// launch_bead_if: a (nb x n) = at column j in J(i) the doubled average rank of IF(i, j) inside the row (other columns are not written),
// saa[b] = their sum of squares (0 for a row of fewer than two partners); flags[1]: a value of an asked row is not finite, [3] internal.
// launch_bead_models: sums (K x nb x C3D_BEAD_FIELDS) = C, A, B of every model and row (0 for fewer than two partners; not written when
// a is null: no ranking); over the partners j with a target t10 > 0 tenths and |i-j| >= min_sep — tgt (n x npad floats, t10 / 10) or,
// where that is null, t10 (n x n ints) — restrained (nb), satisfied and dev_milli (K x nb): their number, the reference's net
// satisfaction count and deviation in thousandths of an A (not written when tgt and t10 are both null).  flags[2]: a pair of an asked bead
// further apart than 50 000 A (or not a number).
hipError_t launch_bead_if(const double* IF, int n, int range, const int* beads, int nb, unsigned* a, long long* saa, int* flags, hipStream_t s);
hipError_t launch_bead_models(const double* xyz, int n, int K, int range, const int* beads, int nb, const unsigned* a, const long long* saa, const float* tgt,
                              int npad, const int* t10, int min_sep, long long* sums, int* restrained, int* satisfied, long long* dev_milli, int* flags,
                              hipStream_t s);
// A bead's exposed surface (c3d_accessibility; k_access).  xyz as above; points (device): P x 3 doubles, unit vectors; R = radius + probe,
// R2 = R R, keep2 = 4 R2 (1 + 2^-20), the neighbour bound (c3d_score_access.inc), all three formed by the caller.  exposed (K x n on the
// device) = per bead the number of its points x_i + R u_p that lie strictly inside the sphere of radius R of no other bead of the model.
// flags (one int, cleared by the caller): [0] a coordinate of a model is not finite or has |x| >= 1e6, outside the bound's proof.
hipError_t launch_accessibility(const double* xyz, int n, int K, const double* points, int P, double R, double R2, double keep2, int* exposed, int* flags,
                                hipStream_t s);
// Compartment eigenvectors (c3d_compartments; k_cpt_*, c3d_score_compartment.inc).  A batch is nb maps in flight, map b of it the call's map
// q0 + b: map 0 is IF when has_if (uploaded into slot 0 of X by the caller), the n_models maps after it one picked model each — pick
// (device) lists them, indices into the K models of xyz — and the map after those the consensus, the list's mean distance map.  Every
// array of CptWork is on the device and indexed by b: X nb x n x n, E, m, D nb x n, V, U, W, P nb x nv x n, c nb x kCptVecs, stats
// nb x kCptStats (share, residual, same_side at 0, 3, 6 + a; agreement at 9 + 3 a + b2); F (nv x n, one for the call) holds IF's finished
// vectors; flags (2 ints, cleared by the caller): [0] IF is asymmetric (1), not finite (2) or negative (4) somewhere, [1] a vector
// projected to 0 in some round.
// launch_compartment_if_check: flags[0] of the n x n matrix M.  launch_compartment_build: E, X (in place for IF), m and D of the batch.
// launch_compartment_round: one round — V <- Y unless `first`, Gram-Schmidt, U = D V, W = X U - c, P = X W.  launch_compartment_finish:
// Y of the last round, share, residual and, for IF or where the call has no IF, the sign rule of the largest entry.
// launch_compartment_fit: the maps other than IF against F — sign, agreement, same_side.
constexpr int kCptVecs = 3;       // C3D_COMPARTMENT_MAX_VECTORS
constexpr int kCptRows = 8;       // rows of X a workgroup of the product kernel owns
constexpr int kCptStats = 24;
struct CptMaps {
    int n, q0, nb, has_if, n_models;
    const double* xyz;
    const int* pick;
};
struct CptWork {
    double *X, *E, *m, *D, *V, *U, *W, *P, *c, *stats, *F;
    int* flags;
};
hipError_t launch_compartment_if_check(const double* M, int n, int* flags, hipStream_t s);
hipError_t launch_compartment_build(const CptMaps& maps, const CptWork& w, int min_sep, hipStream_t s);
hipError_t launch_compartment_round(const CptMaps& maps, const CptWork& w, int nv, bool first, hipStream_t s);
hipError_t launch_compartment_finish(const CptMaps& maps, const CptWork& w, int nv, hipStream_t s);
hipError_t launch_compartment_fit(const CptMaps& maps, const CptWork& w, int nv, hipStream_t s);
// Insulation profiles and domain boundaries (c3d_insulation; k_ins_*, c3d_score_insulation.inc).  The Q maps of a call: map 0 is IF when
// has_if — its upper band at band_if, row a the n x 2 wmax doubles M(a, a+1 .. a + 2 wmax), zeros beyond the matrix, packed and checked by
// the host — the n_models maps after it one picked model each (pick, device: indices into the K models of xyz) and, with `consensus`, a
// last map whose band launch_insulation_band writes to band_cons in the same layout: the pick list's mean distance, or with `contact`
// the number of its models closer than cutoff.  w[0..nw) are the windows, ascending, wmax the last.  Every result row is n long and row
// (q nw + k) belongs to map q and window k.
// launch_insulation_band: band_cons.  launch_insulation_squares: mean (Q nw rows); `stage` (C3D_INSULATION_STAGE) picks the form that computes a tile's
// distances once into LDS (wmax <= kInsStageMax only), the same bytes either way.  launch_insulation_profile: score, boundary and strength from
// mean.  launch_insulation_fit: fit_r ((Q - 1) nw) and fit_counts ((Q - 1) nw x 4) of the maps after IF from score, boundary, strength.
constexpr int kInsTile = 32;          // beads a workgroup of k_ins_squares owns
constexpr int kInsStageMax = 40;      // the largest wmax at which the tile's (kInsTile + wmax - 1)^2 distances can be staged in LDS
struct InsJob {
    int n, Q, has_if, n_models, consensus, contact, nw, wmax;
    int w[8];                         // C3D_INSULATION_MAX_WINDOWS
    double cutoff;
    const double* xyz;
    const int* pick;
    const double* band_if;
    double* band_cons;
};
hipError_t launch_insulation_band(const InsJob& job, hipStream_t s);
hipError_t launch_insulation_squares(const InsJob& job, bool stage, double* mean, hipStream_t s);
hipError_t launch_insulation_profile(const InsJob& job, const double* mean, double* score, int* boundary, double* strength, hipStream_t s);
hipError_t launch_insulation_fit(const InsJob& job, const double* score, const int* boundary, const double* strength, double min_strength, int tol,
                                 double* fit_r, int* fit_counts, hipStream_t s);
// Balancing a raw contact matrix (c3d_balance_matrix; k_bal_*, c3d_score_balance.inc).  M is the call's copy of the matrix, n rows of pitch
// np = balance_pitch(n) doubles with the pad column 0; w has np entries, s, code and cnt n each; code[i] is 0 for a kept bin, else the
// mask's reason (C3D_BALANCE's `masked`).  rec is the round record, kBalRecord doubles { var_t, mbar, t, stop word }, zeroed by the host
// before the first round; history has max_iters + 1 doubles.
// launch_balance_count: cnt[i] = #{ j : |i-j| >= ignore_diags, M(i,j) > 0, code[j] == 0 }.  launch_balance_round: round t — the marginals
// s from w, then the update, which writes rec and history[t] and, unless the round stops, the new w (`kept` = |U|; half_power: sqrt-VC).
// Both kernels return at once when the stop word is set, so rounds may be enqueued beyond the stopping one.  launch_balance_apply: the
// final scale of w by sqrt(target / mbar) and, with `matrix`, M(i,j) <- (w_i w_j) M(i,j) in place.
constexpr int kBalRecord = 4;
constexpr int kBalConverged = 1, kBalExhausted = 2, kBalDiverged = 3;      // the stop word
constexpr int kBalBatch = 16;         // rounds the host enqueues between two looks at the record
inline int balance_pitch(int n) { return (n + 1) & ~1; }
struct BalJob {
    int n, np, ignore_diags;
    double* M;
    double* w;
    double* s;
    int* code;
    int* cnt;
    double* rec;
    double* history;
};
hipError_t launch_balance_count(const BalJob& job, hipStream_t s);
hipError_t launch_balance_round(const BalJob& job, int kept, int t, int max_iters, double tol, bool half_power, hipStream_t s);
hipError_t launch_balance_apply(const BalJob& job, double target, bool matrix, hipStream_t s);
// Loop enrichment (c3d_loops; k_loop_*, c3d_score_loop.inc).  The Q maps of a call as in InsJob: map 0 is IF when has_if, its band at
// band_if — row a the S doubles M(a, a + s_lo .. a + s_lo + S - 1), s_lo = min_sep - 2w, zeros beyond the matrix, packed and checked by
// the host — then n_models picked models (pick, device: indices into the models of xyz) and, with `consensus`, a last map whose band
// launch_loop_expected writes to band_cons first.  mask: n ints on the device, non-zero for a bin that is not mappable (all zero when
// the caller gave none).  expected: Q x S, row q map q's E[s_lo .. s_lo + S - 1].  A pixel flag array is B x n bytes, [s - min_sep][i].
// launch_loop_expected: band_cons, expected.  launch_loop_scan (IF only): ratio (4 x B x n, may be null) and cand (may be null), the
// candidate flags under `rule`.  launch_loop_peaks: peak (the candidates that survive the suppression), rows (3 n: a row's candidates,
// peaks, inside pixels with a masked end), offset (n: the peaks before row i), peaks (max_peaks x 2, ascending (i, j)) and report[4].
// launch_loop_list: at (Q x L x 6) and closed (Q x 2) for the L pairs of `list` (device, L x 2).  launch_loop_apa: apa
// (Q x (2w+1)^2) and p2ll (Q).
constexpr int kLoopTile = 32;         // k_loop_scan: a workgroup owns kLoopTile x kLoopTile pixels
struct LoopJob {
    int n, Q, has_if, n_models, consensus, p, w, min_sep, max_sep, s_lo, S;
    const double* xyz;
    const int* pick;
    const int* mask;
    const double* band_if;
    double* band_cons;
    double* expected;
};
struct LoopPeakRule {
    double thr[4];                    // donut, lower-left, horizontal, vertical
    double min_obs;
};
hipError_t launch_loop_expected(const LoopJob& job, hipStream_t s);
hipError_t launch_loop_scan(const LoopJob& job, const LoopPeakRule& rule, double* ratio, unsigned char* cand, hipStream_t s);
hipError_t launch_loop_peaks(const LoopJob& job, int merge, int max_peaks, const unsigned char* cand, unsigned char* peak, int* rows, int* offset, int* peaks, int* report,
                             hipStream_t s);
hipError_t launch_loop_list(const LoopJob& job, const int* list, int L, double* at, int* closed, hipStream_t s);
hipError_t launch_loop_apa(const LoopJob& job, const int* list, int L, int corner, double* apa, double* p2ll, hipStream_t s);
// Entanglement of a model (c3d_entanglement; k_ent_*, c3d_score_entangle.inc).  xyz: K models of n x 3 doubles on the device; S = n - 1
// segments; a pair of segments is counted when min_sep <= |s - t| <= max_sep (max_sep already resolved: never 0 here).
// launch_entangle_rows: seg_writhe, seg_acn (K x S) = a segment's sums of g and |g| over its counted partners, writhe, acn (K) = their sums.
// launch_entangle_table: link, link_abs (K x D x D) = the sums over the pairs of domain p with domain q, domains the runs
// bounds[p] .. bounds[p+1] - 1 (bounds: D + 1 ints on the device); (p, q) and (q, p) hold the same bits.
hipError_t launch_entangle_rows(const double* xyz, int n, int K, int min_sep, int max_sep, double* seg_writhe, double* seg_acn, double* writhe, double* acn,
                                hipStream_t s);
hipError_t launch_entangle_table(const double* xyz, int n, int K, int min_sep, int max_sep, const int* bounds, int D, double* link, double* link_abs,
                                 hipStream_t s);
// Two contact maps against one another (c3d_map_similarity; k_sim_*, c3d_score_mapsim.inc).  maps: n_maps matrices of n x n doubles on the
// device; strata lo <= s <= hi, S = hi - lo + 1.  launch_mapsim_smooth: band (n_maps x S x n, cleared here) = row s - lo of map m holds the
// smoothed X_m(i, i + s) at half-width h for i < n - s, zeros behind.  launch_mapsim_strata: moments and counts (P x S x 3, P the pairs
// p < q in the order (0,1), (0,2), ..., (1,2), ...) = { Cxy, Cxx, Cyy } and { N, A, B } of include/c3d.h's definitions 2 to 4.
// pair index -> (p, q), p < q
__host__ __device__ inline void mapsim_pair(int idx, int n_maps, int* p, int* q) {
    int a = 0;
    while (idx >= n_maps - 1 - a) { idx -= n_maps - 1 - a; ++a; }
    *p = a;
    *q = a + 1 + idx;
}
hipError_t launch_mapsim_smooth(const double* maps, int n, int n_maps, int h, int lo, int hi, double* band, hipStream_t s);
hipError_t launch_mapsim_strata(const double* band, int n, int n_maps, int lo, int hi, bool keep_zeros, double* moments, long long* counts, hipStream_t s);

// Target matrix entry: NOE target in Angstrom, 0 = no restraint (host c3d_set_restraints and K1).
inline float encode_target_host(float t) { return t > 0 ? t : 0.0f; }

}  // namespace c3d
