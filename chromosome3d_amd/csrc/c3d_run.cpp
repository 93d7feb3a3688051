// c3d_run.cpp — host unit of libc3d.so: schedule -> launch program and its executor, the L-BFGS and pair-target allocations, timing,
// c3d_run_steps / c3d_run / c3d_centre.  (The table test hooks of the step texts are a unit of their own: c3d_debug.cpp.)
// Reference boundary: chromosome3D.pl:254-289 (build_models: `cns_solve < dgsa.inp`) and the deck it writes (:882-1846).  What CNS does per
// model (deck :1574-1829) becomes a flat "program" of SA steps; a range of it runs as ONE cluster launch (run_cluster, c3d_cluster.hip) where
// the replicas fit the chip's XCDs, else as one launch per step (two replica groups on two streams, replayed from hipGraphs).  Every copy
// and memset is ordered on the context's own stream: contexts of different host threads never meet on the legacy stream.
#include <chrono>

#include "c3d_ctx.h"

using namespace c3d::host;

// ---- what the other host units call (c3d_ctx.h)
namespace c3d::host {
void drop_graphs(c3d_ctx* c) {
    for (auto& kv : c->graphs) (void)hipGraphExecDestroy(kv.second);
    c->graphs.clear();
}

// The kind step k of a minimiser stage runs; kinds 3 / 6 / 9 = first step of a method's run (fresh state).  A stage of kind 5 starts with the
// two-point step-size minimiser (kinds 6 / 5) and hands over to FIRE (3 / 2) after nbb = bb_steps of them if the exit test has not ended the
// stage by then: the two-point method has no descent guarantee — one replica in a few hundred ends in a cycle of long moves instead of a
// minimum — and FIRE finishes what it leaves (the CPU restatement does the same: c3o_run_schedule).  Option final_minimiser = 0 (nbb = 0): kind
// 5 runs as FIRE throughout.  A stage of kind 8 runs L-BFGS (kinds 9 / 8) for its first final_minimiser_steps steps and hands over to FIRE the
// same way; option final_minimiser does not apply to it.
static int minimiser_step_kind(int stage_kind, int k, int nbb) {
    if (k >= nbb) return k == nbb ? kFireFirst : kFire;
    return stage_kind == kLbfgs ? (k == 0 ? kLbfgsFirst : kLbfgs) : (k == 0 ? kTwoPointFirst : kTwoPoint);
}

void build_program(c3d_ctx* c) {
    c->program.clear();
    for (size_t s = 0; s < c->stages.size(); ++s) {
        const c3d_stage& st = c->stages[s];
        if (stage_is_minimiser(st.kind)) {
            const int nbb = (st.kind == kTwoPoint && c->final_bb) || st.kind == kLbfgs ? std::min(st.nsteps, c->bb_steps) : 0;
            for (int k = 0; k < st.nsteps; ++k)
                c->program.push_back({dev_step(c, minimiser_step_kind(st.kind, k, nbb), 0.0f, st.w_all, st.w_vdw, st.repel_s, 0.0f), (int)s, true});
        } else {
            if (s == 0 || stage_is_minimiser(c->stages[s - 1].kind))      // MD begins
                c->program.push_back({dev_step(c, kMdBegin, 0.0f, st.w_all, st.w_vdw, st.repel_s, st.t_bath), (int)s, false});
            for (int k = 0; k < st.nsteps; ++k)
                c->program.push_back({dev_step(c, st.kind, st.dt, st.w_all, st.w_vdw, st.repel_s, st.t_bath), (int)s, true});
        }
    }
    c->pc = 0;
    c->zero_weight = c->has_two_point = c->has_lbfgs = false;
    for (const Op& op : c->program) { c->zero_weight |= op.p.w_rs == 0.0f; c->has_two_point |= kind_is_two_point(op.p.kind); c->has_lbfgs |= kind_is_lbfgs(op.p.kind); }
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

int active_groups(const c3d_ctx* c) { return std::min(c->ngroups, std::max(c->nrep, 1)); }

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
}  // namespace c3d::host

namespace {
void group_range(const c3d_ctx* c, int g, int& base, int& count) {
    const int G = active_groups(c);
    const int q = c->nrep / G, r = c->nrep % G;
    base = g * q + std::min(g, r);
    count = q + (g < r ? 1 : 0);
}

// The symmetric-tile kernels evaluate the clamp form only (k_pairs_sym reads rs and mrs, not the tails): decided per op from the model in
// force, which c3d_set_model may change on a live context; a general tail runs k_step's general form.  The tile list and slabs exist
// whenever `symmetric` is on (c3d_init_replicas).
bool use_sym(const c3d_ctx* c) {
    return c->sym > 0 && c->d_sym_scratch && !c3d::general_tail(dev_model(c));
}

// The L-BFGS history (2 x 8 pairs x 3 x cols elements a replica: sized for the largest memory, so that lbfgs_memory never reallocates), the
// tile sums and the state, zeroed; allocated outside any stream capture (run_ops_segment), freed with the replica buffers.  T = float with
// LbfgsBuffers and npad columns, double with LbfgsBuffers64 and cols64(n) columns (6.3 MB a replica at 16384 beads)
template <class T, class Buffers>
int ensure_lbfgs(c3d_ctx* c, Buffers& lb, int cols) {
    if (lb.hist) return C3D_OK;
    const size_t hist = c3d::lbfgs_hist_floats(cols) * c->nrep, part = (size_t)c->nrep * c->ntiles * c3d::kLbfgsQ;
    HIP_TRY(hipMalloc(&lb.hist, sizeof(T) * hist));
    HIP_TRY(hipMalloc(&lb.part, sizeof(T) * part));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMalloc(&lb.S[k], sizeof(c3d::LbfgsState) * c->nrep));
    HIP_TRY(hipMemsetAsync(lb.hist, 0, sizeof(T) * hist, c->stream));
    HIP_TRY(hipMemsetAsync(lb.part, 0, sizeof(T) * part, c->stream));
    for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(lb.S[k], 0, sizeof(c3d::LbfgsState) * c->nrep, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // the step launches run on the group streams
    return C3D_OK;
}

// Per-step kernel beyond the cluster kernel's reach (no narrow column block: every n > 1024), device potential 4: the resident per-pair
// constants of row pairs (DevModel::tgs2), built on first use after the targets or the model changed
int ensure_pair_targets(c3d_ctx* c, const c3d::DevModel& m) {
    if (c->buf.tgs2 || !c->pair_targets || !c3d::pair_targets_fit(m) || c->npad <= 1024 || !c->buf.tgt) return C3D_OK;
    HIP_TRY(hipMalloc(&c->buf.tgs2, sizeof(float) * c3d::pair_targets_floats(c->n, c->npad)));
    LAUNCH_TRY("pair targets", c3d::launch_pair_targets(m, c->buf.tgt, c->buf.tgs2, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // the step launches run on the group streams
    return C3D_OK;
}
// The kernel an op runs on the per-step path and its form: launch_op launches what this says, run_ops_segment records it for the range's
// last op (a graph replay does not pass through launch_op)
// (m64: the op's fp64 model where the caller has built it, precision 64 only)
KernelRecord op_kernel(const c3d_ctx* c, const c3d::DevModel& m, const Op& op, const c3d::Model64* m64 = nullptr) {
    KernelRecord k;
    if (c->precision == 64) {
        k.family = c3d::kind_is_lbfgs(op.p.kind) ? KernelRecord::LBFGS_EVAL64 : KernelRecord::STEP64;
        k.f64 = c3d::form64(m64 ? *m64 : c3d::model64(m, c->model), c->stages[op.stage].w_all, c->f64_column_chunk);
    } else if (!c3d::kind_is_lbfgs(op.p.kind) && use_sym(c)) {      // (symmetric tiles do not apply to L-BFGS steps)
        k.family = KernelRecord::PAIRS_SYM;
        k.pot = c3d::device_pot(m.noe_pot);
        k.rs1 = c3d::sym_rs1(m);
    } else {
        k.family = c3d::kind_is_lbfgs(op.p.kind) ? KernelRecord::LBFGS_EVAL : KernelRecord::STEP;
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
        const c3d::Model64 m64 = c3d::model64(m, c->model);
        const c3d::Step64 p = c3d::step64(m64, op.p.kind, st.dt, st.w_all, st.w_vdw, st.repel_s, st.t_bath);
        const c3d::Fire64 fp = c3d::fire64(c->fire);
        const c3d::Form64 f = op_kernel(c, m, op, &m64).f64;
        if (c3d::kind_is_lbfgs(op.p.kind)) {         // two launches, as in fp32: forces + tile sums, then sums + direction + move
            hipError_t e = c3d::launch_lbfgs_eval64(m, m64, p, f, c->b64, c->lb64, par, c->lbfgs_mem, c->gstream[g]);
            if (e == hipSuccess) e = c3d::launch_lbfgs_move64(m, m64, p, fp, c->b64, c->lb64, par, c->lbfgs_mem, c->gstream[g]);
            LAUNCH_TRY("fp64 L-BFGS step launch", e);
        } else LAUNCH_TRY("fp64 step launch", c3d::launch_step64(m, m64, p, fp, f, c->b64, par, c->gstream[g]));
        return C3D_OK;
    }
    const KernelRecord k = op_kernel(c, m, op);
    if (k.family == KernelRecord::LBFGS_EVAL) {       // two launches: forces + tile sums, then sums + direction + move
        hipError_t e = c3d::launch_lbfgs_eval(m, op.p, c->buf, c->lb, par, c->lbfgs_mem, k.step, c->gstream[g]);
        if (e == hipSuccess) e = c3d::launch_lbfgs_move(m, op.p, dev_fire(c), c->buf, c->lb, par, c->lbfgs_mem, c->gstream[g]);
        LAUNCH_TRY("L-BFGS step launch", e);
        return C3D_OK;
    }
    LAUNCH_TRY("step launch", k.family == KernelRecord::PAIRS_SYM
                                  ? c3d::launch_step_sym(m, op.p, dev_fire(c), c->buf, par, c->d_sym_tiles, c->d_sym_scratch, c->gstream[g])
                                  : c3d::launch_step(m, op.p, dev_fire(c), c->buf, par, k.step, c->gstream[g]));
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

// ops [pc, pc + nops) ran in `launches` launches: the counted steps among them, the program counter
void account_ops(c3d_ctx* c, size_t nops, long launches) {
    for (size_t k = 0; k < nops; ++k)
        if (c->program[c->pc + k].counted) { ++c->steps_done; ++c->last_steps; }
    c->last_launches += launches;
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
    for (size_t k = 0; k < nops && !pl.two_point; ++k) pl.two_point = c3d::kind_is_two_point(c->program[c->pc + k].p.kind);
    c->inject_misplaced = false;
    c->h_tmo[2] = 0;
    const auto h0 = std::chrono::steady_clock::now();
    LAUNCH_TRY("cluster launch", c3d::launch_cluster(m, dev_fire(c), pl, c3d::anneal_io(c->buf, c->parity), c->buf.tgt, c->d_crec, c->d_prog,
                                                     c->op_run[c->pc], c->op_skip[c->pc], (int)nops, seq << 20, c->h_tmo_dev,
                                                     c->d_claim + c3d_ctx::kClaimWords * seq, c->stream));
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
    c->parity ^= 1;
    account_ops(c, nops, 1);
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

// run program ops [pc, pc + nops): eager or via cached graphs; every replica group advances on its own stream (fork from / join into
// stream 0 around the call)
int run_ops_segment(c3d_ctx* c, size_t nops, bool zero_w, bool lbfgs = false) {
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
        if (int rc = c->precision == 64 ? ensure_lbfgs<double>(c, c->lb64, c3d::cols64(c->n)) : ensure_lbfgs<float>(c, c->lb, c->npad)) return rc;
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
                    if (int rc = launch_op(c, c->program[c->pc + k], g, par)) return rc;
                    par ^= 1;
                }
            }
        } else {
            // one graph per (range, parity, group); homogeneous minimiser ranges (same stage, all kind 2, all 5 or all 8) share a graph
            // regardless of pc (kind 8 keeps its ring head and counts on the device); a stage of kind 5 or 8 has a minimiser part and a FIRE part
            const Op& first = c->program[c->pc];
            const Op& last = c->program[c->pc + chunk - 1];
            const int kd = first.p.kind, method = kd == c3d::kTwoPoint ? 1 : kd == c3d::kLbfgs ? 2 : 0;        // (0 FIRE, 1 two-point, 2 L-BFGS)
            long sig = (long)c->pc;
            if (!c3d::kind_is_md(kd) && !c3d::kind_is_first(kd) && last.p.kind == kd && first.stage == last.stage) sig = -(long)(first.stage + 1) - 1000000L * method;
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
                    LAUNCH_TRY("hipStreamEndCapture", ce);
                    hipGraphExec_t ge = nullptr;
                    hipError_t ie = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
                    (void)hipGraphDestroy(gr);
                    LAUNCH_TRY("hipGraphInstantiate", ie);
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
        account_ops(c, chunk, (long)chunk);
        done += chunk;
    }
    for (int g = 1; g < G; ++g) {
        HIP_TRY(hipEventRecord(c->gev[g], c->gstream[g]));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->gev[g], 0));
    }
    if (c->precision == 64) {
        // the fp32 buffers of the current parity receive a copy of the state (read-back, energies, scoring, the minimiser's exit test)
        LAUNCH_TRY("fp64 export", c3d::launch_export64(dev_model(c), c->b64, c->parity, c->buf.X[c->parity], c->buf.V[c->parity], c->buf.P[c->parity], c->stream));
        c->last_path = 3;
    }
    c->ran = op_kernel(c, dev_model(c), c->program[c->pc - 1]);
    return C3D_OK;
}

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
        const bool z = !p64 && p0.w_rs == 0.0f, tp = !p64 && c3d::kind_is_two_point(p0.kind), lb = c3d::kind_is_lbfgs(p0.kind);
        size_t k = 1;
        while (c->pc + k < end) {
            const c3d::DevStep& p = c->program[c->pc + k].p;
            if ((!p64 && p.w_rs == 0.0f) != z || (!p64 && c3d::kind_is_two_point(p.kind)) != tp || c3d::kind_is_lbfgs(p.kind) != lb) break;
            ++k;
        }
        if (int rc = run_ops_segment(c, k, z, lb)) return rc;
    }
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

// are the last step's per-tile sums (functions of every velocity / force component) all finite?
int partials_finite(c3d_ctx* c, bool* ok) {
    const size_t cnt = (size_t)c->nrep * c->ntiles * 4;
    if (int rc = read_back(c, c->buf.P[c->parity], sizeof(float) * cnt)) return rc;
    const float* h = static_cast<const float*>(c->h_stage);
    *ok = true;
    for (size_t k = 0; k < cnt; ++k) if (!std::isfinite(h[k])) { *ok = false; break; }
    return C3D_OK;
}
}  // namespace

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
    if (int rc = begin_timing(c)) return rc;
    if (int rc = run_ops(c, nops)) return rc;
    if (int rc = end_timing(c)) return rc;
    if (done) *done = counted;
    return C3D_OK;
}

extern "C" int c3d_centre(c3d_ctx* c) {
    if (!c || !c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_centre: bad state");
    C3D_ENTRY(c, 0u);
    LAUNCH_TRY("centre launch", c3d::launch_centre(dev_model(c), c->buf, c->parity, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

extern "C" int c3d_run(c3d_ctx* c) {
    if (!c) return fail(C3D_ERR_INVALID, "c3d_run: null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_run: call c3d_init_replicas first");
    C3D_ENTRY(c, 0u);
    if (int rc = begin_timing(c)) return rc;
    const int last_stage = (int)c->stages.size() - 1;
    const bool early = c->gtol > 0.0f && last_stage >= 0 && c3d::stage_is_minimiser(c->stages[last_stage].kind);
    // everything before the final minimisation
    size_t nfixed = c->program.size() - c->pc;
    if (early) {
        nfixed = 0;
        while (c->pc + nfixed < c->program.size() && c->program[c->pc + nfixed].stage != last_stage) ++nfixed;
    }
    if (int rc = run_ops(c, nfixed)) return rc;
    if (early) {
        // chunks of exactly check_every steps (> 0: c3d_set_schedule) until every replica's RMS force < gtol: the test falls after the steps
        // c3o_run_schedule tests, (it + 1) % check_every == 0 counted from the stage's start.  Odd or even: a range of any length runs from
        // either parity, and the sums read here and the graph keys follow c->parity.
        while (c->pc < c->program.size()) {
            const size_t chunk = std::min<size_t>((size_t)c->check_every, c->program.size() - c->pc);
            if (int rc = run_ops(c, chunk)) return rc;
            double rms = 0;
            if (int rc = max_rms_force(c, &rms)) return rc;
            if (rms < c->gtol) break;
        }
        c->pc = c->program.size();
    }
    LAUNCH_TRY("centre launch", c3d::launch_centre(dev_model(c), c->buf, c->parity, c->stream));
    c->ev1_recorded = false;                       // work was queued behind the last multi-step launch
    if (int rc = end_timing(c)) return rc;
    // a blown-up trajectory (NaN/Inf) must not reach the caller as a "model"
    bool finite = true;
    if (int rc = partials_finite(c, &finite)) return rc;
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
