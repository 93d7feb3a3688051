// c3d_config.cpp — host unit of libc3d.so: the context's configuration.  The defaults, c3d_set_model, c3d_set_schedule, c3d_set_option and
// c3d_get_stat — the last two as one table each, a row per key — and the configuration as the kernels take it (dev_model, dev_step, dev_fire).
#include <climits>

#include "c3d_ctx.h"

using namespace c3d::host;

namespace {
// the length the clamp form divides (d - t) by: rswitch, or mrswitch for device potential 4 (1 / DevModel::inv_rs in either case)
float clamp_scale(const c3d_ctx* c) { return dev_model(c).noe_pot == 4 ? c->model.mrswitch : c->model.rswitch; }

// What a change of configuration (c3d_set_model / c3d_set_schedule / c3d_set_option) makes stale
enum Stale : unsigned { STALE_REPLICAS = 1, STALE_GRAPHS = 2, STALE_PAIR_TARGETS = 4, STALE_PROGRAM = 8 };
// the caller holds the gate when this releases anything device-side (drop_stale_gated)
void drop_stale(c3d_ctx* c, unsigned stale) {
    if (stale & STALE_REPLICAS) free_replica_buffers(c);
    if (stale & STALE_PAIR_TARGETS) dev_free(c->buf.tgs2);
    if (stale & STALE_PROGRAM) build_program(c);       // drops the graphs
    else if (stale & STALE_GRAPHS) drop_graphs(c);
}
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
bool holds_lbfgs_stage(const c3d_ctx* c) { return std::any_of(c->stages.begin(), c->stages.end(), [](const c3d_stage& s) { return s.kind == c3d::kLbfgs; }); }

// ---- options: how a row admits a value.  Each stores the value and returns nullptr, or returns the refusal (the row's, handed in, unless
// the key has a second one) and stores nothing.  M is the member of c3d_ctx the key sets.
using Admit = const char* (*)(c3d_ctx* c, double value, const char* refusal);
template <class Member, class V> const char* store(Member& m, V v) { m = v; return nullptr; }
template <auto M> const char* flag(c3d_ctx* c, double v, const char*) { return store(c->*M, v != 0); }
template <auto M> const char* tristate(c3d_ctx* c, double v, const char*) { return store(c->*M, v < 0 ? -1 : (v != 0)); }
template <auto M, int... Set> const char* one_of(c3d_ctx* c, double v, const char* refusal) { return ((v != Set) && ...) ? refusal : store(c->*M, (int)v); }
template <auto M, int Lo, int Hi> const char* whole_in(c3d_ctx* c, double v, const char* refusal) { return v != (int)v || v < Lo || v > Hi ? refusal : store(c->*M, (int)v); }
template <auto M, int Lo, int Hi> const char* truncated_in(c3d_ctx* c, double v, const char* refusal) { return v < Lo || v > Hi ? refusal : store(c->*M, (int)v); }   // 1.5 is admitted as 1
template <auto M, bool (*Valid)(int)> const char* chunk(c3d_ctx* c, double v, const char* refusal) { return v != (int)v || (v != 0 && !Valid((int)v)) ? refusal : store(c->*M, (int)v); }   // 0 or of the instantiated set
// the keys with logic of their own
const char* set_resident(c3d_ctx* c, double v, const char*) { c->resident_skip = 0; return store(c->resident, v < 0 ? -1 : (v != 0)); }
const char* set_precision(c3d_ctx* c, double v, const char* refusal) {
    if (v != 32 && v != 64) return refusal;
    if (v == 64 && !c->f64_lbfgs && holds_lbfgs_stage(c)) return "precision 64: the schedule holds a stage of kind 8 (L-BFGS), which has no fp64 form";
    return store(c->precision, (int)v);
}
const char* set_f64_lbfgs(c3d_ctx* c, double v, const char* refusal) {
    if (v != 0 && v != 1) return refusal;
    if (v == 0 && c->precision == 64 && holds_lbfgs_stage(c)) return "f64_lbfgs: precision is 64 and the schedule holds a stage of kind 8 (L-BFGS); change one of them first";
    return store(c->f64_lbfgs, v != 0);
}
const char* set_symmetric(c3d_ctx* c, double v, const char*) { return store(c->sym, v > 0); }
const char* set_static_placement(c3d_ctx* c, double v, const char*) { c->inject_misplaced = v == 2; return store(c->static_place, v != 0); }
const char* set_num_xcc(c3d_ctx* c, double v, const char*) { return store(c->num_xcc, (int)v); }               // unchecked
const char* set_xcd_count(c3d_ctx* c, double v, const char* refusal) { return (int)v < 1 || (int)v > 8 || c->xcd_base + (int)v > 8 ? refusal : store(c->xcd_count, (int)v); }
const char* set_xcd_base(c3d_ctx* c, double v, const char* refusal) { return (int)v < 0 || (int)v + c->xcd_count > 8 ? refusal : store(c->xcd_base, (int)v); }
const char* set_late_tiles(c3d_ctx* c, double v, const char*) { return store(c->cluster_late, v != 0 ? -1 : 0); }
const char* set_spin_wait(c3d_ctx* c, double v, const char*) { return store(c->spin_wait_us, v < 0 ? 0 : v); }
const char* set_resident_min_ops(c3d_ctx* c, double v, const char*) { return store(c->resident_min_ops, v < 1 ? 1 : (int)v); }
const char* set_graph_chunk(c3d_ctx* c, double v, const char* refusal) { return v < 8 ? refusal : store(c->graph_chunk, (int)v & ~1); }   // even: a chunk returns to the starting parity

constexpr unsigned R = STALE_REPLICAS, G = STALE_GRAPHS, T = STALE_PAIR_TARGETS, P = STALE_PROGRAM;
using X = c3d_ctx;
// One row per key of c3d_set_option (c3d.h describes them).  `stale` is what a new value invalidates: R the replica state — such a key is
// to be set before c3d_init_replicas —, G the cached graphs, T the pair targets, P the launch program (and with it the graphs).
const struct Option { const char* key; unsigned stale; Admit admit; const char* refusal; } kOptions[] = {
    {"use_graph",                 0,     flag<&X::use_graph>},
    {"rows_per_wave",             G,     one_of<&X::rpw, 1, 2, 4>, "rows_per_wave must be 1, 2 or 4"},
    {"replica_groups",            G,     truncated_in<&X::ngroups, 1, X::kMaxGroups>, "replica_groups must be 1..4"},
    {"event_timing",              0,     flag<&X::event_timing>},
    {"kernel_timing",             0,     flag<&X::kernel_timing>},
    {"resident",                  0,     set_resident},
    {"precision",                 R | G, set_precision, "precision must be 32 or 64"},
    {"eval_rows_per_wave",        0,     one_of<&X::eval_rpw, 2, 4, -2>, "eval_rows_per_wave must be 4, 2 (packed pair term) or -2 (two rows per wave, scalar pair term)"},
    {"pair_targets",              T | G, flag<&X::pair_targets>},
    {"wide_tiles",                G,     flag<&X::wide_tiles>},
    {"symmetric",                 R | G, set_symmetric},   // takes effect at the next c3d_init_replicas
    {"start",                     0,     one_of<&X::start_mode, 0, 1>, "start must be 0 (random coil) or 1 (extended strand)"},
    {"cluster",                   0,     tristate<&X::cluster>},
    {"resident_inject_timeout",   0,     flag<&X::inject_timeout>},
    {"narrow_columns",            R | G, flag<&X::narrow_columns>},
    {"cluster_static_placement",  0,     set_static_placement},   // 0: per-XCD atomic slot counters; 2: test hook
    {"cluster_inject_incomplete", 0,     flag<&X::inject_incomplete>},
    {"cluster_num_xcc",           R,     set_num_xcc},   // test hook: pretend a partitioned device
    {"prefetch_ranks",            0,     flag<&X::prefetch_ranks>},
    {"device_ranks",              0,     one_of<&X::device_ranks, -1, 0, 1>, "device_ranks is 0 (the device beyond 5120 beads), 1 (the device for every symmetric matrix) or -1 (the host)"},
    {"final_minimiser_steps",     P,     truncated_in<&X::bb_steps, 2, INT_MAX>, "c3d_set_option: final_minimiser_steps >= 2"},
    {"final_minimiser",           P,     one_of<&X::final_bb, 0, 1>, "c3d_set_option: final_minimiser is 0 (FIRE) or 1 (two-point step size)"},
    {"lbfgs_memory",              G,     whole_in<&X::lbfgs_mem, 1, c3d::kLbfgsMaxPairs>, "c3d_set_option: lbfgs_memory is 1..8"},   // from the next stage's first step
    {"cluster_xcd_count",         R,     set_xcd_count, "cluster_xcd_count: 1..8, and cluster_xcd_base + cluster_xcd_count <= 8"},   // re-plans
    {"cluster_xcd_base",          0,     set_xcd_base, "cluster_xcd_base: 0 .. 8 - cluster_xcd_count"},   // (the plan depends on the count only)
    {"cluster_late_tiles",        R,     set_late_tiles},
    {"cluster_geometry",          R,     truncated_in<&X::cluster_geom, 0, 1699>, "cluster_geometry = 100 compute waves + 10 rows per wave + helper waves"},
    {"spin_wait_us",              0,     set_spin_wait},
    {"resident_min_ops",          0,     set_resident_min_ops},
    {"stage_dma",                 G,     flag<&X::stage_dma>},
    {"max_beads",                 0,     whole_in<&X::max_beads, C3D_MAX_BEADS_DEFAULT, C3D_MAX_BEADS_LIMIT>, "max_beads must be an integer from 5120 to 16384"},
    {"embed_max_beads",           0,     whole_in<&X::embed_max_beads, C3D_EMBED_MAX_BEADS_DEFAULT, C3D_EMBED_MAX_BEADS_LIMIT>, "embed_max_beads must be an integer from 4549 to 16384"},
    {"f64_max_beads",             0,     whole_in<&X::f64_max_beads, C3D_F64_MAX_BEADS_DEFAULT, C3D_F64_MAX_BEADS_LIMIT>, "f64_max_beads must be an integer from 2560 to 16384"},
    {"f64_lbfgs",                 0,     set_f64_lbfgs, "f64_lbfgs must be 0 or 1"},   // releases nothing on the device
    {"f64_column_chunk",          G,     chunk<&X::f64_column_chunk, c3d::column_chunk64_valid>, "f64_column_chunk must be 0 (by size), 256, 512 or 1024"},
    {"embed_form",                0,     one_of<&X::embed_form, 0, 1>, "embed_form is 0 (k_dg_eig while it fits, tiled beyond) or 1 (tiled)"},
    {"embed_batch",               0,     whole_in<&X::embed_batch, 0, INT_MAX>, "embed_batch is 0 (by the scratch budget) or a number of replicas"},
    {"column_chunk",              G,     chunk<&X::column_chunk, c3d::column_chunk_valid>, "column_chunk must be 0 (the library's choice), 256, 1024 or 2048"},
    {"graph_chunk",               G,     set_graph_chunk, "graph_chunk must be >= 8"},
};

// ---- stats: a row reads a value on the host (get) or enters the device for it (enter)
template <auto M> double value(const c3d_ctx* c) { return (double)(c->*M); }
template <auto M> double planned(const c3d_ctx* c) { return c->cl_ok ? (double)(c->cl_plan.*M) : 0.0; }   // of the multi-step plan in force
// max over the replicas of the RMS force component at the last minimiser evaluation (what c3d_run compares with gtol); meaningful after a
// FIRE step only
int rms_force(const c3d_ctx* c, double* out) {
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_get_stat: rms_force needs replicas");
    C3D_ENTRY(c, 0u);
    return max_rms_force(const_cast<c3d_ctx*>(c), out);      // (writes *out only where it succeeds)
}
// memory drops of the last L-BFGS stage, summed over the replicas (device state of the parity its last step wrote)
int lbfgs_resets(const c3d_ctx* c, double* out) {
    *out = 0;
    const c3d::LbfgsState* dev = c->lbfgs_parity < 0 ? nullptr : c->precision == 64 ? c->lb64.S[c->lbfgs_parity] : c->lb.S[c->lbfgs_parity];
    if (!dev) return C3D_OK;
    C3D_ENTRY(c, 0u);
    if (int rc = read_back(const_cast<c3d_ctx*>(c), dev, sizeof(c3d::LbfgsState) * c->nrep)) return rc;
    const c3d::LbfgsState* h = static_cast<const c3d::LbfgsState*>(c->h_stage);
    long r = 0;
    for (int k = 0; k < c->nrep; ++k) r += h[k].resets;
    *out = (double)r;
    return C3D_OK;
}
// One row per key of c3d_get_stat (c3d.h describes them)
const struct Stat { const char* key; double (*get)(const c3d_ctx*); int (*enter)(const c3d_ctx*, double*); } kStats[] = {
    {"graph_captures", value<&X::graph_captures>},
    {"last_kernel_us", [](const c3d_ctx* c) { return 1e3 * c->last_kernel_ms; }},
    {"last_host_launch_us", value<&X::last_host_launch_us>},
    {"last_host_sync_us", value<&X::last_host_sync_us>},
    {"graph_launches", value<&X::graph_launches>},
    {"graphs_cached", [](const c3d_ctx* c) { return (double)c->graphs.size(); }},
    {"step_launches", value<&X::step_launches>},
    {"resident_launches", value<&X::resident_launches>},
    {"cluster_launches", value<&X::cluster_launches>},
    {"resident_fallbacks", value<&X::resident_fallbacks>},
    {"cluster_incomplete", value<&X::cluster_incomplete>},
    {"spin_completions", value<&X::spin_completions>},
    {"cluster_static_placement", value<&X::static_place>},
    {"cluster_placement_mismatches", value<&X::placement_mismatches>},
    {"num_xcc", value<&X::num_xcc>},
    {"rms_force", nullptr, rms_force},
    {"lbfgs_steps", value<&X::lbfgs_steps>},
    {"lbfgs_resets", nullptr, lbfgs_resets},
    {"k1_recomputed", value<&X::k1_recomputed>},
    {"k1_patched", value<&X::k1_patched>},
    {"last_path", value<&X::last_path>},
    {"rank_prefetch_hits", value<&X::rank_prefetch_hits>},
    {"device_rank_runs", value<&X::device_rank_runs>},
    {"score_wide_runs", value<&X::score_wide_runs>},
    {"compare_runs", value<&X::compare_runs>},
    {"f64_evals", value<&X::f64_evals>},
    {"superpose_runs", value<&X::superpose_runs>},
    {"rmsd_table_runs", value<&X::rmsd_table_runs>},
    {"ensemble_map_runs", value<&X::ensemble_map_runs>},
    {"ensemble_score_runs", value<&X::ensemble_score_runs>},
    {"geometry_runs", value<&X::geometry_runs>},
    {"separation_runs", value<&X::separation_runs>},
    {"stratified_runs", value<&X::stratified_runs>},
    {"stratified_if_ms", value<&X::stratified_if_ms>},
    {"stratified_models_ms", value<&X::stratified_models_ms>},
    {"bead_runs", value<&X::bead_runs>},
    {"bead_if_ms", value<&X::bead_if_ms>},
    {"bead_models_ms", value<&X::bead_models_ms>},
    {"cluster_xcd_count", value<&X::xcd_count>},
    {"cluster_xcd_base", value<&X::xcd_base>},
    {"cluster_ok", value<&X::cl_ok>},
    {"cluster_parts", planned<&c3d::ClusterPlan::parts>},
    {"cluster_rows_per_wave", planned<&c3d::ClusterPlan::rpw>},
    {"cluster_late_tiles", planned<&c3d::ClusterPlan::late_tiles>},
    {"cluster_compute_waves", planned<&c3d::ClusterPlan::cw>},
    {"cluster_helper_waves", planned<&c3d::ClusterPlan::helpers>},
    {"cluster_wgs_per_cu", planned<&c3d::ClusterPlan::wgs_per_cu>},
    {"replica_groups", [](const c3d_ctx* c) { return (double)active_groups(c); }},
    {"embed_form", value<&X::last_embed_form>},
    {"embed_batches", value<&X::last_embed_batches>},
    {"units_loaded", [](const c3d_ctx*) { return (double)units_loaded(); }},                           // code objects this PROCESS has loaded (all devices)
    {"units_loaded_mask", [](const c3d_ctx* c) { return (double)units_loaded_mask(c->device); }},      // bit per unit, this context's device
};

template <class Row, size_t N> const Row* find_row(const Row (&rows)[N], const char* key) {
    for (const Row& r : rows) if (!strcmp(key, r.key)) return &r;
    return nullptr;
}
}  // namespace

namespace c3d::host {
const char* option_key(int k) { return k >= 0 && k < (int)std::size(kOptions) ? kOptions[k].key : nullptr; }
const char* stat_key(int k) { return k >= 0 && k < (int)std::size(kStats) ? kStats[k].key : nullptr; }

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
c3d::DevFire dev_fire(const c3d_ctx* c) {
    c3d::DevFire f;
    f.dt_start = c->fire.dt_start; f.dt_max = c->fire.dt_max; f.f_inc = c->fire.f_inc; f.f_dec = c->fire.f_dec;
    f.alpha_start = c->fire.alpha_start; f.f_alpha = c->fire.f_alpha; f.max_step = c->fire.max_step; f.n_min = c->fire.n_min;
    return f;
}
}  // namespace c3d::host

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
        if (st[k].kind == c3d::kLbfgs && c->precision == 64 && !c->f64_lbfgs)
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
    const Option* row = find_row(kOptions, key);
    if (!row) return fail(C3D_ERR_INVALID, std::string("unknown option ") + key);
    if (const char* refusal = row->admit(c, value, row->refusal)) return fail(C3D_ERR_INVALID, refusal);
    return drop_stale_gated(c, row->stale);
}

extern "C" int c3d_get_stat(const c3d_ctx* c, const char* key, double* value) {
    if (!c || !key || !value) return fail(C3D_ERR_INVALID, "c3d_get_stat: null argument");
    const Stat* row = find_row(kStats, key);
    if (!row) return fail(C3D_ERR_INVALID, std::string("c3d_get_stat: unknown key ") + key);
    if (row->enter) return row->enter(c, value);
    *value = row->get(c);
    return C3D_OK;
}
