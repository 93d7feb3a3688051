// config_transcript.cpp — what the configuration entries of libc3d.so do to a context, as text (tests/test_config_transcript.py holds it
// against tests/golden/config_transcript.txt byte for byte).
//
// The host units run here on the CPU against the fake HIP layer of tools/sanitize/hip_stub.cpp: plain g++, no sanitizer.  Every call of
// c3d_set_option / c3d_set_model / c3d_set_schedule / c3d_get_stat below becomes one line of four tab-separated fields:
//     the call <TAB> its return code <TAB> c3d_last_error() when the code is not 0 <TAB> what changed
// `"` in the third field stands for the text of the line above; the fourth holds the watched context members that differ from the line
// before, as `name: old -> new` joined by `; ` (for c3d_get_stat: `value <%.17g>`).  A line `# <state> <what>` opens a fresh context:
//     A  as c3d_create leaves it
//     B  targets from a 40 x 40 matrix, 4 replicas, fp32, eight steps on the per-step path (cluster 0, resident 0): graphs are cached; a stand-in for
//        the pair targets, which 40 beads are too few for
//     C  the same at precision 64: the fp64 state exists
// Only the first context of a state prints its set-up; the later ones must reach the same members (a `set-up differs` line otherwise).
// Everything printed is an integer, a string or a value that was stored as given, never the result of floating-point arithmetic: the
// file is the same on every machine.
//
// The two key lists are this program's OWN (sorted, each key once), not the library's: a key the library gains or loses without this file
// shows as a difference.  `config_transcript keys` prints them beside the library's tables for the test to compare; build with
// -DC3D_NO_CONFIG_TABLES against sources older than the tables (the golden file was made that way from the commit before them).
#include "../../chromosome3d_amd/csrc/c3d_ctx.h"

namespace {
const char* const kOptions[] = {
    "cluster", "cluster_geometry", "cluster_inject_incomplete", "cluster_late_tiles", "cluster_num_xcc", "cluster_static_placement",
    "cluster_xcd_base", "cluster_xcd_count", "column_chunk", "device_ranks", "embed_batch", "embed_form", "embed_max_beads",
    "eval_rows_per_wave", "event_timing", "f64_column_chunk", "f64_lbfgs", "f64_max_beads", "final_minimiser", "final_minimiser_steps",
    "graph_chunk", "kernel_timing", "lbfgs_memory", "max_beads", "narrow_columns", "pair_targets", "precision", "prefetch_ranks",
    "replica_groups", "resident", "resident_inject_timeout", "resident_min_ops", "rows_per_wave", "spin_wait_us", "stage_dma", "start",
    "symmetric", "use_graph", "wide_tiles"};
const char* const kStats[] = {
    "bead_if_ms", "bead_models_ms", "bead_runs", "cluster_compute_waves", "cluster_helper_waves", "cluster_incomplete", "cluster_late_tiles",
    "cluster_launches", "cluster_ok", "cluster_parts", "cluster_placement_mismatches", "cluster_rows_per_wave", "cluster_static_placement",
    "cluster_wgs_per_cu", "cluster_xcd_base", "cluster_xcd_count", "compare_runs", "device_rank_runs", "embed_batches", "embed_form",
    "ensemble_map_runs", "ensemble_score_runs", "f64_evals", "geometry_runs", "graph_captures", "graph_launches", "graphs_cached",
    "k1_patched", "k1_recomputed", "last_host_launch_us", "last_host_sync_us", "last_kernel_us", "last_path", "lbfgs_resets", "lbfgs_steps",
    "num_xcc", "rank_prefetch_hits", "replica_groups", "resident_fallbacks", "resident_launches", "rms_force", "rmsd_table_runs",
    "score_wide_runs", "separation_runs", "spin_completions", "step_launches", "stratified_if_ms", "stratified_models_ms", "stratified_runs",
    "superpose_runs", "units_loaded", "units_loaded_mask"};
constexpr int kNumOptions = 39, kNumStats = 52;
static_assert(sizeof(kOptions) / sizeof(*kOptions) == kNumOptions && sizeof(kStats) / sizeof(*kStats) == kNumStats, "key counts");
// no NaN, no infinity, nothing outside int: the library casts unchecked
const double kValues[] = {-2, -1, 0, 0.5, 1, 1.5, 2, 3, 4, 5, 7, 8, 9, 9.7, 32, 64, 255, 256, 512, 1024, 1699,
                          1700, 2048, 2559, 2560, 4548, 4549, 5119, 5120, 5120.5, 16384, 16385, 1e6};
constexpr int kBeads = 40, kReplicas = 4;

using Snapshot = std::vector<std::pair<std::string, std::string>>;
std::string text(const char* fmt, double v) { char b[64]; snprintf(b, sizeof b, fmt, v); return b; }
std::string stage_text(const c3d_stage& s) {
    char b[160];
    snprintf(b, sizeof b, "(%d %d %.9g %.9g %.9g %.9g %.9g)", s.kind, s.nsteps, s.dt, s.w_all, s.w_vdw, s.repel_s, s.t_bath);
    return b;
}

// every member an option, c3d_set_model or c3d_set_schedule can write, and the state they make stale
Snapshot snapshot(const c3d_ctx* c) {
    Snapshot s;
#define INT(x) s.emplace_back(#x, std::to_string((long long)(c->x)))
#define REAL(x) s.emplace_back(#x, text("%.9g", c->x))
#define IS_NULL(x) s.emplace_back(#x " null", c->x ? "0" : "1")
    INT(use_graph); INT(rpw); INT(ngroups); INT(event_timing); INT(kernel_timing); INT(resident); INT(resident_skip); INT(resident_min_ops);
    INT(precision); INT(eval_rpw); INT(pair_targets); INT(wide_tiles); INT(sym); INT(start_mode); INT(cluster); INT(inject_timeout);
    INT(narrow_columns); INT(static_place); INT(inject_misplaced); INT(inject_incomplete); INT(num_xcc); INT(prefetch_ranks); INT(device_ranks);
    INT(bb_steps); INT(final_bb); INT(lbfgs_mem); INT(xcd_count); INT(xcd_base); INT(cluster_late); INT(cluster_geom);
    s.emplace_back("spin_wait_us", text("%.17g", c->spin_wait_us));
    INT(stage_dma); INT(max_beads); INT(embed_max_beads); INT(f64_max_beads); INT(f64_lbfgs); INT(f64_column_chunk); INT(embed_form);
    INT(embed_batch); INT(column_chunk); INT(graph_chunk);
    INT(model.min_sep); INT(model.noe_pot); INT(model.rep_sep); INT(model.ang_mode); REAL(model.s_noe); REAL(model.rswitch); REAL(model.asym);
    REAL(model.k_bond); REAL(model.b0); REAL(model.k_ang); REAL(model.a0); REAL(model.r0_rep); REAL(model.k_rep); REAL(model.mass);
    REAL(model.fbeta); REAL(model.masym); REAL(model.mrswitch); INT(model.msoexp);
    {   // a short schedule in full, a long one by the kinds and step counts of its stages
        std::string st = std::to_string(c->stages.size()) + ":";
        for (const c3d_stage& g : c->stages) st += c->stages.size() <= 4 ? stage_text(g) : " " + std::to_string(g.kind) + "x" + std::to_string(g.nsteps);
        s.emplace_back("stages", st);
    }
    REAL(fire.dt_start); REAL(fire.dt_max); REAL(fire.f_inc); REAL(fire.f_dec); REAL(fire.alpha_start); REAL(fire.f_alpha); REAL(fire.max_step);
    INT(fire.n_min); REAL(gtol); INT(check_every);
    INT(zero_weight); INT(has_two_point); INT(has_lbfgs);
    INT(have_targets); INT(have_replicas); INT(cl_ok); INT(crec_bytes); INT(lbfgs_parity); INT(prog_dirty); INT(program.size()); INT(graphs.size());
    IS_NULL(buf.X[0]); IS_NULL(buf.tgs2); IS_NULL(b64.t10); IS_NULL(b64.T);
#undef INT
#undef REAL
#undef IS_NULL
    return s;
}

struct Transcript {
    c3d_ctx* c = nullptr;
    Snapshot prev;
    std::string last_error;
    bool quiet = false;
    Snapshot reference[3];                 // what the set-up of state A / B / C reached the first time

    // one line: the call, its code, the refusal, what it changed (or `shown`, c3d_get_stat's value)
    void line(const std::string& call, int rc, const std::string& shown = "") {
        std::string err = rc ? c3d_last_error() : "", changes = shown;
        if (c) {
            const Snapshot now = snapshot(c);
            for (size_t k = 0; k < now.size(); ++k)
                if (now[k].second != prev[k].second) changes += (changes.empty() ? "" : "; ") + now[k].first + ": " + prev[k].second + " -> " + now[k].second;
            prev = now;
        }
        if (quiet && rc == 0) return;
        if (rc && err == last_error) err = "\"";
        else if (rc) last_error = err;
        std::string out = call + "\t" + std::to_string(rc) + "\t" + err + "\t" + changes;
        while (out.back() == '\t') out.pop_back();
        puts(out.c_str());
    }
    void option(const char* key, double v) { line(std::string("set_option ") + key + " " + text("%g", v), c3d_set_option(c, key, v)); }
    void stat(const char* key) {
        double v = -1;
        const int rc = c3d_get_stat(c, key, &v);
        line(std::string("get_stat ") + key, rc, rc ? "" : "value " + text("%.17g", v));
    }
    void model(const std::string& what, const c3d_model& m) { line("set_model " + what, c3d_set_model(c, &m)); }
    void schedule(const std::string& what, const std::vector<c3d_stage>& st, const c3d_fire_params* fire, float gtol, int check_every) {
        line("set_schedule " + what, c3d_set_schedule(c, st.data(), (int)st.size(), fire, gtol, check_every));
    }

    void close() { if (c) c3d_destroy(c); c = nullptr; }
    // a fresh context in state A, B or C
    void open(char state, const std::string& what) {
        close();
        printf("# %c %s\n", state, what.c_str());
        last_error.clear();
        if (c3d_create(0, &c) != C3D_OK) { printf("c3d_create failed: %s\n", c3d_last_error()); exit(1); }
        prev = snapshot(c);
        Snapshot& ref = reference[state - 'A'];
        quiet = !ref.empty();
        if (!quiet && state == 'A')
            for (const auto& m : prev) printf("default\t%s\t%s\n", m.first.c_str(), m.second.c_str());
        if (state != 'A') {
            std::vector<double> IF((size_t)kBeads * kBeads);
            for (int i = 0; i < kBeads; ++i)
                for (int j = 0; j < kBeads; ++j) IF[(size_t)i * kBeads + j] = 100.0 / (1 + (i > j ? i - j : j - i));
            line("set_if_matrix 40", c3d_set_if_matrix(c, IF.data(), kBeads, 0.5, 11.0));
            option("cluster", 0);
            option("resident", 0);
            if (state == 'C') option("precision", 64);
            line("init_replicas 4", c3d_init_replicas(c, kReplicas, 82364, 0));
            long done = 0;
            line("run_steps 8", c3d_run_steps(c, 8, &done));
            // the library builds pair targets beyond 1024 padded beads only: stand-ins, so that what releases them shows
            line("(pair targets planted)", hipMalloc(&c->buf.tgs2, 64) == hipSuccess ? 0 : 1);
        }
        if (ref.empty()) ref = prev;
        else if (ref != prev) puts("set-up differs");
        quiet = false;
    }
};

// a stage of the given kind among two plain ones
std::vector<c3d_stage> stages_with(int kind, int nsteps) {
    return {{2, 10, 0.0f, 1.0f, 20.0f, 0.5f, 0.0f}, {kind, nsteps, 0.003f, 1.0f, 1.0f, 0.85f, 300.0f}};
}

int print_keys() {
    for (const char* k : kOptions) printf("own option %s\n", k);
    for (const char* k : kStats) printf("own stat %s\n", k);
#ifndef C3D_NO_CONFIG_TABLES
    for (int k = 0; const char* key = c3d::host::option_key(k); ++k) printf("table option %s\n", key);
    for (int k = 0; const char* key = c3d::host::stat_key(k); ++k) printf("table stat %s\n", key);
#endif
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    for (int k = 1; k < kNumOptions; ++k) if (strcmp(kOptions[k - 1], kOptions[k]) >= 0) { fprintf(stderr, "option keys: not sorted at %s\n", kOptions[k]); return 2; }
    for (int k = 1; k < kNumStats; ++k) if (strcmp(kStats[k - 1], kStats[k]) >= 0) { fprintf(stderr, "stat keys: not sorted at %s\n", kStats[k]); return 2; }
    if (argc > 1 && !strcmp(argv[1], "keys")) return print_keys();
    Transcript t;

    // ---- every option over every value, a fresh context per key and state
    for (char state : {'A', 'B', 'C'})
        for (const char* key : kOptions) {
            t.open(state, std::string("option ") + key);
            for (double v : kValues) t.option(key, v);
        }
    for (char state : {'A', 'B'}) {
        t.open(state, "unknown options, null arguments");
        t.option("no_such_option", 1);
        t.option("Use_graph", 1);
        t.line("set_option (null key) 1", c3d_set_option(t.c, nullptr, 1));
        t.line("set_option use_graph 1 (null context)", c3d_set_option(nullptr, "use_graph", 1));
    }

    // ---- the keys whose admission depends on another's value
    for (char state : {'A', 'B'}) {
        t.open(state, "cluster_xcd_count 4, then cluster_xcd_base");
        t.option("cluster_xcd_count", 4);
        for (double v : kValues) t.option("cluster_xcd_base", v);
        t.open(state, "cluster_xcd_base 4, then cluster_xcd_count");
        t.option("cluster_xcd_base", 4);
        for (double v : kValues) t.option("cluster_xcd_count", v);
    }
    for (char state : {'A', 'B'}) {
        t.open(state, "a kind-8 stage, then precision 64");
        t.schedule("kind 8", stages_with(8, 20), nullptr, 0.0f, 0);
        t.option("precision", 64);
        t.option("f64_lbfgs", 1);
        t.option("precision", 64);
        t.option("f64_lbfgs", 0);                  // refused while both hold
        t.option("precision", 32);
        t.option("f64_lbfgs", 0);
        t.open(state, "precision 64, then a kind-8 stage");
        t.option("precision", 64);
        t.schedule("kind 8", stages_with(8, 20), nullptr, 0.0f, 0);
        t.option("f64_lbfgs", 1);
        t.schedule("kind 8", stages_with(8, 20), nullptr, 0.0f, 0);
        t.option("f64_lbfgs", 0);                  // refused while both hold
        t.schedule("kind 2", stages_with(2, 20), nullptr, 0.0f, 0);
        t.option("f64_lbfgs", 0);
    }

    // ---- c3d_set_model
    for (char state : {'A', 'B', 'C'}) {
        t.open(state, "model");
        c3d_model d;
        c3d_default_model(&d);
        c3d_model m;
        m = d; m.mass = 0; t.model("mass 0", m);
        m = d; m.rswitch = 0; t.model("rswitch 0", m);
        m = d; m.min_sep = 0; t.model("min_sep 0", m);
        m = d; m.rep_sep = 0; t.model("rep_sep 0", m);
        m = d; m.rep_sep = 4; t.model("rep_sep 4", m);
        m = d; m.noe_pot = -1; t.model("noe_pot -1", m);
        m = d; m.noe_pot = 4; t.model("noe_pot 4", m);
        m = d; m.mrswitch = 0; t.model("mrswitch 0", m);
        m = d; m.msoexp = 3; t.model("msoexp 3", m);
        m = d; m.msoexp = 0; t.model("msoexp 0", m);
        m = d; m.msoexp = 1; t.model("msoexp 1", m);
        m = d; m.min_sep = 6; t.model("min_sep 6", m);          // refused once the targets exist
        m = d; m.noe_pot = 1; m.rep_sep = 3; m.k_rep = 2.5f; t.model("noe_pot 1 rep_sep 3 k_rep 2.5", m);
        t.model("default", d);
        t.line("set_model (null model)", c3d_set_model(t.c, nullptr));
        t.line("set_model (null context)", c3d_set_model(nullptr, &d));
    }

    // ---- c3d_set_schedule
    for (char state : {'A', 'B', 'C'}) {
        t.open(state, "schedule");
        c3d_fire_params fire;
        c3d_default_fire(&fire);
        fire.dt_max = 0.01f; fire.n_min = 7;
        t.schedule("kind 3", stages_with(3, 20), nullptr, 0.0f, 0);
        t.schedule("kind -1", stages_with(-1, 20), nullptr, 0.0f, 0);
        t.schedule("kind 9", stages_with(9, 20), nullptr, 0.0f, 0);
        t.schedule("nsteps -1", stages_with(1, -1), nullptr, 0.0f, 0);
        t.schedule("no stages", {}, nullptr, 0.0f, 0);
        t.line("set_schedule (null stages)", c3d_set_schedule(t.c, nullptr, 2, nullptr, 0.0f, 0));
        t.line("set_schedule (null context)", c3d_set_schedule(nullptr, stages_with(1, 5).data(), 2, nullptr, 0.0f, 0));
        t.schedule("kind 8", stages_with(8, 20), nullptr, 0.0f, 0);      // refused under precision 64 (state C)
        t.schedule("kind 1, check_every 0", stages_with(1, 20), nullptr, 0.5f, 0);
        t.schedule("kind 0, check_every 100", stages_with(0, 12), nullptr, 0.25f, 100);
        t.schedule("kind 5, fire given", stages_with(5, 30), &fire, 0.0f, -3);
        t.schedule("kind 2, zero weight", {{2, 6, 0.0f, 0.0f, 1.0f, 0.85f, 0.0f}}, nullptr, 0.0f, 0);
    }

    // ---- c3d_get_stat
    for (char state : {'A', 'B'}) {
        t.open(state, "stats");
        for (const char* key : kStats) t.stat(key);
        t.stat("no_such_stat");
        t.stat("Graph_captures");
        double v = 0;
        t.line("get_stat (null key)", c3d_get_stat(t.c, nullptr, &v));
        t.line("get_stat graph_captures (null value)", c3d_get_stat(t.c, "graph_captures", nullptr));
        t.line("get_stat graph_captures (null context)", c3d_get_stat(nullptr, "graph_captures", &v));
    }
    t.close();
    return 0;
}
