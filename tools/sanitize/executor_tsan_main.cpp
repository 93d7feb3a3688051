// executor_tsan_main.cpp — libc3d's context code and the c3d_batch executor under ThreadSanitizer, on the CPU, against the fake HIP layer
// of hip_stub.cpp (tools/sanitize/run.sh builds and runs it).
//
//   0. a code object that fails to load: c3d_create reports it (C3D_ERR_HIP, message naming the unit) and does not remember it as loaded
//   1. c3d_batch --devices 4 --lanes 2 --map-devices-to 0   eight contexts of one process starting together on one device: the start that
//                                                           met a device exception on the GPU box in round 5
//   2. c3d_batch --devices 8 --lanes 3                      the production shape on an 8-GPU node: 24 contexts (the stub shows 8 devices)
//   3. an API storm: twelve threads, each with its own context, through configurations that want DIFFERENT code objects (the shipped
//      potential, the three other potentials' multi-step units, fp64, symmetric tiles, the embedding, the tear16 hook) while the others
//      launch — the loader must take each unit once, and never beside another HIP call.
// Passes when TSan reports nothing (halt_on_error) and the stub counted no load that overlapped a HIP call (hip_stub.cpp).
#include <sys/stat.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/c3d.h"

int c3d_batch_main(int argc, char** argv);          // c3d_batch_main.cpp built with -Dmain=c3d_batch_main
extern "C" long c3d_stub_violations();
extern "C" void c3d_stub_fail_next_loads(int n);
extern "C" long c3d_stub_launches();
extern "C" long c3d_stub_loads();
extern "C" long c3d_stub_cluster_launches();

#define REQ(x) do { if (!(x)) { fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, #x, c3d_last_error()); exit(1); } } while (0)

static void write_matrix(const std::string& path, int n, unsigned seed) {
    std::mt19937_64 g(seed);
    std::uniform_real_distribution<double> u(0.5, 1.5);
    std::vector<double> m((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            const double v = i == j ? 5000.0 : 900.0 * u(g) / (double)(j - i);
            m[(size_t)i * n + j] = m[(size_t)j * n + i] = v;
        }
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) fprintf(f, "%.10f ", m[(size_t)i * n + j]);
        fputs("\r\n", f);
    }
    fclose(f);
}

static int run_batch(std::vector<std::string> args) {
    std::vector<char*> argv;
    args.insert(args.begin(), "c3d_batch");
    for (std::string& a : args) argv.push_back(&a[0]);
    return c3d_batch_main((int)argv.size(), argv.data());
}

static void api_storm(int device_count) {
    std::atomic<int> failures{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 12; ++t)
        th.emplace_back([t, device_count, &failures] {
            c3d_ctx* c = nullptr;
            if (c3d_create(t % device_count, &c) != C3D_OK) { ++failures; return; }
            const int n = 40 + 7 * t;
            std::vector<double> IF((size_t)n * n);
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) IF[(size_t)i * n + j] = i == j ? 4000.0 : 700.0 / (double)std::abs(i - j);
            c3d_model m;
            c3d_default_model(&m);
            bool ok = true;
            for (int round = 0; round < 3 && ok; ++round) {
                const int what = (t + round) % 6;
                if (what == 1) { m.noe_pot = 0; }                       // other potentials: their own multi-step units, on demand
                else if (what == 2) { m.noe_pot = 1; }
                else if (what == 3) { m.noe_pot = 2; }
                else { c3d_default_model(&m); }
                ok = ok && c3d_set_model(c, &m) == C3D_OK;
                ok = ok && c3d_set_option(c, "precision", what == 4 ? 64 : 32) == C3D_OK;
                ok = ok && c3d_set_option(c, "symmetric", what == 5 ? 1 : 0) == C3D_OK;
                ok = ok && c3d_set_if_matrix(c, IF.data(), n, 0.5, 11.0) == C3D_OK;
                ok = ok && c3d_init_replicas(c, 4, 82364, 0) == C3D_OK;
                if (what == 0) ok = ok && c3d_embed_replicas(c, 10) == C3D_OK;
                long done = 0;
                ok = ok && c3d_run_steps(c, 30, &done) == C3D_OK;
                ok = ok && c3d_run(c) == C3D_OK;
                std::vector<double> e(12), rho(4), dev(4);
                std::vector<int32_t> rank(4), sat(4);
                ok = ok && c3d_rank(c, rank.data()) == C3D_OK;
                ok = ok && c3d_score_replicas(c, IF.data(), 3, sat.data(), dev.data(), rho.data()) == C3D_OK;
                std::vector<double> sim(16), rmsd(16);
                ok = ok && c3d_compare_replicas(c, nullptr, 0, sim.data(), rmsd.data()) == C3D_OK;
                std::vector<double> emap(3 * (size_t)n * n);
                const int32_t picked[3] = {3, 0, 0};
                double erho[2];
                ok = ok && c3d_ensemble_map(c, nullptr, 0, picked, 3, 7.6, emap.data(), emap.data() + (size_t)n * n, emap.data() + 2 * (size_t)n * n) == C3D_OK;
                ok = ok && c3d_ensemble_score(c, IF.data(), 3, nullptr, 0, nullptr, 0, 7.6, &erho[0], &erho[1]) == C3D_OK;
                ok = ok && c3d_ensemble_map(c, nullptr, 0, picked, 0, 7.6, emap.data(), nullptr, nullptr) == C3D_ERR_INVALID;
                std::vector<int64_t> clashes(4);
                std::vector<int32_t> bead(4 * (size_t)n);
                std::vector<double> nearest(4 * (size_t)n), chain(4 * C3D_GEOMETRY_FIELDS), prof(3 * (size_t)n);
                ok = ok && c3d_geometry_replicas(c, nullptr, 0, 3.5, 1, clashes.data(), bead.data(), nearest.data(), chain.data()) == C3D_OK;
                ok = ok && c3d_separation_profile(c, nullptr, 0, picked, 3, 7.6, prof.data(), prof.data() + n, prof.data() + 2 * (size_t)n) == C3D_OK;
                ok = ok && c3d_geometry_replicas(c, nullptr, 0, 3.5, n, clashes.data(), nullptr, nullptr, nullptr) == C3D_ERR_INVALID;
                std::vector<double> srho(4 * (size_t)n), sscc(4);
                std::vector<int64_t> ssums(4 * (size_t)n * C3D_STRATUM_FIELDS);
                ok = ok && c3d_stratified_score(c, IF.data(), 3, 0, nullptr, 0, srho.data(), sscc.data(), ssums.data()) == C3D_OK;
                ok = ok && c3d_stratified_score(c, IF.data(), 3, 2, nullptr, 0, srho.data(), nullptr, nullptr) == C3D_ERR_INVALID;
                std::vector<int32_t> brestr(n), bsat(4 * (size_t)n);
                std::vector<int64_t> bsums(4 * (size_t)n * C3D_BEAD_FIELDS), bdev(4 * (size_t)n);
                ok = ok && c3d_bead_scores(c, IF.data(), 3, nullptr, 0, nullptr, 0, srho.data(), bsums.data(), brestr.data(), bsat.data(), bdev.data()) == C3D_OK;
                ok = ok && c3d_bead_scores(c, nullptr, 3, picked, 3, nullptr, 0, srho.data(), nullptr, nullptr, nullptr, nullptr) == C3D_ERR_INVALID;
                double access_ms = -1;
                ok = ok && c3d_accessibility(c, nullptr, 0, 1.965, 1.965, nullptr, 24, bead.data(), &access_ms) == C3D_OK && access_ms >= 0;
                ok = ok && c3d_accessibility(c, nullptr, 0, 1.965, 1.965, nullptr, C3D_ACCESS_MAX_POINTS + 1, bead.data(), nullptr) == C3D_ERR_INVALID;
                // (the stub's models are all zeros, maps without spread: iters = 0 keeps the start vectors independent)
                std::vector<double> cvec(6 * 2 * (size_t)n), cexp(6 * (size_t)n), cshare(12), cres(12), cagree(5 * 4), cside(5 * 2);
                double cpt_ms = -1;
                ok = ok && c3d_compartments(c, IF.data(), nullptr, 0, nullptr, 0, C3D_COMPARTMENT_CONSENSUS, 1, 2, 0, nullptr, cexp.data(), cvec.data(), cshare.data(),
                                            cres.data(), cagree.data(), cside.data(), &cpt_ms) == C3D_OK && cpt_ms >= 0;
                ok = ok && c3d_compartments(c, nullptr, nullptr, 0, picked, 3, 0, 1, C3D_COMPARTMENT_MAX_VECTORS + 1, 0, nullptr, nullptr, cvec.data(), nullptr, nullptr,
                                            nullptr, nullptr, nullptr) == C3D_ERR_INVALID;
                // (IF + 4 models + consensus: 6 maps, 2 windows)
                const int32_t iwin[2] = {2, 5}, ibad[2] = {5, 2};
                std::vector<double> imean(6 * 2 * (size_t)n), iscore(6 * 2 * (size_t)n), istr(6 * 2 * (size_t)n), ifit(5 * 2);
                std::vector<int32_t> ibound(6 * 2 * (size_t)n), icounts(5 * 2 * 4);
                double ins_ms = -1;
                ok = ok && c3d_insulation(c, IF.data(), nullptr, 0, nullptr, 0, C3D_INSULATION_CONSENSUS, iwin, 2, 0.0, 0.1, 1, imean.data(), iscore.data(), ibound.data(),
                                          istr.data(), ifit.data(), icounts.data(), &ins_ms) == C3D_OK && ins_ms >= 0;
                ok = ok && c3d_insulation(c, nullptr, nullptr, 0, picked, 3, C3D_INSULATION_CONTACT, iwin, 2, 7.6, 0.0, 0, imean.data(), nullptr, ibound.data(), nullptr,
                                          nullptr, nullptr, nullptr) == C3D_OK;
                ok = ok && c3d_insulation(c, nullptr, nullptr, 0, picked, 3, 0, ibad, 2, 0.0, 0.0, 0, imean.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                                          nullptr) == C3D_ERR_INVALID;
                // (IF + 4 models + consensus: 6 maps, w = 2, separations 5..20, the list taken from the peaks; then a list of two with a masked bin)
                const double lthr[4] = {0.5, 0.5, 0.5, 0.5};
                const int32_t lpix[4] = {8, 20, 1, 12};
                std::vector<double> lexp(6 * 28), lratio(4 * 16 * (size_t)n), lat(6 * 6 * 64), lapa(6 * 25), lp2(6);
                std::vector<int32_t> lpeaks(2 * 64), lclosed(2 * 6), lmask(n, 0);
                int32_t lrep[C3D_LOOP_REPORT];
                lmask[3] = 1;
                double loop_ms = -1;
                ok = ok && c3d_loops(c, IF.data(), nullptr, 0, nullptr, 0, C3D_LOOP_CONSENSUS, nullptr, 0, 2, 5, 20, lthr, 0.0, 1, 1, nullptr, 0, 64, lexp.data(), lratio.data(),
                                     lpeaks.data(), lrep, lat.data(), lclosed.data(), lapa.data(), lp2.data(), &loop_ms) == C3D_OK && loop_ms >= 0 && lrep[2] <= 64;
                ok = ok && c3d_loops(c, nullptr, nullptr, 0, picked, 3, 0, lmask.data(), 1, 2, 5, 20, nullptr, 0.0, 0, 2, lpix, 2, 0, nullptr, nullptr, nullptr, nullptr,
                                     lat.data(), lclosed.data(), lapa.data(), lp2.data(), nullptr) == C3D_OK && lclosed[0] <= 2;
                ok = ok && c3d_loops(c, nullptr, nullptr, 0, picked, 3, 0, nullptr, 2, 2, 5, 20, nullptr, 0.0, 0, 1, lpix, 2, 0, nullptr, nullptr, nullptr, nullptr,
                                     lat.data(), nullptr, nullptr, nullptr, nullptr) == C3D_ERR_INVALID;
                // (4 models of n - 1 segments, three domains; then a window that cuts the chain short; then bounds that do not end at S)
                const int32_t ebounds[4] = {0, 7, 8, n - 1}, ebad[4] = {0, 7, 8, n};
                std::vector<double> ewr(4), eacn(4), eseg(2 * 4 * (size_t)(n - 1)), elink(2 * 4 * 9);
                double ent_ms = -1;
                ok = ok && c3d_entanglement(c, nullptr, 0, 2, 0, ebounds, 3, ewr.data(), eacn.data(), eseg.data(), eseg.data() + 4 * (size_t)(n - 1), elink.data(),
                                            elink.data() + 4 * 9, &ent_ms) == C3D_OK && ent_ms >= 0 && elink[1] == elink[3];
                ok = ok && c3d_entanglement(c, nullptr, 0, 3, 10, nullptr, 0, ewr.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == C3D_OK;
                ok = ok && c3d_entanglement(c, nullptr, 0, 2, 0, ebad, 3, nullptr, nullptr, nullptr, nullptr, elink.data(), nullptr, nullptr) == C3D_ERR_INVALID;
                // (the raw matrix: IF itself, an odd and an even n over the threads; bin 1 masked by the caller)
                std::vector<double> bw(n), bbal((size_t)n * n), bhist(51), brep(C3D_BALANCE_REPORT);
                std::vector<int32_t> bmask(n, 0), bcode(n);
                bmask[1] = 1;
                double bal_ms = -1;
                ok = ok && c3d_balance_matrix(c, IF.data(), n, C3D_BALANCE_ICE, round == 1 ? C3D_BALANCE_CHECK_EVERY_ROUND : 0, 2, 10, bmask.data(), nullptr, 1e-5, 50, 1.0,
                                              bw.data(), bcode.data(), bbal.data(), bhist.data(), brep.data(), &bal_ms) == C3D_OK && bal_ms >= 0 && bcode[1] == 1 && bw[1] == 0.0 &&
                           brep[3] == (double)(n - 1);
                ok = ok && c3d_balance_matrix(c, IF.data(), n, C3D_BALANCE_SQRT_VC, 0, 0, 1, nullptr, nullptr, 0.0, 0, 2.0, bw.data(), nullptr, nullptr, nullptr, brep.data(),
                                              nullptr) == C3D_OK && brep[0] == 1.0;
                ok = ok && c3d_balance_matrix(c, IF.data(), n, C3D_BALANCE_VC, 0, 2, 10, nullptr, bw.data(), 0.0, 0, 1.0, bw.data(), nullptr, nullptr, nullptr, nullptr,
                                              nullptr) == C3D_ERR_INVALID;
                // (IF against itself and against IF with one pair of entries doubled: three maps, two half-widths, separations 1..8; then
                // half-widths out of order)
                std::vector<double> smaps(3 * (size_t)n * n);
                for (int m = 0; m < 3; ++m) std::copy(IF.begin(), IF.end(), smaps.begin() + (size_t)m * n * n);
                smaps[2 * (size_t)n * n + 1 * n + 3] *= 2.0; smaps[2 * (size_t)n * n + 3 * n + 1] *= 2.0;
                const int32_t sh[2] = {0, 2}, shbad[2] = {2, 2};
                std::vector<double> sscc2(2 * 9), srho2(2 * 3 * 8), smom(2 * 3 * 8 * 3), ssm(2 * 3 * 8 * (size_t)n);
                std::vector<int64_t> scnt(2 * 3 * 8 * 3);
                double sim_ms = -1;
                ok = ok && c3d_map_similarity(c, smaps.data(), 3, n, sh, 2, 1, 8, round == 1 ? C3D_MAPSIM_KEEP_ZEROS : 0, sscc2.data(), srho2.data(), smom.data(), scnt.data(),
                                              ssm.data(), &sim_ms) == C3D_OK && sim_ms >= 0 && sscc2[0] == 1.0 && memcmp(&sscc2[1], &sscc2[3], sizeof(double)) == 0 && ssm[0] == IF[1];
                ok = ok && c3d_map_similarity(c, smaps.data(), 2, n, sh, 1, 0, 0, 0, sscc2.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == C3D_OK;
                ok = ok && c3d_map_similarity(c, smaps.data(), 3, n, shbad, 2, 1, 8, 0, sscc2.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == C3D_ERR_INVALID;
                if (what == 2) { unsigned long long a, b, d; ok = ok && c3d_debug_tear16(c, 4, &a, &b, &d) == C3D_OK; }
            }
            if (!ok) { fprintf(stderr, "api storm thread %d: %s\n", t, c3d_last_error()); ++failures; }
            c3d_destroy(c);
        });
    for (std::thread& x : th) x.join();
    REQ(failures.load() == 0);
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: executor_tsan <scratch dir>\n"); return 2; }
    const std::string tmp = argv[1];
    std::vector<std::string> mats;
    const int sizes[] = {37, 35, 60, 96, 73, 113, 150, 57, 80};
    for (int k = 0; k < 9; ++k) {
        const std::string p = tmp + "/chrS" + std::to_string(k + 1) + "_1mb_matrix.txt";
        write_matrix(p, sizes[k], 100u + (unsigned)k);
        mats.push_back(p);
    }
    // 0. a code object that fails to load is reported by c3d_create — and not remembered as loaded: the next c3d_create loads it
    setenv("C3D_STUB_DEVICES", "1", 1);
    {
        c3d_stub_fail_next_loads(2);                    // the next two load attempts report an error: two c3d_create calls fail at their first unit
        c3d_ctx* c = nullptr;
        REQ(c3d_create(0, &c) == C3D_ERR_HIP && c == nullptr);
        REQ(strstr(c3d_last_error(), "loading the code object of the") != nullptr);
        REQ(c3d_create(0, &c) == C3D_ERR_HIP && c == nullptr);
        REQ(c3d_create(0, &c) == C3D_OK && c != nullptr);
        double loaded = -1;
        REQ(c3d_get_stat(c, "units_loaded", &loaded) == C3D_OK && loaded == 4.0);
        c3d_destroy(c);
    }
    const long failed_attempts = 2;
    // 1. the start of round 5's exception: eight contexts, one device
    {
        std::vector<std::string> a = mats;
        a.insert(a.end(), {"--out", tmp + "/four", "-m", "6", "--devices", "4", "--lanes", "2", "--map-devices-to", "0"});
        REQ(run_batch(a) == 0);
    }
    const long loads_one_device = c3d_stub_loads();
    REQ(loads_one_device == 4 + failed_attempts);     // the default job's four units, once for the process (+ the two attempts that were made to fail): nobody loaded anything later
    // 2. the production shape: 8 devices x 3 lanes
    setenv("C3D_STUB_DEVICES", "8", 1);
    {
        std::vector<std::string> a = mats;
        a.insert(a.end(), {"--out", tmp + "/eight", "-m", "6", "--devices", "8", "--lanes", "3"});
        REQ(run_batch(a) == 0);
    }
    REQ(c3d_stub_loads() == 4 + failed_attempts + 4 * 7);   // device 0 had them; seven more devices x four units
    // 3. configurations that want other units, from twelve threads at once
    api_storm(8);
    printf("executor under TSan: %ld HIP calls (%ld multi-step launches), %ld unit loads, %ld load/launch overlaps\n", c3d_stub_launches(),
           c3d_stub_cluster_launches(), c3d_stub_loads(), c3d_stub_violations());
    REQ(c3d_stub_violations() == 0);
    REQ(c3d_stub_cluster_launches() > 0);
    return 0;
}
