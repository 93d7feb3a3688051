// hip_stub.cpp — a fake HIP layer for ThreadSanitizer runs of libc3d's HOST code on a box without a GPU (tools/sanitize/run.sh).
//
// The host units — c3d_api.cpp (context), c3d_config.cpp (configuration), c3d_gate.cpp (code-object loader), c3d_run.cpp (launch program, executor of c3d_run), c3d_debug.cpp (table test hooks),
// c3d_analysis.cpp (scoring) — and c3d_batch_main.cpp (per-device lists, lanes, the XCD broker) are compiled as they are, with -fsanitize=thread, and linked against THIS file instead of libamdhip64 and the kernels'
// translation units: "device" memory is host memory, a stream is a counter, a copy is a memcpy, every kernel launcher returns success and
// computes nothing — except K1, which is restated on the host so that the executor has restraints to write, and the multi-step launcher,
// which writes the completion mark its kernel would write (every seventh launch does not: the abandoned-launch path runs too).
//
// Beyond what TSan sees by itself, the stub CHECKS the loader's contract (c3d_gate.cpp "code objects"): a unit's load function and any HIP
// call of the library must never overlap in time, whatever the thread.  Every function below counts as device work (LaunchScope) except
// the device queries and pure look-ups — hipGetDeviceCount, hipSetDevice, hipGetDevicePropertiesR0600, hipDeviceGetAttribute,
// hipHostGetDevicePointer, hipGetErrorString, hipGetLastError — so allocation, release, stream / event / graph creation and destruction and synchronisation
// are checked as well as launches, copies and fills; c3d_stub_violations() counts the overlaps, the harness fails on any.
// Test infrastructure; never linked into the product.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../chromosome3d_amd/csrc/c3d_internal.h"

namespace {
std::atomic<int> g_launching{0}, g_loading{0};
std::atomic<long> g_violations{0}, g_launches{0}, g_loads{0}, g_cluster_launches{0};
struct LaunchScope {
    LaunchScope() {
        g_launching.fetch_add(1);
        if (g_loading.load() != 0) g_violations.fetch_add(1);
        g_launches.fetch_add(1);
        std::this_thread::yield();                    // widen the window
    }
    ~LaunchScope() { g_launching.fetch_sub(1); }
};
std::atomic<int> g_fail_next_load{0};          // c3d_stub_fail_next_loads(n): the next n unit loads report an error (the loader's error path)
struct LoadScope {
    LoadScope() {
        g_loading.fetch_add(1);
        if (g_launching.load() != 0) g_violations.fetch_add(1);
        g_loads.fetch_add(1);
        std::this_thread::sleep_for(std::chrono::microseconds(300));     // a load takes milliseconds on the device: stay inside for a while
        if (g_launching.load() != 0) g_violations.fetch_add(1);
    }
    ~LoadScope() { g_loading.fetch_sub(1); }
};
int stub_devices() {
    const char* e = getenv("C3D_STUB_DEVICES");
    const int n = e ? atoi(e) : 1;
    return n < 1 ? 1 : (n > 64 ? 64 : n);
}
thread_local int t_device = 0;
}  // namespace

extern "C" long c3d_stub_violations() { return g_violations.load(); }
extern "C" void c3d_stub_fail_next_loads(int n) { g_fail_next_load.store(n); }
static hipError_t load_result() {
    int left = g_fail_next_load.load();
    while (left > 0 && !g_fail_next_load.compare_exchange_weak(left, left - 1)) { }
    return left > 0 ? hipErrorSharedObjectInitFailed : hipSuccess;
}
extern "C" long c3d_stub_launches() { return g_launches.load(); }
extern "C" long c3d_stub_loads() { return g_loads.load(); }
extern "C" long c3d_stub_cluster_launches() { return g_cluster_launches.load(); }

// ---- the HIP API the host code calls ----------------------------------------------------------------------------------------------
extern "C" {
hipError_t hipGetDeviceCount(int* n) { *n = stub_devices(); return hipSuccess; }
hipError_t hipSetDevice(int d) { if (d < 0 || d >= stub_devices()) return hipErrorInvalidDevice; t_device = d; return hipSuccess; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600* p, int) {
    memset(p, 0, sizeof(*p));
    snprintf(p->gcnArchName, sizeof(p->gcnArchName), "gfx950:sramecc+:xnack-");
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t a, int) { *v = a == hipDeviceAttributeNumberOfXccs ? 8 : 0; return hipSuccess; }
hipError_t hipGetLastError() { return hipSuccess; }      // (c3d_compare_replicas clears the error of a refused allocation)
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
hipError_t hipMalloc(void** p, size_t n) { LaunchScope ls; *p = calloc(n ? n : 1, 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { LaunchScope ls; free(p); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { LaunchScope ls; *p = calloc(n ? n : 1, 1); return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipHostFree(void* p) { LaunchScope ls; free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) { LaunchScope ls; memcpy(dst, src, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* dst, int v, size_t n, hipStream_t) { LaunchScope ls; memset(dst, v, n); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, hipMemcpyKind, hipStream_t) {
    LaunchScope ls;
    for (size_t r = 0; r < height; ++r) memcpy(static_cast<char*>(dst) + r * dpitch, static_cast<const char*>(src) + r * spitch, width);
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { LaunchScope ls; *s = reinterpret_cast<hipStream_t>(calloc(1, 8)); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) { LaunchScope ls; free(s); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { LaunchScope ls; return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t* e) { LaunchScope ls; *e = reinterpret_cast<hipEvent_t>(calloc(1, 8)); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { LaunchScope ls; *e = reinterpret_cast<hipEvent_t>(calloc(1, 8)); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { LaunchScope ls; free(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { LaunchScope ls; return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { LaunchScope ls; *ms = 0.001f; return hipSuccess; }
// stream capture / graphs: the per-step path replays graphs; here a capture records nothing and a graph launch is one "launch"
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) { LaunchScope ls; return hipSuccess; }
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t* g) { LaunchScope ls; *g = reinterpret_cast<hipGraph_t>(calloc(1, 8)); return hipSuccess; }
hipError_t hipGraphInstantiate(hipGraphExec_t* ge, hipGraph_t, hipGraphNode_t*, char*, size_t) { LaunchScope ls; *ge = reinterpret_cast<hipGraphExec_t>(calloc(1, 8)); return hipSuccess; }
hipError_t hipGraphDestroy(hipGraph_t g) { LaunchScope ls; free(g); return hipSuccess; }
hipError_t hipGraphExecDestroy(hipGraphExec_t g) { LaunchScope ls; free(g); return hipSuccess; }
hipError_t hipGraphLaunch(hipGraphExec_t, hipStream_t) { LaunchScope ls; return hipSuccess; }
}

// ---- the kernels' translation units: launchers that launch nothing, loaders that load nothing -------------------------------------
namespace c3d {

hipError_t preload_device_unit() { LoadScope l; return load_result(); }
hipError_t preload_cluster_base_unit() { LoadScope l; return load_result(); }
hipError_t preload_cluster_unit(int pot, bool) { LoadScope l; return pot >= 0 && pot <= 4 ? load_result() : hipErrorInvalidValue; }
hipError_t preload_score_unit() { LoadScope l; return load_result(); }
hipError_t preload_embed_unit() { LoadScope l; return load_result(); }
hipError_t preload_f64_unit() { LoadScope l; return load_result(); }
hipError_t preload_sym_unit() { LoadScope l; return load_result(); }

hipError_t launch_step(const DevModel&, const DevStep&, const DevFire&, const DevBuffers&, int, const StepForm&, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_eval_forces(const DevModel&, const DevStep&, const DevBuffers&, int, float*, bool, int, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_energy(const DevModel& m, const DevStep&, const DevBuffers& b, int, float, float, double, hipStream_t) {
    LaunchScope ls;
    for (int r = 0; r < m.nrep; ++r) { b.E[4 * r] = 1000.0 + 7.0 * ((r * 5) % m.nrep); b.E[4 * r + 1] = 1.0; b.E[4 * r + 2] = 2.0; b.E[4 * r + 3] = 0.0; }   // distinct "energies": c3d_rank has something to order
    return hipSuccess;
}
hipError_t launch_centre(const DevModel&, const DevBuffers&, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
size_t pair_targets_floats(int n, int npad) { return (size_t)n * npad; }
hipError_t launch_pair_targets(const DevModel&, const float*, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_eval(const DevModel&, const DevStep&, const DevBuffers&, const LbfgsBuffers&, int, int, const StepForm&, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_move(const DevModel&, const DevStep&, const DevFire&, const DevBuffers&, const LbfgsBuffers&, int, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_direction(const DevModel&, const DevFire&, int, const double*, const LbfgsState*, const int*, LbfgsState*, double*, int*, hipStream_t) { LaunchScope ls; return hipSuccess; }
AnnealIO anneal_io(const DevBuffers& b, int parity) {
    const int q = parity ^ 1;
    AnnealIO io;
    io.pin = b.P[parity]; io.xin = b.X[parity]; io.vin = b.V[parity]; io.vinit = b.Vinit; io.sin = b.S[parity];
    io.xout = b.X[q]; io.vout = b.V[q]; io.pout = b.P[q]; io.sout = b.S[q];
    return io;
}
bool cluster_plan(const DevModel& m, int num_cus, int num_xcc, int, int, int xcd_count, ClusterPlan* plan) {
    if (m.npad > 1024 || num_xcc != 8) return false;
    ClusterPlan pl{};
    pl.rpw = 4; pl.cw = 12; pl.helpers = 4; pl.wgs_per_cu = 1; pl.parts = (m.n + 47) / 48; pl.per_xcd = (m.nrep_g + xcd_count - 1) / xcd_count;
    pl.grid = num_cus; pl.threads = 1024; pl.units = 96; pl.device = 0; pl.lds = 84 * 1024; pl.expected = (unsigned)(m.nrep_g * pl.parts);
    pl.xcd_count = xcd_count;
    *plan = pl;
    return pl.per_xcd * pl.parts <= num_cus / 8;
}
size_t cluster_record_bytes(const DevModel& m, const ClusterPlan&) { return (size_t)2 * m.nrep_g * (m.npad + m.npad / 4) * 16; }
hipError_t launch_cluster(const DevModel&, const DevFire&, const ClusterPlan&, const AnnealIO&, const float*, void*, const StepRun*, int, int, int,
                          unsigned tag_base, unsigned* timeout, unsigned*, hipStream_t) {
    LaunchScope ls;
    // the kernel's last workgroup writes the completion mark into the host-mapped word; every seventh launch "loses" a workgroup
    if (g_cluster_launches.fetch_add(1) % 7 != 6) __atomic_store_n(&timeout[1], tag_base | 1u, __ATOMIC_RELEASE);
    return hipSuccess;
}
hipError_t launch_tear16(int, void*, unsigned*, unsigned long long*, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
void sym_geometry(const DevModel&, int* Q, int* G, int* od, int* dg) { *Q = 1; *G = 1; *od = 0; *dg = 1; }
size_t sym_scratch_floats(const DevModel& m) { return (size_t)m.npad * 8; }
void sym_tile_list(const DevModel&, int2* out) { out[0].x = 0; out[0].y = 0; }
hipError_t launch_step_sym(const DevModel&, const DevStep&, const DevFire&, const DevBuffers&, int, const void*, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_step_scalars(const DevModel&, const DevStep&, const DevFire&, int, const float*, const FireState*, float*, FireState*, hipStream_t) { LaunchScope ls; return hipSuccess; }
int cols64(int n) { return (n + 127) / 128 * 128; }
Model64 model64(const DevModel& d, const c3d_model&) { Model64 m{}; m.n = d.n; m.noe_pot = device_pot(d.noe_pot); return m; }   // (what form64 reads; no kernel runs here)
Step64 step64(const Model64&, int, double, double, double, double, double) { return Step64{}; }
Fire64 fire64(const c3d_fire_params&) { return Fire64{}; }
hipError_t launch_step64(const DevModel&, const Model64&, const Step64&, const Fire64&, const Form64&, const Buffers64&, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_eval64(const DevModel&, const Model64&, const Step64&, const Form64&, const Buffers64&, const LbfgsBuffers64&, int, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_move64(const DevModel&, const Model64&, const Step64&, const Fire64&, const Buffers64&, const LbfgsBuffers64&, int, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_direction64(const Step64&, const Fire64&, int, const double*, const LbfgsState*, const int*, LbfgsState*, double*, int*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_move_rows(const DevFire&, int, int, const float*, int, int, const float*, float*, const float*, float*, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_lbfgs_move_rows64(const Fire64&, int, int, const double*, int, int, const double*, double*, const double*, double*, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_row_finish(const DevModel&, const DevStep&, const DevFire&, int, const float*, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_step_scalars64(const Model64&, const Step64&, const Fire64&, int, const double*, const void*, double*, void*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_row_finish64(const Step64&, const Fire64&, int, const double*, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_tenths64(int, int, const int32_t*, const int32_t*, const int32_t*, int32_t*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_targets64(const Model64&, const Form64&, const int32_t*, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_import64(const DevModel&, const float*, const Buffers64&, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_export64(const DevModel&, const Buffers64&, int, float*, float*, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_eval_forces64(const DevModel&, const Model64&, const Step64&, const Form64&, const Buffers64&, int, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_energy64(const DevModel&, const Model64&, double, const Buffers64&, int, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
size_t fire_state64_bytes() { return 32; }
// K1 restated on the host (chromosome3D.pl:110-162 as c3d_api.cpp's own near-tie redo does it): the executor needs real restraints
hipError_t launch_if_to_target(const double* IF, int n, int npad, double alpha, double K, int min_sep, int, double*, double*, int,
                               int32_t* dist10, float* tgt, unsigned char*, unsigned*, hipStream_t) {
    LaunchScope ls;
    const size_t nn = (size_t)n * n;
    double sum = 0;
    for (size_t k = 0; k < nn; ++k) sum += pow(IF[k], alpha);
    const double mean = sum / ((double)n * (double)n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            double v = pow(IF[(size_t)i * n + j], alpha) / mean;
            long long t = -10;
            if (v != 0) t = llround(10.0 * K / v);
            if (t > 2000000000LL) t = 2000000000LL;
            dist10[(size_t)i * n + j] = (int32_t)t;
            const int sep = i > j ? i - j : j - i;
            tgt[(size_t)i * npad + j] = (sep >= min_sep && t > 0) ? (float)((double)t / 10.0) : 0.0f;
        }
    return hipSuccess;
}
hipError_t launch_dg_smooth(const float*, int, int, float, float, float*, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_dg_embed(const float*, const float*, int, int, int, uint64_t, uint32_t, int, float*, float*, float*, float*, float*, bool, int, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_score(const float*, const float*, const double*, int, int, int, int, int, unsigned, double, double, double, double*, unsigned*, unsigned*,
                        double* partial, int* overflow, hipStream_t) {
    LaunchScope ls;
    (void)partial;
    *overflow = 0;
    return hipSuccess;
}
hipError_t launch_score_bbox(const double*, int, int nrep, double* box, hipStream_t) {
    LaunchScope ls;
    for (int k = 0; k < 6 * nrep; ++k) box[k] = 0.0;
    return hipSuccess;
}
hipError_t launch_score_wide(const double*, const float*, const double*, int, int, int, int, int, unsigned, double, double, double, unsigned*, unsigned*,
                             double*, int*, hipStream_t) { LaunchScope ls; return hipSuccess; }
// the IF ranks restated on the host (average ranks of the doubled upper triangle): c3d_score_replicas divides by their sum of squares
hipError_t launch_if_rank_keys(const double* M, int n, int range, unsigned long long*, size_t, size_t, int* asym, hipStream_t) {
    LaunchScope ls;
    *asym = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + range; j < n; ++j)
            if (M[(size_t)i * n + j] != M[(size_t)j * n + i]) *asym = 1;
    return hipSuccess;
}
hipError_t launch_if_rank_sort(double* M, int n, int range, unsigned long long*, size_t, size_t, double ma, double* saa_rows, hipStream_t) {
    LaunchScope ls;
    std::vector<double> v;
    for (int i = 0; i < n; ++i)
        for (int j = i + range; j < n; ++j) v.push_back(M[(size_t)i * n + j]);
    std::sort(v.begin(), v.end());
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double r = 0.0;
            if (j - i >= range) {
                const double a = M[(size_t)i * n + j];
                const size_t k = std::lower_bound(v.begin(), v.end(), a) - v.begin(), e = std::upper_bound(v.begin(), v.end(), a) - v.begin();
                r = ((double)k + (double)(e - 1)) + 1.5;
            }
            M[(size_t)i * n + j] = M[(size_t)j * n + i] = r;
        }
    for (int i = 0; i < n; ++i) {
        saa_rows[i] = 0;
        for (int j = 0; j < n; ++j)
            if ((i > j ? i - j : j - i) >= range) saa_rows[i] += (M[(size_t)i * n + j] - ma) * (M[(size_t)i * n + j] - ma);
    }
    return hipSuccess;
}
// c3d_compare_replicas: nothing is ranked; the tables come out as the identity's (1 on the diagonal of the centred-rank sums, 0 elsewhere)
hipError_t launch_compare_coords(const float*, int, int, int, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_compare_ranks(const double*, int, unsigned long long*, size_t, size_t, unsigned*, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_compare_table(const double*, const unsigned*, const double*, int, int K, size_t, double*, double*, double* table, hipStream_t) {
    LaunchScope ls;
    for (int a = 0; a < K; ++a)
        for (int b = 0; b < K; ++b) { table[2 * ((size_t)a * K + b)] = a == b ? 1.0 : 0.0; table[2 * ((size_t)a * K + b) + 1] = 0.0; }
    return hipSuccess;
}

// c3d_superpose_replicas / c3d_rmsd_table: nothing is fitted; every pair comes out as the identity's (residual 0, not mirrored), the fitted
// models as the centred ones and their mean as zero
hipError_t launch_superpose_gather64(const double*, int, int, int, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_superpose_centre(double*, int, int K, double* cent, hipStream_t) {
    LaunchScope ls;
    for (int k = 0; k < 3 * K; ++k) cent[k] = 0.0;
    return hipSuccess;
}
hipError_t launch_superpose_fit(const double*, int KA, const double*, int KB, int, int, bool, const int*, double*, double*, double* fit, int* mirrored,
                                double* res, hipStream_t) {
    LaunchScope ls;
    for (size_t q = 0; q < (size_t)KA * KB; ++q) {
        sup_identity(fit + q * kSupFit);
        mirrored[q] = 0;
        if (res) res[q] = 0.0;
    }
    return hipSuccess;
}
hipError_t launch_superpose_apply(const double*, int, int, const double*, const double*, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_superpose_mean(const double*, int K, int n, double* mean, double* rmsf, double* dev, hipStream_t) {
    LaunchScope ls;
    for (int i = 0; i < 3 * n; ++i) mean[i] = 0.0;
    for (int i = 0; i < n; ++i) rmsf[i] = 0.0;
    if (dev) for (int k = 0; k < K; ++k) dev[k] = 0.0;
    return hipSuccess;
}
hipError_t launch_superpose_store32(const double*, int, int, int, float*, hipStream_t) { LaunchScope ls; return hipSuccess; }
hipError_t launch_superpose_store64(const double*, int, int, int, double*, double*, hipStream_t) { LaunchScope ls; return hipSuccess; }

// c3d_ensemble_map / c3d_ensemble_score: the map restated on the host over the "device" memory, which is the host's here
hipError_t launch_ensemble_map(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact, hipStream_t) {
    LaunchScope ls;
    std::vector<double> d((size_t)Kp);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double sum = 0, dev = 0;
            int cnt = 0;
            for (int k = 0; k < Kp; ++k) {
                const double* x = xyz + (size_t)pick[k] * 3 * n;
                const double ux = x[3 * i] - x[3 * j], uy = x[3 * i + 1] - x[3 * j + 1], uz = x[3 * i + 2] - x[3 * j + 2];
                d[(size_t)k] = sqrt(((ux * ux) + uy * uy) + uz * uz);
                sum += d[(size_t)k];
                cnt += d[(size_t)k] < cutoff ? 1 : 0;
            }
            const double mu = sum / (double)Kp;
            for (int k = 0; k < Kp; ++k) dev += (d[(size_t)k] - mu) * (d[(size_t)k] - mu);
            const size_t a = (size_t)i * n + j, b = (size_t)j * n + i;
            if (mean) mean[a] = mean[b] = mu;
            if (sd) sd[a] = sd[b] = sqrt(dev / (double)Kp);
            if (contact) contact[a] = contact[b] = (double)cnt / (double)Kp;
        }
    return hipSuccess;
}
hipError_t launch_ensemble_corr(const double* A, const double* B, int n, int range, double ma, double* rows, hipStream_t) {
    LaunchScope ls;
    for (int i = 0; i < n; ++i) {
        rows[i] = 0;
        for (int j = 0; j < n; ++j)
            if ((i > j ? i - j : j - i) >= range) rows[i] += (A[(size_t)i * n + j] - ma) * (B[(size_t)i * n + j] - ma);
    }
    return hipSuccess;
}

// c3d_geometry_replicas / c3d_separation_profile: restated on the host over the "device" memory as well
static double stub_dist(const double* x, int i, int j) {
    const double ux = x[3 * i] - x[3 * j], uy = x[3 * i + 1] - x[3 * j + 1], uz = x[3 * i + 2] - x[3 * j + 2];
    return sqrt(((ux * ux) + uy * uy) + uz * uz);
}
hipError_t launch_geometry(const double* xyz, int n, int K, double cutoff, int sep, int* bead_clashes, double* nearest, double* furthest, long long* clashes,
                           double* chain, hipStream_t) {
    LaunchScope ls;
    for (int k = 0; k < K; ++k) {
        const double* x = xyz + (size_t)k * 3 * n;
        long long both = 0;
        double extent = 0, cen[3] = {0, 0, 0}, g = 0;
        for (int i = 0; i < n; ++i) {
            int cnt = 0;
            double lo = INFINITY, hi = 0;
            for (int j = 0; j < n; ++j) {
                const double d = stub_dist(x, i, j);
                if ((i > j ? i - j : j - i) >= sep) { cnt += d <= cutoff ? 1 : 0; lo = d < lo ? d : lo; }
                hi = d > hi ? d : hi;
            }
            bead_clashes[(size_t)k * n + i] = cnt; nearest[(size_t)k * n + i] = lo; furthest[(size_t)k * n + i] = hi;
            both += cnt;
            extent = hi > extent ? hi : extent;
            for (int q = 0; q < 3; ++q) cen[q] += x[3 * i + q];
        }
        clashes[k] = both / 2;
        double* f = chain + (size_t)6 * k;
        for (int gap = 1; gap <= 2; ++gap) {
            double s = 0, v = 0;
            for (int i = 0; i + gap < n; ++i) s += stub_dist(x, i, i + gap);
            const double mu = s / (double)(n - gap);
            for (int i = 0; i + gap < n; ++i) v += (stub_dist(x, i, i + gap) - mu) * (stub_dist(x, i, i + gap) - mu);
            f[2 * gap - 2] = mu; f[2 * gap - 1] = sqrt(v / (double)(n - gap));
        }
        for (int i = 0; i < n; ++i)
            for (int q = 0; q < 3; ++q) g += (x[3 * i + q] - cen[q] / n) * (x[3 * i + q] - cen[q] / n);
        f[4] = sqrt(g / n); f[5] = extent;
    }
    return hipSuccess;
}
hipError_t launch_separation_profile(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact, hipStream_t) {
    LaunchScope ls;
    for (int s = 0; s < n; ++s) {
        const double terms = (double)(n - s) * (double)Kp;
        double sum = 0, dev = 0;
        long long cnt = 0;
        for (int k = 0; k < Kp; ++k)
            for (int i = 0; i + s < n; ++i) {
                const double d = stub_dist(xyz + (size_t)pick[k] * 3 * n, i, i + s);
                sum += d;
                cnt += d < cutoff ? 1 : 0;
            }
        mean[s] = sum / terms;
        for (int k = 0; k < Kp; ++k)
            for (int i = 0; i + s < n; ++i) {
                const double e = stub_dist(xyz + (size_t)pick[k] * 3 * n, i, i + s) - mean[s];
                dev += e * e;
            }
        if (sd) sd[s] = sqrt(dev / terms);
        if (contact) contact[s] = (double)cnt / terms;
    }
    return hipSuccess;
}

// c3d_stratified_score: the doubled average ranks inside every stratum by counting, over the "device" memory
hipError_t launch_stratified_if(const double* IF, int n, int lo, int hi, unsigned* a, long long* saa, int* flags, hipStream_t) {
    LaunchScope ls;
    for (int q = 0; q < kStrFlags; ++q) flags[q] = 0;
    size_t off = 0;
    for (int s = lo; s <= hi; off += (size_t)(n - s), ++s) {
        const int N = n - s;
        saa[s - lo] = 0;
        for (int i = 0; i < N; ++i) {
            const double v = IF[(size_t)i * n + i + s];
            if (!(v == IF[(size_t)(i + s) * n + i])) flags[0] = 1;
            if (!std::isfinite(v)) flags[1] = 1;
            long long r = 1;
            for (int j = 0; j < N; ++j) {
                const double w = IF[(size_t)j * n + j + s];
                r += (w < v ? 1 : 0) + (w <= v ? 1 : 0);
            }
            a[off + i] = (unsigned)r;
            saa[s - lo] += r * r;
        }
    }
    return hipSuccess;
}
hipError_t launch_stratified_models(const double* xyz, int n, int K, int lo, int hi, const unsigned* a, const long long* saa, long long* sums, int* flags,
                                    hipStream_t) {
    LaunchScope ls;
    memset(sums, 0, sizeof(long long) * 3 * (size_t)n * K);
    for (int k = 0; k < K; ++k) {
        const double* x = xyz + (size_t)k * 3 * n;
        size_t off = 0;
        for (int s = lo; s <= hi; off += (size_t)(n - s), ++s) {
            const long long N = n - s, T = N * (N + 1);
            std::vector<long long> q((size_t)N);
            for (int i = 0; i < N; ++i) {
                const double d = stub_dist(x, i, i + s);
                if (!(d <= 50000.0)) flags[2] = 1;
                q[(size_t)i] = d <= 50000.0 ? llround(d * 1000.0) : 0;      // (ties of the "%.3f" rounding: of no account to the harness)
            }
            long long sab = 0, sbb = 0;
            for (int i = 0; i < N; ++i) {
                long long r = 1;
                for (int j = 0; j < N; ++j) r += (q[(size_t)j] < q[(size_t)i] ? 1 : 0) + (q[(size_t)j] <= q[(size_t)i] ? 1 : 0);
                sab += (long long)a[off + i] * r;
                sbb += r * r;
            }
            long long* const out = sums + ((size_t)k * n + s) * 3;
            out[0] = N * sab - T * T; out[1] = N * saa[s - lo] - T * T; out[2] = N * sbb - T * T;
        }
    }
    return hipSuccess;
}

// c3d_bead_scores: the doubled average ranks inside every asked row by counting, and the tallies, over the "device" memory
hipError_t launch_bead_if(const double* IF, int n, int range, const int* beads, int nb, unsigned* a, long long* saa, int* flags, hipStream_t) {
    LaunchScope ls;
    for (int b = 0; b < nb; ++b) {
        const int i = beads ? beads[b] : b;
        const double* row = IF + (size_t)i * n;
        saa[b] = 0;
        for (int j = 0; j < n; ++j) {
            if ((i > j ? i - j : j - i) < range) continue;
            if (!std::isfinite(row[j])) flags[1] = 1;
            long long r = 1;
            for (int m = 0; m < n; ++m)
                if ((i > m ? i - m : m - i) >= range) r += (row[m] < row[j] ? 1 : 0) + (row[m] <= row[j] ? 1 : 0);
            a[(size_t)b * n + j] = (unsigned)r;
            saa[b] += r * r;
        }
    }
    return hipSuccess;
}
hipError_t launch_bead_models(const double* xyz, int n, int K, int range, const int* beads, int nb, const unsigned* a, const long long* saa, const float* tgt,
                              int npad, const int* t10, int min_sep, long long* sums, int* restrained, int* satisfied, long long* dev_milli, int* flags,
                              hipStream_t) {
    LaunchScope ls;
    std::vector<long long> q((size_t)n);
    for (int k = 0; k < K; ++k) {
        const double* x = xyz + (size_t)k * 3 * n;
        for (int b = 0; b < nb; ++b) {
            const int i = beads ? beads[b] : b;
            long long N = 0, sab = 0, sbb = 0, cnt = 0, sat = 0, dev = 0;
            for (int j = 0; j < n; ++j) {
                const double d = stub_dist(x, i, j);
                if (!(d <= 50000.0)) flags[2] = 1;
                q[(size_t)j] = d <= 50000.0 ? llround(d * 1000.0) : 0;      // (ties of the "%.3f" rounding: of no account to the harness)
                N += (i > j ? i - j : j - i) >= range ? 1 : 0;
            }
            for (int j = 0; j < n; ++j) {
                const int sep = i > j ? i - j : j - i;
                if (a && sep >= range) {
                    long long r = 1;
                    for (int m = 0; m < n; ++m)
                        if ((i > m ? i - m : m - i) >= range) r += (q[(size_t)m] < q[(size_t)j] ? 1 : 0) + (q[(size_t)m] <= q[(size_t)j] ? 1 : 0);
                    sab += (long long)a[(size_t)b * n + j] * r;
                    sbb += r * r;
                }
                if ((tgt || t10) && sep >= min_sep && sep > 0) {
                    const long long t = tgt ? (long long)lrintf(tgt[(size_t)i * npad + j] * 10.0f) : (long long)t10[(size_t)i * n + j];
                    if (t <= 0) continue;
                    const double dd = (double)q[(size_t)j] / 1000.0, tv = (double)t / 10.0;
                    ++cnt;
                    sat += (dd < tv + 0.5 ? 1 : 0) - (dd < tv - 0.5 ? 1 : 0);
                    if (dd > tv + 0.2) dev += q[(size_t)j] - 100 * t;
                    if (dd < tv - 0.2) dev += 100 * t - q[(size_t)j];
                }
            }
            const size_t at = (size_t)k * nb + b;
            if (a) {
                const long long T = N * (N + 1);
                const bool on = N > 1;
                sums[3 * at] = on ? N * sab - T * T : 0; sums[3 * at + 1] = on ? N * saa[b] - T * T : 0; sums[3 * at + 2] = on ? N * sbb - T * T : 0;
            }
            if (tgt || t10) { if (k == 0) restrained[b] = (int)cnt; satisfied[at] = (int)sat; dev_milli[at] = dev; }
        }
    }
    return hipSuccess;
}

// c3d_accessibility: plain brute force over all j, over the "device" memory (no neighbour list: keep2 is not used)
hipError_t launch_accessibility(const double* xyz, int n, int K, const double* points, int P, double R, double R2, double, int* exposed, int* flags, hipStream_t) {
    LaunchScope ls;
    for (int k = 0; k < K; ++k) {
        const double* x = xyz + (size_t)k * 3 * n;
        for (int i = 0; i < n; ++i) {
            int open = 0;
            for (int q = 0; q < 3; ++q)
                if (!(std::fabs(x[3 * i + q]) < 1e6)) flags[0] = 1;
            for (int p = 0; p < P; ++p) {
                volatile double c[3];                                        // (volatile: every product and sum rounded on its own)
                for (int q = 0; q < 3; ++q) { volatile double t = R * points[3 * p + q]; c[q] = x[3 * i + q] + t; }
                bool buried = false;
                for (int j = 0; j < n && !buried; ++j) {
                    if (j == i) continue;
                    const double e0 = c[0] - x[3 * j], e1 = c[1] - x[3 * j + 1], e2 = c[2] - x[3 * j + 2];
                    volatile double s = e0 * e0, t1 = e1 * e1, t2 = e2 * e2;
                    s = s + t1;
                    s = s + t2;
                    buried = s < R2;
                }
                open += buried ? 0 : 1;
            }
            exposed[(size_t)k * n + i] = open;
        }
    }
    return hipSuccess;
}

// c3d_compartments: the five launchers restated on the host with plain loops in index order (the definitions of include/c3d.h; no tiles,
// no block reduction: the sums' orders are not the device's)
static double stub_cpt_entry(const CptMaps& S, const double* Xb, int b, int i, int j) {
    const int q = S.q0 + b, mi = q - S.has_if, n = S.n;
    if (S.has_if && q == 0) return Xb[(size_t)i * n + j];
    const int* pick = mi < S.n_models ? S.pick + mi : S.pick;
    const int cnt = mi < S.n_models ? 1 : S.n_models;
    double sum = 0.0;
    for (int k = 0; k < cnt; ++k) sum += stub_dist(S.xyz + (size_t)pick[k] * 3 * n, i, j);
    return sum / (double)cnt;
}
static void stub_cpt_sign_largest(double* v, int n) {
    int at = 0;
    for (int j = 1; j < n; ++j)
        if (std::fabs(v[j]) > std::fabs(v[at])) at = j;
    if (v[at] < 0.0)
        for (int j = 0; j < n; ++j) v[j] = -v[j];
}
// out = X u - sub 1, one map
static void stub_cpt_product(const double* X, int n, const double* u, double sub, double* out) {
    for (int i = 0; i < n; ++i) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += X[(size_t)i * n + j] * u[j];
        out[i] = s - sub;
    }
}
static void stub_cpt_take_y(const CptWork& w, int b, int n, int nv, double* out) {
    for (int a = 0; a < nv; ++a) {
        const double* W = w.W + ((size_t)b * nv + a) * n;
        const double* P = w.P + ((size_t)b * nv + a) * n;
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += W[j];
        for (int j = 0; j < n; ++j) out[(size_t)a * n + j] = w.D[(size_t)b * n + j] * (P[j] - w.m[(size_t)b * n + j] * s) / (double)n;
    }
}
hipError_t launch_compartment_if_check(const double* M, int n, int* flags, hipStream_t) {
    LaunchScope ls;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double v = M[(size_t)i * n + j];
            if (v != M[(size_t)j * n + i]) flags[0] |= 1;
            if (!std::isfinite(v)) flags[0] |= 2;
            if (v < 0.0) flags[0] |= 4;
        }
    return hipSuccess;
}
hipError_t launch_compartment_build(const CptMaps& S, const CptWork& w, int min_sep, hipStream_t) {
    LaunchScope ls;
    const int n = S.n;
    for (int b = 0; b < S.nb; ++b) {
        double* X = w.X + (size_t)b * n * n;
        double* E = w.E + (size_t)b * n;
        E[0] = 0.0;
        for (int s = 1; s < n; ++s) {
            double sum = 0.0;
            for (int i = 0; i + s < n; ++i) sum += stub_cpt_entry(S, X, b, i, i + s);
            E[s] = sum / (double)(n - s);
        }
        for (int i = 0; i < n; ++i) {
            for (int j = i + 1; j < n; ++j) {
                const double e = E[j - i];
                X[(size_t)i * n + j] = X[(size_t)j * n + i] = j - i >= min_sep && e != 0.0 ? stub_cpt_entry(S, X, b, i, j) / e : 1.0;
            }
            X[(size_t)i * n + i] = 1.0;
        }
        for (int i = 0; i < n; ++i) {
            double sum = 0.0, dev = 0.0;
            for (int j = 0; j < n; ++j) sum += X[(size_t)i * n + j];
            const double mean = sum / (double)n;
            for (int j = 0; j < n; ++j) dev += (X[(size_t)i * n + j] - mean) * (X[(size_t)i * n + j] - mean);
            const double q = sqrt(dev / (double)n);
            w.m[(size_t)b * n + i] = mean;
            w.D[(size_t)b * n + i] = q > 0.0 ? 1.0 / q : 0.0;
        }
    }
    return hipSuccess;
}
hipError_t launch_compartment_round(const CptMaps& S, const CptWork& w, int nv, bool first, hipStream_t) {
    LaunchScope ls;
    const int n = S.n;
    for (int b = 0; b < S.nb; ++b) {
        double* V = w.V + (size_t)b * nv * n;
        if (!first) stub_cpt_take_y(w, b, n, nv, V);
        for (int a = 0; a < nv; ++a) {
            double* va = V + (size_t)a * n;
            for (int p = 0; p < a; ++p) {
                const double* vp = V + (size_t)p * n;
                double d = 0.0;
                for (int j = 0; j < n; ++j) d += vp[j] * va[j];
                for (int j = 0; j < n; ++j) va[j] -= d * vp[j];
            }
            double nn = 0.0;
            for (int j = 0; j < n; ++j) nn += va[j] * va[j];
            if (!(nn > 0.0)) w.flags[1] = 1;
            const double norm = sqrt(nn);
            for (int j = 0; j < n; ++j) va[j] /= norm;
            double* u = w.U + ((size_t)b * nv + a) * n;
            double c = 0.0;
            for (int j = 0; j < n; ++j) { u[j] = w.D[(size_t)b * n + j] * va[j]; c += w.m[(size_t)b * n + j] * u[j]; }
            w.c[(size_t)b * kCptVecs + a] = c;
        }
        for (int a = 0; a < nv; ++a) {
            stub_cpt_product(w.X + (size_t)b * n * n, n, w.U + ((size_t)b * nv + a) * n, w.c[(size_t)b * kCptVecs + a], w.W + ((size_t)b * nv + a) * n);
            stub_cpt_product(w.X + (size_t)b * n * n, n, w.W + ((size_t)b * nv + a) * n, 0.0, w.P + ((size_t)b * nv + a) * n);
        }
    }
    return hipSuccess;
}
hipError_t launch_compartment_finish(const CptMaps& S, const CptWork& w, int nv, hipStream_t) {
    LaunchScope ls;
    const int n = S.n;
    for (int b = 0; b < S.nb; ++b) {
        double* V = w.V + (size_t)b * nv * n;
        double* Y = w.U + (size_t)b * nv * n;
        stub_cpt_take_y(w, b, n, nv, Y);
        double live = 0.0;
        for (int j = 0; j < n; ++j) live += w.D[(size_t)b * n + j] > 0.0 ? 1.0 : 0.0;
        for (int a = 0; a < nv; ++a) {
            double* va = V + (size_t)a * n;
            const double* ya = Y + (size_t)a * n;
            double lam = 0.0, res = 0.0;
            for (int j = 0; j < n; ++j) lam += va[j] * ya[j];
            for (int j = 0; j < n; ++j) res += (ya[j] - lam * va[j]) * (ya[j] - lam * va[j]);
            w.stats[(size_t)b * kCptStats + a] = live > 0.0 ? lam / live : 0.0;
            w.stats[(size_t)b * kCptStats + 3 + a] = sqrt(res);
            if (!S.has_if || S.q0 + b == 0) stub_cpt_sign_largest(va, n);
        }
    }
    return hipSuccess;
}
hipError_t launch_compartment_fit(const CptMaps& S, const CptWork& w, int nv, hipStream_t) {
    LaunchScope ls;
    const int n = S.n;
    for (int b = 0; b < S.nb; ++b) {
        if (S.q0 + b == 0) continue;
        double* V = w.V + (size_t)b * nv * n;
        for (int a = 0; a < nv; ++a) {
            double* va = V + (size_t)a * n;
            const double* fa = w.F + (size_t)a * n;
            double d = 0.0, same = 0.0;
            for (int j = 0; j < n; ++j) d += va[j] * fa[j];
            if (d < 0.0) { for (int j = 0; j < n; ++j) va[j] = -va[j]; }
            else if (!(d > 0.0)) stub_cpt_sign_largest(va, n);
            for (int j = 0; j < n; ++j) same += va[j] * fa[j] > 0.0 ? 1.0 : 0.0;
            w.stats[(size_t)b * kCptStats + 6 + a] = same / (double)n;
        }
        for (int a = 0; a < nv; ++a)
            for (int f = 0; f < nv; ++f) {
                const double* va = V + (size_t)a * n;
                const double* ff = w.F + (size_t)f * n;
                double sv = 0.0, sf = 0.0, sxy = 0.0, sxx = 0.0, syy = 0.0;
                for (int j = 0; j < n; ++j) { sv += va[j]; sf += ff[j]; }
                const double mv = sv / (double)n, mf = sf / (double)n;
                for (int j = 0; j < n; ++j) { sxy += (va[j] - mv) * (ff[j] - mf); sxx += (va[j] - mv) * (va[j] - mv); syy += (ff[j] - mf) * (ff[j] - mf); }
                w.stats[(size_t)b * kCptStats + 9 + 3 * a + f] = std::fabs(sxy / sqrt(sxx * syy));
            }
    }
    return hipSuccess;
}

// c3d_insulation: the four launchers restated on the host with plain loops in index order (the definitions of include/c3d.h; no tiles,
// no rings, no block reduction: the sums' orders are not the device's)
static double stub_ins_cell(const InsJob& J, int q, int a, int b) {
    const int n = J.n, mi = q - J.has_if;
    if (J.has_if && q == 0) return J.band_if[(size_t)a * 2 * J.wmax + (b - a - 1)];
    if (mi >= J.n_models) return J.band_cons[(size_t)a * 2 * J.wmax + (b - a - 1)];
    const double d = stub_dist(J.xyz + (size_t)J.pick[mi] * 3 * n, a, b);
    return J.contact ? (d < J.cutoff ? 1.0 : 0.0) : d;
}
hipError_t launch_insulation_band(const InsJob& J, hipStream_t) {
    LaunchScope ls;
    const int n = J.n, W2 = 2 * J.wmax;
    for (int a = 0; a < n; ++a)
        for (int col = 0; col < W2; ++col) {
            const int b = a + 1 + col;
            double v = 0.0;
            if (col >= 1 && b < n) {
                for (int k = 0; k < J.n_models; ++k) {
                    const double d = stub_dist(J.xyz + (size_t)J.pick[k] * 3 * n, a, b);
                    v += J.contact ? (d < J.cutoff ? 1.0 : 0.0) : d;
                }
                if (!J.contact) v /= (double)J.n_models;
            }
            J.band_cons[(size_t)a * W2 + col] = v;
        }
    return hipSuccess;
}
hipError_t launch_insulation_squares(const InsJob& J, bool, double* mean, hipStream_t) {
    LaunchScope ls;
    const int n = J.n;
    for (int q = 0; q < J.Q; ++q)
        for (int k = 0; k < J.nw; ++k)
            for (int i = 0; i < n; ++i) {
                const int w = J.w[k];
                double sum = 0.0;
                const bool inside = i >= w && i <= n - 1 - w;
                for (int a = i - w; inside && a <= i - 1; ++a)
                    for (int b = i + 1; b <= i + w; ++b) sum += stub_ins_cell(J, q, a, b);
                const bool pooled = J.contact && q - J.has_if >= J.n_models;
                mean[((size_t)q * J.nw + k) * n + i] = inside ? sum / (double)(w * w * (pooled ? J.n_models : 1)) : std::nan("");
            }
    return hipSuccess;
}
hipError_t launch_insulation_profile(const InsJob& J, const double* mean, double* score, int* boundary, double* strength, hipStream_t) {
    LaunchScope ls;
    const int n = J.n;
    for (int row = 0; row < J.Q * J.nw; ++row) {
        const double* m = mean + (size_t)row * n;
        double* s = score + (size_t)row * n;
        double sum = 0.0, cnt = 0.0;
        for (int i = 0; i < n; ++i)
            if (m[i] > 0.0) { sum += m[i]; cnt += 1.0; }
        for (int i = 0; i < n; ++i) s[i] = m[i] > 0.0 ? std::log2(m[i] / (sum / cnt)) : std::nan("");
        const bool minima = (J.has_if && row / J.nw == 0) || J.contact;
        for (int i = 0; i < n; ++i) {
            const double yi = minima ? -s[i] : s[i];
            int mark = 0;
            double prom = 0.0;
            if (i >= 1 && i + 1 < n && yi > (minima ? -s[i - 1] : s[i - 1]) && yi > (minima ? -s[i + 1] : s[i + 1])) {
                double lmin = yi, rmin = yi;
                for (int j = i - 1; j >= 0 && (minima ? -s[j] : s[j]) <= yi; --j) lmin = std::fmin(lmin, minima ? -s[j] : s[j]);
                for (int j = i + 1; j < n && (minima ? -s[j] : s[j]) <= yi; ++j) rmin = std::fmin(rmin, minima ? -s[j] : s[j]);
                mark = 1;
                prom = yi - std::fmax(lmin, rmin);
            }
            boundary[(size_t)row * n + i] = mark;
            strength[(size_t)row * n + i] = prom;
        }
    }
    return hipSuccess;
}
hipError_t launch_insulation_fit(const InsJob& J, const double* score, const int* boundary, const double* strength, double min_strength, int tol, double* fit_r,
                                 int* fit_counts, hipStream_t) {
    LaunchScope ls;
    const int n = J.n;
    for (int q = 1; q < J.Q; ++q)
        for (int k = 0; k < J.nw; ++k) {
            const size_t rf = (size_t)k * n, rm = ((size_t)q * J.nw + k) * n, out = (size_t)(q - 1) * J.nw + k;
            double sx = 0.0, sy = 0.0, cnt = 0.0, sxy = 0.0, sxx = 0.0, syy = 0.0;
            for (int i = 0; i < n; ++i)
                if (!std::isnan(score[rm + i]) && !std::isnan(score[rf + i])) { sx += score[rm + i]; sy += score[rf + i]; cnt += 1.0; }
            const double mx = sx / cnt, my = sy / cnt;
            for (int i = 0; i < n; ++i)
                if (!std::isnan(score[rm + i]) && !std::isnan(score[rf + i])) {
                    const double ex = score[rm + i] - mx, ey = score[rf + i] - my;
                    sxy += ex * ey; sxx += ex * ex; syy += ey * ey;
                }
            if (fit_r) fit_r[out] = cnt >= 3.0 && sxx > 0.0 && syy > 0.0 ? sxy / sqrt(sxx * syy) : std::nan("");
            int c[4] = {0, 0, 0, 0};
            for (int i = 0; i < n; ++i) {
                const bool in_f = boundary[rf + i] && strength[rf + i] >= min_strength, in_m = boundary[rm + i] && strength[rm + i] >= min_strength;
                bool near_f = false, near_m = false;
                for (int j = i - std::min(tol, i); j <= i + std::min(tol, n - 1 - i); ++j) {
                    near_f = near_f || (boundary[rf + j] && strength[rf + j] >= min_strength);
                    near_m = near_m || (boundary[rm + j] && strength[rm + j] >= min_strength);
                }
                c[0] += in_f; c[1] += in_m; c[2] += in_f && near_m; c[3] += in_m && near_f;
            }
            for (int f = 0; f < 4 && fit_counts; ++f) fit_counts[out * 4 + f] = c[f];
        }
    return hipSuccess;
}

// c3d_loops: the five launchers restated on the host with plain loops in the order of the definitions (include/c3d.h; no tiles, no LDS,
// no block reduction: the orders of E's and the pile-up's sums are not the device's)
static double stub_loop_cell(const LoopJob& J, int q, int a, int b) {
    const int mi = q - J.has_if;
    if (J.has_if && q == 0) return J.band_if[(size_t)a * J.S + (b - a - J.s_lo)];
    if (mi >= J.n_models) return J.band_cons[(size_t)a * J.S + (b - a - J.s_lo)];
    return stub_dist(J.xyz + (size_t)J.pick[mi] * 3 * J.n, a, b);
}
static void stub_loop_pixel(const LoopJob& J, int q, int i, int j, double* out6) {
    const int n = J.n, w = J.w, p = J.p;
    const double* E = J.expected + (size_t)q * J.S;
    const double m = stub_loop_cell(J, q, i, j), e = E[j - i - J.s_lo];
    out6[0] = m; out6[1] = e;
    for (int x = 0; x < 4; ++x) out6[2 + x] = std::nan("");
    if (i < w || j + w > n - 1 || J.mask[i] || J.mask[j] || e == 0.0) return;
    double sm[4] = {0, 0, 0, 0}, se[4] = {0, 0, 0, 0};
    for (int a = -w; a <= w; ++a)
        for (int b = -w; b <= w; ++b) {
            const int ca = i + a, cb = j + b;
            if (J.mask[ca] || J.mask[cb]) continue;
            const bool out = std::abs(a) > p || std::abs(b) > p;
            const bool in[4] = {out && a != 0 && b != 0, out && a >= 1 && b <= -1, std::abs(a) <= 1 && std::abs(b) > p, std::abs(b) <= 1 && std::abs(a) > p};
            const double cm = stub_loop_cell(J, q, ca, cb), ce = E[cb - ca - J.s_lo];
            for (int x = 0; x < 4; ++x)
                if (in[x]) { sm[x] += cm; se[x] += ce; }
        }
    for (int x = 0; x < 4; ++x)
        if (sm[x] != 0.0 && se[x] != 0.0) out6[2 + x] = m / ((sm[x] / se[x]) * e);
}
hipError_t launch_loop_expected(const LoopJob& J, hipStream_t) {
    LaunchScope ls;
    const int n = J.n;
    for (int a = 0; J.consensus && a < n; ++a)
        for (int col = 0; col < J.S; ++col) {
            const int b = a + J.s_lo + col;
            double v = 0.0;
            for (int k = 0; b < n && k < J.n_models; ++k) v += stub_dist(J.xyz + (size_t)J.pick[k] * 3 * n, a, b);
            J.band_cons[(size_t)a * J.S + col] = b < n ? v / (double)J.n_models : 0.0;
        }
    for (int q = 0; q < J.Q; ++q)
        for (int col = 0; col < J.S; ++col) {
            const int s = J.s_lo + col;
            double sum = 0.0, cnt = 0.0;
            for (int i = 0; i + s < n; ++i)
                if (!J.mask[i] && !J.mask[i + s]) { sum += stub_loop_cell(J, q, i, i + s); cnt += 1.0; }
            J.expected[(size_t)q * J.S + col] = cnt > 0.0 ? sum / cnt : 0.0;
        }
    return hipSuccess;
}
hipError_t launch_loop_scan(const LoopJob& J, const LoopPeakRule& rule, double* ratio, unsigned char* cand, hipStream_t) {
    LaunchScope ls;
    const int n = J.n, B = J.max_sep - J.min_sep + 1;
    for (int s = J.min_sep; s <= J.max_sep; ++s)
        for (int i = 0; i < n; ++i) {
            double v[6] = {-1.0, 0.0, std::nan(""), std::nan(""), std::nan(""), std::nan("")};
            if (i + s <= n - 1) stub_loop_pixel(J, 0, i, i + s, v);
            const size_t out = (size_t)(s - J.min_sep) * n + i;
            for (int x = 0; x < 4 && ratio; ++x) ratio[(size_t)x * B * n + out] = v[2 + x];
            if (cand) cand[out] = v[2] >= rule.thr[0] && v[3] >= rule.thr[1] && v[4] >= rule.thr[2] && v[5] >= rule.thr[3] && v[0] >= rule.min_obs;
        }
    return hipSuccess;
}
hipError_t launch_loop_peaks(const LoopJob& J, int merge, int max_peaks, const unsigned char* cand, unsigned char* peak, int* rows, int* offset, int* peaks, int* report,
                             hipStream_t) {
    LaunchScope ls;
    const int n = J.n;
    int total[3] = {0, 0, 0};
    for (int i = 0; i < n; ++i) {
        int c = 0, pk = 0, lost = 0;
        for (int s = J.min_sep; s <= J.max_sep; ++s) {
            const size_t at = (size_t)(s - J.min_sep) * n + i;
            const int j = i + s;
            bool keep = cand[at] != 0;
            for (int di = -merge; keep && di <= merge; ++di)
                for (int dj = -merge; keep && dj <= merge; ++dj) {
                    const int i2 = i + di, j2 = j + dj, s2 = j2 - i2;
                    if ((di == 0 && dj == 0) || i2 < 0 || i2 >= n || s2 < J.min_sep || s2 > J.max_sep || !cand[(size_t)(s2 - J.min_sep) * n + i2]) continue;
                    const double m = stub_loop_cell(J, 0, i, j), m2 = stub_loop_cell(J, 0, i2, j2);
                    if (m2 > m || (m2 == m && (i2 < i || (i2 == i && j2 < j)))) keep = false;
                }
            peak[at] = keep;
            c += cand[at]; pk += keep;
            lost += i >= J.w && j + J.w <= n - 1 && (J.mask[i] || J.mask[j]);
            if (keep && total[1] + pk - 1 < max_peaks) { peaks[2 * (total[1] + pk - 1)] = i; peaks[2 * (total[1] + pk - 1) + 1] = j; }
        }
        rows[3 * i] = c; rows[3 * i + 1] = pk; rows[3 * i + 2] = lost;
        offset[i] = total[1];
        total[0] += c; total[1] += pk; total[2] += lost;
    }
    report[0] = total[0]; report[1] = total[1]; report[2] = std::min(total[1], max_peaks); report[3] = total[2];
    return hipSuccess;
}
hipError_t launch_loop_list(const LoopJob& J, const int* list, int L, double* at, int* closed, hipStream_t) {
    LaunchScope ls;
    for (int q = 0; q < J.Q; ++q) {
        int scored = 0, shut = 0;
        for (int l = 0; l < L; ++l) {
            double* v = at + ((size_t)q * L + l) * 6;
            stub_loop_pixel(J, q, list[2 * l], list[2 * l + 1], v);
            if (std::isnan(v[2]) || std::isnan(v[3])) continue;
            ++scored;
            shut += J.has_if && q == 0 ? (v[2] > 1.0 && v[3] > 1.0) : (v[2] < 1.0 && v[3] < 1.0);
        }
        closed[2 * q] = scored; closed[2 * q + 1] = shut;
    }
    return hipSuccess;
}
hipError_t launch_loop_apa(const LoopJob& J, const int* list, int L, int corner, double* apa, double* p2ll, hipStream_t) {
    LaunchScope ls;
    const int n = J.n, w = J.w, side = 2 * w + 1;
    for (int q = 0; q < J.Q; ++q) {
        double* A = apa + (size_t)q * side * side;
        for (int a = -w; a <= w; ++a)
            for (int b = -w; b <= w; ++b) {
                double sum = 0.0, cnt = 0.0;
                for (int l = 0; l < L; ++l) {
                    const int i = list[2 * l], j = list[2 * l + 1], ca = i + a, cb = j + b;
                    if (i < w || j + w > n - 1 || J.mask[ca] || J.mask[cb]) continue;
                    const double e = J.expected[(size_t)q * J.S + (cb - ca - J.s_lo)];
                    if (e == 0.0) continue;
                    sum += stub_loop_cell(J, q, ca, cb) / e; cnt += 1.0;
                }
                A[(a + w) * side + (b + w)] = cnt > 0.0 ? sum / cnt : std::nan("");
            }
        double sum = 0.0;
        for (int a = w - corner + 1; a <= w; ++a)
            for (int b = -w; b <= -w + corner - 1; ++b) sum += A[(a + w) * side + (b + w)];
        p2ll[q] = A[w * side + w] / (sum / (double)(corner * corner));
    }
    return hipSuccess;
}

// c3d_balance_matrix: the three launchers restated on the host with plain loops in index order (the definitions of include/c3d.h; no
// tiles, no column pairs, no block reduction: the sums' orders are not the device's)
hipError_t launch_balance_count(const BalJob& J, hipStream_t) {
    LaunchScope ls;
    for (int i = 0; i < J.n; ++i) {
        int cnt = 0;
        for (int j = 0; j < J.n; ++j)
            if (std::abs(i - j) >= J.ignore_diags && J.code[j] == 0 && J.M[(size_t)i * J.np + j] > 0.0) ++cnt;
        J.cnt[i] = cnt;
    }
    return hipSuccess;
}
hipError_t launch_balance_round(const BalJob& J, int kept, int t, int max_iters, double tol, bool half_power, hipStream_t) {
    LaunchScope ls;
    if (J.rec[3] != 0.0) return hipSuccess;
    const int n = J.n;
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        double row = 0.0;
        for (int j = 0; j < n && J.code[i] == 0; ++j)
            if (std::abs(i - j) >= J.ignore_diags) row += J.M[(size_t)i * J.np + j] * J.w[j];
        J.s[i] = J.code[i] == 0 ? J.w[i] * row : 0.0;
        sum += J.s[i];
    }
    const double mbar = sum / (double)kept;
    double var = 0.0;
    for (int i = 0; i < n; ++i)
        if (J.code[i] == 0) var += (J.s[i] / mbar - 1.0) * (J.s[i] / mbar - 1.0);
    var /= (double)kept;
    int stop = var < tol ? kBalConverged : t == max_iters ? kBalExhausted : 0;
    for (int i = 0; i < n && !stop; ++i) {
        if (J.code[i] != 0) continue;
        const double r = J.s[i] / mbar;
        J.w[i] /= half_power ? std::sqrt(r) : r;
        if (!(J.w[i] > 0.0 && std::isfinite(J.w[i]))) stop = kBalDiverged;
    }
    J.history[t] = var;
    J.rec[0] = var; J.rec[1] = mbar; J.rec[2] = (double)t; J.rec[3] = (double)stop;
    return hipSuccess;
}
hipError_t launch_balance_apply(const BalJob& J, double target, bool matrix, hipStream_t) {
    LaunchScope ls;
    const double f = std::sqrt(target / J.rec[1]);
    for (int i = 0; i < J.n; ++i) J.w[i] *= f;
    for (int i = 0; i < J.n && matrix; ++i)
        for (int j = 0; j < J.n; ++j) J.M[(size_t)i * J.np + j] = (J.w[i] * J.w[j]) * J.M[(size_t)i * J.np + j];
    return hipSuccess;
}

// c3d_entanglement: the two launchers restated on the host with plain loops in index order (include/c3d.h; no tiles, no LDS)
static double stub_half_angle(const double* u, const double* v, const double* w) {
    const double nu = sqrt(((u[0] * u[0]) + u[1] * u[1]) + u[2] * u[2]), nv = sqrt(((v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2]),
                 nw = sqrt(((w[0] * w[0]) + w[1] * w[1]) + w[2] * w[2]);
    const double num = u[0] * (v[1] * w[2] - v[2] * w[1]) + u[1] * (v[2] * w[0] - v[0] * w[2]) + u[2] * (v[0] * w[1] - v[1] * w[0]);
    const double den = nu * nv * nw + (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) * nw + (u[0] * w[0] + u[1] * w[1] + u[2] * w[2]) * nv +
                       (v[0] * w[0] + v[1] * w[1] + v[2] * w[2]) * nu;
    return num == 0.0 && den == 0.0 ? 0.0 : atan2(num, den);
}
// 2 pi g(s, t)
static double stub_ent_pair(const double* x, int s, int t) {
    double a[3], b[3], c[3], d[3];
    for (int q = 0; q < 3; ++q) {
        a[q] = x[3 * t + q] - x[3 * s + q]; c[q] = x[3 * (t + 1) + q] - x[3 * s + q];
        d[q] = x[3 * t + q] - x[3 * (s + 1) + q]; b[q] = x[3 * (t + 1) + q] - x[3 * (s + 1) + q];
    }
    return stub_half_angle(a, b, c) + stub_half_angle(a, d, b);
}
hipError_t launch_entangle_rows(const double* xyz, int n, int K, int min_sep, int max_sep, double* seg_writhe, double* seg_acn, double* writhe, double* acn,
                                hipStream_t) {
    LaunchScope ls;
    const int S = n - 1;
    const double two_pi = 2.0 * M_PI;
    for (int k = 0; k < K; ++k) {
        const double* x = xyz + (size_t)k * 3 * n;
        double tw = 0, ta = 0;
        for (int s = 0; s < S; ++s) {
            double w = 0, a = 0;
            for (int t = 0; t < S; ++t) {
                const int gap = s > t ? s - t : t - s;
                if (gap < min_sep || gap > max_sep) continue;
                const double g = stub_ent_pair(x, s, t);
                w += g; a += fabs(g);
            }
            seg_writhe[(size_t)k * S + s] = w / two_pi; seg_acn[(size_t)k * S + s] = a / two_pi;
            tw += w / two_pi; ta += a / two_pi;
        }
        writhe[k] = tw; acn[k] = ta;
    }
    return hipSuccess;
}
hipError_t launch_entangle_table(const double* xyz, int n, int K, int min_sep, int max_sep, const int* bounds, int D, double* link, double* link_abs,
                                 hipStream_t) {
    LaunchScope ls;
    const double two_pi = 2.0 * M_PI;
    for (int k = 0; k < K; ++k) {
        const double* x = xyz + (size_t)k * 3 * n;
        for (int p = 0; p < D; ++p)
            for (int q = p; q < D; ++q) {
                double w = 0, a = 0;
                for (int s = bounds[p]; s < bounds[p + 1]; ++s)
                    for (int t = bounds[q]; t < bounds[q + 1]; ++t) {
                        const int gap = s > t ? s - t : t - s;
                        if (gap < min_sep || gap > max_sep) continue;
                        const double g = stub_ent_pair(x, s, t);
                        w += g; a += fabs(g);
                    }
                const size_t base = (size_t)k * D * D;
                link[base + (size_t)p * D + q] = link[base + (size_t)q * D + p] = w / two_pi;
                link_abs[base + (size_t)p * D + q] = link_abs[base + (size_t)q * D + p] = a / two_pi;
            }
    }
    return hipSuccess;
}

// c3d_map_similarity: the two launchers restated on the host with plain loops in index order (the definitions of include/c3d.h: the
// direct double loop of the box mean, sequential sums, the doubled average ranks by counting; no tiles, no sort, no block reduction)
hipError_t launch_mapsim_smooth(const double* maps, int n, int n_maps, int h, int lo, int hi, double* band, hipStream_t) {
    LaunchScope ls;
    const int S = hi - lo + 1;
    for (int m = 0; m < n_maps; ++m) {
        const double* M = maps + (size_t)m * n * n;
        for (int s = lo; s <= hi; ++s)
            for (int i = 0; i < n; ++i) {
                double X = 0.0;
                if (i < n - s) {
                    const int j = i + s, r0 = std::max(0, i - h), r1 = std::min(n - 1, i + h), c0 = std::max(0, j - h), c1 = std::min(n - 1, j + h);
                    for (int r = r0; r <= r1; ++r) {
                        double t = M[(size_t)r * n + c0];
                        for (int c = c0 + 1; c <= c1; ++c) t += M[(size_t)r * n + c];
                        X = r == r0 ? t : X + t;
                    }
                    X /= (double)((r1 - r0 + 1) * (c1 - c0 + 1));
                }
                band[((size_t)m * S + (s - lo)) * n + i] = X;
            }
    }
    return hipSuccess;
}
hipError_t launch_mapsim_strata(const double* band, int n, int n_maps, int lo, int hi, bool keep_zeros, double* moments, long long* counts, hipStream_t) {
    LaunchScope ls;
    const int S = hi - lo + 1, pairs = n_maps * (n_maps - 1) / 2;
    for (int pr = 0; pr < pairs; ++pr) {
        int p, q;
        mapsim_pair(pr, n_maps, &p, &q);
        for (int s = lo; s <= hi; ++s) {
            const double* x = band + ((size_t)p * S + (s - lo)) * n;
            const double* y = band + ((size_t)q * S + (s - lo)) * n;
            const int N0 = n - s;
            std::vector<int> kept;
            for (int i = 0; i < N0; ++i)
                if (keep_zeros || !(x[i] == 0.0 && y[i] == 0.0)) kept.push_back(i);
            const long long N = (long long)kept.size();
            double sx = 0, sy = 0, cxy = 0, cxx = 0, cyy = 0;
            for (int i : kept) { sx += x[i]; sy += y[i]; }
            const double mx = N ? sx / (double)N : 0.0, my = N ? sy / (double)N : 0.0;
            long long saa = 0, sbb = 0;
            for (int i : kept) {
                cxy += (x[i] - mx) * (y[i] - my); cxx += (x[i] - mx) * (x[i] - mx); cyy += (y[i] - my) * (y[i] - my);
                long long a = 1, b = 1;
                for (int k : kept) { a += (x[k] < x[i]) + (x[k] <= x[i]); b += (y[k] < y[i]) + (y[k] <= y[i]); }
                saa += a * a; sbb += b * b;
            }
            const size_t at = ((size_t)pr * S + (s - lo)) * 3;
            const long long T = N * (N + 1);
            moments[at] = cxy; moments[at + 1] = cxx; moments[at + 2] = cyy;
            counts[at] = N; counts[at + 1] = N * saa - T * T; counts[at + 2] = N * sbb - T * T;
        }
    }
    return hipSuccess;
}

}  // namespace c3d
