// c3d_gate.cpp — host unit of libc3d.so: the code-object loader and the gate that every HIP call of a context runs under ("code objects"
// below), the process option "preload".  g_units and t_entry_depth live here alone; the other host units see struct Entry, the macros
// C3D_ENTRY / C3D_GATE and three small functions (c3d_ctx.h).
#include <atomic>
#include <condition_variable>
#include <mutex>

#include "c3d_ctx.h"

using namespace c3d::host;

namespace {
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
std::atomic<int> g_preload{1};                     // process option "preload": what c3d_create loads (preload_units)
}  // namespace

namespace c3d::host {
Entry::Entry(const c3d_ctx* c, unsigned extra, bool launches) {
    if (hipSetDevice(c->device) != hipSuccess) { rc = fail(C3D_ERR_HIP, "hipSetDevice failed"); return; }
    if (launches) rc = ensure_units(c->device, units_wanted(c) | extra);
    if (rc != C3D_OK) return;
    if (t_entry_depth++ == 0) { g_units.rw.lock_shared(); locked = true; }
}
Entry::~Entry() {
    if (rc != C3D_OK) return;
    --t_entry_depth;
    if (locked) g_units.rw.unlock_shared();
}

int preload_units(int device) {
    const int pre = g_preload.load();
    return pre ? ensure_units(device, pre >= 2 ? kUnitsAll : kUnitsDefault) : C3D_OK;
}
long units_loaded() { return g_units.loads.load(); }
unsigned units_loaded_mask(int device) { return g_units.loaded[device & (kMaxDevices - 1)].load(); }
}  // namespace c3d::host

extern "C" int c3d_set_process_option(const char* key, double value) {
    if (!key) return fail(C3D_ERR_INVALID, "c3d_set_process_option: null key");
    if (!strcmp(key, "preload")) {
        if (value != 0 && value != 1 && value != 2) return fail(C3D_ERR_INVALID, "c3d_set_process_option: preload is 0, 1 or 2");
        g_preload.store((int)value);
        return C3D_OK;
    }
    return fail(C3D_ERR_INVALID, std::string("c3d_set_process_option: unknown key ") + key);
}
