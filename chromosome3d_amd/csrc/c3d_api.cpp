// c3d_api.cpp — C-ABI host of libc3d.so: the context's lifetime, device buffers, targets (K1), start structures and the embedding,
// coordinates in floats and doubles, c3d_eval*.  Compiled with hipcc (-x hip) for the HIP runtime API only, like the other five host units:
// c3d_config.cpp (model, schedule, options, stats), c3d_gate.cpp (code objects, the gate every entry runs under), c3d_run.cpp (schedule ->
// launch program, its executor), c3d_debug.cpp (the table test hooks) and c3d_analysis.cpp (score, compare, superpose); c3d_ctx.h holds what they share.  The kernels live in
// c3d_device.hip (per-step), c3d_cluster.hip (multi-step), c3d_embed.hip, c3d_score.hip, c3d_f64.hip, c3d_sym.hip.
#include <cstdlib>

#include "c3d_ctx.h"

using namespace c3d::host;

namespace {
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
// four random words of (seed, replica) for one bead and purpose: the key is the pair, the counter what it is drawn for
void philox_draw(uint64_t seed, uint32_t replica, uint32_t bead, uint32_t purpose, uint32_t out[4]) {
    const uint32_t ctr[4] = {bead, purpose, 0u, 0u};
    const uint32_t key[2] = {(uint32_t)(seed & 0xFFFFFFFFu) ^ (replica * 0x9E3779B9u), (uint32_t)(seed >> 32) + replica};
    philox4x32(ctr, key, out);
}
void normals4(uint64_t seed, uint32_t replica, uint32_t bead, uint32_t purpose, double g[4]) {
    uint32_t r[4];
    philox_draw(seed, replica, bead, purpose, r);
    const double two_pi = 6.283185307179586476925286766559;
    double a = sqrt(-2.0 * log(u01(r[0]))), b = two_pi * u01(r[1]);
    g[0] = a * cos(b); g[1] = a * sin(b);
    a = sqrt(-2.0 * log(u01(r[2]))); b = two_pi * u01(r[3]);
    g[2] = a * cos(b); g[3] = a * sin(b);
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

void set_dims(c3d_ctx* c, int n) {
    c->n = n;
    c->npad = (n + 255) / 256 * 256;   // one column block of the pair kernel = 256 columns
    c->ntiles = (n + c3d::kTileRows - 1) / c3d::kTileRows;
    c->rep_floats = (size_t)3 * c->npad;
}

// Coordinate `comp` of the k-th padding bead behind a replica's beads: far from the chain and from one another (k64_import places them
// the same way).  Whole numbers of at most 34080 (kPadCoord = 1e4, k < 256): exact in float, so the doubles of c3d_set_coords_f64 are these.
float pad_coord(int comp, int k) { return c3d::kPadCoord * (float)(comp + 1) + 16.0f * (float)k; }

// AoS host (nrep*n*3) -> SoA padded device layout
void pack(const c3d_ctx* c, const float* aos, std::vector<float>& soa, bool pad_far) {
    soa.assign(c->rep_floats * c->nrep, 0.0f);
    for (int r = 0; r < c->nrep; ++r) {
        float* base = soa.data() + c->rep_floats * r;
        for (int comp = 0; comp < 3; ++comp) {
            for (int i = 0; i < c->n; ++i) base[(size_t)comp * c->npad + i] = aos[((size_t)r * c->n + i) * 3 + comp];
            if (pad_far)
                for (int i = c->n; i < c->npad; ++i) base[(size_t)comp * c->npad + i] = pad_coord(comp, i - c->n);
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

// the three energies of a replica (NOE, bond + angle, repel) out of the four sums a replica's energy kernel leaves in the stage
void copy_energies(const c3d_ctx* c, double* e) {
    const double* h = static_cast<const double*>(c->h_stage);
    for (int r = 0; r < c->nrep; ++r) for (int k = 0; k < 3; ++k) e[3 * r + k] = h[4 * r + k];
}
// the last stage's repel contact scale (0.85 without a schedule): what the embedding's lower bound and c3d_get_energies evaluate at
float final_repel_s(const c3d_ctx* c) { return c->stages.empty() ? 0.85f : c->stages.back().repel_s; }

// fp64 state <- the fp32 coordinates of the current parity (start structures, c3d_set_coords, the DG embedding); velocities zero
int import64(c3d_ctx* c) {
    LAUNCH_TRY("fp64 import", c3d::launch_import64(dev_model(c), c->buf.X[c->parity], c->b64, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}
}  // namespace

namespace c3d::host {
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
// fp64 target matrix from the resident integer tenths, in the encoding the current model's kernel expects (c3d_f64.hip pair64)
int build_targets64(c3d_ctx* c) {
    const c3d::Model64 m = c3d::model64(dev_model(c), c->model);
    LAUNCH_TRY("fp64 targets", c3d::launch_targets64(m, c3d::form64(m, 0.0, 0), c->b64.t10, c->b64.T, c->stream));   // (the encoding follows pot and gen alone)
    HIP_TRY(hipStreamSynchronize(c->stream));
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
}  // namespace c3d::host

// =============================================================================================
extern "C" int c3d_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
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
    // Code objects (c3d_gate.cpp "code objects"): what a default job launches from is loaded HERE, on this thread, before the context makes its first
    // HIP resource — not by a helper thread beside the caller's first launches, as in rounds 4-5 (that saved the first job of a process ~13 ms
    // and is where the one device exception of round 5 was met).  Later contexts of the device find the units loaded (one atomic load).
    if (const int rc = preload_units(device)) return rc;
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
    LAUNCH_TRY("K1 launch", c3d::launch_if_to_target(dIF.p, n, c->npad, alpha, K, c->model.min_sep, c->model.rep_sep, dP.p, dpart.p, npartial, ddist.p,
                                                     c->buf.tgt, dflags.p, dnflag.p, c->stream));
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
        if ((i > j ? i - j : j - i) < c->model.min_sep) continue;      // closer than min_sep: no restraint, as in the matrix entry and k64_targets
        const float t = (float)((double)rt10[k] / 10.0);
        enc[(size_t)i * c->npad + j] = c3d::encode_target_host(t);
        enc[(size_t)j * c->npad + i] = c3d::encode_target_host(t);
    }
    dev_free(c->buf.tgt); dev_free(c->buf.tgs2);
    HIP_TRY(hipMalloc(&c->buf.tgt, sizeof(float) * enc.size()));
    HIP_TRY(hipMemcpyAsync(c->buf.tgt, enc.data(), sizeof(float) * enc.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->h_dist10.clear();
    // the list itself, for a precision-64 context (c3d_init_replicas): 0-based, i < j, the last entry of a pair as in `enc` above
    // (k64_targets drops the pairs closer than min_sep itself); `held` = the pairs that carry a restraint, what c3d_num_restraints reports
    int held = 0;
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
            if (last > 0 && (int)(key[q].first % n) - (int)(key[q].first / n) >= c->model.min_sep) ++held;
            last = 0;
        }
    }
    c->R = held;
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
                uint32_t u[4];
                philox_draw(seed, rid, (uint32_t)i, 2u, u);
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
                LAUNCH_TRY("fp64 tenths", c3d::launch_tenths64(n, (int)R, dl.p, dl.p + R, dl.p + 2 * R, c->b64.t10, c->stream));
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
        if (int rc = build_targets64(c)) return rc;                // every time: the model may have changed since the last call
        if (int rc = import64(c)) return rc;
    }
    return C3D_OK;
}

// A7: the lower bound of pairs without a restraint, the last stage's repel contact distance (formed in float)
static float dg_lower(const c3d_ctx* c) { return final_repel_s(c) * c->model.r0_rep; }

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
    LAUNCH_TRY("embed launch", e);
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->last_embed_form = tiled ? 1 : 0;
    c->last_embed_batches = (nrep + batch - 1) / batch;
    return c->precision == 64 ? import64(c) : C3D_OK;
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
    LAUNCH_TRY("smoothing launch", c3d::launch_dg_smooth(c->buf.tgt, n, c->npad, c->model.b0, dg_lower(c), U.p, L.p, c->stream));
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
    return c->precision == 64 ? import64(c) : C3D_OK;
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
            for (int i = n; i < np; ++i) dst[i] = pad_coord(comp, i - n);
        }
    for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipMemcpyAsync(c->b64.X[k], h, sizeof(double) * n3, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(c->b64.V[k], 0, sizeof(double) * n3, c->stream));
    }
    LAUNCH_TRY("fp64 export", c3d::launch_export64(dev_model(c), c->b64, c->parity, c->buf.X[c->parity], c->buf.V[c->parity], c->buf.P[c->parity], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

extern "C" int c3d_eval(c3d_ctx* c, float w_all, float w_vdw, float repel_s, float* F, double* e) {
    if (!c || !c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_eval: bad state");
    C3D_ENTRY(c, 0u);
    const c3d::DevModel m = dev_model(c);
    const c3d::DevStep p = dev_step(c, 3, 0.0f, w_all, w_vdw, repel_s, 0.0f);
    if (F) {
        LAUNCH_TRY("eval launch", c3d::launch_eval_forces(m, p, c->buf, c->parity, c->d_feval, c3d::general_step(m, p), c->eval_rpw,
                                                          c3d::column_chunk_for(m, c->column_chunk), c->stream));
        if (int rc = get_soa(c, c->d_feval, F)) return rc;
    }
    if (e) {
        const double rr = (double)repel_s * (double)c->model.r0_rep;
        LAUNCH_TRY("energy launch", c3d::launch_energy(m, p, c->buf, c->parity, c->model.s_noe, c->model.k_rep, rr * rr, c->stream));
        if (int rc = read_back(c, c->buf.E, sizeof(double) * 4 * (size_t)c->nrep)) return rc;
        copy_energies(c, e);
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
    const c3d::Model64 m64 = c3d::model64(m, c->model);
    if (F) {
        const c3d::Step64 p = c3d::step64(m64, 3, 0.0, w_all, w_vdw, repel_s, 0.0);
        LAUNCH_TRY("fp64 eval launch", c3d::launch_eval_forces64(m, m64, p, c3d::form64(m64, w_all, c->f64_column_chunk), c->b64, c->parity, c->b64.F, c->stream));
        if (int rc = get_soa64(c, c->b64.F, F)) return rc;
    }
    if (e) {
        const double rr = repel_s * (double)c->model.r0_rep;
        LAUNCH_TRY("fp64 energy launch", c3d::launch_energy64(m, m64, rr * rr, c->b64, c->parity, c->b64.F + n3, c->stream));
        if (int rc = read_back(c, c->b64.F + n3, sizeof(double) * 4 * (size_t)c->nrep)) return rc;
        copy_energies(c, e);
    }
    ++c->f64_evals;
    return C3D_OK;
}

extern "C" int c3d_get_energies(c3d_ctx* c, double* e) {
    if (!c || !e) return fail(C3D_ERR_INVALID, "c3d_get_energies: null argument");
    return c3d_eval(c, 1.0f, 1.0f, final_repel_s(c), nullptr, e);
}

extern "C" int c3d_rank(c3d_ctx* c, int32_t* rank) {
    if (!c || !rank) return fail(C3D_ERR_INVALID, "c3d_rank: null argument");
    std::vector<double> e((size_t)3 * std::max(c->nrep, 1));
    if (int rc = c3d_get_energies(c, e.data())) return rc;
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
    LAUNCH_TRY("tear16 launch", c3d::launch_tear16(c->num_cus, buf.p, stop.p, stats.p, iterations, c->stream));
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
