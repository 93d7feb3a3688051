// c3d_analysis.cpp — host unit of libc3d.so: the output side.  What a run's models are worth and how they relate, from the coordinates
// resident on the device (kernels: c3d_score.hip): c3d_score_replicas, c3d_compare_replicas, c3d_superpose_replicas, c3d_rmsd_table,
// c3d_ensemble_map, c3d_ensemble_score, c3d_geometry_replicas, c3d_separation_profile, c3d_stratified_score, c3d_bead_scores, c3d_accessibility (with the host-only c3d_sphere_points), c3d_compartments (with the host-only c3d_compartment_start), c3d_insulation, c3d_loops, c3d_entanglement, the input side's c3d_balance_matrix and c3d_map_similarity, and the test hooks c3d_debug_if_ranks / c3d_debug_distance_ranks.  What they share comes first: typed
// scratch slots (Slot, Block, Carve, CallScratch), the ranker (rank_matrix) and the models of a call (model_set_check, model_set_coords, gather_models).
#include <limits>

#include "c3d_ctx.h"

using namespace c3d::host;

// ---- scratch: one device allocation per call (or the context's d_score), carved into typed slots ----
// `count` elements of T at byte offset `off` of an allocation: a layout says type and size once, at() gives the pointer
template <class T>
struct Slot {
    size_t off = 0, count = 0;
    size_t bytes() const { return sizeof(T) * count; }
    T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};
// two slots that one copy reads back from first.at(): taken together, so that nothing lies between them but `first`'s rounding, if any
template <class A, class B>
struct Block {
    Slot<A> first;
    Slot<B> second;
    size_t second_at() const { return second.off - first.off; }       // where `second` begins in the copy
    size_t bytes() const { return second_at() + second.bytes(); }
};
// take() gives the next slot and moves on by its size rounded up to 256 bytes; take_packed() a block without rounding between its slots.
// The four layouts below are a Carve with names for its slots.
struct Carve {
    size_t total = 0;
    template <class T>
    Slot<T> take(size_t count) { const Slot<T> s{total, count}; total += (s.bytes() + 255) & ~(size_t)255; return s; }
    template <class A, class B>
    Block<A, B> take_packed(size_t na, size_t nb) { const Slot<A> a{total, na}; const Slot<B> b{total + a.bytes(), nb}; take<char>(a.bytes() + b.bytes()); return {a, b}; }
};
// what ranking a matrix needs beside the matrix: the sort keys, the per-row sums of (rank - mean)^2 and the asymmetry flag
struct RankSlots { Slot<unsigned long long> keys; Slot<double> rows; Slot<int> asym; };

// the scratch of one call: freed when it goes, whatever the exit path
struct CallScratch : DevTmp<char> {
    int alloc(size_t bytes, const char* who) {
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) return C3D_OK;
        p = nullptr;
        (void)hipGetLastError();
        const std::string msg = std::string(who) + ": no device memory for " + std::to_string(bytes) + " bytes of scratch (" + hipGetErrorString(e) + ")";
        return fail(e == hipErrorOutOfMemory ? C3D_ERR_NOMEM : C3D_ERR_HIP, msg);
    }
};
// device -> the pinned stage, then the n row sums there added in index order: a fixed order, so the same bits every call
static int read_row_sum(c3d_ctx* c, const double* d_rows, int n, double* sum) {
    if (int rc = read_back(c, d_rows, sizeof(double) * (size_t)n)) return rc;
    const double* const rows = static_cast<const double*>(c->h_stage);
    double s = 0;
    for (int i = 0; i < n; ++i) s += rows[i];
    *sum = s;
    return C3D_OK;
}

// ---- the ranker ----
// pairs i < j, j - i >= range, of an n x n matrix: half the ranked multiset
static size_t rank_half_pairs(int n, int range) {
    const size_t w = n > range ? (size_t)(n - range) : 0;
    return w * (w + 1) / 2;
}
// The n x n matrix at d_M ranked in place (c3d_score.hip k_rank_*: launch_if_rank_keys, launch_if_rank_sort), the host's ranks bit for bit;
// R's slots lie in the allocation at `base`.  *sum = its n row sums of (rank - mean)^2 added in index order.  *symmetric = false, and
// nothing ranked or summed, when M(i,j) != M(j,i) for a ranked pair: the caller ranks on the host or refuses.
static int rank_matrix(c3d_ctx* c, void* base, double* d_M, const RankSlots& R, int range, size_t mh, size_t slots, double* sum, bool* symmetric) {
    const int n = c->n;
    LAUNCH_TRY("rank key launch", c3d::launch_if_rank_keys(d_M, n, range, R.keys.at(base), mh, slots, R.asym.at(base), c->stream));
    if (int rc = read_back(c, R.asym.at(base), R.asym.bytes())) return rc;
    *symmetric = *static_cast<const int*>(c->h_stage) == 0;
    if (!*symmetric) return C3D_OK;
    const double ma = 0.5 * (2.0 * (double)mh + 1.0);
    LAUNCH_TRY("rank sort launch", c3d::launch_if_rank_sort(d_M, n, range, R.keys.at(base), mh, slots, ma, R.rows.at(base), c->stream));
    return read_row_sum(c, R.rows.at(base), n, sum);
}

// ---- the models of a call ----
// What an entry over the K = nrep + n_extra models of a call refuses first, in this order (`lacking`: the entry's own wording of why it
// needs min_beads beads).  The entry's own checks follow, then model_set_coords.
static int model_set_check(const c3d_ctx* c, const char* who, int min_beads, const char* lacking, const double* extra_xyz, int n_extra) {
    const std::string w = std::string(who) + ": ";
    if (!c) return fail(C3D_ERR_INVALID, w + "null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, w + "call c3d_init_replicas first");
    if (c->n < min_beads) return fail(C3D_ERR_INVALID, w + "models of fewer than " + std::to_string(min_beads) + " beads have " + lacking);
    if (n_extra < 0 || (n_extra > 0 && !extra_xyz)) return fail(C3D_ERR_INVALID, w + "n_extra < 0, or extra models without coordinates");
    if ((long)c->nrep + n_extra > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, w + "more than C3D_COMPARE_MAX_MODELS models");
    return C3D_OK;
}
static int model_set_coords(const c3d_ctx* c, const char* who, const double* extra_xyz, int n_extra) {
    return n_extra > 0 ? c3d::check_model_coords(extra_xyz, (size_t)3 * c->n * n_extra, who) : C3D_OK;
}
// Which coordinates of the replicas an entry reads.  STATE: the fp64 state itself on a precision-64 context, else the floats widened —
// superposition, rmsd table and the ensemble's maps.  FLOAT_MIRROR: the floats widened on every context, which on a precision-64 context are
// the state rounded to float — c3d_compare_replicas and its hook, whose host twin c3d_model_similarity is fed the floats of c3d_get_coords
// (tests/test_gpu_compare.py holds the tables to that).
enum class ModelSource { STATE, FLOAT_MIRROR };
// The only way models reach the device: replicas first .. first + nrep - 1, then n_extra models of the caller, n x 3 doubles each at d_xyz
static int gather_models(c3d_ctx* c, ModelSource src, int first, int nrep, double* d_xyz, const double* extra_xyz, int n_extra, const char* what) {
    const int n = c->n;
    const hipError_t e = src == ModelSource::STATE && c->precision == 64
                             ? c3d::launch_superpose_gather64(c->b64.X[c->parity] + (size_t)first * 3 * c3d::cols64(n), n, c3d::cols64(n), nrep, d_xyz, c->stream)
                             : c3d::launch_compare_coords(c->buf.X[c->parity] + (size_t)first * c->rep_floats, n, c->npad, nrep, d_xyz, c->stream);
    if (e != hipSuccess) return fail(C3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    if (n_extra > 0)
        HIP_TRY(hipMemcpyAsync(d_xyz + (size_t)3 * n * nrep, extra_xyz, sizeof(double) * 3 * (size_t)n * n_extra, hipMemcpyHostToDevice, c->stream));
    return C3D_OK;
}

// ---- scoring (c3d_score.hip k_score_*, k_rank_*) ----
// c3d_score_replicas' scratch inside d_score: the rank matrix (which first holds the matrix itself when the device ranks it), rounded
// coordinates, per-row sums, the two fixed histograms, the overflow flag, the replicas' bounding boxes (read by the re-run of a wide call
// only) and, when the device ranks, the rank slots
struct ScoreScratch : Carve {
    Slot<double> rank, xr, part, box;
    Slot<unsigned> hist, below;
    Slot<int> ovf;
    RankSlots rk;
    ScoreScratch(int n, int nrep, unsigned nbins, size_t key_slots) {
        rank = take<double>((size_t)n * n);
        xr = take<double>(3 * (size_t)n * nrep);
        part = take<double>(4 * (size_t)n * nrep);
        hist = take<unsigned>((size_t)nbins * nrep);
        below = take<unsigned>((size_t)nbins * nrep);
        ovf = take<int>(1);
        box = take<double>(6 * (size_t)nrep);
        if (key_slots) {
            rk.keys = take<unsigned long long>(key_slots);
            rk.rows = take<double>((size_t)n);
            rk.asym = take<int>(1);
        }
    }
};
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

// test hook: the rank matrix, m and saa as the device computes them for c3d_score_replicas (whatever the option device_ranks says)
extern "C" int c3d_debug_if_ranks(c3d_ctx* c, const double* IF, int range, double* rank, double* saa, size_t* m) {
    if (!c || !IF || !rank || !saa || !m || range < 1) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: bad arguments");
    if (!c->have_targets) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: set the IF matrix / restraints first");
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int n = c->n;
    const size_t mh = rank_half_pairs(n, range), slots = c3d::if_rank_key_slots(mh);
    if (mh < 1) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: range leaves no pairs");
    const ScoreScratch L(n, c->have_replicas ? c->nrep : 0, 1u << 18, slots);
    if (int rc = score_scratch(c, L.total)) return rc;
    double* const d_rank = L.rank.at(c->d_score);
    bool symmetric = false;
    HIP_TRY(hipMemcpyAsync(d_rank, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
    if (int rc = rank_matrix(c, c->d_score, d_rank, L.rk, range, mh, slots, saa, &symmetric)) return rc;
    if (!symmetric) return fail(C3D_ERR_INVALID, "c3d_debug_if_ranks: the matrix is not symmetric over the ranked pairs (the host ranks such a matrix)");
    HIP_TRY(hipMemcpyAsync(rank, d_rank, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *m = 2 * mh;
    return C3D_OK;
}

// The IF side of c3d_score_replicas' coefficient: the rank matrix on the device (NULL: no coefficient asked for), m ranked pairs, their mean
// rank and sum of squares about it.  `host`: the ranks the host computed in this call; the copy to the device reads it, so it lives as long.
struct IfSide {
    std::vector<double> host;
    const double* d_rank = nullptr;
    size_t m = 0;
    double ma = 0, saa = 0;
    double mb() const { return 0.5 * ((double)m + 1.0); }      // the models' side: the mean of the ranks 1..m, ties or not
};
// Step 1, who ranks IF.  *prefetched: c3d_set_if_matrix's helper thread ranked this matrix (same numbers: memcmp) at this range.  Returns whether
// the device is tried (option device_ranks): 1 = for every matrix, 0 = beyond the default bead limit where no prefetch covers it, -1 = never.
static bool score_try_device(c3d_ctx* c, const double* IF, int range, bool* prefetched) {
    const int n = c->n;
    c->ifr.join();
    *prefetched = c->ifr.valid && c->ifr.n == n && c->ifr.range == range && c->ifr.matrix.size() == (size_t)n * n &&
                  memcmp(c->ifr.matrix.data(), IF, sizeof(double) * (size_t)n * n) == 0;
    return c->device_ranks > 0 || (c->device_ranks == 0 && n > C3D_MAX_BEADS_DEFAULT && !*prefetched);
}
// ... and the ranks into the scratch: the device's where it is tried and finds the matrix symmetric, else the prefetched or c3d::if_pair_ranks'
static int score_if_ranks(c3d_ctx* c, const double* IF, int range, bool try_device, bool prefetched, const ScoreScratch& L, size_t mh, size_t slots, IfSide* a) {
    const int n = c->n;
    double* const d_rank = L.rank.at(c->d_score);
    bool ranked = false;
    if (try_device) {
        if (2 * mh < 2) return fail(C3D_ERR_INVALID, "c3d_score_replicas: range leaves no pairs");
        HIP_TRY(hipMemcpyAsync(d_rank, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
        if (int rc = rank_matrix(c, c->d_score, d_rank, L.rk, range, mh, slots, &a->saa, &ranked)) return rc;
        if (ranked) { a->m = 2 * mh; a->ma = 0.5 * ((double)a->m + 1.0); ++c->device_rank_runs; }
    }
    if (!ranked) {
        const std::vector<double>* ranks = &a->host;
        if (prefetched && c->device_ranks <= 0) {
            ranks = &c->ifr.rank; a->m = c->ifr.m; a->ma = c->ifr.mean; a->saa = c->ifr.saa;
            ++c->rank_prefetch_hits;
        } else {
            c3d::if_pair_ranks(IF, n, range, a->host, a->m, a->ma, a->saa);
        }
        if (a->m < 2) return fail(C3D_ERR_INVALID, "c3d_score_replicas: range leaves no pairs");
        HIP_TRY(hipMemcpyAsync(d_rank, ranks->data(), sizeof(double) * ranks->size(), hipMemcpyHostToDevice, c->stream));
    }
    a->d_rank = d_rank;
    return C3D_OK;
}
// the per-row sums, and behind them the overflow flag, into the pinned stage; *overflow = a pair lay beyond the histogram of the pass
static int score_read_sums(c3d_ctx* c, const ScoreScratch& L, bool* overflow) {
    const size_t part_bytes = L.part.bytes();
    if (int rc = ensure_stage(c, part_bytes + 64)) return rc;
    char* const stage = static_cast<char*>(c->h_stage);
    HIP_TRY(hipMemcpyAsync(stage, L.part.at(c->d_score), part_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(stage + part_bytes, L.ovf.at(c->d_score), sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *overflow = *reinterpret_cast<const int*>(stage + part_bytes) != 0;
    return C3D_OK;
}
// Step 2, the first pass: distances histogrammed in `nbins` bins of 0.001 A
static int score_first_pass(c3d_ctx* c, const IfSide& a, int range, unsigned nbins, const ScoreScratch& L, bool* overflow) {
    void* const base = c->d_score;
    LAUNCH_TRY("score launch", c3d::launch_score(c->buf.X[c->parity], c->buf.tgt, a.d_rank, c->n, c->npad, c->nrep, range, c->model.min_sep, nbins, a.ma, a.mb(), 0.5,
                                                 L.xr.at(base), L.hist.at(base), L.below.at(base), L.part.at(base), L.ovf.at(base), c->stream));
    return score_read_sums(c, L, overflow);
}
// Step 3, the sized re-run.  A pair lies beyond the fixed histogram: the same kernels again with a histogram that holds the bounding box of
// the widest replica's rounded coordinates (the diagonal bounds every pair distance), replicas in batches whose two histograms fit
// C3D_SCORE_SCRATCH_BYTES.  Replicas are independent and the histogram is integer: same numbers whatever the batch, and for a replica that
// fitted the fixed histogram the numbers of the first pass.  Up to 50 000 A, the limit of c3d_spearman_if_dist_batch: a box wider than that
// along one axis holds such a pair for certain (the two beads at its ends) and is refused at once; a box whose diagonal alone is longer may
// hold none (the host accepts such a model), so it gets the largest histogram and the pass decides.
static int score_sized_rerun(c3d_ctx* c, const IfSide& a, int range, const ScoreScratch& L) {
    const int n = c->n, nrep = c->nrep;
    constexpr unsigned kMaxBins = 50000001u;             // distances 0 .. 50 000.000 A in thousandths
    const char* const too_far = "c3d_score_replicas: a pair distance exceeds 50000 A (the limit of device and host scoring)";
    double* const d_xr = L.xr.at(c->d_score);
    double* const d_box = L.box.at(c->d_score);
    int* const d_ovf = L.ovf.at(c->d_score);
    LAUNCH_TRY("score launch", c3d::launch_score_bbox(d_xr, n, nrep, d_box, c->stream));
    if (int rc = read_back(c, d_box, L.box.bytes())) return rc;
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
    HIP_TRY(hipMemsetAsync(d_ovf, 0, sizeof(int), c->stream));
    for (int r0 = 0; r0 < nrep; r0 += batch) {
        const int nb = std::min(batch, nrep - r0);
        LAUNCH_TRY("score launch", c3d::launch_score_wide(d_xr + (size_t)r0 * 3 * n, c->buf.tgt, a.d_rank, n, c->npad, nb, range, c->model.min_sep, wbins, a.ma, a.mb(), 0.5,
                                                          wide.p, wide.p + (size_t)wbins * batch, L.part.at(c->d_score) + (size_t)r0 * n * 4, d_ovf, c->stream));
    }
    bool overflow = false;
    if (int rc = score_read_sums(c, L, &overflow)) return rc;
    if (overflow) return fail(C3D_ERR_INVALID, too_far);
    ++c->score_wide_runs;
    return C3D_OK;
}

// K6 on the device: count_satisfied_tbl_rows / sum_noe_dev (:447-485, :581-600) and, when IF is given,
// spearman_IF_pdb.pl's coefficient for every replica, from the coordinates resident on the GPU.
// Distances are histogrammed in 2^18 bins of 0.001 A; a call in which a pair is further apart is scored again with a histogram sized to
// the models (score_sized_rerun).  The IF ranks come from the helper thread of c3d_set_if_matrix, from c3d::if_pair_ranks or from the
// device (option device_ranks; c3d.h).
extern "C" int c3d_score_replicas(c3d_ctx* c, const double* IF, int range, int32_t* satisfied, double* sum_dev, double* rho) {
    if (!c || range < 1) return fail(C3D_ERR_INVALID, "c3d_score_replicas: bad arguments");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, "c3d_score_replicas: call c3d_init_replicas first");
    if (rho && !IF) return fail(C3D_ERR_INVALID, "c3d_score_replicas: the Spearman coefficient needs the IF matrix");
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int n = c->n, nrep = c->nrep;
    const unsigned nbins = 1u << 18;      // distances up to 262 A in thousandths
    const bool spearman = IF && rho;
    bool prefetched = false, overflow = false;
    const bool try_device = spearman && score_try_device(c, IF, range, &prefetched);
    const size_t mh = rank_half_pairs(n, range), slots = try_device ? c3d::if_rank_key_slots(mh) : 0;
    const ScoreScratch L(n, nrep, nbins, slots);
    if (int rc = score_scratch(c, L.total)) return rc;
    IfSide a;
    if (spearman)
        if (int rc = score_if_ranks(c, IF, range, try_device, prefetched, L, mh, slots, &a)) return rc;
    if (int rc = score_first_pass(c, a, range, nbins, L, &overflow)) return rc;
    if (overflow)
        if (int rc = score_sized_rerun(c, a, range, L)) return rc;
    const double* const part = static_cast<const double*>(c->h_stage);
    for (int r = 0; r < nrep; ++r) {
        double sab = 0, sbb = 0, sat = 0, dev = 0;
        for (int i = 0; i < n; ++i) {    // fixed order: deterministic
            const double* q = part + ((size_t)r * n + i) * 4;
            sab += q[0]; sbb += q[1]; sat += q[2]; dev += q[3];
        }
        if (satisfied) satisfied[r] = (int32_t)llround(sat);
        if (sum_dev) sum_dev[r] = dev;
        if (rho) rho[r] = sab / sqrt(a.saa * sbb);
    }
    return C3D_OK;
}

// ---- the models against one another by their distances (c3d_score.hip k_cmp_*) ----
// c3d_compare_replicas' scratch: the models' fp64 coordinates, k + e of every pair and model, the sort keys of one model, the row sums of the
// distances, their totals, the table pass's per-chunk sums and the two tables
struct CompareScratch : Carve {
    Slot<double> xyz, rowsum, sums, partial, table;
    Slot<unsigned> ke;
    Slot<unsigned long long> keys;
    CompareScratch(int n, int K, size_t m, size_t slots) {
        const size_t nb = (size_t)c3d::model_blocks(K);
        xyz = take<double>(3 * (size_t)n * K);
        ke = take<unsigned>(m * K);
        keys = take<unsigned long long>(slots);
        rowsum = take<double>((size_t)n * K);
        sums = take<double>((size_t)K);
        partial = take<double>(512 * nb * nb * (size_t)c3d::compare_table_chunks(m, K));
        table = take<double>(2 * (size_t)K * K);
    }
};

// The replicas (and n_extra models given by the caller) against one another: c3d_model_similarity for every ordered pair, on the device.
// Reads X[parity] only: the float mirror on a precision-64 context too (ModelSource).
extern "C" int c3d_compare_replicas(c3d_ctx* c, const double* extra_xyz, int n_extra, double* spearman, double* rmsd) {
    if (int rc = model_set_check(c, "c3d_compare_replicas", 3, "no distances to rank", extra_xyz, n_extra)) return rc;
    if (!spearman && !rmsd) return fail(C3D_ERR_INVALID, "c3d_compare_replicas: both outputs are NULL");
    if (int rc = model_set_coords(c, "c3d_compare_replicas", extra_xyz, n_extra)) return rc;
    const int n = c->n, nrep = c->nrep, K = nrep + n_extra;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const size_t m = (size_t)n * (n - 1) / 2, slots = c3d::if_rank_key_slots(m);
    const CompareScratch L(n, K, m, slots);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_compare_replicas")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    unsigned* const d_ke = L.ke.at(tmp.p);
    double* const d_rowsum = L.rowsum.at(tmp.p);
    if (int rc = gather_models(c, ModelSource::FLOAT_MIRROR, 0, nrep, d_xyz, extra_xyz, n_extra, "compare launch")) return rc;
    for (int k = 0; k < K; ++k)
        LAUNCH_TRY("compare launch", c3d::launch_compare_ranks(d_xyz + (size_t)3 * n * k, n, L.keys.at(tmp.p), m, slots, d_ke + m * k, d_rowsum + (size_t)n * k, c->stream));
    LAUNCH_TRY("compare launch", c3d::launch_compare_table(d_xyz, d_ke, d_rowsum, n, K, m, L.sums.at(tmp.p), L.partial.at(tmp.p), L.table.at(tmp.p), c->stream));
    if (int rc = read_back(c, L.table.at(tmp.p), L.table.bytes())) return rc;
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
    const CompareScratch L(n, 1, m, slots);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_debug_distance_ranks")) return rc;
    if (int rc = gather_models(c, ModelSource::FLOAT_MIRROR, replica, 1, L.xyz.at(tmp.p), nullptr, 0, "compare launch")) return rc;
    LAUNCH_TRY("compare launch", c3d::launch_compare_ranks(L.xyz.at(tmp.p), n, L.keys.at(tmp.p), m, slots, L.ke.at(tmp.p), L.rowsum.at(tmp.p), c->stream));
    if (int rc = read_back(c, L.ke.at(tmp.p), sizeof(unsigned) * m)) return rc;
    const unsigned* const ke = static_cast<const unsigned*>(c->h_stage);
    for (size_t q = 0; q < m; ++q) rank[q] = 0.5 * (double)ke[q] + 1.0;
    return C3D_OK;
}

// ---- the models of a run in one frame (c3d_score.hip k_sup_*) ----
// the one allocation of a call: models (the target of a superposition is model K), centroids, per-chunk sums, the pairs' sums and fits, the
// block c3d_rmsd_table reads back (residuals, mirror bits), a second set of mirror bits, then (superposition only) the fitted models and the
// block c3d_superpose_replicas reads back: K sums of squares, the mean (3 n), the rmsf (n) and, packed behind these doubles, the first pass's
// mirror bits.  The table's block keeps the rounding between its two slots.
struct SuperposeScratch : Carve {
    Slot<double> xyz, cent, partial, cov, fit, fitted;
    Slot<int> mir2;
    Block<double, int> pair_out, out;
    SuperposeScratch(int n, int models, int KB, size_t pairs, bool superposition) {
        xyz = take<double>(3 * (size_t)n * models);
        cent = take<double>(3 * (size_t)models);
        partial = take<double>(c3d::superpose_partial_doubles(n, KB));
        cov = take<double>(c3d::kSupCov * pairs);
        fit = take<double>(c3d::kSupFit * pairs);
        pair_out = {take<double>(pairs), take<int>(pairs)};
        mir2 = take<int>(pairs);
        fitted = take<double>(superposition ? 3 * (size_t)n * models : 0);
        out = take_packed<double, int>(superposition ? pairs + 4 * (size_t)n : 0, superposition ? pairs : 0);
    }
};

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
    if (int rc = model_set_coords(c, "c3d_superpose_replicas", ref_xyz, reference == -1 ? 1 : 0)) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const SuperposeScratch L(n, K + 1, 1, (size_t)K, true);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_superpose_replicas")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    double* const d_target = d_xyz + (size_t)3 * n * K;
    double* const d_cent = L.cent.at(tmp.p);
    double* const d_partial = L.partial.at(tmp.p);
    double* const d_cov = L.cov.at(tmp.p);
    double* const d_fit = L.fit.at(tmp.p);
    double* const d_fitted = L.fitted.at(tmp.p);
    double* const d_out = L.out.first.at(tmp.p);
    double* const d_mean = d_out + K;
    double* const d_rmsf = d_mean + 3 * (size_t)n;
    int* const d_mir = L.out.second.at(tmp.p);      // the first pass's bits: what the caller gets
    if (int rc = gather_models(c, ModelSource::STATE, 0, K, d_xyz, ref_xyz, reference == -1 ? 1 : 0, "superpose launch")) return rc;
    if (reference >= 0)
        HIP_TRY(hipMemcpyAsync(d_target, d_xyz + (size_t)3 * n * reference, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    hipError_t e = c3d::launch_superpose_centre(d_xyz, n, K + 1, d_cent, c->stream);
    if (e == hipSuccess)
        e = c3d::launch_superpose_fit(d_xyz, K, d_target, 1, n, reference >= 0 ? reference : c3d::kSupNoIdent, (flags & C3D_SUPERPOSE_MIRROR) != 0, nullptr, d_partial, d_cov,
                                      d_fit, d_mir, d_out, c->stream);
    if (e == hipSuccess) e = c3d::launch_superpose_apply(d_xyz, K, n, d_fit, iters == 0 ? d_cent + 3 * (size_t)K : nullptr, d_fitted, c->stream);
    for (int it = 0; it < iters && e == hipSuccess; ++it) {
        // the mean of the fitted models is the next target; every model gets a rotation onto it, its handedness as the first pass left it
        e = c3d::launch_superpose_mean(d_fitted, K, n, d_mean, d_rmsf, nullptr, c->stream);
        if (e != hipSuccess) break;
        HIP_TRY(hipMemcpyAsync(d_target, d_mean, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        e = c3d::launch_superpose_centre(d_target, n, 1, d_cent + 3 * (size_t)K, c->stream);
        if (e == hipSuccess) e = c3d::launch_superpose_fit(d_xyz, K, d_target, 1, n, c3d::kSupNoIdent, false, d_mir, d_partial, d_cov, d_fit, L.mir2.at(tmp.p), nullptr, c->stream);
        if (e == hipSuccess) e = c3d::launch_superpose_apply(d_xyz, K, n, d_fit, nullptr, d_fitted, c->stream);
    }
    // iters = 0: d_out[k] keeps the fit's residual against the target; else it becomes the squared distance from the final mean
    if (e == hipSuccess) e = c3d::launch_superpose_mean(d_fitted, K, n, d_mean, d_rmsf, iters > 0 ? d_out : nullptr, c->stream);
    LAUNCH_TRY("superpose launch", e);
    if (int rc = read_back(c, d_out, L.out.bytes())) return rc;
    if (apply) {
        if (c->precision == 64) {
            const size_t n3 = (size_t)K * 3 * c3d::cols64(n);
            LAUNCH_TRY("superpose launch", c3d::launch_superpose_store64(d_fitted, n, c3d::cols64(n), K, c->b64.X[0], c->b64.X[1], c->stream));
            for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(c->b64.V[k], 0, sizeof(double) * n3, c->stream));
            LAUNCH_TRY("fp64 export", c3d::launch_export64(dev_model(c), c->b64, c->parity, c->buf.X[c->parity], c->buf.V[c->parity], c->buf.P[c->parity], c->stream));
        } else {
            LAUNCH_TRY("superpose launch", c3d::launch_superpose_store32(d_fitted, n, c->npad, K, c->buf.X[c->parity], c->stream));
            for (int k = 0; k < 2; ++k) HIP_TRY(hipMemsetAsync(c->buf.V[k], 0, sizeof(float) * c->rep_floats * K, c->stream));
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    const double* const h = static_cast<const double*>(c->h_stage);
    const int* const hm = reinterpret_cast<const int*>(static_cast<const char*>(c->h_stage) + L.out.second_at());
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
    if (int rc = model_set_check(c, "c3d_rmsd_table", 3, "no orientation to fit", extra_xyz, n_extra)) return rc;
    if (flags & ~C3D_SUPERPOSE_MIRROR) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: unknown flag bits (the table moves nothing: C3D_SUPERPOSE_MIRROR alone)");
    if (!rmsd && !mirrored) return fail(C3D_ERR_INVALID, "c3d_rmsd_table: both outputs are NULL");
    if (int rc = model_set_coords(c, "c3d_rmsd_table", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const size_t pairs = (size_t)K * K;
    const SuperposeScratch L(n, K, K, pairs, false);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_rmsd_table")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    hipError_t e = c3d::launch_superpose_centre(d_xyz, n, K, L.cent.at(tmp.p), c->stream);
    if (e == hipSuccess)
        e = c3d::launch_superpose_fit(d_xyz, K, d_xyz, K, n, 0, (flags & C3D_SUPERPOSE_MIRROR) != 0, nullptr, L.partial.at(tmp.p), L.cov.at(tmp.p), L.fit.at(tmp.p),
                                      L.pair_out.second.at(tmp.p), L.pair_out.first.at(tmp.p), c->stream);
    LAUNCH_TRY("superpose launch", e);
    if (int rc = read_back(c, L.pair_out.first.at(tmp.p), L.pair_out.bytes())) return rc;
    const double* const h = static_cast<const double*>(c->h_stage);
    const int* const hm = reinterpret_cast<const int*>(static_cast<const char*>(c->h_stage) + L.pair_out.second_at());
    for (size_t q = 0; q < pairs; ++q) {
        if (rmsd) rmsd[q] = sqrt(h[q] / (double)n);
        if (mirrored) mirrored[q] = hm[q];
    }
    ++c->rmsd_table_runs;
    return C3D_OK;
}

// ---- the ensemble's distance map (c3d_score.hip k_ens_*) ----
// the one allocation of a call: the models, the pick list, up to three n x n matrices (the map's outputs; the score's rank matrix of IF and
// the map it ranks next) and, for the score, the rank slots with the row sums of the two sides' products between them
struct EnsembleScratch : Carve {
    Slot<double> xyz, mat[3], rows2;
    Slot<int32_t> pick;
    RankSlots rk;
    EnsembleScratch(int n, int K, int Kp, int matrices, size_t key_slots) {
        xyz = take<double>(3 * (size_t)n * K);
        pick = take<int32_t>((size_t)Kp);
        for (int k = 0; k < matrices; ++k) mat[k] = take<double>((size_t)n * n);
        if (key_slots) {
            rk.keys = take<unsigned long long>(key_slots);
            rk.rows = take<double>((size_t)n);
            rows2 = take<double>((size_t)n);
            rk.asym = take<int>(1);
        }
    }
};
// what both entries refuse before any launch; on success *list holds the Kp model indices in summation order
static int ensemble_check(const c3d_ctx* c, const char* who, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, std::vector<int32_t>* list) {
    if (int rc = model_set_check(c, who, 2, "no pair", extra_xyz, n_extra)) return rc;
    const std::string w = std::string(who) + ": ";
    if (n_pick < 0) return fail(C3D_ERR_INVALID, w + "n_pick < 0");
    if ((n_pick > 0) != (pick != nullptr)) return fail(C3D_ERR_INVALID, w + "a pick list without a length, or a length without a list (all models: NULL and 0)");
    if (n_pick > c3d::kEnsMaxPicks) return fail(C3D_ERR_INVALID, w + "more than 4096 picks");
    const int K = c->nrep + n_extra;
    for (int k = 0; k < n_pick; ++k)
        if (pick[k] < 0 || pick[k] >= K) return fail(C3D_ERR_INVALID, w + "a pick index outside 0..K-1");
    if (n_pick > 0) list->assign(pick, pick + n_pick);
    else {
        list->resize((size_t)K);
        for (int k = 0; k < K; ++k) (*list)[(size_t)k] = k;
    }
    return C3D_OK;
}
static bool ensemble_cutoff_ok(double cutoff) { return std::isfinite(cutoff) && cutoff > 0.0; }

extern "C" int c3d_ensemble_map(c3d_ctx* c, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, double cutoff, double* mean, double* sd,
                                double* contact) {
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, "c3d_ensemble_map", extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    if (!mean && !sd && !contact) return fail(C3D_ERR_INVALID, "c3d_ensemble_map: every output is NULL");
    if (contact && !ensemble_cutoff_ok(cutoff)) return fail(C3D_ERR_INVALID, "c3d_ensemble_map: the contact map needs a finite cutoff > 0");
    if (int rc = model_set_coords(c, "c3d_ensemble_map", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size();
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    double* const outs[3] = {mean, sd, contact};
    const int matrices = (mean ? 1 : 0) + (sd ? 1 : 0) + (contact ? 1 : 0);
    const EnsembleScratch L(n, K, Kp, matrices, 0);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_ensemble_map")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    int* const d_pick = L.pick.at(tmp.p);
    double* d_out[3] = {nullptr, nullptr, nullptr};
    for (int k = 0, slot = 0; k < 3; ++k)
        if (outs[k]) d_out[k] = L.mat[slot++].at(tmp.p);
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipMemcpyAsync(d_pick, list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    LAUNCH_TRY("ensemble launch", c3d::launch_ensemble_map(d_xyz, n, d_pick, Kp, contact ? cutoff : 0.0, d_out[0], d_out[1], d_out[2], c->stream));
    // straight into the caller's matrices: the pinned stage would have to grow to their size
    for (int k = 0; k < 3; ++k)
        if (outs[k]) HIP_TRY(hipMemcpyAsync(outs[k], d_out[k], sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->ensemble_map_runs;
    return C3D_OK;
}

extern "C" int c3d_ensemble_score(c3d_ctx* c, const double* IF, int range, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, double cutoff,
                                  double* rho_mean, double* rho_contact) {
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, "c3d_ensemble_score", extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    if (!rho_mean && !rho_contact) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: both outputs are NULL");
    if (!IF) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: the Spearman coefficient needs the IF matrix");
    if (range < 1) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: range < 1");
    if (rho_contact && !ensemble_cutoff_ok(cutoff)) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: the contact map needs a finite cutoff > 0");
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size();
    const size_t mh = rank_half_pairs(n, range), slots = c3d::if_rank_key_slots(mh);
    if (mh < 1) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: range leaves no pairs");
    if (int rc = model_set_coords(c, "c3d_ensemble_score", extra_xyz, n_extra)) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    // two matrices: IF, ranked once, and the map that is ranked against it — the mean first, then the contact frequencies in the same slot
    const EnsembleScratch L(n, K, Kp, 2, slots);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_ensemble_score")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    int* const d_pick = L.pick.at(tmp.p);
    double* const d_A = L.mat[0].at(tmp.p);
    double* const d_B = L.mat[1].at(tmp.p);
    HIP_TRY(hipMemcpyAsync(d_A, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
    double saa = 0;
    bool symmetric = false;
    if (int rc = rank_matrix(c, tmp.p, d_A, L.rk, range, mh, slots, &saa, &symmetric)) return rc;
    if (!symmetric) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: the matrix is not symmetric over the ranked pairs (no host ranking here)");
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipMemcpyAsync(d_pick, list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    const double ma = 0.5 * (2.0 * (double)mh + 1.0);
    double* const want[2] = {rho_mean, rho_contact};
    for (int k = 0; k < 2; ++k) {
        if (!want[k]) continue;
        // the kernel and arguments of c3d_ensemble_map for this output alone: the same bits
        LAUNCH_TRY("ensemble launch", c3d::launch_ensemble_map(d_xyz, n, d_pick, Kp, k ? cutoff : 0.0, k ? nullptr : d_B, nullptr, k ? d_B : nullptr, c->stream));
        double sbb = 0, sab = 0;
        if (int rc = rank_matrix(c, tmp.p, d_B, L.rk, range, mh, slots, &sbb, &symmetric)) return rc;
        if (!symmetric) return fail(C3D_ERR_HIP, "c3d_ensemble_score: the device's map is not symmetric (cannot happen)");
        LAUNCH_TRY("ensemble launch", c3d::launch_ensemble_corr(d_A, d_B, n, range, ma, L.rows2.at(tmp.p), c->stream));
        if (int rc = read_row_sum(c, L.rows2.at(tmp.p), n, &sab)) return rc;
        *want[k] = sab / sqrt(saa * sbb);
    }
    ++c->ensemble_score_runs;
    return C3D_OK;
}

// ---- a model's geometry and the distance against separation (c3d_score.hip k_geo_*, k_sep_*) ----
// c3d_geometry_replicas' one allocation: the models, per bead the clash partners, the nearest counted partner and the furthest bead, per
// model the clash count and the chain fields
struct GeometryScratch : Carve {
    Slot<double> xyz, nearest, furthest, chain;
    Slot<int32_t> bead;
    Slot<long long> clashes;
    GeometryScratch(int n, int K) {
        xyz = take<double>(3 * (size_t)n * K);
        bead = take<int32_t>((size_t)n * K);
        nearest = take<double>((size_t)n * K);
        furthest = take<double>((size_t)n * K);
        clashes = take<long long>((size_t)K);
        chain = take<double>((size_t)C3D_GEOMETRY_FIELDS * K);
    }
};

extern "C" int c3d_geometry_replicas(c3d_ctx* c, const double* extra_xyz, int n_extra, double cutoff, int sep, int64_t* clashes, int32_t* bead_clashes,
                                     double* nearest, double* chain) {
    if (int rc = model_set_check(c, "c3d_geometry_replicas", 3, "no (i,i+2) distance", extra_xyz, n_extra)) return rc;
    if (!clashes && !bead_clashes && !nearest && !chain) return fail(C3D_ERR_INVALID, "c3d_geometry_replicas: every output is NULL");
    if (sep < 1 || sep > c->n - 1) return fail(C3D_ERR_INVALID, "c3d_geometry_replicas: sep outside 1..n-1");
    const bool counting = clashes || bead_clashes;
    if (counting && !ensemble_cutoff_ok(cutoff)) return fail(C3D_ERR_INVALID, "c3d_geometry_replicas: the clash count needs a finite cutoff > 0");
    if (int rc = model_set_coords(c, "c3d_geometry_replicas", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const GeometryScratch L(n, K);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_geometry_replicas")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    static_assert(sizeof(long long) == sizeof(int64_t), "the device's counts are the caller's int64_t");
    LAUNCH_TRY("geometry launch", c3d::launch_geometry(d_xyz, n, K, counting ? cutoff : -1.0, sep, L.bead.at(tmp.p), L.nearest.at(tmp.p), L.furthest.at(tmp.p),
                                                       L.clashes.at(tmp.p), L.chain.at(tmp.p), c->stream));
    // straight into the caller's arrays: the per-bead ones are 8 n K bytes, which the pinned stage would have to grow to
    if (clashes) HIP_TRY(hipMemcpyAsync(clashes, L.clashes.at(tmp.p), L.clashes.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (bead_clashes) HIP_TRY(hipMemcpyAsync(bead_clashes, L.bead.at(tmp.p), L.bead.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (nearest) HIP_TRY(hipMemcpyAsync(nearest, L.nearest.at(tmp.p), L.nearest.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (chain) HIP_TRY(hipMemcpyAsync(chain, L.chain.at(tmp.p), L.chain.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->geometry_runs;
    return C3D_OK;
}

// c3d_separation_profile's one allocation: the models, the pick list and the three profiles
struct SeparationScratch : Carve {
    Slot<double> xyz, out[3];
    Slot<int32_t> pick;
    SeparationScratch(int n, int K, int Kp) {
        xyz = take<double>(3 * (size_t)n * K);
        pick = take<int32_t>((size_t)Kp);
        for (int k = 0; k < 3; ++k) out[k] = take<double>((size_t)n);
    }
};

extern "C" int c3d_separation_profile(c3d_ctx* c, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, double cutoff, double* mean, double* sd,
                                      double* contact) {
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, "c3d_separation_profile", extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    if (!mean && !sd && !contact) return fail(C3D_ERR_INVALID, "c3d_separation_profile: every output is NULL");
    if (contact && !ensemble_cutoff_ok(cutoff)) return fail(C3D_ERR_INVALID, "c3d_separation_profile: the contact profile needs a finite cutoff > 0");
    if (int rc = model_set_coords(c, "c3d_separation_profile", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size();
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const SeparationScratch L(n, K, Kp);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, "c3d_separation_profile")) return rc;
    double* const d_xyz = L.xyz.at(tmp.p);
    int* const d_pick = L.pick.at(tmp.p);
    double* const outs[3] = {mean, sd, contact};
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipMemcpyAsync(d_pick, list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    // the mean is formed whatever was asked for: the sd is taken about it
    LAUNCH_TRY("separation launch", c3d::launch_separation_profile(d_xyz, n, d_pick, Kp, contact ? cutoff : 0.0, L.out[0].at(tmp.p), sd ? L.out[1].at(tmp.p) : nullptr,
                                                                   contact ? L.out[2].at(tmp.p) : nullptr, c->stream));
    for (int k = 0; k < 3; ++k)
        if (outs[k]) HIP_TRY(hipMemcpyAsync(outs[k], L.out[k].at(tmp.p), L.out[k].bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    ++c->separation_runs;
    return C3D_OK;
}

// ---- IF against model distance inside every genomic separation (c3d_score.hip k_str_*) ----
// c3d_stratified_score's one allocation: the models, the doubled IF ranks of every stratum (packed, diagonal-major), their sums of squares,
// C, A, B of every model and stratum, and the flag words.  IF itself lies in the context's d_score.
struct StratifiedScratch : Carve {
    Slot<double> xyz;
    Slot<unsigned> a;
    Slot<long long> saa, sums;
    Slot<int> flags;
    StratifiedScratch(int n, int K, int lo, int hi) {
        xyz = take<double>(3 * (size_t)n * K);
        a = take<unsigned>(c3d::stratified_pairs(n, lo, hi));
        saa = take<long long>((size_t)(hi - lo + 1));
        sums = take<long long>((size_t)C3D_STRATUM_FIELDS * n * K);
        flags = take<int>(c3d::kStrFlags);
    }
};
// the device time of the two passes (stats "stratified_if_ms", "stratified_models_ms"): four events of the call, destroyed when it goes
struct PassEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~PassEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

extern "C" int c3d_stratified_score(c3d_ctx* c, const double* IF, int range, int max_sep, const double* extra_xyz, int n_extra, double* rho, double* scc,
                                    int64_t* sums) {
    const char* const who = "c3d_stratified_score";
    if (int rc = model_set_check(c, who, 2, "no pair", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra;
    if (!IF) return fail(C3D_ERR_INVALID, "c3d_stratified_score: the coefficient needs the IF matrix");
    if (range < 1) return fail(C3D_ERR_INVALID, "c3d_stratified_score: range < 1");
    if (max_sep < 0 || max_sep > n - 1 || (max_sep > 0 && max_sep < range)) return fail(C3D_ERR_INVALID, "c3d_stratified_score: max_sep is 0 (for n-1) or in range..n-1");
    if (range > n - 1) return fail(C3D_ERR_INVALID, "c3d_stratified_score: range leaves no stratum (range > n-1)");
    if (!rho && !scc && !sums) return fail(C3D_ERR_INVALID, "c3d_stratified_score: every output is NULL");
    if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int lo = range, hi = max_sep ? max_sep : n - 1;
    if (int rc = score_scratch(c, sizeof(double) * (size_t)n * n)) return rc;
    double* const d_IF = static_cast<double*>(c->d_score);
    const StratifiedScratch L(n, K, lo, hi);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
    static_assert(sizeof(long long) == sizeof(int64_t), "the device's sums are the caller's int64_t");
    HIP_TRY(hipMemcpyAsync(d_IF, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    LAUNCH_TRY("stratified launch", c3d::launch_stratified_if(d_IF, n, lo, hi, L.a.at(tmp.p), L.saa.at(tmp.p), L.flags.at(tmp.p), c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    if (int rc = read_back(c, L.flags.at(tmp.p), L.flags.bytes())) return rc;
    const int* const flags = static_cast<const int*>(c->h_stage);
    if (flags[1]) return fail(C3D_ERR_INVALID, "c3d_stratified_score: an IF entry of the strata asked for is not finite");
    if (flags[0]) return fail(C3D_ERR_INVALID, "c3d_stratified_score: the matrix is not symmetric over the strata asked for");
    if (flags[3]) return fail(C3D_ERR_HIP, "c3d_stratified_score: internal: the ranks of a stratum do not add up to N(N+1)");
    double* const d_xyz = L.xyz.at(tmp.p);
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));
    LAUNCH_TRY("stratified launch", c3d::launch_stratified_models(d_xyz, n, K, lo, hi, L.a.at(tmp.p), L.saa.at(tmp.p), L.sums.at(tmp.p), L.flags.at(tmp.p), c->stream));
    HIP_TRY(hipEventRecord(ev.e[3], c->stream));
    if (int rc = read_back(c, L.flags.at(tmp.p), L.flags.bytes())) return rc;
    if (static_cast<const int*>(c->h_stage)[2]) return fail(C3D_ERR_INVALID, "c3d_stratified_score: a pair distance exceeds 50000 A (the limit of device and host scoring)");
    // the sums straight into the caller's array, or into one of the call: 24 n K bytes, which the pinned stage would have to grow to
    std::vector<int64_t> own;
    if (!sums) own.resize(L.sums.count);
    int64_t* const h = sums ? sums : own.data();
    HIP_TRY(hipMemcpyAsync(h, L.sums.at(tmp.p), L.sums.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms_if = 0, ms_models = 0;
    HIP_TRY(hipEventElapsedTime(&ms_if, ev.e[0], ev.e[1]));
    HIP_TRY(hipEventElapsedTime(&ms_models, ev.e[2], ev.e[3]));
    c->stratified_if_ms = ms_if;
    c->stratified_models_ms = ms_models;
    // rho and scc on the host, from the integers, with the header's expressions in the header's order
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < K && (rho || scc); ++k) {
        double num = 0, den = 0;
        bool any = false;
        for (int s = 0; s < n; ++s) {
            double r = nan;
            const int64_t* const q = h + ((size_t)k * n + s) * C3D_STRATUM_FIELDS;
            if (s >= lo && s <= hi && q[1] > 0 && q[2] > 0) {
                const double N = (double)(n - s), cN = N * N * N;
                const double root = sqrt((double)q[1] * (double)q[2]);
                r = (double)q[0] / root;
                num += (double)q[0] / cN;
                den += root / cN;
                any = true;
            }
            if (rho) rho[(size_t)k * n + s] = r;
        }
        if (scc) scc[k] = any ? num / den : nan;
    }
    ++c->stratified_runs;
    return C3D_OK;
}

// ---- a model's fit to the data bead by bead (c3d_score.hip k_bead_*) ----
// c3d_bead_scores' one allocation: the models, the bead list (if one was given), the doubled IF ranks of the rows asked for (B x n, only
// where a coefficient was asked for), their sums of squares, C, A, B and the tallies of every model and row, and the flag words.  IF itself
// lies in the context's d_score.
struct BeadScratch : Carve {
    Slot<double> xyz;
    Slot<int32_t> list, restrained, satisfied;
    Slot<unsigned> a;
    Slot<long long> saa, sums, dev;
    Slot<int> flags;
    BeadScratch(int n, int K, int B, bool listed, bool ranked) {
        xyz = take<double>(3 * (size_t)n * K);
        if (listed) list = take<int32_t>((size_t)B);
        if (ranked) a = take<unsigned>((size_t)B * n);
        saa = take<long long>((size_t)B);
        sums = take<long long>((size_t)C3D_BEAD_FIELDS * B * K);
        restrained = take<int32_t>((size_t)B);
        satisfied = take<int32_t>((size_t)B * K);
        dev = take<long long>((size_t)B * K);
        flags = take<int>(c3d::kStrFlags);
    }
};

extern "C" int c3d_bead_scores(c3d_ctx* c, const double* IF, int range, const int32_t* beads, int n_beads, const double* extra_xyz, int n_extra, double* rho,
                               int64_t* sums, int32_t* restrained, int32_t* satisfied, int64_t* dev_milli) {
    const char* const who = "c3d_bead_scores";
    if (int rc = model_set_check(c, who, 2, "no pair", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra;
    const bool ranked = rho || sums, tallied = restrained || satisfied || dev_milli;
    if (range < 1) return fail(C3D_ERR_INVALID, "c3d_bead_scores: range < 1");
    if (range > n - 1) return fail(C3D_ERR_INVALID, "c3d_bead_scores: range leaves no row a partner (range > n-1)");
    if (ranked && !IF) return fail(C3D_ERR_INVALID, "c3d_bead_scores: the coefficient needs the IF matrix");
    if (!ranked && !tallied) return fail(C3D_ERR_INVALID, "c3d_bead_scores: every output is NULL");
    if (!beads && n_beads != 0) return fail(C3D_ERR_INVALID, "c3d_bead_scores: n_beads without a bead list (NULL and 0 ask for every bead)");
    if (beads) {
        if (n_beads <= 0) return fail(C3D_ERR_INVALID, "c3d_bead_scores: a bead list with n_beads <= 0");
        for (int b = 0; b < n_beads; ++b)
            if (beads[b] < 0 || beads[b] >= n || (b > 0 && beads[b] <= beads[b - 1]))
                return fail(C3D_ERR_INVALID, "c3d_bead_scores: the bead list holds indices 0..n-1, strictly ascending");
    }
    if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    // the targets of the tallies: the float matrix every context fills; the integer tenths of a precision-64 context where it is not there
    const float* const d_tgt = c->buf.tgt;
    const int* const d_t10 = d_tgt ? nullptr : c->b64.t10;
    if (tallied && !d_tgt && !d_t10) return fail(C3D_ERR_INVALID, "c3d_bead_scores: the tallies need the context's target matrix");
    const int B = beads ? n_beads : n;
    double* d_IF = nullptr;
    if (ranked) {
        if (int rc = score_scratch(c, sizeof(double) * (size_t)n * n)) return rc;
        d_IF = static_cast<double*>(c->d_score);
    }
    const BeadScratch L(n, K, B, beads != nullptr, ranked);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(int) == sizeof(int32_t), "the device's sums and counts are the caller's int64_t and int32_t");
    const int* const d_list = beads ? L.list.at(tmp.p) : nullptr;
    int* const d_flags = L.flags.at(tmp.p);
    HIP_TRY(hipMemsetAsync(d_flags, 0, L.flags.bytes(), c->stream));
    if (beads) HIP_TRY(hipMemcpyAsync(L.list.at(tmp.p), beads, L.list.bytes(), hipMemcpyHostToDevice, c->stream));
    float ms_if = 0, ms_models = 0;
    if (ranked) {
        HIP_TRY(hipMemcpyAsync(d_IF, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(ev.e[0], c->stream));
        LAUNCH_TRY("bead launch", c3d::launch_bead_if(d_IF, n, range, d_list, B, L.a.at(tmp.p), L.saa.at(tmp.p), d_flags, c->stream));
        HIP_TRY(hipEventRecord(ev.e[1], c->stream));
        if (int rc = read_back(c, d_flags, L.flags.bytes())) return rc;
        const int* const flags = static_cast<const int*>(c->h_stage);
        if (flags[1]) return fail(C3D_ERR_INVALID, "c3d_bead_scores: an IF entry of the rows asked for is not finite");
        if (flags[3]) return fail(C3D_ERR_HIP, "c3d_bead_scores: internal: the ranks of a row do not add up to N(N+1)");
        HIP_TRY(hipEventElapsedTime(&ms_if, ev.e[0], ev.e[1]));
    }
    double* const d_xyz = L.xyz.at(tmp.p);
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipEventRecord(ev.e[2], c->stream));
    LAUNCH_TRY("bead launch", c3d::launch_bead_models(d_xyz, n, K, range, d_list, B, ranked ? L.a.at(tmp.p) : nullptr, L.saa.at(tmp.p), tallied ? d_tgt : nullptr, c->npad,
                                                      tallied ? d_t10 : nullptr, c->model.min_sep, L.sums.at(tmp.p), L.restrained.at(tmp.p), L.satisfied.at(tmp.p),
                                                      L.dev.at(tmp.p), d_flags, c->stream));
    HIP_TRY(hipEventRecord(ev.e[3], c->stream));
    if (int rc = read_back(c, d_flags, L.flags.bytes())) return rc;
    if (static_cast<const int*>(c->h_stage)[2]) return fail(C3D_ERR_INVALID, "c3d_bead_scores: a pair distance exceeds 50000 A (the limit of device and host scoring)");
    // straight into the caller's arrays (the sums into one of the call where only rho was asked for), as c3d_stratified_score does
    std::vector<int64_t> own;
    if (rho && !sums) own.resize(L.sums.count);
    int64_t* const h = sums ? sums : own.data();
    if (ranked) HIP_TRY(hipMemcpyAsync(h, L.sums.at(tmp.p), L.sums.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (restrained) HIP_TRY(hipMemcpyAsync(restrained, L.restrained.at(tmp.p), L.restrained.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (satisfied) HIP_TRY(hipMemcpyAsync(satisfied, L.satisfied.at(tmp.p), L.satisfied.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (dev_milli) HIP_TRY(hipMemcpyAsync(dev_milli, L.dev.at(tmp.p), L.dev.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipEventElapsedTime(&ms_models, ev.e[2], ev.e[3]));
    c->bead_if_ms = ms_if;
    c->bead_models_ms = ms_models;
    // rho on the host, from the integers, with the header's expression
    if (rho) {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (size_t r = 0; r < (size_t)K * B; ++r) {
            const int64_t* const q = h + r * C3D_BEAD_FIELDS;
            rho[r] = q[1] > 0 && q[2] > 0 ? (double)q[0] / sqrt((double)q[1] * (double)q[2]) : nan;
        }
    }
    ++c->bead_runs;
    return C3D_OK;
}

// ---- a bead's exposed surface (c3d_score.hip k_access) ----
// c3d_accessibility's one allocation: the models, the points, the K x n counts and the flag word
struct AccessScratch : Carve {
    Slot<double> xyz, points;
    Slot<int32_t> exposed;
    Slot<int> flags;
    AccessScratch(int n, int K, int P) {
        xyz = take<double>(3 * (size_t)n * K);
        points = take<double>(3 * (size_t)P);
        exposed = take<int32_t>((size_t)n * K);
        flags = take<int>(1);
    }
};

extern "C" int c3d_sphere_points(int n_points, double* u) {
    if (n_points < 1 || n_points > C3D_ACCESS_MAX_POINTS) return fail(C3D_ERR_INVALID, "c3d_sphere_points: n_points outside 1..C3D_ACCESS_MAX_POINTS");
    if (!u) return fail(C3D_ERR_INVALID, "c3d_sphere_points: null buffer");
    const double pi = 3.14159265358979323846, golden = pi * (3.0 - sqrt(5.0));
    for (int k = 0; k < n_points; ++k) {
        const double z = 1.0 - (double)(2 * k + 1) / (double)n_points, r = sqrt(1.0 - z * z), phi = (double)k * golden;
        u[3 * k] = r * cos(phi);
        u[3 * k + 1] = r * sin(phi);
        u[3 * k + 2] = z;
    }
    return C3D_OK;
}

extern "C" int c3d_accessibility(c3d_ctx* c, const double* extra_xyz, int n_extra, double radius, double probe, const double* points, int n_points, int32_t* exposed,
                                 double* device_ms) {
    const char* const who = "c3d_accessibility";
    if (int rc = model_set_check(c, who, 2, "no other bead to bury a point", extra_xyz, n_extra)) return rc;
    if (!exposed) return fail(C3D_ERR_INVALID, "c3d_accessibility: exposed is NULL");
    if (n_points < 1 || n_points > C3D_ACCESS_MAX_POINTS) return fail(C3D_ERR_INVALID, "c3d_accessibility: n_points outside 1..C3D_ACCESS_MAX_POINTS");
    if (!std::isfinite(radius) || radius <= 0.0) return fail(C3D_ERR_INVALID, "c3d_accessibility: radius is not finite or <= 0");
    if (!std::isfinite(probe) || probe < 0.0) return fail(C3D_ERR_INVALID, "c3d_accessibility: probe is not finite or < 0");
    const double R = radius + probe;
    if (!(R >= 0.01 && R <= 1e5)) return fail(C3D_ERR_INVALID, "c3d_accessibility: radius + probe outside 0.01 .. 1e5 A");
    std::vector<double> lattice;
    if (points) {
        for (int p = 0; p < n_points; ++p) {
            const double* const u = points + 3 * (size_t)p;
            const double norm2 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
            if (!(fabs(norm2 - 1.0) <= 1e-9))      // (a component that is not finite fails the comparison too)
                return fail(C3D_ERR_INVALID, "c3d_accessibility: point " + std::to_string(p) + " is not a unit vector (squared norm within 1e-9 of 1)");
        }
    } else {
        lattice.resize(3 * (size_t)n_points);
        if (int rc = c3d_sphere_points(n_points, lattice.data())) return rc;
    }
    if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const AccessScratch L(n, K, n_points);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ev.e[k]));
    static_assert(sizeof(int) == sizeof(int32_t), "the device's counts are the caller's int32_t");
    double* const d_xyz = L.xyz.at(tmp.p);
    int* const d_flags = L.flags.at(tmp.p);
    // the products of the definition's constants, formed here once: R2 as the kernel compares with it, and the neighbour bound
    const double R2 = R * R, keep2 = 4.0 * R2 * (1.0 + 0x1p-20);
    HIP_TRY(hipMemsetAsync(d_flags, 0, L.flags.bytes(), c->stream));
    HIP_TRY(hipMemcpyAsync(L.points.at(tmp.p), points ? points : lattice.data(), L.points.bytes(), hipMemcpyHostToDevice, c->stream));
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    LAUNCH_TRY("accessibility launch", c3d::launch_accessibility(d_xyz, n, K, L.points.at(tmp.p), n_points, R, R2, keep2, L.exposed.at(tmp.p), d_flags, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    if (int rc = read_back(c, d_flags, L.flags.bytes())) return rc;
    if (static_cast<const int*>(c->h_stage)[0])
        return fail(C3D_ERR_INVALID, "c3d_accessibility: a replica's coordinate is not finite or has |x| >= 1e6 (the limit of the extra models, and of the neighbour bound)");
    // straight into the caller's array, as c3d_geometry_replicas copies its per-bead counts
    HIP_TRY(hipMemcpyAsync(exposed, L.exposed.at(tmp.p), L.exposed.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (device_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *device_ms = ms;
    }
    return C3D_OK;
}

// ---- compartment eigenvectors (c3d_score.hip k_cpt_*) ----
// c3d_compartments' one allocation: the models, the pick list, the start vectors, IF's finished vectors and, per map in flight (slots), X,
// E, m, D, the four vector sets of a round, c and the results; the two flag words
struct CompartmentScratch : Carve {
    Slot<double> xyz, start, F, X, E, m, D, V, U, W, P, c, stats;
    Slot<int32_t> pick;
    Slot<int> flags;
    CompartmentScratch(int n, int K, int Kp, int nv, int slots) {
        const size_t S = (size_t)slots, vec = S * nv * n;
        xyz = take<double>(3 * (size_t)n * K);
        pick = take<int32_t>((size_t)Kp);
        start = take<double>((size_t)nv * n);
        F = take<double>((size_t)nv * n);
        X = take<double>(S * n * n);
        E = take<double>(S * n);
        m = take<double>(S * n);
        D = take<double>(S * n);
        V = take<double>(vec);
        U = take<double>(vec);
        W = take<double>(vec);
        P = take<double>(vec);
        c = take<double>(S * c3d::kCptVecs);
        stats = take<double>(S * c3d::kCptStats);
        flags = take<int>(2);
    }
};

static bool compartment_vectors_ok(int n, int n_vec) { return n_vec >= 1 && n_vec <= C3D_COMPARTMENT_MAX_VECTORS && n_vec <= n - 1; }

extern "C" int c3d_compartment_start(int n, int n_vec, double* start) {
    if (n < 3) return fail(C3D_ERR_INVALID, "c3d_compartment_start: n < 3");
    if (!compartment_vectors_ok(n, n_vec)) return fail(C3D_ERR_INVALID, "c3d_compartment_start: n_vec outside 1..min(3, n-1)");
    if (!start) return fail(C3D_ERR_INVALID, "c3d_compartment_start: null buffer");
    for (int a = 0; a < n_vec; ++a)
        for (int i = 0; i < n; ++i) {
            uint32_t h = 4u * (uint32_t)i + (uint32_t)a + 0x9E3779B9u;
            h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
            start[(size_t)a * n + i] = ((double)h + 0.5) / 4294967296.0 - 0.5;      // every step exact in fp64
        }
    return C3D_OK;
}

extern "C" int c3d_compartments(c3d_ctx* c, const double* IF, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, int flags, int min_sep,
                                int n_vec, int iters, const double* start, double* expected, double* vectors, double* share, double* residual, double* agreement,
                                double* same_side, double* device_ms) {
    const char* const who = "c3d_compartments";
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, who, extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size(), nv = n_vec;
    if (n < 3) return fail(C3D_ERR_INVALID, "c3d_compartments: maps of fewer than 3 beads have no correlation to diagonalise (n < 3)");
    if (Kp > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, "c3d_compartments: more than 256 picks");
    if (!compartment_vectors_ok(n, n_vec)) return fail(C3D_ERR_INVALID, "c3d_compartments: n_vec outside 1..min(3, n-1)");
    if (iters < 0 || iters > C3D_COMPARTMENT_MAX_ITERS) return fail(C3D_ERR_INVALID, "c3d_compartments: iters outside 0..C3D_COMPARTMENT_MAX_ITERS");
    if (min_sep < 1 || min_sep > n - 1) return fail(C3D_ERR_INVALID, "c3d_compartments: min_sep outside 1..n-1");
    if (flags & ~C3D_COMPARTMENT_CONSENSUS) return fail(C3D_ERR_INVALID, "c3d_compartments: unknown flag bits");
    const bool consensus = (flags & C3D_COMPARTMENT_CONSENSUS) != 0;
    if (consensus && Kp < 1) return fail(C3D_ERR_INVALID, "c3d_compartments: the consensus of an empty list");
    if (!expected && !vectors && !share && !agreement && !same_side)
        return fail(C3D_ERR_INVALID, "c3d_compartments: expected, vectors, share, agreement and same_side are all NULL");
    if ((agreement || same_side) && !IF) return fail(C3D_ERR_INVALID, "c3d_compartments: agreement and same_side need the IF matrix");
    std::vector<double> own;
    if (start) {
        for (size_t q = 0; q < (size_t)nv * n; ++q)
            if (!std::isfinite(start[q])) return fail(C3D_ERR_INVALID, "c3d_compartments: a start vector is not finite");
    } else {
        own.resize((size_t)nv * n);
        if (int rc = c3d_compartment_start(n, nv, own.data())) return rc;
    }
    if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    const int has_if = IF ? 1 : 0, Q = has_if + Kp + (consensus ? 1 : 0);
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    // maps in flight: as many X slots as fit the budget, one at least
    const size_t map_bytes = sizeof(double) * (size_t)n * n;
    const int slots = (int)std::min<size_t>((size_t)Q, std::max<size_t>(1, (size_t)C3D_SCORE_SCRATCH_BYTES / map_bytes));
    const CompartmentScratch L(n, K, Kp, nv, slots);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ev.e[k]));
    c3d::CptWork w;
    w.X = L.X.at(tmp.p); w.E = L.E.at(tmp.p); w.m = L.m.at(tmp.p); w.D = L.D.at(tmp.p);
    w.V = L.V.at(tmp.p); w.U = L.U.at(tmp.p); w.W = L.W.at(tmp.p); w.P = L.P.at(tmp.p);
    w.c = L.c.at(tmp.p); w.stats = L.stats.at(tmp.p); w.F = L.F.at(tmp.p); w.flags = L.flags.at(tmp.p);
    const size_t vec_bytes = sizeof(double) * (size_t)nv * n;
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    HIP_TRY(hipMemsetAsync(w.flags, 0, L.flags.bytes(), c->stream));
    HIP_TRY(hipMemcpyAsync(L.start.at(tmp.p), start ? start : own.data(), vec_bytes, hipMemcpyHostToDevice, c->stream));
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, L.xyz.at(tmp.p), extra_xyz, n_extra, "superpose launch")) return rc;
    HIP_TRY(hipMemcpyAsync(L.pick.at(tmp.p), list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    // the results of every batch gather here: the caller's arrays are written once the last batch is through
    std::vector<double> hE(expected ? (size_t)Q * n : 0), hV(vectors ? (size_t)Q * nv * n : 0), hS((size_t)Q * c3d::kCptStats);
    for (int q0 = 0; q0 < Q; q0 += slots) {
        const int nb = std::min(slots, Q - q0);
        const c3d::CptMaps maps{n, q0, nb, has_if, Kp, L.xyz.at(tmp.p), L.pick.at(tmp.p)};
        if (has_if && q0 == 0) {
            HIP_TRY(hipMemcpyAsync(w.X, IF, map_bytes, hipMemcpyHostToDevice, c->stream));
            LAUNCH_TRY("compartment launch", c3d::launch_compartment_if_check(w.X, n, w.flags, c->stream));
            if (int rc = read_back(c, w.flags, L.flags.bytes())) return rc;
            const int bad = static_cast<const int*>(c->h_stage)[0];
            if (bad & 2) return fail(C3D_ERR_INVALID, "c3d_compartments: an IF entry is not finite");
            if (bad & 4) return fail(C3D_ERR_INVALID, "c3d_compartments: an IF entry is negative");
            if (bad & 1) return fail(C3D_ERR_INVALID, "c3d_compartments: the IF matrix is not symmetric");
        }
        for (int b = 0; b < nb; ++b)
            HIP_TRY(hipMemcpyAsync(w.V + (size_t)b * nv * n, L.start.at(tmp.p), vec_bytes, hipMemcpyDeviceToDevice, c->stream));
        LAUNCH_TRY("compartment launch", c3d::launch_compartment_build(maps, w, min_sep, c->stream));
        for (int r = 0; r <= iters; ++r) LAUNCH_TRY("compartment launch", c3d::launch_compartment_round(maps, w, nv, r == 0, c->stream));
        LAUNCH_TRY("compartment launch", c3d::launch_compartment_finish(maps, w, nv, c->stream));
        if (has_if) {
            if (q0 == 0) HIP_TRY(hipMemcpyAsync(w.F, w.V, vec_bytes, hipMemcpyDeviceToDevice, c->stream));
            LAUNCH_TRY("compartment launch", c3d::launch_compartment_fit(maps, w, nv, c->stream));
        }
        if (expected) HIP_TRY(hipMemcpyAsync(hE.data() + (size_t)q0 * n, w.E, sizeof(double) * (size_t)nb * n, hipMemcpyDeviceToHost, c->stream));
        if (vectors) HIP_TRY(hipMemcpyAsync(hV.data() + (size_t)q0 * nv * n, w.V, vec_bytes * nb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hS.data() + (size_t)q0 * c3d::kCptStats, w.stats, sizeof(double) * (size_t)nb * c3d::kCptStats, hipMemcpyDeviceToHost, c->stream));
        if (int rc = read_back(c, w.flags, L.flags.bytes())) return rc;
        if (static_cast<const int*>(c->h_stage)[1]) return fail(C3D_ERR_INVALID, "c3d_compartments: dependent start vectors (a vector projected to exactly 0)");
    }
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (expected) memcpy(expected, hE.data(), sizeof(double) * hE.size());
    if (vectors) memcpy(vectors, hV.data(), sizeof(double) * hV.size());
    for (int q = 0; q < Q; ++q) {
        const double* const st = hS.data() + (size_t)q * c3d::kCptStats;
        for (int a = 0; a < nv; ++a) {
            if (share) share[(size_t)q * nv + a] = st[a];
            if (residual) residual[(size_t)q * nv + a] = st[3 + a];
            if (q >= has_if && has_if) {
                const size_t r = (size_t)(q - 1) * nv + a;
                if (same_side) same_side[r] = st[6 + a];
                for (int f = 0; f < nv && agreement; ++f) agreement[r * nv + f] = st[9 + 3 * a + f];
            }
        }
    }
    if (device_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *device_ms = ms;
    }
    return C3D_OK;
}

// ---- insulation profiles and domain boundaries (c3d_score.hip k_ins_*) ----
// c3d_insulation's one allocation: 24 n K of coordinates, the pick list, 16 n w_max per band (IF's, packed by the host; the consensus',
// written on the device), 28 Q n_win n of results (mean, score, strength, boundary) and the fit's (Q - 1) n_win doubles and 4-tuples.
// 455 beads x 20 models with IF, the consensus and windows {5, 10, 25}: 1.4 MB; 16384 x 20 with windows {8, 32, 128}: 105 MB (7.9 MB of
// coordinates, 33.6 MB a band, 30.3 MB of results) — no n x n map, which alone is 2 GiB there.
struct InsulationScratch : Carve {
    Slot<double> xyz, band_if, band_cons, mean, score, strength, fit_r;
    Slot<int32_t> pick, boundary, fit_counts;
    InsulationScratch(int n, int K, int Kp, int Q, int nw, int wmax, bool has_if, bool consensus) {
        const size_t rows = (size_t)Q * nw * n, band = (size_t)n * 2 * wmax, fits = has_if ? (size_t)(Q - 1) * nw : 0;
        xyz = take<double>(3 * (size_t)n * K);
        pick = take<int32_t>((size_t)Kp);
        band_if = take<double>(has_if ? band : 0);
        band_cons = take<double>(consensus ? band : 0);
        mean = take<double>(rows);
        score = take<double>(rows);
        strength = take<double>(rows);
        boundary = take<int32_t>(rows);
        fit_r = take<double>(fits);
        fit_counts = take<int32_t>(4 * fits);
    }
};

extern "C" int c3d_insulation(c3d_ctx* c, const double* IF, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, int flags, const int32_t* windows,
                              int n_win, double cutoff, double min_strength, int tol, double* mean, double* score, int32_t* boundary, double* strength, double* fit_r,
                              int32_t* fit_counts, double* device_ms) {
    const char* const who = "c3d_insulation";
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, who, extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size(), nw = n_win;
    if (n < 3) return fail(C3D_ERR_INVALID, "c3d_insulation: maps of fewer than 3 beads have no bead with a square (n < 3)");
    if (Kp > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, "c3d_insulation: more than 256 picks");
    if (flags & ~(C3D_INSULATION_CONSENSUS | C3D_INSULATION_CONTACT | C3D_INSULATION_STAGE)) return fail(C3D_ERR_INVALID, "c3d_insulation: unknown flag bits");
    const bool consensus = (flags & C3D_INSULATION_CONSENSUS) != 0, contact = (flags & C3D_INSULATION_CONTACT) != 0;
    if (nw < 1 || nw > C3D_INSULATION_MAX_WINDOWS || !windows) return fail(C3D_ERR_INVALID, "c3d_insulation: n_win outside 1..C3D_INSULATION_MAX_WINDOWS, or no windows");
    for (int k = 0; k < nw; ++k) {
        if (windows[k] < 1 || windows[k] > C3D_INSULATION_MAX_WINDOW) return fail(C3D_ERR_INVALID, "c3d_insulation: a window outside 1..C3D_INSULATION_MAX_WINDOW");
        if (k > 0 && windows[k] <= windows[k - 1]) return fail(C3D_ERR_INVALID, "c3d_insulation: the windows are not strictly ascending");
        if (2 * windows[k] + 1 > n) return fail(C3D_ERR_INVALID, "c3d_insulation: a window leaves no bead inside (2w + 1 > n)");
    }
    if (consensus && Kp < 1) return fail(C3D_ERR_INVALID, "c3d_insulation: the consensus of an empty list");
    if (contact && !ensemble_cutoff_ok(cutoff)) return fail(C3D_ERR_INVALID, "c3d_insulation: the contact flag needs a finite cutoff > 0");
    if (!std::isfinite(min_strength) || min_strength < 0.0) return fail(C3D_ERR_INVALID, "c3d_insulation: min_strength is not finite or < 0");
    if (tol < 0) return fail(C3D_ERR_INVALID, "c3d_insulation: tol < 0");
    if (!mean && !score && !boundary && !strength && !fit_r && !fit_counts) return fail(C3D_ERR_INVALID, "c3d_insulation: every output is NULL");
    if ((fit_r || fit_counts) && !IF) return fail(C3D_ERR_INVALID, "c3d_insulation: fit_r and fit_counts need the IF matrix");
    if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    const int wmax = windows[nw - 1], W2 = 2 * wmax, has_if = IF ? 1 : 0, Q = has_if + Kp + (consensus ? 1 : 0);
    // IF's upper band, row a the cells (a, a+1 .. a + 2 w_max), zeros beyond the matrix; what the squares read of it, 2 <= b - a, is checked here
    std::vector<double> band;
    if (has_if) {
        band.assign((size_t)n * W2, 0.0);
        for (int a = 0; a < n; ++a)
            for (int col = 0; col < W2 && a + 1 + col < n; ++col) {
                const int b = a + 1 + col;
                const double v = IF[(size_t)a * n + b];
                if (col >= 1) {
                    if (!std::isfinite(v)) return fail(C3D_ERR_INVALID, "c3d_insulation: an IF entry is not finite");
                    if (v < 0.0) return fail(C3D_ERR_INVALID, "c3d_insulation: an IF entry is negative");
                    if (v != IF[(size_t)b * n + a]) return fail(C3D_ERR_INVALID, "c3d_insulation: the IF matrix is not symmetric");
                }
                band[(size_t)a * W2 + col] = v;
            }
    }
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const InsulationScratch L(n, K, Kp, Q, nw, wmax, has_if != 0, consensus);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ev.e[k]));
    c3d::InsJob job{};
    job.n = n; job.Q = Q; job.has_if = has_if; job.n_models = Kp; job.consensus = consensus ? 1 : 0; job.contact = contact ? 1 : 0; job.nw = nw; job.wmax = wmax;
    for (int k = 0; k < nw; ++k) job.w[k] = windows[k];
    job.cutoff = cutoff;
    job.xyz = L.xyz.at(tmp.p); job.pick = L.pick.at(tmp.p); job.band_if = L.band_if.at(tmp.p); job.band_cons = L.band_cons.at(tmp.p);
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, L.xyz.at(tmp.p), extra_xyz, n_extra, "insulation launch")) return rc;
    HIP_TRY(hipMemcpyAsync(L.pick.at(tmp.p), list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    if (has_if) HIP_TRY(hipMemcpyAsync(L.band_if.at(tmp.p), band.data(), L.band_if.bytes(), hipMemcpyHostToDevice, c->stream));
    if (consensus) LAUNCH_TRY("insulation launch", c3d::launch_insulation_band(job, c->stream));
    const bool stage = wmax <= c3d::kInsStageMax && (flags & C3D_INSULATION_STAGE) != 0;
    LAUNCH_TRY("insulation launch", c3d::launch_insulation_squares(job, stage, L.mean.at(tmp.p), c->stream));
    LAUNCH_TRY("insulation launch", c3d::launch_insulation_profile(job, L.mean.at(tmp.p), L.score.at(tmp.p), L.boundary.at(tmp.p), L.strength.at(tmp.p), c->stream));
    if (has_if && Q > 1 && (fit_r || fit_counts))
        LAUNCH_TRY("insulation launch", c3d::launch_insulation_fit(job, L.score.at(tmp.p), L.boundary.at(tmp.p), L.strength.at(tmp.p), min_strength, tol,
                                                                   L.fit_r.at(tmp.p), L.fit_counts.at(tmp.p), c->stream));
    if (mean) HIP_TRY(hipMemcpyAsync(mean, L.mean.at(tmp.p), L.mean.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (score) HIP_TRY(hipMemcpyAsync(score, L.score.at(tmp.p), L.score.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (strength) HIP_TRY(hipMemcpyAsync(strength, L.strength.at(tmp.p), L.strength.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (boundary) HIP_TRY(hipMemcpyAsync(boundary, L.boundary.at(tmp.p), L.boundary.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (Q > 1 && fit_r) HIP_TRY(hipMemcpyAsync(fit_r, L.fit_r.at(tmp.p), L.fit_r.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (Q > 1 && fit_counts) HIP_TRY(hipMemcpyAsync(fit_counts, L.fit_counts.at(tmp.p), L.fit_counts.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (device_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *device_ms = ms;
    }
    return C3D_OK;
}

// ---- loop enrichment (c3d_score.hip k_loop_*) ----
// c3d_loops' one allocation: 24 n K of coordinates, the pick list, the mask (4 n), 8 n S per band (IF's, packed by the host; the
// consensus', written on the device; S = B + 4w separations, fewer where n - 1 clips them), 8 Q S of expected values; with IF the scan's
// 32 B n of ratios (only when `ratio` is asked for), 2 B n of pixel flags, 16 n of row counts and offsets and 8 max_peaks of peaks; the
// list (8 L) with its 48 Q L of `at`, and 8 Q ((2w+1)^2 + 2) of pile-ups, P2LL and `closed`.
// 455 beads x 20 models with IF and the consensus, w = 5, separations 11..200, ratio and 4096 peaks: 9.1 MB (1.5 MB of bands, 2.8 MB of
// ratios, 4.3 MB for the list); 16384 x 20 with w = 20, B = 512 and a list of 4096 pixels, no IF: 12.3 MB (7.9 MB of coordinates, 4.2 MB
// for the list and its pile-ups), 90.1 MB with the consensus band; IF alone there, dense: 77.6 MB of band, 268 MB of ratios, 16.8 MB of flags.
struct LoopScratch : Carve {
    Slot<double> xyz, band_if, band_cons, expected, ratio, at, apa, p2ll;
    Slot<int32_t> pick, mask, rows, offset, peaks, report, list, closed;
    Slot<unsigned char> cand, peak;
    LoopScratch(int n, int K, int Kp, int Q, int S, int B, int w, bool has_if, bool consensus, bool want_ratio, bool want_peaks, int max_peaks, int Lmax) {
        const size_t pixels = (size_t)B * n, side = 2 * (size_t)w + 1;
        xyz = take<double>(Kp > 0 ? 3 * (size_t)n * K : 0);
        pick = take<int32_t>((size_t)Kp);
        mask = take<int32_t>((size_t)n);
        band_if = take<double>(has_if ? (size_t)n * S : 0);
        band_cons = take<double>(consensus ? (size_t)n * S : 0);
        expected = take<double>((size_t)Q * S);
        ratio = take<double>(want_ratio ? 4 * pixels : 0);
        cand = take<unsigned char>(want_peaks ? pixels : 0);
        peak = take<unsigned char>(want_peaks ? pixels : 0);
        rows = take<int32_t>(want_peaks ? 3 * (size_t)n : 0);
        offset = take<int32_t>(want_peaks ? (size_t)n : 0);
        peaks = take<int32_t>(want_peaks ? 2 * (size_t)max_peaks : 0);
        report = take<int32_t>(C3D_LOOP_REPORT);
        list = take<int32_t>(2 * (size_t)Lmax);
        at = take<double>(6 * (size_t)Q * Lmax);
        closed = take<int32_t>(2 * (size_t)Q);
        apa = take<double>((size_t)Q * side * side);
        p2ll = take<double>((size_t)Q);
    }
};

extern "C" int c3d_loops(c3d_ctx* c, const double* IF, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, int flags, const int32_t* mask, int p, int w,
                         int min_sep, int max_sep, const double* thr, double min_obs, int merge, int corner, const int32_t* list_in, int n_list, int max_peaks,
                         double* expected, double* ratio, int32_t* peaks, int32_t* report, double* at, int32_t* closed, double* apa, double* p2ll, double* device_ms) {
    const char* const who = "c3d_loops";
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, who, extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    if (flags & ~(C3D_LOOP_CONSENSUS | C3D_LOOP_IF_ONLY)) return fail(C3D_ERR_INVALID, "c3d_loops: unknown flag bits");
    const bool consensus = (flags & C3D_LOOP_CONSENSUS) != 0, if_only = (flags & C3D_LOOP_IF_ONLY) != 0;
    if (if_only && (n_pick > 0 || consensus)) return fail(C3D_ERR_INVALID, "c3d_loops: C3D_LOOP_IF_ONLY with a pick list or the consensus");
    if (if_only) list.clear();
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size();
    if (Kp > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, "c3d_loops: more than 256 picks");
    if (!IF && Kp < 1) return fail(C3D_ERR_INVALID, "c3d_loops: neither the IF matrix nor a model (C3D_LOOP_IF_ONLY without IF)");
    if (w < 1 || w > C3D_LOOP_MAX_WINDOW) return fail(C3D_ERR_INVALID, "c3d_loops: w outside 1..C3D_LOOP_MAX_WINDOW");
    if (p < 0 || p >= w) return fail(C3D_ERR_INVALID, "c3d_loops: p outside 0..w-1");
    if (min_sep < 2 * w + 1) return fail(C3D_ERR_INVALID, "c3d_loops: min_sep < 2w + 1 (a window would touch the diagonal)");
    if (max_sep < min_sep || max_sep > n - 1) return fail(C3D_ERR_INVALID, "c3d_loops: max_sep outside min_sep..n-1");
    const int B = max_sep - min_sep + 1;
    if (B > C3D_LOOP_MAX_BAND) return fail(C3D_ERR_INVALID, "c3d_loops: more than C3D_LOOP_MAX_BAND separations (B)");
    if (merge < 0 || merge > w) return fail(C3D_ERR_INVALID, "c3d_loops: merge outside 0..w");
    if (corner < 1 || corner > w) return fail(C3D_ERR_INVALID, "c3d_loops: corner outside 1..w");
    if (!std::isfinite(min_obs) || min_obs < 0.0) return fail(C3D_ERR_INVALID, "c3d_loops: min_obs is not finite or < 0");
    if (max_peaks < 0 || max_peaks > C3D_LOOP_MAX_LIST) return fail(C3D_ERR_INVALID, "c3d_loops: max_peaks outside 0..C3D_LOOP_MAX_LIST");
    if (!expected && !ratio && !peaks && !report && !at && !closed && !apa && !p2ll) return fail(C3D_ERR_INVALID, "c3d_loops: every output is NULL");
    if ((ratio || peaks || report) && !IF) return fail(C3D_ERR_INVALID, "c3d_loops: ratio, peaks and report need the IF matrix");
    const bool want_list = at || closed || apa || p2ll;
    if (want_list && !list_in && !IF) return fail(C3D_ERR_INVALID, "c3d_loops: at, closed, apa and p2ll need a list: list_in, or the peaks of the IF matrix");
    if (list_in && (n_list < 0 || n_list > C3D_LOOP_MAX_LIST)) return fail(C3D_ERR_INVALID, "c3d_loops: n_list outside 0..C3D_LOOP_MAX_LIST");
    if (!list_in && n_list != 0) return fail(C3D_ERR_INVALID, "c3d_loops: n_list without list_in");
    const bool want_peaks = IF && (peaks || report || (want_list && !list_in));
    if (want_peaks) {
        if (!thr) return fail(C3D_ERR_INVALID, "c3d_loops: peaks without thresholds (thr is NULL)");
        for (int x = 0; x < 4; ++x)
            if (!std::isfinite(thr[x]) || thr[x] <= 0.0) return fail(C3D_ERR_INVALID, "c3d_loops: a threshold (thr) is not finite or <= 0");
    }
    for (int l = 0; list_in && l < n_list; ++l) {
        const int i = list_in[2 * l], j = list_in[2 * l + 1];
        if (i < 0 || i >= j || j > n - 1 || j - i < min_sep || j - i > max_sep)
            return fail(C3D_ERR_INVALID, "c3d_loops: a list entry is not a pair i < j <= n-1 with j - i in min_sep..max_sep");
    }
    if (Kp > 0)
        if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    const int has_if = IF ? 1 : 0, Q = has_if + Kp + (consensus ? 1 : 0);
    const int s_lo = min_sep - 2 * w, s_hi = std::min(max_sep + 2 * w, n - 1), S = s_hi - s_lo + 1;
    // IF's band, row a the cells (a, a + s_lo .. a + s_hi), zeros beyond the matrix; all of it is read (E of every separation), all of it checked
    std::vector<double> band;
    if (has_if) {
        band.assign((size_t)n * S, 0.0);
        for (int a = 0; a < n; ++a)
            for (int col = 0; col < S && a + s_lo + col < n; ++col) {
                const int b = a + s_lo + col;
                const double v = IF[(size_t)a * n + b];
                if (!std::isfinite(v)) return fail(C3D_ERR_INVALID, "c3d_loops: an IF entry is not finite");
                if (v < 0.0) return fail(C3D_ERR_INVALID, "c3d_loops: an IF entry is negative");
                if (v != IF[(size_t)b * n + a]) return fail(C3D_ERR_INVALID, "c3d_loops: the IF matrix is not symmetric");
                band[(size_t)a * S + col] = v;
            }
    }
    std::vector<int32_t> bins((size_t)n, 0);
    for (int i = 0; mask && i < n; ++i) bins[(size_t)i] = mask[i] != 0;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const int Lmax = list_in ? n_list : (want_list ? max_peaks : 0);
    const LoopScratch L(n, K, Kp, Q, S, B, w, has_if != 0, consensus, ratio != nullptr, want_peaks, max_peaks, Lmax);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ev.e[k]));
    c3d::LoopJob job{};
    job.n = n; job.Q = Q; job.has_if = has_if; job.n_models = Kp; job.consensus = consensus ? 1 : 0; job.p = p; job.w = w; job.min_sep = min_sep; job.max_sep = max_sep;
    job.s_lo = s_lo; job.S = S;
    job.xyz = L.xyz.at(tmp.p); job.pick = L.pick.at(tmp.p); job.mask = L.mask.at(tmp.p); job.band_if = L.band_if.at(tmp.p); job.band_cons = L.band_cons.at(tmp.p);
    job.expected = L.expected.at(tmp.p);
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    if (Kp > 0) {
        if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, L.xyz.at(tmp.p), extra_xyz, n_extra, "loop launch")) return rc;
        HIP_TRY(hipMemcpyAsync(L.pick.at(tmp.p), list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(L.mask.at(tmp.p), bins.data(), L.mask.bytes(), hipMemcpyHostToDevice, c->stream));
    if (has_if) HIP_TRY(hipMemcpyAsync(L.band_if.at(tmp.p), band.data(), L.band_if.bytes(), hipMemcpyHostToDevice, c->stream));
    LAUNCH_TRY("loop launch", c3d::launch_loop_expected(job, c->stream));
    int32_t rep[C3D_LOOP_REPORT] = {0, 0, 0, 0};
    if (has_if && (ratio || want_peaks)) {
        c3d::LoopPeakRule rule{};
        for (int x = 0; x < 4 && want_peaks; ++x) rule.thr[x] = thr[x];
        rule.min_obs = min_obs;
        LAUNCH_TRY("loop launch", c3d::launch_loop_scan(job, rule, ratio ? L.ratio.at(tmp.p) : nullptr, want_peaks ? L.cand.at(tmp.p) : nullptr, c->stream));
        if (want_peaks) {
            LAUNCH_TRY("loop launch", c3d::launch_loop_peaks(job, merge, max_peaks, L.cand.at(tmp.p), L.peak.at(tmp.p), L.rows.at(tmp.p), L.offset.at(tmp.p),
                                                             L.peaks.at(tmp.p), L.report.at(tmp.p), c->stream));
            // the number of written peaks sizes the list pass: the one look of the host at the device inside the call
            HIP_TRY(hipMemcpyAsync(rep, L.report.at(tmp.p), sizeof(rep), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    const int n_listed = list_in ? n_list : rep[2];
    const int32_t* d_list = list_in ? L.list.at(tmp.p) : L.peaks.at(tmp.p);
    if (want_list) {
        if (list_in && n_list > 0) HIP_TRY(hipMemcpyAsync(L.list.at(tmp.p), list_in, sizeof(int32_t) * 2 * (size_t)n_list, hipMemcpyHostToDevice, c->stream));
        if (at || closed) LAUNCH_TRY("loop launch", c3d::launch_loop_list(job, d_list, n_listed, L.at.at(tmp.p), L.closed.at(tmp.p), c->stream));
        if (apa || p2ll) LAUNCH_TRY("loop launch", c3d::launch_loop_apa(job, d_list, n_listed, corner, L.apa.at(tmp.p), L.p2ll.at(tmp.p), c->stream));
    }
    if (expected) HIP_TRY(hipMemcpyAsync(expected, L.expected.at(tmp.p), L.expected.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (ratio) HIP_TRY(hipMemcpyAsync(ratio, L.ratio.at(tmp.p), L.ratio.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (peaks && rep[2] > 0) HIP_TRY(hipMemcpyAsync(peaks, L.peaks.at(tmp.p), sizeof(int32_t) * 2 * (size_t)rep[2], hipMemcpyDeviceToHost, c->stream));
    if (at && n_listed > 0) HIP_TRY(hipMemcpyAsync(at, L.at.at(tmp.p), sizeof(double) * 6 * (size_t)Q * n_listed, hipMemcpyDeviceToHost, c->stream));
    if (closed) HIP_TRY(hipMemcpyAsync(closed, L.closed.at(tmp.p), L.closed.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (apa) HIP_TRY(hipMemcpyAsync(apa, L.apa.at(tmp.p), L.apa.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (p2ll) HIP_TRY(hipMemcpyAsync(p2ll, L.p2ll.at(tmp.p), L.p2ll.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (report) std::copy(rep, rep + C3D_LOOP_REPORT, report);
    if (device_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *device_ms = ms;
    }
    return C3D_OK;
}

// ---- entanglement: writhe, average crossing number, linking (c3d_score.hip k_ent_*) ----
// c3d_entanglement's one allocation: the models, per segment the two row sums, per model the two totals, and when a table is asked for the
// bounds and the two K x D x D tables
struct EntangleScratch : Carve {
    Slot<double> xyz, seg_writhe, seg_acn, writhe, acn, link, link_abs;
    Slot<int32_t> bounds;
    EntangleScratch(int n, int K, int D) {
        xyz = take<double>(3 * (size_t)n * K);
        seg_writhe = take<double>((size_t)(n - 1) * K);
        seg_acn = take<double>((size_t)(n - 1) * K);
        writhe = take<double>((size_t)K);
        acn = take<double>((size_t)K);
        if (D > 0) {
            bounds = take<int32_t>((size_t)D + 1);
            link = take<double>((size_t)D * D * K);
            link_abs = take<double>((size_t)D * D * K);
        }
    }
};

extern "C" int c3d_entanglement(c3d_ctx* c, const double* extra_xyz, int n_extra, int min_sep, int max_sep, const int32_t* bounds, int n_domains, double* writhe,
                                double* acn, double* seg_writhe, double* seg_acn, double* link, double* link_abs, double* device_ms) {
    const char* const who = "c3d_entanglement";
    if (int rc = model_set_check(c, who, 4, "no pair of segments that is not adjacent", extra_xyz, n_extra)) return rc;
    const int n = c->n, K = c->nrep + n_extra, S = n - 1;
    if (!writhe && !acn && !seg_writhe && !seg_acn && !link && !link_abs) return fail(C3D_ERR_INVALID, "c3d_entanglement: every output is NULL");
    if (min_sep < 2 || min_sep > S - 1) return fail(C3D_ERR_INVALID, "c3d_entanglement: min_sep outside 2..S-1 (S = n-1 segments)");
    if (max_sep < 0 || max_sep > S - 1 || (max_sep > 0 && max_sep < min_sep)) return fail(C3D_ERR_INVALID, "c3d_entanglement: max_sep is 0 (for S-1) or in min_sep..S-1");
    const bool table = link || link_abs;
    if (table) {
        if (!bounds) return fail(C3D_ERR_INVALID, "c3d_entanglement: a domain table needs bounds");
        if (n_domains < 1 || n_domains > C3D_ENTANGLE_MAX_DOMAINS) return fail(C3D_ERR_INVALID, "c3d_entanglement: n_domains outside 1..C3D_ENTANGLE_MAX_DOMAINS");
        if (bounds[0] != 0 || bounds[n_domains] != S) return fail(C3D_ERR_INVALID, "c3d_entanglement: bounds do not run from 0 to S");
        for (int p = 0; p < n_domains; ++p)
            if (bounds[p + 1] <= bounds[p]) return fail(C3D_ERR_INVALID, "c3d_entanglement: bounds are not strictly increasing");
    }
    if (int rc = model_set_coords(c, who, extra_xyz, n_extra)) return rc;
    const int D = table ? n_domains : 0, hi = max_sep == 0 ? S - 1 : max_sep;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const EntangleScratch L(n, K, D);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ev.e[k]));
    double* const d_xyz = L.xyz.at(tmp.p);
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    if (int rc = gather_models(c, ModelSource::STATE, 0, c->nrep, d_xyz, extra_xyz, n_extra, "entanglement launch")) return rc;
    if (writhe || acn || seg_writhe || seg_acn)
        LAUNCH_TRY("entanglement launch", c3d::launch_entangle_rows(d_xyz, n, K, min_sep, hi, L.seg_writhe.at(tmp.p), L.seg_acn.at(tmp.p), L.writhe.at(tmp.p),
                                                                     L.acn.at(tmp.p), c->stream));
    if (table) {
        HIP_TRY(hipMemcpyAsync(L.bounds.at(tmp.p), bounds, L.bounds.bytes(), hipMemcpyHostToDevice, c->stream));
        LAUNCH_TRY("entanglement launch", c3d::launch_entangle_table(d_xyz, n, K, min_sep, hi, L.bounds.at(tmp.p), D, L.link.at(tmp.p), L.link_abs.at(tmp.p), c->stream));
    }
    // straight into the caller's arrays, as c3d_geometry_replicas copies its per-bead ones
    if (writhe) HIP_TRY(hipMemcpyAsync(writhe, L.writhe.at(tmp.p), L.writhe.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (acn) HIP_TRY(hipMemcpyAsync(acn, L.acn.at(tmp.p), L.acn.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (seg_writhe) HIP_TRY(hipMemcpyAsync(seg_writhe, L.seg_writhe.at(tmp.p), L.seg_writhe.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (seg_acn) HIP_TRY(hipMemcpyAsync(seg_acn, L.seg_acn.at(tmp.p), L.seg_acn.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (link) HIP_TRY(hipMemcpyAsync(link, L.link.at(tmp.p), L.link.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (link_abs) HIP_TRY(hipMemcpyAsync(link_abs, L.link_abs.at(tmp.p), L.link_abs.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (device_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
        *device_ms = ms;
    }
    return C3D_OK;
}

// ---- balancing a raw contact matrix (c3d_score.hip k_bal_*) ----
// c3d_balance_matrix's one allocation: the call's copy of the matrix, n rows of pitch np = n rounded up to even (8 n np bytes; `balanced` is
// formed in place over it), then O(n): the weights (np), the marginals, the mask codes and counts, the history (max_iters + 1), the round
// record and the check's flags.  455 beads, 200 rounds: 1.67 MB; 16384 beads: 2 GiB + 0.4 MB.
struct BalanceScratch : Carve {
    Slot<double> M, w, s, history, rec;
    Slot<int> code, cnt, flags;
    BalanceScratch(int n, int np, int max_iters) {
        M = take<double>((size_t)n * np);
        w = take<double>((size_t)np);
        s = take<double>((size_t)n);
        code = take<int>((size_t)n);
        cnt = take<int>((size_t)n);
        history = take<double>((size_t)max_iters + 1);
        rec = take<double>(c3d::kBalRecord);
        flags = take<int>(1);
    }
};

extern "C" int c3d_balance_matrix(c3d_ctx* c, const double* M, int n, int method, int flags, int ignore_diags, int min_nnz, const int32_t* mask_in, const double* w0,
                                  double tol, int max_iters, double target, double* weights, int32_t* masked, double* balanced, double* history, double* report,
                                  double* device_ms) {
    const char* const who = "c3d_balance_matrix";
    if (!c) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: null context");
    if (!M) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: no matrix");
    if (n < 2) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: fewer than 2 bins (n < 2)");
    if (n > c->max_beads)
        return fail(C3D_ERR_INVALID, "c3d_balance_matrix: " + std::to_string(n) + " bins: more than max_beads = " + std::to_string(c->max_beads) +
                                         " (c3d_set_option(\"max_beads\", n) goes up to " + std::to_string(C3D_MAX_BEADS_LIMIT) + ")");
    if (method != C3D_BALANCE_ICE && method != C3D_BALANCE_VC && method != C3D_BALANCE_SQRT_VC) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: unknown method");
    if (flags & ~C3D_BALANCE_CHECK_EVERY_ROUND) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: unknown flag bits");
    if (ignore_diags < 0) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: ignore_diags < 0");
    if (!(target > 0.0) || !std::isfinite(target)) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: target is not finite or <= 0");
    if (method == C3D_BALANCE_ICE) {
        if (!(tol >= 0.0)) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: tol < 0 (or not a number)");
        if (max_iters < 0 || max_iters > C3D_BALANCE_MAX_ITERS) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: max_iters outside 0..C3D_BALANCE_MAX_ITERS");
    } else {
        if (w0) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: VC and sqrt-VC take no start weights (w0 != NULL)");
        max_iters = 1;              // VC and sqrt-VC are the loop with one update and no tolerance
        tol = 0.0;
    }
    const bool half_power = method == C3D_BALANCE_SQRT_VC;
    const int np = c3d::balance_pitch(n);
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const BalanceScratch L(n, np, max_iters);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    PassEvents ev;
    for (int k = 0; k < 2; ++k) HIP_TRY(hipEventCreate(&ev.e[k]));
    c3d::BalJob job{};
    job.n = n; job.np = np; job.ignore_diags = ignore_diags;
    job.M = L.M.at(tmp.p); job.w = L.w.at(tmp.p); job.s = L.s.at(tmp.p); job.code = L.code.at(tmp.p); job.cnt = L.cnt.at(tmp.p);
    job.rec = L.rec.at(tmp.p); job.history = L.history.at(tmp.p);
    const size_t row_bytes = sizeof(double) * (size_t)n;
    // the matrix as the caller holds it (pitch n) for the check that c3d_compartments makes of IF, then in the call's pitch
    HIP_TRY(hipMemsetAsync(L.flags.at(tmp.p), 0, L.flags.bytes(), c->stream));
    HIP_TRY(hipMemcpyAsync(job.M, M, row_bytes * n, hipMemcpyHostToDevice, c->stream));
    LAUNCH_TRY("balance launch", c3d::launch_compartment_if_check(job.M, n, L.flags.at(tmp.p), c->stream));
    if (int rc = read_back(c, L.flags.at(tmp.p), L.flags.bytes())) return rc;
    const int bad = static_cast<const int*>(c->h_stage)[0];
    if (bad & 2) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: an entry of the matrix is not finite");
    if (bad & 4) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: an entry of the matrix is negative");
    if (bad & 1) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: the matrix is not symmetric");
    if (np != n) {
        HIP_TRY(hipMemsetAsync(job.M, 0, L.M.bytes(), c->stream));
        HIP_TRY(hipMemcpy2DAsync(job.M, sizeof(double) * (size_t)np, M, row_bytes, row_bytes, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipEventRecord(ev.e[0], c->stream));
    // the mask: nnz over all columns, then the closure over the kept ones until it removes nothing
    std::vector<int32_t> code(n, 0);
    HIP_TRY(hipMemsetAsync(job.code, 0, L.code.bytes(), c->stream));
    LAUNCH_TRY("balance launch", c3d::launch_balance_count(job, c->stream));
    if (int rc = read_back(c, job.cnt, L.cnt.bytes())) return rc;
    const int need = std::max(min_nnz, 1);
    for (int i = 0; i < n; ++i) code[i] = mask_in && mask_in[i] != 0 ? 1 : static_cast<const int*>(c->h_stage)[i] < need ? 2 : 0;
    for (bool removed = true; removed;) {
        HIP_TRY(hipMemcpyAsync(job.code, code.data(), L.code.bytes(), hipMemcpyHostToDevice, c->stream));
        LAUNCH_TRY("balance launch", c3d::launch_balance_count(job, c->stream));
        if (int rc = read_back(c, job.cnt, L.cnt.bytes())) return rc;      // (synchronised: `code` may change now)
        removed = false;
        for (int i = 0; i < n; ++i)
            if (code[i] == 0 && static_cast<const int*>(c->h_stage)[i] == 0) { code[i] = 3; removed = true; }
    }
    int by[4] = {0, 0, 0, 0};
    for (int i = 0; i < n; ++i) ++by[code[i]];
    const int kept = by[0];
    if (kept < 2) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: the mask leaves fewer than 2 bins (|U| < 2)");
    std::vector<double> w(np, 0.0);
    for (int i = 0; i < n; ++i) {
        if (code[i] != 0) continue;
        if (w0 && !(w0[i] > 0.0 && std::isfinite(w0[i]))) return fail(C3D_ERR_INVALID, "c3d_balance_matrix: a start weight of a kept bin is not finite or <= 0");
        w[i] = w0 ? w0[i] : 1.0;
    }
    HIP_TRY(hipMemcpyAsync(job.w, w.data(), L.w.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(job.rec, 0, L.rec.bytes(), c->stream));
    // the rounds, kBalBatch of them (one with C3D_BALANCE_CHECK_EVERY_ROUND) between two looks at the record; rounds enqueued beyond the
    // stopping one return at once
    const int batch = (flags & C3D_BALANCE_CHECK_EVERY_ROUND) ? 1 : c3d::kBalBatch;
    double rec[c3d::kBalRecord] = {0, 0, 0, 0};
    for (int t = 0; t <= max_iters && rec[3] == 0.0;) {
        for (int k = 0; k < batch && t <= max_iters; ++k, ++t)
            LAUNCH_TRY("balance launch", c3d::launch_balance_round(job, kept, t, max_iters, tol, half_power, c->stream));
        if (int rc = read_back(c, job.rec, L.rec.bytes())) return rc;
        memcpy(rec, c->h_stage, sizeof rec);
    }
    if ((int)rec[3] == c3d::kBalDiverged) return fail(C3D_ERR_DIVERGED, "c3d_balance_matrix: a weight stopped being finite and positive in round " + std::to_string((int)rec[2]));
    if (rec[3] == 0.0) return fail(C3D_ERR_HIP, "c3d_balance_matrix: the rounds ended without a stop word");
    const int T = (int)rec[2];
    LAUNCH_TRY("balance launch", c3d::launch_balance_apply(job, target, balanced != nullptr, c->stream));
    HIP_TRY(hipEventRecord(ev.e[1], c->stream));
    // read-backs: into the call's own buffers first, so that a failure leaves the caller's untouched
    std::vector<double> hw(weights ? n : 0), hh(history ? (size_t)T + 1 : 0);
    if (weights) HIP_TRY(hipMemcpyAsync(hw.data(), job.w, row_bytes, hipMemcpyDeviceToHost, c->stream));
    if (history) HIP_TRY(hipMemcpyAsync(hh.data(), job.history, sizeof(double) * hh.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float ms = 0;
    if (device_ms) HIP_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
    if (balanced) {                  // the one output too large for a second copy: written last, when nothing can fail but this copy
        HIP_TRY(hipMemcpy2DAsync(balanced, row_bytes, job.M, sizeof(double) * (size_t)np, row_bytes, (size_t)n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (weights) memcpy(weights, hw.data(), row_bytes);
    if (history) memcpy(history, hh.data(), sizeof(double) * hh.size());
    if (masked) memcpy(masked, code.data(), sizeof(int32_t) * (size_t)n);
    if (report) {
        const double r[C3D_BALANCE_REPORT] = {(double)T, (int)rec[3] == c3d::kBalConverged ? 1.0 : 0.0, rec[0], (double)kept, (double)by[1], (double)by[2], (double)by[3], rec[1]};
        memcpy(report, r, sizeof r);
    }
    if (device_ms) *device_ms = ms;
    return C3D_OK;
}

// ---- two contact maps against one another: the stratum-adjusted coefficient (c3d_score.hip k_sim_*) ----
// c3d_map_similarity's one allocation: the call's copy of the maps (8 n_maps n^2 bytes), one half-width's smoothed bands, diagonal-major
// (8 n_maps S n), that half-width's moments and counts (48 P S) and the check's flags.
struct MapSimScratch : Carve {
    Slot<double> maps, band, moments;
    Slot<long long> counts;
    Slot<int> flags;
    MapSimScratch(int n, int n_maps, int S, int pairs) {
        maps = take<double>((size_t)n_maps * n * n);
        band = take<double>((size_t)n_maps * S * n);
        moments = take<double>((size_t)pairs * S * 3);
        counts = take<long long>((size_t)pairs * S * 3);
        flags = take<int>(1);
    }
};
// a start and an end event a half-width, destroyed when the call goes
struct MapSimEvents {
    std::vector<hipEvent_t> e;
    ~MapSimEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

extern "C" int c3d_map_similarity(c3d_ctx* c, const double* maps, int n_maps, int n, const int32_t* h, int n_h, int min_sep, int max_sep, int flags, double* scc,
                                  double* rho, double* moments, int64_t* counts, double* smoothed, double* device_ms) {
    const char* const who = "c3d_map_similarity";
    if (!c) return fail(C3D_ERR_INVALID, "c3d_map_similarity: null context");
    if (!maps) return fail(C3D_ERR_INVALID, "c3d_map_similarity: no maps");
    if (n_maps < 2 || n_maps > C3D_MAPSIM_MAX_MAPS) return fail(C3D_ERR_INVALID, "c3d_map_similarity: n_maps outside 2..C3D_MAPSIM_MAX_MAPS");
    if (n < 3) return fail(C3D_ERR_INVALID, "c3d_map_similarity: fewer than 3 bins (n < 3)");
    if (n > c->max_beads)
        return fail(C3D_ERR_INVALID, "c3d_map_similarity: " + std::to_string(n) + " bins: more than max_beads = " + std::to_string(c->max_beads) +
                                         " (c3d_set_option(\"max_beads\", n) goes up to " + std::to_string(C3D_MAX_BEADS_LIMIT) + ")");
    if (!h || n_h < 1 || n_h > C3D_MAPSIM_MAX_WIDTHS) return fail(C3D_ERR_INVALID, "c3d_map_similarity: n_h outside 1..C3D_MAPSIM_MAX_WIDTHS (or no half-widths)");
    for (int k = 0; k < n_h; ++k) {
        if (h[k] < 0 || h[k] > C3D_MAPSIM_MAX_H) return fail(C3D_ERR_INVALID, "c3d_map_similarity: a half-width outside 0..C3D_MAPSIM_MAX_H");
        if (k > 0 && h[k] <= h[k - 1]) return fail(C3D_ERR_INVALID, "c3d_map_similarity: the half-widths are not strictly ascending");
    }
    if (min_sep < 0 || min_sep > n - 1) return fail(C3D_ERR_INVALID, "c3d_map_similarity: min_sep outside 0..n-1");
    if (max_sep < 0 || max_sep > n - 1 || (max_sep > 0 && max_sep < min_sep)) return fail(C3D_ERR_INVALID, "c3d_map_similarity: max_sep is 0 (for n-1) or in min_sep..n-1");
    if (flags & ~C3D_MAPSIM_KEEP_ZEROS) return fail(C3D_ERR_INVALID, "c3d_map_similarity: unknown flag bits");
    const int lo = min_sep, hi = max_sep ? max_sep : n - 1, S = hi - lo + 1, pairs = n_maps * (n_maps - 1) / 2;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    const MapSimScratch L(n, n_maps, S, pairs);
    CallScratch tmp;
    if (int rc = tmp.alloc(L.total, who)) return rc;
    MapSimEvents ev;
    ev.e.assign(2 * (size_t)n_h, nullptr);
    for (hipEvent_t& x : ev.e) HIP_TRY(hipEventCreate(&x));
    static_assert(sizeof(long long) == sizeof(int64_t), "the device's counts are the caller's int64_t");
    double* const d_maps = L.maps.at(tmp.p);
    const size_t map_count = (size_t)n * n;
    HIP_TRY(hipMemcpyAsync(d_maps, maps, sizeof(double) * map_count * n_maps, hipMemcpyHostToDevice, c->stream));
    for (int m = 0; m < n_maps; ++m) {
        HIP_TRY(hipMemsetAsync(L.flags.at(tmp.p), 0, L.flags.bytes(), c->stream));
        LAUNCH_TRY("map similarity launch", c3d::launch_compartment_if_check(d_maps + map_count * m, n, L.flags.at(tmp.p), c->stream));
        if (int rc = read_back(c, L.flags.at(tmp.p), L.flags.bytes())) return rc;
        const int bad = static_cast<const int*>(c->h_stage)[0];
        const std::string which = "c3d_map_similarity: map " + std::to_string(m) + ": ";
        if (bad & 2) return fail(C3D_ERR_INVALID, which + "an entry of the matrix is not finite");
        if (bad & 4) return fail(C3D_ERR_INVALID, which + "an entry of the matrix is negative");
        if (bad & 1) return fail(C3D_ERR_INVALID, which + "the matrix is not symmetric");
    }
    // a half-width at a time: the bands, the strata, then the read-backs into the call's own buffers (`smoothed`, the one output too large
    // for a second copy, straight into the caller's)
    const size_t per_h = (size_t)pairs * S * 3, band_count = (size_t)n_maps * S * n;
    std::vector<double> hm(per_h * n_h);
    std::vector<int64_t> hc(per_h * n_h);
    for (int k = 0; k < n_h; ++k) {
        HIP_TRY(hipEventRecord(ev.e[2 * k], c->stream));
        LAUNCH_TRY("map similarity launch", c3d::launch_mapsim_smooth(d_maps, n, n_maps, h[k], lo, hi, L.band.at(tmp.p), c->stream));
        LAUNCH_TRY("map similarity launch", c3d::launch_mapsim_strata(L.band.at(tmp.p), n, n_maps, lo, hi, (flags & C3D_MAPSIM_KEEP_ZEROS) != 0, L.moments.at(tmp.p),
                                                                      L.counts.at(tmp.p), c->stream));
        HIP_TRY(hipEventRecord(ev.e[2 * k + 1], c->stream));
        HIP_TRY(hipMemcpyAsync(hm.data() + per_h * k, L.moments.at(tmp.p), L.moments.bytes(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(hc.data() + per_h * k, L.counts.at(tmp.p), L.counts.bytes(), hipMemcpyDeviceToHost, c->stream));
        if (smoothed) HIP_TRY(hipMemcpyAsync(smoothed + band_count * k, L.band.at(tmp.p), L.band.bytes(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    double ms = 0;
    for (int k = 0; k < n_h && device_ms; ++k) {
        float one = 0;
        HIP_TRY(hipEventElapsedTime(&one, ev.e[2 * k], ev.e[2 * k + 1]));
        ms += (double)one;
    }
    // rho, w and scc on the host, from the moments and the integers, with the header's expressions in the header's order
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < n_h && (rho || scc); ++k) {
        double* const table = scc ? scc + (size_t)k * n_maps * n_maps : nullptr;
        for (int m = 0; m < n_maps && table; ++m) table[(size_t)m * n_maps + m] = 1.0;
        for (int pr = 0; pr < pairs; ++pr) {
            double num = 0, den = 0;
            bool any = false;
            for (int s = 0; s < S; ++s) {
                const size_t at = per_h * k + ((size_t)pr * S + s) * 3;
                const double* const mo = hm.data() + at;
                const int64_t* const q = hc.data() + at;
                double r = nan;
                if (q[0] >= 3 && q[1] > 0 && q[2] > 0 && mo[1] > 0.0 && mo[2] > 0.0) {
                    const double N = (double)q[0];
                    const double w = sqrt((double)q[1] * (double)q[2]) / (((4.0 * N) * N) * N);
                    r = mo[0] / sqrt(mo[1] * mo[2]);
                    num += w * r;
                    den += w;
                    any = true;
                }
                if (rho) rho[((size_t)k * pairs + pr) * S + s] = r;
            }
            int p, q;
            c3d::mapsim_pair(pr, n_maps, &p, &q);
            if (table) table[(size_t)p * n_maps + q] = table[(size_t)q * n_maps + p] = any ? num / den : nan;
        }
    }
    if (moments) memcpy(moments, hm.data(), sizeof(double) * hm.size());
    if (counts) memcpy(counts, hc.data(), sizeof(int64_t) * hc.size());
    if (device_ms) *device_ms = ms;
    return C3D_OK;
}
