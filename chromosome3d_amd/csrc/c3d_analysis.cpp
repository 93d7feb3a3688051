// c3d_analysis.cpp — host unit of libc3d.so: the output side.  What a run's models are worth and how they relate, from the coordinates
// resident on the device (kernels: c3d_score.hip): c3d_score_replicas, c3d_compare_replicas, c3d_superpose_replicas, c3d_rmsd_table,
// c3d_ensemble_map, c3d_ensemble_score and the test hooks c3d_debug_if_ranks / c3d_debug_distance_ranks.  Each call carves its device scratch out of one allocation (Carve).
#include "c3d_ctx.h"

using namespace c3d::host;

// Byte offsets into one device allocation: take() returns where a slot begins and moves on by its size rounded up to 256 bytes.  The
// three layouts below are a Carve with names for its slots.
struct Carve {
    size_t total = 0;
    size_t take(size_t bytes) { const size_t off = total; total += (bytes + 255) & ~(size_t)255; return off; }
};
// the slot at byte offset `off` of the allocation at `base`, as T
template <class T>
static T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }

// c3d_score_replicas' scratch inside d_score (byte offsets): the rank matrix (which first holds the matrix itself when the device ranks it),
// rounded coordinates, per-row sums, the two fixed histograms, the overflow flag, the replicas' bounding boxes (read by the re-run of a
// wide call only) and, when the device ranks, the sort keys, the per-row sums of squares and the asymmetry flag
struct ScoreScratch : Carve {
    size_t rank = 0, xr = 0, part = 0, hist = 0, below = 0, ovf = 0, box = 0, keys = 0, saa = 0, asym = 0;
};
static ScoreScratch score_layout(int n, int nrep, unsigned nbins, size_t key_slots) {
    ScoreScratch L;
    L.rank = L.take(sizeof(double) * (size_t)n * n);
    L.xr = L.take(sizeof(double) * 3 * (size_t)n * nrep);
    L.part = L.take(sizeof(double) * 4 * (size_t)n * nrep);
    L.hist = L.take(sizeof(unsigned) * (size_t)nbins * nrep);
    L.below = L.take(sizeof(unsigned) * (size_t)nbins * nrep);
    L.ovf = L.take(sizeof(int));
    L.box = L.take(sizeof(double) * 6 * (size_t)nrep);
    if (key_slots) {
        L.keys = L.take(sizeof(unsigned long long) * key_slots);
        L.saa = L.take(sizeof(double) * (size_t)n);
        L.asym = L.take(sizeof(int));
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
    double* const d_rank = at<double>(c->d_score, L.rank);
    unsigned long long* const d_keys = at<unsigned long long>(c->d_score, L.keys);
    HIP_TRY(hipMemcpyAsync(d_rank, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
    LAUNCH_TRY("rank key launch", c3d::launch_if_rank_keys(d_rank, n, range, d_keys, mh, slots, at<int>(c->d_score, L.asym), c->stream));
    if (int rc = read_back(c, at<int>(c->d_score, L.asym), sizeof(int))) return rc;
    *symmetric = *static_cast<const int*>(c->h_stage) == 0;
    if (!*symmetric) return C3D_OK;
    const double ma = 0.5 * (2.0 * (double)mh + 1.0);
    LAUNCH_TRY("rank sort launch", c3d::launch_if_rank_sort(d_rank, n, range, d_keys, mh, slots, ma, at<double>(c->d_score, L.saa), c->stream));
    if (int rc = read_back(c, at<double>(c->d_score, L.saa), sizeof(double) * (size_t)n)) return rc;
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
    HIP_TRY(hipMemcpyAsync(rank, at<double>(c->d_score, L.rank), sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost, c->stream));
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
    double* const d_rank = spearman ? at<double>(c->d_score, L.rank) : nullptr;
    double* const d_xr = at<double>(c->d_score, L.xr);
    double* const d_part = at<double>(c->d_score, L.part);
    int* const d_ovf = at<int>(c->d_score, L.ovf);
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
            HIP_TRY(hipMemcpyAsync(d_rank, ranks->data(), sizeof(double) * ranks->size(), hipMemcpyHostToDevice, c->stream));
        }
    }
    const double mb = 0.5 * ((double)m + 1.0);     // mean of the ranks 1..m, ties or not
    LAUNCH_TRY("score launch", c3d::launch_score(c->buf.X[c->parity], c->buf.tgt, d_rank, n, c->npad, nrep, range, c->model.min_sep, nbins, ma, mb, 0.5, d_xr,
                                                 at<unsigned>(c->d_score, L.hist), at<unsigned>(c->d_score, L.below), d_part, d_ovf, c->stream));
    // the per-row sums, and behind them the overflow flag, into the pinned stage; *overflow = a pair lay beyond the histogram of the pass
    const size_t part_bytes = sizeof(double) * 4 * (size_t)n * nrep;
    auto read_sums = [&](bool* overflow) -> int {
        if (int rc = ensure_stage(c, part_bytes + 64)) return rc;
        char* const stage = static_cast<char*>(c->h_stage);
        HIP_TRY(hipMemcpyAsync(stage, d_part, part_bytes, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(stage + part_bytes, d_ovf, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *overflow = *reinterpret_cast<const int*>(stage + part_bytes) != 0;
        return C3D_OK;
    };
    bool overflow = false;
    if (int rc = read_sums(&overflow)) return rc;
    if (overflow) {
        // A pair lies beyond the fixed histogram: the same kernels again with a histogram that holds the bounding box of the widest
        // replica's rounded coordinates (the diagonal bounds every pair distance), replicas in batches whose two histograms fit
        // C3D_SCORE_SCRATCH_BYTES.  Replicas are independent and the histogram is integer: same numbers whatever the batch, and for a
        // replica that fitted the fixed histogram the numbers of the first pass.  Up to 50 000 A, the limit of c3d_spearman_if_dist_batch:
        // a box wider than that along one axis holds such a pair for certain (the two beads at its ends) and is refused at once; a box whose
        // diagonal alone is longer may hold none (the host accepts such a model), so it gets the largest histogram and the pass decides.
        constexpr unsigned kMaxBins = 50000001u;             // distances 0 .. 50 000.000 A in thousandths
        const char* const too_far = "c3d_score_replicas: a pair distance exceeds 50000 A (the limit of device and host scoring)";
        double* const d_box = at<double>(c->d_score, L.box);
        LAUNCH_TRY("score launch", c3d::launch_score_bbox(d_xr, n, nrep, d_box, c->stream));
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
        HIP_TRY(hipMemsetAsync(d_ovf, 0, sizeof(int), c->stream));
        for (int r0 = 0; r0 < nrep; r0 += batch) {
            const int nb = std::min(batch, nrep - r0);
            LAUNCH_TRY("score launch", c3d::launch_score_wide(d_xr + (size_t)r0 * 3 * n, c->buf.tgt, d_rank, n, c->npad, nb, range, c->model.min_sep, wbins, ma, mb,
                                                              0.5, wide.p, wide.p + (size_t)wbins * batch, d_part + (size_t)r0 * n * 4, d_ovf, c->stream));
        }
        if (int rc = read_sums(&overflow)) return rc;
        if (overflow) return fail(C3D_ERR_INVALID, too_far);
        ++c->score_wide_runs;
    }
    const double* const part = static_cast<const double*>(c->h_stage);
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
struct CompareScratch : Carve {
    size_t xyz = 0, ke = 0, keys = 0, rowsum = 0, sums = 0, partial = 0, table = 0;
};
static CompareScratch compare_layout(int n, int K, size_t m, size_t slots) {
    const size_t nb = (size_t)(K + c3d::kCmpModels - 1) / c3d::kCmpModels;
    CompareScratch L;
    L.xyz = L.take(sizeof(double) * 3 * (size_t)n * K);
    L.ke = L.take(sizeof(unsigned) * m * K);
    L.keys = L.take(sizeof(unsigned long long) * slots);
    L.rowsum = L.take(sizeof(double) * (size_t)n * K);
    L.sums = L.take(sizeof(double) * (size_t)K);
    L.partial = L.take(sizeof(double) * 512 * nb * nb * (size_t)c3d::compare_table_chunks(m, K));
    L.table = L.take(sizeof(double) * 2 * (size_t)K * K);
    return L;
}
// the call's scratch: freed when `tmp` goes, whatever the exit path
static int compare_alloc(DevTmp<char>& tmp, size_t bytes, const char* who) {
    const hipError_t e = hipMalloc(&tmp.p, bytes);
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
    double* const d_xyz = at<double>(tmp.p, L.xyz);
    unsigned* const d_ke = at<unsigned>(tmp.p, L.ke);
    double* const d_rowsum = at<double>(tmp.p, L.rowsum);
    double* const d_table = at<double>(tmp.p, L.table);
    LAUNCH_TRY("compare launch", c3d::launch_compare_coords(c->buf.X[c->parity], n, c->npad, nrep, d_xyz, c->stream));
    if (n_extra > 0)
        HIP_TRY(hipMemcpyAsync(d_xyz + (size_t)3 * n * nrep, extra_xyz, sizeof(double) * 3 * (size_t)n * n_extra, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < K; ++k)
        LAUNCH_TRY("compare launch", c3d::launch_compare_ranks(d_xyz + (size_t)3 * n * k, n, at<unsigned long long>(tmp.p, L.keys), m, slots, d_ke + m * k,
                                                               d_rowsum + (size_t)n * k, c->stream));
    LAUNCH_TRY("compare launch", c3d::launch_compare_table(d_xyz, d_ke, d_rowsum, n, K, m, at<double>(tmp.p, L.sums), at<double>(tmp.p, L.partial), d_table, c->stream));
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
    double* const d_xyz = at<double>(tmp.p, L.xyz);
    hipError_t e = c3d::launch_compare_coords(c->buf.X[c->parity] + (size_t)replica * c->rep_floats, n, c->npad, 1, d_xyz, c->stream);
    if (e == hipSuccess)
        e = c3d::launch_compare_ranks(d_xyz, n, at<unsigned long long>(tmp.p, L.keys), m, slots, at<unsigned>(tmp.p, L.ke), at<double>(tmp.p, L.rowsum), c->stream);
    LAUNCH_TRY("compare launch", e);
    if (int rc = read_back(c, at<unsigned>(tmp.p, L.ke), sizeof(unsigned) * m)) return rc;
    const unsigned* const ke = static_cast<const unsigned*>(c->h_stage);
    for (size_t q = 0; q < m; ++q) rank[q] = 0.5 * (double)ke[q] + 1.0;
    return C3D_OK;
}

// ---- the models of a run in one frame (c3d_score.hip k_sup_*) ----
// the K models of a call as n x 3 doubles each on the device: the replicas' state (the fp64 state itself on a precision-64 context, else the
// floats widened), then n_extra models of the caller
static int superpose_models(c3d_ctx* c, double* d_xyz, const double* extra_xyz, int n_extra) {
    const int n = c->n, nrep = c->nrep;
    LAUNCH_TRY("superpose launch", c->precision == 64 ? c3d::launch_superpose_gather64(c->b64.X[c->parity], n, c3d::cols64(n), nrep, d_xyz, c->stream)
                                                      : c3d::launch_compare_coords(c->buf.X[c->parity], n, c->npad, nrep, d_xyz, c->stream));
    if (n_extra > 0)
        HIP_TRY(hipMemcpyAsync(d_xyz + (size_t)3 * n * nrep, extra_xyz, sizeof(double) * 3 * (size_t)n * n_extra, hipMemcpyHostToDevice, c->stream));
    return C3D_OK;
}
// byte offsets into the one allocation of a call: models (the target of a superposition is model K), centroids, per-chunk sums, the pairs'
// sums, fits and residuals, two sets of mirror bits, then (superposition only) the fitted models and the block read back in one copy
struct SuperposeScratch : Carve {
    size_t xyz = 0, cent = 0, partial = 0, cov = 0, fit = 0, res = 0, mir = 0, mir2 = 0, fitted = 0, out = 0;
};
static SuperposeScratch superpose_layout(int n, int models, int KB, size_t pairs, bool fitted, size_t out_bytes) {
    SuperposeScratch L;
    L.xyz = L.take(sizeof(double) * 3 * (size_t)n * models);
    L.cent = L.take(sizeof(double) * 3 * (size_t)models);
    L.partial = L.take(sizeof(double) * c3d::superpose_partial_doubles(n, KB));
    L.cov = L.take(sizeof(double) * c3d::kSupCov * pairs);
    L.fit = L.take(sizeof(double) * c3d::kSupFit * pairs);
    L.res = L.take(sizeof(double) * pairs);        // (c3d_rmsd_table reads res and mir, neighbours, in one copy)
    L.mir = L.take(sizeof(int) * pairs);
    L.mir2 = L.take(sizeof(int) * pairs);
    L.fitted = L.take(fitted ? sizeof(double) * 3 * (size_t)n * models : 0);
    L.out = L.take(out_bytes);
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
    double* const d_xyz = at<double>(tmp.p, L.xyz);
    double* const d_target = d_xyz + (size_t)3 * n * K;
    double* const d_cent = at<double>(tmp.p, L.cent);
    double* const d_fitted = at<double>(tmp.p, L.fitted);
    double* const d_out = at<double>(tmp.p, L.out);
    double* const d_mean = d_out + K;
    double* const d_rmsf = d_mean + 3 * (size_t)n;
    int* const d_mir = at<int>(d_out, sizeof(double) * out_doubles);     // the first pass's bits: what the caller gets, behind the doubles of the same block
    int* const d_mir2 = at<int>(tmp.p, L.mir2);
    if (int rc = superpose_models(c, d_xyz, ref_xyz, reference == -1 ? 1 : 0)) return rc;
    if (reference >= 0)
        HIP_TRY(hipMemcpyAsync(d_target, d_xyz + (size_t)3 * n * reference, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    hipError_t e = c3d::launch_superpose_centre(d_xyz, n, K + 1, d_cent, c->stream);
    if (e == hipSuccess)
        e = c3d::launch_superpose_fit(d_xyz, K, d_target, 1, n, reference >= 0 ? reference : c3d::kSupNoIdent, (flags & C3D_SUPERPOSE_MIRROR) != 0, nullptr,
                                      at<double>(tmp.p, L.partial), at<double>(tmp.p, L.cov), at<double>(tmp.p, L.fit), d_mir, d_out, c->stream);
    if (e == hipSuccess) e = c3d::launch_superpose_apply(d_xyz, K, n, at<double>(tmp.p, L.fit), iters == 0 ? d_cent + 3 * (size_t)K : nullptr, d_fitted, c->stream);
    for (int it = 0; it < iters && e == hipSuccess; ++it) {
        // the mean of the fitted models is the next target; every model gets a rotation onto it, its handedness as the first pass left it
        e = c3d::launch_superpose_mean(d_fitted, K, n, d_mean, d_rmsf, nullptr, c->stream);
        if (e != hipSuccess) break;
        HIP_TRY(hipMemcpyAsync(d_target, d_mean, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        e = c3d::launch_superpose_centre(d_target, n, 1, d_cent + 3 * (size_t)K, c->stream);
        if (e == hipSuccess)
            e = c3d::launch_superpose_fit(d_xyz, K, d_target, 1, n, c3d::kSupNoIdent, false, d_mir, at<double>(tmp.p, L.partial), at<double>(tmp.p, L.cov), at<double>(tmp.p, L.fit), d_mir2,
                                          nullptr, c->stream);
        if (e == hipSuccess) e = c3d::launch_superpose_apply(d_xyz, K, n, at<double>(tmp.p, L.fit), nullptr, d_fitted, c->stream);
    }
    // iters = 0: d_out[k] keeps the fit's residual against the target; else it becomes the squared distance from the final mean
    if (e == hipSuccess) e = c3d::launch_superpose_mean(d_fitted, K, n, d_mean, d_rmsf, iters > 0 ? d_out : nullptr, c->stream);
    LAUNCH_TRY("superpose launch", e);
    if (int rc = read_back(c, d_out, out_bytes)) return rc;
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
    double* const d_xyz = at<double>(tmp.p, L.xyz);
    if (int rc = superpose_models(c, d_xyz, extra_xyz, n_extra)) return rc;
    hipError_t e = c3d::launch_superpose_centre(d_xyz, n, K, at<double>(tmp.p, L.cent), c->stream);
    if (e == hipSuccess)
        e = c3d::launch_superpose_fit(d_xyz, K, d_xyz, K, n, 0, (flags & C3D_SUPERPOSE_MIRROR) != 0, nullptr, at<double>(tmp.p, L.partial), at<double>(tmp.p, L.cov), at<double>(tmp.p, L.fit),
                                      at<int>(tmp.p, L.mir), at<double>(tmp.p, L.res), c->stream);
    LAUNCH_TRY("superpose launch", e);
    // res and the mirror bits are neighbours in the allocation: one copy
    if (int rc = read_back(c, at<double>(tmp.p, L.res), (L.mir - L.res) + sizeof(int) * pairs)) return rc;
    const double* const h = static_cast<const double*>(c->h_stage);
    const int* const hm = reinterpret_cast<const int*>(static_cast<const char*>(c->h_stage) + (L.mir - L.res));
    for (size_t q = 0; q < pairs; ++q) {
        if (rmsd) rmsd[q] = sqrt(h[q] / (double)n);
        if (mirrored) mirrored[q] = hm[q];
    }
    ++c->rmsd_table_runs;
    return C3D_OK;
}

// ---- the ensemble's distance map (c3d_score.hip k_ens_*) ----
// byte offsets into the one allocation of a call: the models, the pick list, up to three n x n matrices (the map's outputs; the score's
// rank matrix of IF and the map it ranks next) and, for the score, the sort keys, two sets of per-row sums and the asymmetry flag
struct EnsembleScratch : Carve {
    size_t xyz = 0, pick = 0, mat[3] = {0, 0, 0}, keys = 0, rows = 0, rows2 = 0, asym = 0;
};
static EnsembleScratch ensemble_layout(int n, int K, int Kp, int matrices, size_t key_slots) {
    EnsembleScratch L;
    L.xyz = L.take(sizeof(double) * 3 * (size_t)n * K);
    L.pick = L.take(sizeof(int32_t) * (size_t)Kp);
    for (int k = 0; k < matrices; ++k) L.mat[k] = L.take(sizeof(double) * (size_t)n * n);
    if (key_slots) {
        L.keys = L.take(sizeof(unsigned long long) * key_slots);
        L.rows = L.take(sizeof(double) * (size_t)n);
        L.rows2 = L.take(sizeof(double) * (size_t)n);
        L.asym = L.take(sizeof(int));
    }
    return L;
}
// what both entries refuse before any launch; on success *list holds the Kp model indices in summation order
static int ensemble_check(const c3d_ctx* c, const char* who, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, std::vector<int32_t>* list) {
    const std::string w = std::string(who) + ": ";
    if (!c) return fail(C3D_ERR_INVALID, w + "null context");
    if (!c->have_replicas) return fail(C3D_ERR_INVALID, w + "call c3d_init_replicas first");
    if (c->n < 2) return fail(C3D_ERR_INVALID, w + "models of fewer than 2 beads have no pair");
    if (n_extra < 0 || (n_extra > 0 && !extra_xyz)) return fail(C3D_ERR_INVALID, w + "n_extra < 0, or extra models without coordinates");
    if ((long)c->nrep + n_extra > C3D_COMPARE_MAX_MODELS) return fail(C3D_ERR_INVALID, w + "more than C3D_COMPARE_MAX_MODELS models");
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

// the matrix at d_M ranked in place (launch_if_rank_keys, launch_if_rank_sort): *sum = its n row sums of (rank - ma)^2 added in index order;
// *symmetric = false, and nothing ranked, when M(i,j) != M(j,i) for a ranked pair
static int ensemble_rank(c3d_ctx* c, double* d_M, int range, void* base, const EnsembleScratch& L, size_t mh, size_t slots, double* sum, bool* symmetric) {
    const int n = c->n;
    unsigned long long* const d_keys = at<unsigned long long>(base, L.keys);
    LAUNCH_TRY("rank key launch", c3d::launch_if_rank_keys(d_M, n, range, d_keys, mh, slots, at<int>(base, L.asym), c->stream));
    if (int rc = read_back(c, at<int>(base, L.asym), sizeof(int))) return rc;
    *symmetric = *static_cast<const int*>(c->h_stage) == 0;
    if (!*symmetric) return C3D_OK;
    const double ma = 0.5 * (2.0 * (double)mh + 1.0);
    LAUNCH_TRY("rank sort launch", c3d::launch_if_rank_sort(d_M, n, range, d_keys, mh, slots, ma, at<double>(base, L.rows), c->stream));
    if (int rc = read_back(c, at<double>(base, L.rows), sizeof(double) * (size_t)n)) return rc;
    const double* const rows = static_cast<const double*>(c->h_stage);
    double s = 0;
    for (int i = 0; i < n; ++i) s += rows[i];        // fixed order: deterministic
    *sum = s;
    return C3D_OK;
}

extern "C" int c3d_ensemble_map(c3d_ctx* c, const double* extra_xyz, int n_extra, const int32_t* pick, int n_pick, double cutoff, double* mean, double* sd,
                                double* contact) {
    std::vector<int32_t> list;
    if (int rc = ensemble_check(c, "c3d_ensemble_map", extra_xyz, n_extra, pick, n_pick, &list)) return rc;
    if (!mean && !sd && !contact) return fail(C3D_ERR_INVALID, "c3d_ensemble_map: every output is NULL");
    if (contact && !ensemble_cutoff_ok(cutoff)) return fail(C3D_ERR_INVALID, "c3d_ensemble_map: the contact map needs a finite cutoff > 0");
    const int n = c->n, K = c->nrep + n_extra, Kp = (int)list.size();
    if (n_extra > 0)
        if (int rc = c3d::check_model_coords(extra_xyz, (size_t)3 * n * n_extra, "c3d_ensemble_map")) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    double* const outs[3] = {mean, sd, contact};
    const int matrices = (mean ? 1 : 0) + (sd ? 1 : 0) + (contact ? 1 : 0);
    const EnsembleScratch L = ensemble_layout(n, K, Kp, matrices, 0);
    DevTmp<char> tmp;
    if (int rc = compare_alloc(tmp, L.total, "c3d_ensemble_map")) return rc;
    double* const d_xyz = at<double>(tmp.p, L.xyz);
    int* const d_pick = at<int>(tmp.p, L.pick);
    double* d_out[3] = {nullptr, nullptr, nullptr};
    for (int k = 0, slot = 0; k < 3; ++k)
        if (outs[k]) d_out[k] = at<double>(tmp.p, L.mat[slot++]);
    if (int rc = superpose_models(c, d_xyz, extra_xyz, n_extra)) return rc;
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
    if (n_extra > 0)
        if (int rc = c3d::check_model_coords(extra_xyz, (size_t)3 * n * n_extra, "c3d_ensemble_score")) return rc;
    C3D_ENTRY(c, unit_bit(UNIT_SCORE));
    // two matrices: IF, ranked once, and the map that is ranked against it — the mean first, then the contact frequencies in the same slot
    const EnsembleScratch L = ensemble_layout(n, K, Kp, 2, slots);
    DevTmp<char> tmp;
    if (int rc = compare_alloc(tmp, L.total, "c3d_ensemble_score")) return rc;
    double* const d_xyz = at<double>(tmp.p, L.xyz);
    int* const d_pick = at<int>(tmp.p, L.pick);
    double* const d_A = at<double>(tmp.p, L.mat[0]);
    double* const d_B = at<double>(tmp.p, L.mat[1]);
    HIP_TRY(hipMemcpyAsync(d_A, IF, sizeof(double) * (size_t)n * n, hipMemcpyHostToDevice, c->stream));
    double saa = 0;
    bool symmetric = false;
    if (int rc = ensemble_rank(c, d_A, range, tmp.p, L, mh, slots, &saa, &symmetric)) return rc;
    if (!symmetric) return fail(C3D_ERR_INVALID, "c3d_ensemble_score: the matrix is not symmetric over the ranked pairs (no host ranking here)");
    if (int rc = superpose_models(c, d_xyz, extra_xyz, n_extra)) return rc;
    HIP_TRY(hipMemcpyAsync(d_pick, list.data(), sizeof(int32_t) * (size_t)Kp, hipMemcpyHostToDevice, c->stream));
    const double ma = 0.5 * (2.0 * (double)mh + 1.0);
    double* const want[2] = {rho_mean, rho_contact};
    for (int k = 0; k < 2; ++k) {
        if (!want[k]) continue;
        // the kernel and arguments of c3d_ensemble_map for this output alone: the same bits
        LAUNCH_TRY("ensemble launch", c3d::launch_ensemble_map(d_xyz, n, d_pick, Kp, k ? cutoff : 0.0, k ? nullptr : d_B, nullptr, k ? d_B : nullptr, c->stream));
        double sbb = 0;
        if (int rc = ensemble_rank(c, d_B, range, tmp.p, L, mh, slots, &sbb, &symmetric)) return rc;
        if (!symmetric) return fail(C3D_ERR_HIP, "c3d_ensemble_score: the device's map is not symmetric (cannot happen)");
        LAUNCH_TRY("ensemble launch", c3d::launch_ensemble_corr(d_A, d_B, n, range, ma, at<double>(tmp.p, L.rows2), c->stream));
        if (int rc = read_back(c, at<double>(tmp.p, L.rows2), sizeof(double) * (size_t)n)) return rc;
        const double* const rows = static_cast<const double*>(c->h_stage);
        double sab = 0;
        for (int i = 0; i < n; ++i) sab += rows[i];      // fixed order: deterministic
        *want[k] = sab / sqrt(saa * sbb);
    }
    ++c->ensemble_score_runs;
    return C3D_OK;
}
