// c3d_score_compare.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- the models of a run against one another (c3d_compare_replicas) -----------------------------------------------------------------------
// c3d_model_similarity for every ordered pair of K models at once: the Spearman coefficient of the i<j distances and the RMS difference of
// those distances after scaling the first model's by the ratio of the mean distances.  A model is n x 3 doubles, xyz interleaved (a
// replica's floats widened by k_models_gather).  Per model: the keys of its m = n(n-1)/2 distances are sorted with the network that sorts
// the IF keys and every pair finds its tie group's bounds k..e, of which k + e is kept (32 bits; average rank = (k + e) / 2 + 1, centred
// rank = (k + e - (m - 1)) / 2, both exact); the same pass sums the distances per row.  Then one pass over the pairs forms both K x K
// tables: a workgroup takes sixteen models a and sixteen models b, one thread an entry, and walks its chunk of the pairs in tiles of
// kCmpPairs staged in LDS; the per-chunk sums are added in chunk order by k_cmp_table_sum.  No atomics anywhere: the same coordinates give
// the same bits.
//
// The distance is cmp_dist, which has the bits of the host's (c3d_score_core.h says how).  scale * da - db as the host rounds it, by the
// same means: the product first.
__device__ __forceinline__ double cmp_scaled_diff(double scale, double da, double db) { return cmp_rounded(scale * da) - db; }

constexpr int kCmpPairs = 64;        // pairs of a staged tile (kCmpModels models a side: c3d_internal.h)

// keys of one model's distances, row i at rank_row_offset(i, n - 1); the slots from m on get the largest key
__global__ __launch_bounds__(256) void k_cmp_keys(const double* __restrict__ x, int n, unsigned long long* __restrict__ keys, size_t m, size_t slots) {
    const int i = blockIdx.x, tid = threadIdx.x;
    unsigned long long* row = keys + rank_row_offset(i, n - 1);
    for (int j = i + 1 + tid; j < n; j += 256) row[j - i - 1] = rank_key(cmp_dist(x, i, j));
    for (size_t p = m + (size_t)i * 256 + tid; p < slots; p += (size_t)gridDim.x * 256) keys[p] = ~0ull;
}

// ke[pair] = k + e, the first and last sorted position of the pair's tie group; rowsum[i] = sum over j > i of d_ij, in a fixed order
__global__ __launch_bounds__(256) void k_cmp_ranks(const double* __restrict__ x, int n, const unsigned long long* __restrict__ keys, size_t m,
                                                  unsigned* __restrict__ ke, double* __restrict__ rowsum) {
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    unsigned* row = ke + rank_row_offset(i, n - 1);
    double s = 0;
    for (int j = i + 1 + tid; j < n; j += 256) {
        const double d = cmp_dist(x, i, j);
        const unsigned long long key = rank_key(d);
        const size_t k = rank_lower_bound(keys, 0, m, key);
        // one past the group: it is short as a rule, so gallop from k (keys[k + span / 2] is in the group) before the binary search
        size_t e = m;
        if (key != ~0ull) {
            size_t span = 1;
            while (k + span < m && keys[k + span] <= key) span <<= 1;
            e = rank_lower_bound(keys, k + (span >> 1) + 1, k + span < m ? k + span : m, key + 1);
        }
        row[j - i - 1] = (unsigned)(k + (e - 1));
        s += d;
    }
    block_reduce(red, {s}, tid, RedSum());
    if (tid == 0) rowsum[i] = red[0];
}

// sums[k] = sum of model k's distances: its n row sums, in a fixed order
__global__ __launch_bounds__(256) void k_cmp_model_sum(const double* __restrict__ rowsum, int n, double* __restrict__ sums) {
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double s = 0;
    for (int i = tid; i < n; i += 256) s += rowsum[(size_t)k * n + i];
    block_reduce(red, {s}, tid, RedSum());
    if (tid == 0) sums[k] = red[0];
}

// the row i and column j of pair p in row order
__device__ __forceinline__ void cmp_pair_of(size_t p, int n, int* i, int* j) {
    const double b = 2.0 * n - 1.0;
    int r = (int)(0.5 * (b - sqrt(b * b - 8.0 * (double)p)));
    r = r < 0 ? 0 : (r > n - 2 ? n - 2 : r);
    while (r > 0 && rank_row_offset(r, n - 1) > p) --r;
    while (r < n - 2 && rank_row_offset(r + 1, n - 1) <= p) ++r;
    *i = r;
    *j = r + 1 + (int)(p - rank_row_offset(r, n - 1));
}

// partial[chunk][a block][b block][thread] = { sum (ra - mean)(rb - mean), sum (scale_ab d_a - d_b)^2 } over the chunk's pairs, the thread's
// entry being a = 16 blockIdx.y + tid / 16, b = 16 blockIdx.z + tid % 16
__global__ __launch_bounds__(256) void k_cmp_table(const double* __restrict__ xyz, const unsigned* __restrict__ ke, const double* __restrict__ sums,
                                                  int n, int K, size_t m, size_t per_chunk, double* __restrict__ partial) {
    __shared__ double R[2][kCmpPairs][kCmpModels], D[2][kCmpPairs][kCmpModels];
    __shared__ int pi[kCmpPairs], pj[kCmpPairs];
    const int tid = threadIdx.x, la = pair_row(tid), lb = pair_col(tid);
    const int a0 = blockIdx.y * kCmpModels, b0 = blockIdx.z * kCmpModels, a = a0 + la, b = b0 + lb;
    const int sides = a0 == b0 ? 1 : 2, sb = sides - 1;
    const bool live = a < K && b < K;
    double scale = 1.0;
    if (live) { const double sa = sums[a]; if (sa > 0) scale = sums[b] / sa; }
    const double centre = (double)(m - 1);
    const size_t p_begin = (size_t)blockIdx.x * per_chunk, p_end = p_begin + per_chunk < m ? p_begin + per_chunk : m;
    double sab = 0, acc = 0;
    for (size_t p0 = p_begin; p0 < p_end; p0 += kCmpPairs) {
        const int cnt = (int)(p_end - p0 < (size_t)kCmpPairs ? p_end - p0 : (size_t)kCmpPairs);
        if (tid < cnt) cmp_pair_of(p0 + tid, n, &pi[tid], &pj[tid]);
        __syncthreads();
        for (int q = tid; q < sides * kCmpModels * kCmpPairs; q += 256) {
            const int p = q & (kCmpPairs - 1), mdl = (q / kCmpPairs) & (kCmpModels - 1), side = q / (kCmpPairs * kCmpModels);
            const int k = (side ? b0 : a0) + mdl;
            double r = 0, d = 0;
            if (k < K && p < cnt) {
                r = 0.5 * ((double)ke[(size_t)k * m + p0 + p] - centre);
                d = cmp_dist(xyz + (size_t)k * 3 * n, pi[p], pj[p]);
            }
            R[side][p][mdl] = r;
            D[side][p][mdl] = d;
        }
        __syncthreads();
        if (live)
            for (int p = 0; p < cnt; ++p) {
                sab += R[0][p][la] * R[sb][p][lb];
                const double e = cmp_scaled_diff(scale, D[0][p][la], D[sb][p][lb]);
                acc += e * e;
            }
        __syncthreads();
    }
    if (live) {
        double* out = partial + ((((size_t)blockIdx.x * gridDim.y + blockIdx.y) * gridDim.z + blockIdx.z) * 256 + tid) * 2;
        out[0] = sab;
        out[1] = acc;
    }
}

// table[a][b] = the chunks' partial sums of entry (a, b), added in chunk order
__global__ __launch_bounds__(256) void k_cmp_table_sum(const double* __restrict__ partial, int K, int chunks, double* __restrict__ table) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= K * K) return;
    const int a = q / K, b = q - a * K, nb = model_blocks(K);
    const size_t at = (((size_t)(a / kCmpModels) * nb + b / kCmpModels) * 256 + (a % kCmpModels) * 16 + b % kCmpModels) * 2;
    double sab = 0, acc = 0;
    for (int c = 0; c < chunks; ++c) {
        const double* in = partial + (size_t)c * nb * nb * 512 + at;
        sab += in[0];
        acc += in[1];
    }
    table[2 * (size_t)q] = sab;
    table[2 * (size_t)q + 1] = acc;
}

hipError_t launch_compare_coords(const float* xin, int n, int npad, int nrep, double* xyz, hipStream_t s) {
    hipLaunchKernelGGL(k_models_gather<float>, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, xin, n, npad, xyz);
    return hipGetLastError();
}

hipError_t launch_compare_ranks(const double* x, int n, unsigned long long* keys, size_t m, size_t slots, unsigned* ke, double* rowsum,
                                hipStream_t s) {
    hipLaunchKernelGGL(k_cmp_keys, dim3(n), dim3(256), 0, s, x, n, keys, m, slots);
    launch_rank_sort_network(keys, slots, s);
    hipLaunchKernelGGL(k_cmp_ranks, dim3(n), dim3(256), 0, s, x, n, keys, m, ke, rowsum);
    return hipGetLastError();
}

hipError_t launch_compare_table(const double* xyz, const unsigned* ke, const double* rowsum, int n, int K, size_t m, double* sums,
                                double* partial, double* table, hipStream_t s) {
    const int nb = model_blocks(K), chunks = compare_table_chunks(m, K);
    const size_t per_chunk = compare_chunk_pairs(m, K);
    hipLaunchKernelGGL(k_cmp_model_sum, dim3(K), dim3(256), 0, s, rowsum, n, sums);
    hipLaunchKernelGGL(k_cmp_table, dim3(chunks, nb, nb), dim3(256), 0, s, xyz, ke, sums, n, K, m, per_chunk, partial);
    hipLaunchKernelGGL(k_cmp_table_sum, dim3((K * K + 255) / 256), dim3(256), 0, s, partial, K, chunks, table);
    return hipGetLastError();
}
