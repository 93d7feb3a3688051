// c3d_score_bead.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d, after c3d_score_stratified.inc
// (whose network, rank lookup and distance key it uses: str_sort, str_rank2, str_dist_key, str_slots, str_lds)
// ---- a model's fit to the data, bead by bead (c3d_bead_scores) -----------------------------------------------------------------------------
// Row i of the reference's Spearman walk (spearman_IF_pdb.pl:42-70 with r1 = i): J(i) = { j : |i - j| >= range }, N_i = max(0, i - range + 1)
// + max(0, n - i - range) partners, IF(i, j) against the "%.3f" distance of beads i, j.  Both sides are ranked inside the row and the doubled
// average ranks a_j, b_j = #{smaller} + #{not larger} + 1 are integers, so C, A, B (c3d_score_stratified.inc) are exact in 64 bits.
// The row's partners are two runs of j: 0 .. i - range and i + range .. n - 1; position p of the row is bead bead_partner(p).
// k_bead_if, one workgroup an asked bead: the N_i rank_keys of the row of IF — two contiguous pieces of one matrix row, so the loads coalesce —
// padded to P, sorted in LDS; a_j goes as uint32 into a B x n array at column j (columns outside J(i) are never read) with sum a^2 beside it.
// flags[1]: a value of an asked row is not finite; flags[3]: the ranks of a row did not add up to N (N + 1), which no input can cause.
// k_bead_model, one workgroup an (asked bead, model): the row's distance keys sorted in LDS, then ONE pass over every j != i, in which the
// distance is computed once: for j in J(i) b_j is looked up and sum a b, sum b^2 grow; for a restrained partner — a target t10 > 0 tenths
// for (i, j) and |i - j| >= min_sep, k_score_corr's rule, on both sides of i — the reference's satisfaction tally and its deviation
// (count_satisfied_tbl_rows, sum_noe_dev; chromosome3D.pl:447-485, 581-600) grow, the deviation as an integer of thousandths.  All five sums
// go through one block_reduce in int64.  flags[2]: a partner further away than 50 000 A (or not a number).  a == nullptr: no ranking, the
// tallies alone (nothing is sorted); tgt == t10 == nullptr: no tallies.
// One P a call, str_slots(n - range): the longest row (bead 0).  Rows of no or one partner write zeros and sort nothing.

// bead p of row i: the partners below i first
__device__ __forceinline__ int bead_partner(int p, int i, int range, int below) { return p < below ? p : i + range + (p - below); }

__global__ __launch_bounds__(kStrThreads) void k_bead_if(const double* __restrict__ IF, int n, int range, const int* __restrict__ beads, int P,
                                                         unsigned* __restrict__ a_out, long long* __restrict__ saa, int* __restrict__ flags) {
    __shared__ long long red[2 * 256];
    unsigned long long* const t = reinterpret_cast<unsigned long long*>(str_lds);
    const int tid = threadIdx.x, b = blockIdx.x, i = beads ? beads[b] : b;
    const int below = i - range + 1 > 0 ? i - range + 1 : 0, above = n - i - range > 0 ? n - i - range : 0, N = below + above;
    const double* const row = IF + (size_t)i * n;
    for (int p = tid; p < P; p += kStrThreads) {
        unsigned long long key = ~0ull;
        if (p < N) {
            const double v = row[bead_partner(p, i, range, below)];
            if (!(fabs(v) <= 1.7976931348623157e308)) flags[1] = 1;
            key = rank_key(v);
        }
        if (N > 1) t[p] = key;
    }
    if (N <= 1) {                                                    // (the whole workgroup: N depends on the block alone)
        if (tid == 0) saa[b] = 0;
        return;
    }
    __syncthreads();
    str_sort(t, P, tid);
    unsigned* const a_row = a_out + (size_t)b * n;
    long long sa = 0, s1 = 0;
    for (int p = tid; p < N; p += kStrThreads) {
        const int j = bead_partner(p, i, range, below);
        const long long a = str_rank2(t, N, rank_key(row[j]));
        a_row[j] = (unsigned)a;
        sa += a * a;
        s1 += a;
    }
    block_reduce(red, {sa, s1}, tid, RedSum());
    if (tid == 0) {
        saa[b] = red[0];
        if (red[256] != (long long)N * (N + 1)) flags[3] = 1;
    }
}

constexpr int kBeadSums = 5;             // sum a b, sum b^2, restrained partners, net satisfied, deviation in thousandths

__global__ __launch_bounds__(kStrThreads) void k_bead_model(const double* __restrict__ xyz, int n, int range, const int* __restrict__ beads, int nb, int P,
                                                            const unsigned* __restrict__ a_in, const long long* __restrict__ saa,
                                                            const float* __restrict__ tgt, int npad, const int* __restrict__ t10, int min_sep,
                                                            long long* __restrict__ sums, int* __restrict__ restrained, int* __restrict__ satisfied,
                                                            long long* __restrict__ dev_milli, int* __restrict__ flags) {
    __shared__ long long red[kBeadSums * 256];
    unsigned* const t = reinterpret_cast<unsigned*>(str_lds);
    const int tid = threadIdx.x, b = blockIdx.x, k = blockIdx.y, i = beads ? beads[b] : b;
    const int below = i - range + 1 > 0 ? i - range + 1 : 0, above = n - i - range > 0 ? n - i - range : 0, N = below + above;
    const double* x = xyz + (size_t)k * 3 * n;
    const bool ranked = a_in && N > 1, tallied = tgt || t10;
    bool far = false;
    if (ranked) {
        for (int p = tid; p < P; p += kStrThreads) t[p] = p < N ? str_dist_key(x, i, bead_partner(p, i, range, below), &far) : kStrPad32;
        __syncthreads();
        str_sort(t, P, tid);
    }
    const unsigned* const a_row = ranked ? a_in + (size_t)b * n : nullptr;
    long long sab = 0, sbb = 0, cnt = 0, sat = 0, dev = 0;
    for (int j = tid; j < n; j += kStrThreads) {
        const int sep = i > j ? i - j : j - i;
        if (sep == 0) continue;
        const unsigned q = str_dist_key(x, i, j, &far);
        if (ranked && sep >= range) {
            const long long r = str_rank2(t, N, q);
            sab += (long long)a_row[j] * r;
            sbb += r * r;
        }
        if (tallied && sep >= min_sep) {
            // the target in tenths: the float matrix holds t10 / 10 (lrintf undoes it, as k_score_corr reads it), the fp64 context's the integer
            const long long t10v = tgt ? (long long)lrintf(tgt[(size_t)i * npad + j] * 10.0f) : (long long)t10[(size_t)i * n + j];
            if (t10v > 0) {
                const double d = (double)q / 1000.0, tv = (double)t10v / 10.0;
                ++cnt;
                if (d < tv + 0.5) ++sat;
                if (d < tv - 0.5) --sat;
                if (d > tv + 0.2) dev += (long long)q - 100 * t10v;
                if (d < tv - 0.2) dev += 100 * t10v - (long long)q;
            }
        }
    }
    if (far) flags[2] = 1;
    block_reduce(red, {sab, sbb, cnt, sat, dev}, tid, RedSum());
    if (tid == 0) {
        const size_t at = (size_t)k * nb + b;
        if (a_in) {
            const long long Nl = N, T = Nl * (Nl + 1);
            long long* const out = sums + at * C3D_BEAD_FIELDS;
            out[0] = ranked ? Nl * red[0] - T * T : 0;
            out[1] = ranked ? Nl * saa[b] - T * T : 0;
            out[2] = ranked ? Nl * red[256] - T * T : 0;
        }
        if (tallied) {
            if (k == 0) restrained[b] = (int)red[2 * 256];
            satisfied[at] = (int)red[3 * 256];
            dev_milli[at] = red[4 * 256];
        }
    }
}

hipError_t launch_bead_if(const double* IF, int n, int range, const int* beads, int nb, unsigned* a, long long* saa, int* flags, hipStream_t s) {
    const int P = str_slots(n - range);
    hipLaunchKernelGGL(k_bead_if, dim3(nb), dim3(kStrThreads), sizeof(unsigned long long) * (size_t)P, s, IF, n, range, beads, P, a, saa, flags);
    return hipGetLastError();
}

hipError_t launch_bead_models(const double* xyz, int n, int K, int range, const int* beads, int nb, const unsigned* a, const long long* saa, const float* tgt,
                              int npad, const int* t10, int min_sep, long long* sums, int* restrained, int* satisfied, long long* dev_milli, int* flags,
                              hipStream_t s) {
    const int P = str_slots(n - range);
    hipLaunchKernelGGL(k_bead_model, dim3(nb, K), dim3(kStrThreads), a ? sizeof(unsigned) * (size_t)P : 0, s, xyz, n, range, beads, nb, P, a, saa, tgt, npad, t10,
                       min_sep, sums, restrained, satisfied, dev_milli, flags);
    return hipGetLastError();
}

// the dynamic LDS of the longest row a context accepts (16384 keys), beside the stratified kernels' (preload_score_unit)
static hipError_t bead_prepare_unit() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bead_if), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned long long) * 16384));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_bead_model), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned) * 16384));
    return e;
}
