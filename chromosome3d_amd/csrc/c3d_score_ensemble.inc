// c3d_score_ensemble.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- the ensemble's distance map (c3d_ensemble_map, c3d_ensemble_score) ---------------------------------------------------------------------
// Per bead pair, over the Kp picked models in list order: mean of d_k, population sd of d_k about that mean, share of models with
// d_k < cutoff.  A model is n x 3 doubles, xyz interleaved; d_k is cmp_dist's sum and square root, so its bits are the host's.
//
// k_ens_map: a workgroup of 256 threads owns one 64 x 64 tile of the upper triangle (tiles below the diagonal leave at once), a thread a
// 4 x 4 grid of its pairs, rows ty + 16 a and columns tx + 16 b.  Why 64: the coordinates of a tile's 64 row beads and 64 column beads are
// 3 KiB a model in fp64, so a block of kEnsModels = 16 models is 48 KiB — inside the 64 KiB a launch gets without opting in, three
// workgroups to the 160 KiB of a CU — and every staged coordinate then serves 64 pairs, which leaves the loop to the fp64 square roots;
// sixteen pairs a thread keep their sums (16 doubles), deviation sums (16 doubles) and contact counts (16 ints) in registers across the
// whole model loop.  The sd is the two-pass form: the models are walked once for the sums and counts, the mean is formed (one division),
// and they are walked again for the squared deviations — a second square root per pair and model, no cancellation.  A call that wants no
// sd walks once.  The results leave through LDS (the staging buffer, as 64 rows of 65 doubles): the tile is written to (i, j) with lanes
// along j and to (j, i) with lanes along i, rows of 512 bytes both ways.  A diagonal tile computes all of its pairs (d(i, j) and d(j, i)
// have the same bits: the differences differ in sign alone) and stores the pairs i <= j once and their mirror images from the same value.
// No atomics, one fixed order: the same coordinates give the same bits, and the matrices equal their transposes bit for bit.
constexpr int kEnsTile = 64;
constexpr int kEnsLds = kEnsModels * 2 * 3 * kEnsTile;       // doubles: 49 152 bytes; the transposed tile needs 64 x 65 of them

// the tile's values (v[a][b] of every thread) through LDS to both halves of the n x n matrix `out`
__device__ __forceinline__ void ens_store_tile(double* lds, const double (&v)[4][4], double* __restrict__ out, int n, int i0, int j0, int tid) {
    const int tx = tid & 15, ty = tid >> 4;
    const bool diag = i0 == j0;
    __syncthreads();                                         // the last readers of the staged coordinates, or of the tile before this one
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) lds[(ty + 16 * a) * (kEnsTile + 1) + tx + 16 * b] = v[a][b];
    __syncthreads();
    for (int q = tid; q < kEnsTile * kEnsTile; q += 256) {
        const int hi = q >> 6, lo = q & (kEnsTile - 1);
        // (i, j) = (i0 + hi, j0 + lo): lanes along j
        if (i0 + hi < n && j0 + lo < n && (!diag || hi <= lo)) out[(size_t)(i0 + hi) * n + (j0 + lo)] = lds[hi * (kEnsTile + 1) + lo];
        // (j, i) = (j0 + hi, i0 + lo), the value of pair (i0 + lo, j0 + hi): lanes along i
        if (j0 + hi < n && i0 + lo < n && (!diag || lo < hi)) out[(size_t)(j0 + hi) * n + (i0 + lo)] = lds[lo * (kEnsTile + 1) + hi];
    }
}

// the staged block's mc models over the thread's sixteen pairs.  First walk: acc += d, cnt += d < cutoff; second walk (acc holds the mean): dev += (d - mean)^2
template <bool SECOND>
__device__ __forceinline__ void ens_block(const double* lds, int mc, int tx, int ty, double cutoff, double (&acc)[4][4], double (&dev)[4][4], int (&cnt)[4][4]) {
    for (int m = 0; m < mc; ++m) {
        const double* R = lds + (m * 2) * 3 * kEnsTile;
        const double* Cc = R + 3 * kEnsTile;
        double rx[4], ry[4], rz[4], cx[4], cy[4], cz[4];
        for (int a = 0; a < 4; ++a) { rx[a] = R[ty + 16 * a]; ry[a] = R[kEnsTile + ty + 16 * a]; rz[a] = R[2 * kEnsTile + ty + 16 * a]; }
        for (int b = 0; b < 4; ++b) { cx[b] = Cc[tx + 16 * b]; cy[b] = Cc[kEnsTile + tx + 16 * b]; cz[b] = Cc[2 * kEnsTile + tx + 16 * b]; }
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) {
                const double d = dist3(rx[a] - cx[b], ry[a] - cy[b], rz[a] - cz[b]);
                if (!SECOND) {
                    acc[a][b] += d;
                    cnt[a][b] += d < cutoff ? 1 : 0;
                } else {
                    const double e = d - acc[a][b];
                    dev[a][b] += e * e;
                }
            }
    }
}

__global__ __launch_bounds__(256) void k_ens_map(const double* __restrict__ xyz, int n, const int* __restrict__ pick, int Kp, double cutoff,
                                                double* __restrict__ mean, double* __restrict__ sd, double* __restrict__ contact) {
    __shared__ double lds[kEnsLds];
    if (blockIdx.x < blockIdx.y) return;                    // the upper triangle of tiles: row tile blockIdx.y, column tile blockIdx.x
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.y * kEnsTile, j0 = blockIdx.x * kEnsTile;
    double sum[4][4], dev[4][4];
    int cnt[4][4];
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) { sum[a][b] = 0.0; dev[a][b] = 0.0; cnt[a][b] = 0; }
    const int passes = sd ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        for (int m0 = 0; m0 < Kp; m0 += kEnsModels) {
            const int mc = Kp - m0 < kEnsModels ? Kp - m0 : kEnsModels;
            __syncthreads();                                 // the block before this one has been read
            // lds[((m 2 + side) 3 + comp) 64 + p] = coordinate comp of bead (side ? j0 : i0) + p of model pick[m0 + m]; 0 beyond bead n - 1
            for (int q = tid; q < mc * 2 * 3 * kEnsTile; q += 256) {
                const int m = q / (6 * kEnsTile), rest = q - m * (6 * kEnsTile), side = rest / (3 * kEnsTile), e = rest - side * (3 * kEnsTile);
                const size_t g = (size_t)3 * (side ? j0 : i0) + e;
                const double v = g < (size_t)3 * n ? xyz[(size_t)pick[m0 + m] * 3 * n + g] : 0.0;
                const int p = e / 3, comp = e - 3 * p;
                lds[((m * 2 + side) * 3 + comp) * kEnsTile + p] = v;
            }
            __syncthreads();
            if (pass == 0) ens_block<false>(lds, mc, tx, ty, cutoff, sum, dev, cnt);
            else ens_block<true>(lds, mc, tx, ty, cutoff, sum, dev, cnt);
        }
        if (pass == 0)
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) sum[a][b] /= (double)Kp;
    }
    if (mean) ens_store_tile(lds, sum, mean, n, i0, j0, tid);
    if (sd) {
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) dev[a][b] = sqrt(dev[a][b] / (double)Kp);
        ens_store_tile(lds, dev, sd, n, i0, j0, tid);
    }
    if (contact) {
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) dev[a][b] = (double)cnt[a][b] / (double)Kp;
        ens_store_tile(lds, dev, contact, n, i0, j0, tid);
    }
}

hipError_t launch_ensemble_map(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact,
                               hipStream_t s) {
    const unsigned nt = (unsigned)ensemble_tiles(n);
    hipLaunchKernelGGL(k_ens_map, dim3(nt, nt), dim3(256), 0, s, xyz, n, pick, Kp, cutoff, mean, sd, contact);
    return hipGetLastError();
}

hipError_t launch_ensemble_corr(const double* A, const double* B, int n, int range, double ma, double* rows, hipStream_t s) {
    hipLaunchKernelGGL(k_row_corr, dim3(n), dim3(256), 0, s, A, B, n, range, ma, rows);
    return hipGetLastError();
}
