// c3d_score_superpose.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- the models of a run in one frame (c3d_superpose_replicas, c3d_rmsd_table) --------------------------------------------------------------
// Coordinate space, where k_cmp_* (c3d_score_compare.inc) work in distance space.  A model is n x 3 doubles, xyz interleaved, centred in place on its centroid
// (k_sup_centre, a fixed tree).  A fit of model a onto model b is three passes over the beads in one blocking — a workgroup takes sixteen
// models a, sixteen models b and one chunk of kSupBeads beads, stages the 32 models' coordinates of the chunk in LDS (2 x 192 rows of
// kSupRow doubles: 52 224 B, inside the 64 KB a launch gets; the seventeenth column keeps the staging stores, whose stride is a row, off one
// bank) and gives a thread one pair:
//   k_sup_cov       the pair's kSupCov sums: S = sum a_i b_i^T (9), sum |a_i|^2, sum |b_i|^2
//   k_sup_solve     one thread a pair: Horn's quaternion matrix of S by a fixed number of Jacobi sweeps (c3d_superpose.h) -> Q, mirror bit, eigenvalue
//   k_sup_residual  sum |Q a_i - b_i|^2 in the direct form (the Gram form G_a + G_b - 2 lambda cancels to 1e-6 A for near-identical models)
// The per-chunk sums go to `partial` and are added in chunk order by k_sup_block_sum.  A chunk is always kSupBeads beads, so the order of
// every sum follows from n alone — not from the number of models: extra models leave the replicas' entries their bits.  No atomics.
constexpr int kSupBeads = 64;
constexpr int kSupRow = kCmpModels + 1;
constexpr int kSupRows = 3 * kSupBeads;

// cent[k] = the centroid of model k; the model is centred on it in place
__global__ __launch_bounds__(256) void k_sup_centre(double* __restrict__ xyz, int n, double* __restrict__ cent) {
    __shared__ double red[3][256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double* x = xyz + (size_t)k * 3 * n;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int i = tid; i < n; i += 256) { s0 += x[3 * i]; s1 += x[3 * i + 1]; s2 += x[3 * i + 2]; }
    block_reduce(&red[0][0], {s0, s1, s2}, tid, RedSum());
    const double c0 = red[0][0] / (double)n, c1 = red[1][0] / (double)n, c2 = red[2][0] / (double)n;
    for (int i = tid; i < n; i += 256) { x[3 * i] -= c0; x[3 * i + 1] -= c1; x[3 * i + 2] -= c2; }
    if (tid == 0) { cent[3 * k] = c0; cent[3 * k + 1] = c1; cent[3 * k + 2] = c2; }
}

// S[3 p + comp][mdl] = coordinate comp of bead i0 + p of model k0 + mdl; 0 beyond the chunk's cnt beads and beyond model K - 1
__device__ __forceinline__ void sup_stage(double (*S)[kSupRow], const double* __restrict__ models, int k0, int K, int n, int i0, int cnt, int tid) {
    for (int q = tid; q < kCmpModels * kSupRows; q += 256) {
        const int mdl = q / kSupRows, e = q - mdl * kSupRows, k = k0 + mdl;
        S[e][mdl] = k < K && e < 3 * cnt ? models[(size_t)k * 3 * n + (size_t)3 * i0 + e] : 0.0;
    }
}

// partial[chunk][b block][thread][kSupCov]: the thread's pair is a = a0 + tid / 16, b = 16 blockIdx.y + tid % 16; the chunk is blockIdx.x
__global__ __launch_bounds__(256) void k_sup_cov(const double* __restrict__ A, int KA, int a0, const double* __restrict__ B, int KB, int n,
                                                double* __restrict__ partial) {
    __shared__ double SA[kSupRows][kSupRow], SB[kSupRows][kSupRow];
    const int tid = threadIdx.x, la = pair_row(tid), lb = pair_col(tid);
    const int i0 = blockIdx.x * kSupBeads, cnt = n - i0 < kSupBeads ? n - i0 : kSupBeads;
    sup_stage(SA, A, a0, KA, n, i0, cnt, tid);
    sup_stage(SB, B, blockIdx.y * kCmpModels, KB, n, i0, cnt, tid);
    __syncthreads();
    double s[kSupCov];
    for (int t = 0; t < kSupCov; ++t) s[t] = 0.0;
    for (int p = 0; p < cnt; ++p) {
        const double ax = SA[3 * p][la], ay = SA[3 * p + 1][la], az = SA[3 * p + 2][la];
        const double bx = SB[3 * p][lb], by = SB[3 * p + 1][lb], bz = SB[3 * p + 2][lb];
        s[0] += ax * bx; s[1] += ax * by; s[2] += ax * bz;
        s[3] += ay * bx; s[4] += ay * by; s[5] += ay * bz;
        s[6] += az * bx; s[7] += az * by; s[8] += az * bz;
        s[9] += ax * ax + ay * ay + az * az;
        s[10] += bx * bx + by * by + bz * bz;
    }
    double* out = partial + (((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 256 + tid) * kSupCov;
    for (int t = 0; t < kSupCov; ++t) out[t] = s[t];
}

// out[a][b][T] = the chunks' partial sums of the pairs of row block a0, added in chunk order (T doubles a pair)
template <int T>
__global__ __launch_bounds__(256) void k_sup_block_sum(const double* __restrict__ partial, int KA, int a0, int KB, int chunks, double* __restrict__ out) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= kCmpModels * KB) return;
    const int la = q / KB, b = q - la * KB, a = a0 + la, nbB = model_blocks(KB);
    if (a >= KA) return;
    const size_t at = ((size_t)(b / kCmpModels) * 256 + la * 16 + b % kCmpModels) * T;
    double s[T];
    for (int t = 0; t < T; ++t) s[t] = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const double* in = partial + (size_t)c * nbB * 256 * T + at;
        for (int t = 0; t < T; ++t) s[t] += in[t];
    }
    for (int t = 0; t < T; ++t) out[((size_t)a * KB + b) * T + t] = s[t];
}

// fit[pair] from cov[pair].  ident: the pair a == b + ident is a model onto itself and gets the identity (the table's diagonal: 0; the
// reference replica of a superposition: its index; none: a value no pair reaches).  fixed (or null): the handedness of model a was settled
// before — its sums change sign with it, only the proper candidate is solved, and the reflection is folded back into Q.
__global__ __launch_bounds__(256) void k_sup_solve(const double* __restrict__ cov, int KA, int KB, int ident, int mirror, const int* __restrict__ fixed,
                                                  double* __restrict__ fit, int* __restrict__ mirrored) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= KA * KB) return;
    const int a = q / KB, b = q - a * KB;
    double f[kSupFit];
    if (a == b + ident) sup_identity(f);
    else {
        double c[kSupCov];
        for (int t = 0; t < kSupCov; ++t) c[t] = cov[(size_t)q * kSupCov + t];
        const bool flip = fixed && fixed[a] != 0;
        if (flip) for (int t = 0; t < 9; ++t) c[t] = -c[t];
        sup_solve(c, mirror != 0 && !fixed, f);
        if (flip) {
            for (int t = 0; t < 9; ++t) f[t] = -f[t];
            f[9] = 1.0;
        }
    }
    for (int t = 0; t < kSupFit; ++t) fit[(size_t)q * kSupFit + t] = f[t];
    mirrored[q] = f[9] != 0.0 ? 1 : 0;
}

// partial[chunk][b block][thread] = sum over the chunk's beads of |Q a_i - b_i|^2 for the thread's pair, k_sup_cov's blocking
__global__ __launch_bounds__(256) void k_sup_residual(const double* __restrict__ A, int KA, int a0, const double* __restrict__ B, int KB, int n,
                                                     const double* __restrict__ fit, double* __restrict__ partial) {
    __shared__ double SA[kSupRows][kSupRow], SB[kSupRows][kSupRow];
    const int tid = threadIdx.x, la = pair_row(tid), lb = pair_col(tid), a = a0 + la, b = blockIdx.y * kCmpModels + lb;
    const int i0 = blockIdx.x * kSupBeads, cnt = n - i0 < kSupBeads ? n - i0 : kSupBeads;
    sup_stage(SA, A, a0, KA, n, i0, cnt, tid);
    sup_stage(SB, B, blockIdx.y * kCmpModels, KB, n, i0, cnt, tid);
    double Q[9];
    for (int t = 0; t < 9; ++t) Q[t] = a < KA && b < KB ? fit[((size_t)a * KB + b) * kSupFit + t] : 0.0;
    __syncthreads();
    double acc = 0.0;
    for (int p = 0; p < cnt; ++p) {
        const double ax = SA[3 * p][la], ay = SA[3 * p + 1][la], az = SA[3 * p + 2][la];
        const double ex = Q[0] * ax + Q[1] * ay + Q[2] * az - SB[3 * p][lb];
        const double ey = Q[3] * ax + Q[4] * ay + Q[5] * az - SB[3 * p + 1][lb];
        const double ez = Q[6] * ax + Q[7] * ay + Q[8] * az - SB[3 * p + 2][lb];
        acc += ex * ex + ey * ey + ez * ez;
    }
    partial[((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 256 + tid] = acc;
}

// fitted[k][i] = Q_k a_k,i + shift (shift: the target's centroid, or null for the origin); fit holds one entry a model
__global__ __launch_bounds__(256) void k_sup_apply(const double* __restrict__ A, int n, const double* __restrict__ fit, const double* __restrict__ shift,
                                                  double* __restrict__ fitted) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* Q = fit + (size_t)k * kSupFit;
    const double* a = A + ((size_t)k * n + i) * 3;
    double* o = fitted + ((size_t)k * n + i) * 3;
    const double ax = a[0], ay = a[1], az = a[2];
    o[0] = Q[0] * ax + Q[1] * ay + Q[2] * az + (shift ? shift[0] : 0.0);
    o[1] = Q[3] * ax + Q[4] * ay + Q[5] * az + (shift ? shift[1] : 0.0);
    o[2] = Q[6] * ax + Q[7] * ay + Q[8] * az + (shift ? shift[2] : 0.0);
}

// mean[i] = the mean over the K fitted models of bead i, rmsf[i] = sqrt(mean_k |x_k,i - mean_i|^2): one thread a bead, k in order
__global__ __launch_bounds__(256) void k_sup_mean(const double* __restrict__ fitted, int K, int n, double* __restrict__ mean, double* __restrict__ rmsf) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double m0 = 0, m1 = 0, m2 = 0;
    for (int k = 0; k < K; ++k) {
        const double* x = fitted + ((size_t)k * n + i) * 3;
        m0 += x[0]; m1 += x[1]; m2 += x[2];
    }
    m0 /= (double)K; m1 /= (double)K; m2 /= (double)K;
    double v = 0;
    for (int k = 0; k < K; ++k) {
        const double* x = fitted + ((size_t)k * n + i) * 3;
        const double d0 = x[0] - m0, d1 = x[1] - m1, d2 = x[2] - m2;
        v += d0 * d0 + d1 * d1 + d2 * d2;
    }
    mean[3 * i] = m0; mean[3 * i + 1] = m1; mean[3 * i + 2] = m2;
    rmsf[i] = sqrt(v / (double)K);
}

// dev[k] = sum_i |x_k,i - mean_i|^2, a fixed tree
__global__ __launch_bounds__(256) void k_sup_dev(const double* __restrict__ fitted, const double* __restrict__ mean, int n, double* __restrict__ dev) {
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* x = fitted + (size_t)k * 3 * n;
    double s = 0;
    for (int i = tid; i < n; i += 256) {
        const double d0 = x[3 * i] - mean[3 * i], d1 = x[3 * i + 1] - mean[3 * i + 1], d2 = x[3 * i + 2] - mean[3 * i + 2];
        s += d0 * d0 + d1 * d1 + d2 * d2;
    }
    block_reduce(red, {s}, tid, RedSum());
    if (tid == 0) dev[k] = red[0];
}

hipError_t launch_superpose_gather64(const double* X, int n, int np, int nrep, double* xyz, hipStream_t s) {
    hipLaunchKernelGGL(k_models_gather<double>, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, X, n, np, xyz);
    return hipGetLastError();
}

hipError_t launch_superpose_centre(double* xyz, int n, int K, double* cent, hipStream_t s) {
    hipLaunchKernelGGL(k_sup_centre, dim3(K), dim3(256), 0, s, xyz, n, cent);
    return hipGetLastError();
}

hipError_t launch_superpose_fit(const double* A, int KA, const double* B, int KB, int n, int ident, bool mirror, const int* fixed, double* partial,
                                double* cov, double* fit, int* mirrored, double* res, hipStream_t s) {
    const int chunks = superpose_chunks(n), nbB = model_blocks(KB);
    const dim3 sum_grid((kCmpModels * KB + 255) / 256);
    for (int a0 = 0; a0 < KA; a0 += kCmpModels) {
        hipLaunchKernelGGL(k_sup_cov, dim3(chunks, nbB), dim3(256), 0, s, A, KA, a0, B, KB, n, partial);
        hipLaunchKernelGGL(k_sup_block_sum<kSupCov>, sum_grid, dim3(256), 0, s, partial, KA, a0, KB, chunks, cov);
    }
    hipLaunchKernelGGL(k_sup_solve, dim3((KA * KB + 255) / 256), dim3(256), 0, s, cov, KA, KB, ident, mirror ? 1 : 0, fixed, fit, mirrored);
    if (res)
        for (int a0 = 0; a0 < KA; a0 += kCmpModels) {
            hipLaunchKernelGGL(k_sup_residual, dim3(chunks, nbB), dim3(256), 0, s, A, KA, a0, B, KB, n, fit, partial);
            hipLaunchKernelGGL(k_sup_block_sum<1>, sum_grid, dim3(256), 0, s, partial, KA, a0, KB, chunks, res);
        }
    return hipGetLastError();
}

hipError_t launch_superpose_apply(const double* A, int K, int n, const double* fit, const double* shift, double* fitted, hipStream_t s) {
    hipLaunchKernelGGL(k_sup_apply, dim3((n + 255) / 256, K), dim3(256), 0, s, A, n, fit, shift, fitted);
    return hipGetLastError();
}

hipError_t launch_superpose_mean(const double* fitted, int K, int n, double* mean, double* rmsf, double* dev, hipStream_t s) {
    hipLaunchKernelGGL(k_sup_mean, dim3((n + 255) / 256), dim3(256), 0, s, fitted, K, n, mean, rmsf);
    if (dev) hipLaunchKernelGGL(k_sup_dev, dim3(K), dim3(256), 0, s, fitted, mean, n, dev);
    return hipGetLastError();
}

hipError_t launch_superpose_store32(const double* fitted, int n, int npad, int nrep, float* X, hipStream_t s) {
    hipLaunchKernelGGL(k_models_scatter<float>, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, fitted, n, npad, X, (float*)nullptr);
    return hipGetLastError();
}

hipError_t launch_superpose_store64(const double* fitted, int n, int np, int nrep, double* X0, double* X1, hipStream_t s) {
    hipLaunchKernelGGL(k_models_scatter<double>, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, fitted, n, np, X0, X1);
    return hipGetLastError();
}
