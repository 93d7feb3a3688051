// c3d_score_balance.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- balancing a raw contact matrix: ICE, VC and sqrt-VC (c3d_balance_matrix) ---------------------------------------------------------------
// The definitions stand in include/c3d.h; what is said here is who computes what, and in which order every sum runs.
//
// The matrix is the call's own copy, n rows of pitch np = n rounded up to even (every row 16-byte aligned, the pad column 0), and w has np
// entries (the pad entry 0).  A'(i, j) is M(i, j) where |i - j| >= ignore_diags and 0 inside the band: a predicate on the loaded value, no
// second copy.  code[i] is 0 for a kept bin (i in U) and the mask's reason otherwise.
//
//   k_bal_count      the integer twin of the marginals, one workgroup a row: cnt[i] = #{ j : A'(i, j) > 0 and code[j] == 0 }, thread t
//                    the columns t, t + 256, ..., an int block_reduce.  With code all 0 that is nnz_i; with the mask's codes it is the
//                    closure's test (a kept bin whose count is 0 has no kept partner).  The host reads cnt, forms the codes, writes them back.
//   k_bal_marginals  the hot kernel, one pass over the matrix a round.  A workgroup owns kBalRows = 4 consecutive rows; thread t takes the
//                    column pairs 2t, 2t + 1, then 2t + 512, 2t + 513, ... ascending — one 16-byte load of w and one of M a row, the
//                    pair's two products added low column first — and one block_reduce<4> closes the four rows: s_i = w_i * sum.  A
//                    masked row is not read (s_i = 0); a masked column adds 0 because its w is 0.  A tile's rows beyond n - 1 repeat
//                    its last row and are not stored.  s_i depends on n, ignore_diags, the row and w alone.
//   k_bal_update     one workgroup, thread t the bins t, t + 256, ... ascending (a masked bin adds 0.0, which changes no sum): the sum of
//                    s, mbar = sum / |U|, then the centred sum of (s_i / mbar - 1)^2, var = sum / |U| — two passes in that order, each
//                    closed by block_reduce.  Thread 0 writes the round record rec = { var, mbar, t, stop } and history[t]; unless the
//                    round stops, every thread divides its w_i by r_i (by sqrt(r_i) for sqrt-VC), and a weight that is not finite and
//                    positive afterwards turns the stop word to kBalDiverged.
//   k_bal_scale      w_i <- w_i * sqrt(target / mbar), mbar from the record
//   k_bal_apply      M(i, j) <- fl(fl(w_i w_j) M(i, j)) in place, a thread a column pair of a row: two multiplications, nothing to fuse;
//                    w_i w_j and w_j w_i are the same product, so the result is symmetric bit for bit
// Every kernel of a round reads the stop word first and returns at once when it is set: the host enqueues rounds in batches and looks at
// the record between them, and what it finds does not depend on how often it looks.  No atomics anywhere.
constexpr int kBalRows = 4;

__global__ __launch_bounds__(256) void k_bal_count(const double* __restrict__ M, int n, int np, int ignore_diags, const int* __restrict__ code,
                                                  int* __restrict__ cnt) {
    __shared__ int red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double* row = M + (size_t)i * np;
    int v[1] = {0};
    for (int j = tid; j < n; j += 256) {
        const int sep = i > j ? i - j : j - i;
        if (sep >= ignore_diags && code[j] == 0 && row[j] > 0.0) ++v[0];
    }
    block_reduce<1>(red, v, tid, RedSum());
    if (tid == 0) cnt[i] = red[0];
}

__global__ __launch_bounds__(256) void k_bal_marginals(const double* __restrict__ M, int n, int np, int ignore_diags, const double* __restrict__ w,
                                                      const int* __restrict__ code, const double* __restrict__ rec, double* __restrict__ s) {
    __shared__ double red[kBalRows * 256];
    if (rec[3] != 0.0) return;                                         // the call has stopped (uniform: every thread reads the same word)
    const int tid = threadIdx.x, i0 = blockIdx.x * kBalRows;
    const int rows = n - i0 < kBalRows ? n - i0 : kBalRows;             // >= 1: the grid has no tile beyond the last row
    const double* rowp[kBalRows];
    int ri[kBalRows];
    bool live[kBalRows];
    for (int r = 0; r < kBalRows; ++r) {
        ri[r] = i0 + (r < rows ? r : rows - 1);
        rowp[r] = M + (size_t)ri[r] * np;
        live[r] = r < rows && code[ri[r]] == 0;
    }
    double acc[kBalRows] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 2 * tid; j < np; j += 512) {                          // np even: j + 1 < np
        const double2 u = *reinterpret_cast<const double2*>(w + j);
#pragma unroll
        for (int r = 0; r < kBalRows; ++r) {
            if (!live[r]) continue;
            double2 x = *reinterpret_cast<const double2*>(rowp[r] + j);
            const int d0 = ri[r] > j ? ri[r] - j : j - ri[r], d1 = ri[r] > j + 1 ? ri[r] - j - 1 : j + 1 - ri[r];
            if (d0 < ignore_diags) x.x = 0.0;
            if (d1 < ignore_diags) x.y = 0.0;
            acc[r] += x.x * u.x;
            acc[r] += x.y * u.y;
        }
    }
    block_reduce<kBalRows>(red, acc, tid, RedSum());
    if (tid < rows) s[i0 + tid] = code[i0 + tid] == 0 ? w[i0 + tid] * red[tid * 256] : 0.0;
}

__global__ __launch_bounds__(256) void k_bal_update(int n, const int* __restrict__ code, const double* __restrict__ s, double kept, int t, int max_iters,
                                                   double tol, int half_power, double* __restrict__ w, double* __restrict__ rec,
                                                   double* __restrict__ history) {
    __shared__ double red[256];
    __shared__ int bad[256];
    if (rec[3] != 0.0) return;
    const int tid = threadIdx.x;
    double v[1] = {0.0};
    for (int i = tid; i < n; i += 256) v[0] += code[i] == 0 ? s[i] : 0.0;
    const double mbar = block_reduce<1>(red, v, tid, RedSum()) / kept;
    v[0] = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double e = s[i] / mbar - 1.0;
        v[0] += code[i] == 0 ? e * e : 0.0;
    }
    const double var = block_reduce<1>(red, v, tid, RedSum(), true) / kept;
    const int stop = var < tol ? kBalConverged : t == max_iters ? kBalExhausted : 0;
    int b[1] = {0};
    if (!stop)
        for (int i = tid; i < n; i += 256) {
            if (code[i] != 0) continue;
            const double r = s[i] / mbar;
            const double wi = w[i] / (half_power ? sqrt(r) : r);
            w[i] = wi;
            if (!(wi > 0.0 && wi <= 1.7976931348623157e308)) b[0] = 1;
        }
    block_reduce<1>(bad, b, tid, RedSum());
    if (tid == 0) {
        history[t] = var;
        rec[0] = var; rec[1] = mbar; rec[2] = (double)t;
        rec[3] = (double)(bad[0] ? kBalDiverged : stop);              // the last store: nothing of this round is read after it by this kernel
    }
}

__global__ __launch_bounds__(256) void k_bal_scale(int n, double target, const double* __restrict__ rec, double* __restrict__ w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i] = w[i] * sqrt(target / rec[1]);
}

__global__ __launch_bounds__(256) void k_bal_apply(double* __restrict__ M, int n, int np, const double* __restrict__ w) {
    const int i = blockIdx.y, j = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (j >= np) return;
    double2* const at = reinterpret_cast<double2*>(M + (size_t)i * np + j);
    const double2 u = *reinterpret_cast<const double2*>(w + j);
    const double wi = w[i];
    double2 x = *at;
    x.x = (wi * u.x) * x.x;
    x.y = (wi * u.y) * x.y;
    *at = x;
}

hipError_t launch_balance_count(const BalJob& job, hipStream_t s) {
    hipLaunchKernelGGL(k_bal_count, dim3(job.n), dim3(256), 0, s, job.M, job.n, job.np, job.ignore_diags, job.code, job.cnt);
    return hipGetLastError();
}

hipError_t launch_balance_round(const BalJob& job, int kept, int t, int max_iters, double tol, bool half_power, hipStream_t s) {
    hipLaunchKernelGGL(k_bal_marginals, dim3((job.n + kBalRows - 1) / kBalRows), dim3(256), 0, s, job.M, job.n, job.np, job.ignore_diags, job.w, job.code,
                       job.rec, job.s);
    hipLaunchKernelGGL(k_bal_update, dim3(1), dim3(256), 0, s, job.n, job.code, job.s, (double)kept, t, max_iters, tol, half_power ? 1 : 0, job.w, job.rec,
                       job.history);
    return hipGetLastError();
}

hipError_t launch_balance_apply(const BalJob& job, double target, bool matrix, hipStream_t s) {
    hipLaunchKernelGGL(k_bal_scale, dim3((job.n + 255) / 256), dim3(256), 0, s, job.n, target, job.rec, job.w);
    if (matrix) hipLaunchKernelGGL(k_bal_apply, dim3((job.np / 2 + 255) / 256, job.n), dim3(256), 0, s, job.M, job.n, job.np, job.w);
    return hipGetLastError();
}
