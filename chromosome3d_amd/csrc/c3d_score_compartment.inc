// c3d_score_compartment.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- compartment eigenvectors of IF, of a model's distance map and of the consensus map (c3d_compartments) -------------------------------------
// The leading eigenvectors of the Pearson correlation of the rows of the observed/expected map X, by orthogonal iteration.  The definitions
// stand in include/c3d.h; what is said here is who computes what, and in which order every sum runs.
//
// A map is IF (n x n doubles the caller uploaded into the map's slot of X, turned into X in place) or the mean over a pick list of the
// models' cmp_dist distances, summed in list order from 0.0 and divided by the count: k_ens_map's `mean`, bit for bit.  A single model is
// the list of one — 0.0 + d and d / 1.0 are d — so the model maps and the consensus share one expression (cpt_mean_dist).
//
//   k_cpt_if_check   one workgroup a row: M(i,j) == M(j,i), finite, >= 0, or a bit of flags[0]
//   k_cpt_expected   one workgroup a (separation s, map): thread t adds M(i, i+s) for i = t, t + 256, ... ascending, block_reduce, / (n - s)
//   k_cpt_build      one workgroup a 64 x 64 tile of the upper triangle and a map, a thread a 4 x 4 grid of its pairs as in k_ens_map: X of
//                    every pair i < j once, 1 on the diagonal, both halves stored from the one value through ens_store_tile.  In place for
//                    IF: a workgroup reads its own upper tile only, and all of it before the barrier that opens ens_store_tile.
//   k_cpt_rowstats   one workgroup a (row, map): mean, then the squared deviations about it, columns t, t + 256, ... ascending
//   k_cpt_ortho      one workgroup a map, thread t the entries t, t + 256, ... of every vector (a thread reads and writes its own entries
//                    only; what crosses threads goes through block_reduce): V <- Y of the round before (cpt_take_y), Gram-Schmidt in index
//                    order, U = D V, c_a = m . U_a
//   k_cpt_product    the hot kernel, out = X U - sub (twice a round: W = X U - c, then P = X W).  A workgroup owns kCptRows = 8 rows of
//                    one map (blockIdx.y).  n even: thread t takes the column pairs 2t, 2t + 1, then 2t + 512, 2t + 513, ... ascending —
//                    one 16-byte load of U a vector and one of X a row, the pair's two products added low column first; n odd (rows of X
//                    are then not all 16-byte aligned): the columns t, t + 256, ... with 8-byte loads.  The entries of U a thread needs
//                    are the same for the eight rows: loaded once a column step, kept in registers across the rows, so X is read once and
//                    U once per eight rows, whatever n_vec is.  8 n_vec accumulators a thread; one block_reduce<8 n_vec> closes the
//                    eight rows (48 KiB of LDS at three vectors).  A tile's rows beyond n - 1 repeat its last row and are not stored.
//   k_cpt_finish     one workgroup a map: Y of the last round, lambda = v . y, the residual, live = #{D > 0}, share; the sign rule of the
//                    largest entry for IF, and for every map of a call without IF
//   k_cpt_fit        one workgroup a map other than IF: the sign against F (IF's finished vectors), |Pearson r| of every pair of
//                    vectors (two-pass: means, then the three centred sums through one block_reduce<3>), the same-side count
// Every sum is per-thread terms in ascending index order closed by block_reduce: its order follows from n and n_vec (and the pick list)
// alone, there are no atomics, and a map's arithmetic does not depend on which other maps share its batch.
__device__ __forceinline__ double cpt_mean_dist(const double* __restrict__ xyz, int n, const int* __restrict__ pick, int cnt, int i, int j) {
    double sum = 0.0;
    for (int k = 0; k < cnt; ++k) sum += cmp_dist(xyz + (size_t)pick[k] * 3 * n, i, j);
    return sum / (double)cnt;
}
// where map b of the batch takes its entries from
struct CptSource {
    bool is_if;
    const int* pick;
    int cnt;
};
__device__ __forceinline__ CptSource cpt_source(const CptMaps& S, int b) {
    const int q = S.q0 + b, mi = q - S.has_if;
    CptSource r;
    r.is_if = S.has_if && q == 0;
    const bool single = mi < S.n_models;
    r.pick = single ? S.pick + (mi < 0 ? 0 : mi) : S.pick;
    r.cnt = single ? 1 : S.n_models;
    return r;
}

__global__ __launch_bounds__(256) void k_cpt_if_check(const double* __restrict__ M, int n, int* __restrict__ flags) {
    const int i = blockIdx.x;
    int bad = 0;
    for (int j = threadIdx.x; j < n; j += 256) {
        const double v = M[(size_t)i * n + j];
        if (v != M[(size_t)j * n + i]) bad |= 1;
        if (!(fabs(v) <= 1.7976931348623157e308)) bad |= 2;
        if (v < 0.0) bad |= 4;
    }
    if (bad) atomicOr(&flags[0], bad);
}

__global__ __launch_bounds__(256) void k_cpt_expected(CptMaps S, const double* __restrict__ X, double* __restrict__ E) {
    __shared__ double red[256];
    const int s = blockIdx.x, b = blockIdx.y, n = S.n, tid = threadIdx.x;
    const CptSource src = cpt_source(S, b);
    const double* Xb = X + (size_t)b * n * n;
    double v[1] = {0.0};
    if (s > 0)
        for (int i = tid; i < n - s; i += 256) v[0] += src.is_if ? Xb[(size_t)i * n + i + s] : cpt_mean_dist(S.xyz, n, src.pick, src.cnt, i, i + s);
    const double sum = block_reduce<1>(red, v, tid, RedSum());
    if (tid == 0) E[(size_t)b * n + s] = s > 0 ? sum / (double)(n - s) : 0.0;
}

__global__ __launch_bounds__(256) void k_cpt_build(CptMaps S, double* __restrict__ X, const double* __restrict__ E, int min_sep) {
    __shared__ double lds[kEnsTile * (kEnsTile + 1)];
    if (blockIdx.x < blockIdx.y) return;                    // the upper triangle of tiles: row tile blockIdx.y, column tile blockIdx.x
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, n = S.n, b = blockIdx.z;
    const int i0 = blockIdx.y * kEnsTile, j0 = blockIdx.x * kEnsTile;
    const CptSource src = cpt_source(S, b);
    double* Xb = X + (size_t)b * n * n;
    const double* Eb = E + (size_t)b * n;
    double v[4][4];
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty + 16 * a, j = j0 + tx + 16 * c;
            double x = 1.0;                                  // the diagonal (min_sep >= 1), and what is never stored
            if (i < j && j < n && j - i >= min_sep) {
                const double e = Eb[j - i];
                if (e != 0.0) x = (src.is_if ? Xb[(size_t)i * n + j] : cpt_mean_dist(S.xyz, n, src.pick, src.cnt, i, j)) / e;
            }
            v[a][c] = x;
        }
    ens_store_tile(lds, v, Xb, n, i0, j0, tid);
}

__global__ __launch_bounds__(256) void k_cpt_rowstats(const double* __restrict__ X, int n, double* __restrict__ m, double* __restrict__ D) {
    __shared__ double red[256];
    const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const double* row = X + ((size_t)b * n + i) * n;
    double v[1] = {0.0};
    for (int j = tid; j < n; j += 256) v[0] += row[j];
    const double mean = block_reduce<1>(red, v, tid, RedSum()) / (double)n;
    v[0] = 0.0;
    for (int j = tid; j < n; j += 256) {
        const double e = row[j] - mean;
        v[0] += e * e;
    }
    const double q = sqrt(block_reduce<1>(red, v, tid, RedSum(), true) / (double)n);
    if (tid == 0) {
        m[(size_t)b * n + i] = mean;
        D[(size_t)b * n + i] = q > 0.0 ? 1.0 / q : 0.0;
    }
}

// sum over a thread's own entries of x[j] y[j], closed by the block reduction (x, y: n doubles)
__device__ __forceinline__ double cpt_dot(double* red, const double* x, const double* y, int n, int tid) {
    double v[1] = {0.0};
    for (int j = tid; j < n; j += 256) v[0] += x[j] * y[j];
    return block_reduce<1>(red, v, tid, RedSum(), true);
}
// y_a = D (P_a - m s_a) / n with s_a = 1 . W_a, into out_a
__device__ __forceinline__ void cpt_take_y(double* red, const double* m, const double* D, const double* W, const double* P, int n, int nv, double* out, int tid) {
    for (int a = 0; a < nv; ++a) {
        double v[1] = {0.0};
        for (int j = tid; j < n; j += 256) v[0] += W[(size_t)a * n + j];
        const double s = block_reduce<1>(red, v, tid, RedSum(), true);
        for (int j = tid; j < n; j += 256) out[(size_t)a * n + j] = D[j] * (P[(size_t)a * n + j] - m[j] * s) / (double)n;
    }
}

__global__ __launch_bounds__(256) void k_cpt_ortho(CptWork w, int n, int nv, int first) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* m = w.m + (size_t)b * n;
    const double* D = w.D + (size_t)b * n;
    double* V = w.V + (size_t)b * nv * n;
    double* U = w.U + (size_t)b * nv * n;
    if (!first) cpt_take_y(red, m, D, w.W + (size_t)b * nv * n, w.P + (size_t)b * nv * n, n, nv, V, tid);
    for (int a = 0; a < nv; ++a) {
        double* Va = V + (size_t)a * n;
        for (int p = 0; p < a; ++p) {
            const double* Vp = V + (size_t)p * n;
            const double d = cpt_dot(red, Vp, Va, n, tid);
            for (int j = tid; j < n; j += 256) Va[j] -= d * Vp[j];
        }
        const double nn = cpt_dot(red, Va, Va, n, tid);
        if (!(nn > 0.0) && tid == 0) w.flags[1] = 1;        // projected to 0 (or not a number): the call is refused once the batch is through
        const double norm = sqrt(nn);
        for (int j = tid; j < n; j += 256) Va[j] /= norm;
    }
    for (int a = 0; a < nv; ++a) {
        double v[1] = {0.0};
        for (int j = tid; j < n; j += 256) {
            const double u = D[j] * V[(size_t)a * n + j];
            U[(size_t)a * n + j] = u;
            v[0] += m[j] * u;
        }
        const double c = block_reduce<1>(red, v, tid, RedSum(), true);
        if (tid == 0) w.c[(size_t)b * kCptVecs + a] = c;
    }
}

template <int NV, bool PAIRS>
__global__ __launch_bounds__(256) void k_cpt_product(const double* __restrict__ X, int n, const double* __restrict__ U, const double* __restrict__ sub,
                                                    double* __restrict__ out) {
    __shared__ double red[kCptRows * NV * 256];
    const int tid = threadIdx.x, b = blockIdx.y, i0 = blockIdx.x * kCptRows;
    const int rows = n - i0 < kCptRows ? n - i0 : kCptRows;             // >= 1: the grid has no tile beyond the last row
    const double* Ub = U + (size_t)b * NV * n;
    const double* rowp[kCptRows];
    for (int r = 0; r < kCptRows; ++r) rowp[r] = X + ((size_t)b * n + i0 + (r < rows ? r : rows - 1)) * n;
    double acc[kCptRows * NV];
    for (int q = 0; q < kCptRows * NV; ++q) acc[q] = 0.0;
    if (PAIRS) {
        for (int j = 2 * tid; j < n; j += 512) {                      // n even: j + 1 < n
            double2 u[NV];
#pragma unroll
            for (int a = 0; a < NV; ++a) u[a] = *reinterpret_cast<const double2*>(Ub + (size_t)a * n + j);
#pragma unroll
            for (int r = 0; r < kCptRows; ++r) {
                const double2 x = *reinterpret_cast<const double2*>(rowp[r] + j);
#pragma unroll
                for (int a = 0; a < NV; ++a) {
                    acc[r * NV + a] += x.x * u[a].x;
                    acc[r * NV + a] += x.y * u[a].y;
                }
            }
        }
    } else {
        for (int j = tid; j < n; j += 256) {
            double u[NV];
#pragma unroll
            for (int a = 0; a < NV; ++a) u[a] = Ub[(size_t)a * n + j];
#pragma unroll
            for (int r = 0; r < kCptRows; ++r) {
                const double x = rowp[r][j];
#pragma unroll
                for (int a = 0; a < NV; ++a) acc[r * NV + a] += x * u[a];
            }
        }
    }
    block_reduce<kCptRows * NV>(red, acc, tid, RedSum());
    if (tid < kCptRows * NV) {
        const int r = tid / NV, a = tid - r * NV;
        if (r < rows) out[((size_t)b * NV + a) * n + i0 + r] = red[tid * 256] - (sub ? sub[(size_t)b * kCptVecs + a] : 0.0);
    }
}

// the sign rule of the largest entry: the entry of largest magnitude becomes positive, the lowest index on ties
__device__ __forceinline__ void cpt_sign_largest(double* red, double* Va, int n, int tid) {
    double v[1] = {0.0};
    for (int j = tid; j < n; j += 256) v[0] = fmax(v[0], fabs(Va[j]));
    const double mx = block_reduce<1>(red, v, tid, RedMax(), true);
    v[0] = (double)n;
    for (int j = tid; j < n; j += 256)
        if (fabs(Va[j]) == mx) { v[0] = (double)j; break; }
    const double at = block_reduce<1>(red, v, tid, RedMin(), true);
    const bool flip = at < (double)n && Va[(int)at] < 0.0;             // (a vector that is not a number has no such entry)
    __syncthreads();                                                   // every thread has read the entry before its owner turns it
    if (flip)
        for (int j = tid; j < n; j += 256) Va[j] = -Va[j];
}

__global__ __launch_bounds__(256) void k_cpt_finish(CptMaps S, CptWork w, int nv) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x, n = S.n;
    const double* m = w.m + (size_t)b * n;
    const double* D = w.D + (size_t)b * n;
    double* V = w.V + (size_t)b * nv * n;
    double* Y = w.U + (size_t)b * nv * n;                              // U has been read by the round's first product: Y takes its place
    cpt_take_y(red, m, D, w.W + (size_t)b * nv * n, w.P + (size_t)b * nv * n, n, nv, Y, tid);
    double v[1] = {0.0};
    for (int j = tid; j < n; j += 256) v[0] += D[j] > 0.0 ? 1.0 : 0.0;
    const double live = block_reduce<1>(red, v, tid, RedSum(), true);
    for (int a = 0; a < nv; ++a) {
        double* Va = V + (size_t)a * n;
        const double* Ya = Y + (size_t)a * n;
        const double lam = cpt_dot(red, Va, Ya, n, tid);
        v[0] = 0.0;
        for (int j = tid; j < n; j += 256) {
            const double e = Ya[j] - lam * Va[j];
            v[0] += e * e;
        }
        const double res = sqrt(block_reduce<1>(red, v, tid, RedSum(), true));
        if (tid == 0) {
            w.stats[(size_t)b * kCptStats + a] = live > 0.0 ? lam / live : 0.0;
            w.stats[(size_t)b * kCptStats + 3 + a] = res;
        }
        if (!S.has_if || S.q0 + b == 0) cpt_sign_largest(red, Va, n, tid);
    }
}

__global__ __launch_bounds__(256) void k_cpt_fit(CptMaps S, CptWork w, int nv) {
    __shared__ double red[3 * 256];
    const int b = blockIdx.x, tid = threadIdx.x, n = S.n;
    if (S.q0 + b == 0) return;                                         // IF itself
    double* V = w.V + (size_t)b * nv * n;
    for (int a = 0; a < nv; ++a) {
        double* Va = V + (size_t)a * n;
        const double* Fa = w.F + (size_t)a * n;
        const double d = cpt_dot(red, Va, Fa, n, tid);
        if (d < 0.0) {
            for (int j = tid; j < n; j += 256) Va[j] = -Va[j];
        } else if (!(d > 0.0)) {
            cpt_sign_largest(red, Va, n, tid);
        }
        double v[1] = {0.0};
        for (int j = tid; j < n; j += 256) v[0] += Va[j] * Fa[j] > 0.0 ? 1.0 : 0.0;
        const double same = block_reduce<1>(red, v, tid, RedSum(), true);
        if (tid == 0) w.stats[(size_t)b * kCptStats + 6 + a] = same / (double)n;
    }
    for (int a = 0; a < nv; ++a)
        for (int f = 0; f < nv; ++f) {
            const double* Va = V + (size_t)a * n;
            const double* Ff = w.F + (size_t)f * n;
            double s[3] = {0.0, 0.0, 0.0};
            for (int j = tid; j < n; j += 256) { s[0] += Va[j]; s[1] += Ff[j]; }
            block_reduce<3>(red, s, tid, RedSum(), true);
            const double mv = red[0] / (double)n, mf = red[256] / (double)n;
            s[0] = s[1] = s[2] = 0.0;
            for (int j = tid; j < n; j += 256) {
                const double x = Va[j] - mv, y = Ff[j] - mf;
                s[0] += x * y; s[1] += x * x; s[2] += y * y;
            }
            block_reduce<3>(red, s, tid, RedSum(), true);
            if (tid == 0) w.stats[(size_t)b * kCptStats + 9 + 3 * a + f] = fabs(red[0] / sqrt(red[256] * red[512]));
        }
}

hipError_t launch_compartment_if_check(const double* M, int n, int* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_cpt_if_check, dim3(n), dim3(256), 0, s, M, n, flags);
    return hipGetLastError();
}

hipError_t launch_compartment_build(const CptMaps& maps, const CptWork& w, int min_sep, hipStream_t s) {
    const int n = maps.n;
    const unsigned nt = (unsigned)ensemble_tiles(n);
    hipLaunchKernelGGL(k_cpt_expected, dim3(n, maps.nb), dim3(256), 0, s, maps, w.X, w.E);
    hipLaunchKernelGGL(k_cpt_build, dim3(nt, nt, maps.nb), dim3(256), 0, s, maps, w.X, w.E, min_sep);
    hipLaunchKernelGGL(k_cpt_rowstats, dim3(n, maps.nb), dim3(256), 0, s, w.X, n, w.m, w.D);
    return hipGetLastError();
}

template <int NV>
static void cpt_launch_products(const CptMaps& maps, const CptWork& w, hipStream_t s) {
    const int n = maps.n;
    const dim3 grid((n + kCptRows - 1) / kCptRows, maps.nb);
    if (n % 2 == 0) {
        hipLaunchKernelGGL((k_cpt_product<NV, true>), grid, dim3(256), 0, s, w.X, n, w.U, w.c, w.W);
        hipLaunchKernelGGL((k_cpt_product<NV, true>), grid, dim3(256), 0, s, w.X, n, w.W, static_cast<const double*>(nullptr), w.P);
    } else {
        hipLaunchKernelGGL((k_cpt_product<NV, false>), grid, dim3(256), 0, s, w.X, n, w.U, w.c, w.W);
        hipLaunchKernelGGL((k_cpt_product<NV, false>), grid, dim3(256), 0, s, w.X, n, w.W, static_cast<const double*>(nullptr), w.P);
    }
}

hipError_t launch_compartment_round(const CptMaps& maps, const CptWork& w, int nv, bool first, hipStream_t s) {
    if (nv < 1 || nv > kCptVecs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cpt_ortho, dim3(maps.nb), dim3(256), 0, s, w, maps.n, nv, first ? 1 : 0);
    if (nv == 1) cpt_launch_products<1>(maps, w, s);
    else if (nv == 2) cpt_launch_products<2>(maps, w, s);
    else cpt_launch_products<3>(maps, w, s);
    return hipGetLastError();
}

hipError_t launch_compartment_finish(const CptMaps& maps, const CptWork& w, int nv, hipStream_t s) {
    hipLaunchKernelGGL(k_cpt_finish, dim3(maps.nb), dim3(256), 0, s, maps, w, nv);
    return hipGetLastError();
}

hipError_t launch_compartment_fit(const CptMaps& maps, const CptWork& w, int nv, hipStream_t s) {
    hipLaunchKernelGGL(k_cpt_fit, dim3(maps.nb), dim3(256), 0, s, maps, w, nv);
    return hipGetLastError();
}
