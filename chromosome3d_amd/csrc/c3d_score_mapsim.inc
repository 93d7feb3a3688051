// c3d_score_mapsim.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- two contact maps against one another inside every genomic separation: HiCRep's stratum-adjusted coefficient (c3d_map_similarity) ---------
// The call's copy of the maps is n_maps matrices of n x n doubles.  For one half-width h at a time k_sim_smooth writes the band lo <= s <= hi of
// every smoothed map diagonal-major — band[m][s - lo][i] = X_m(i, i + s), i < n - s, zeros behind (the layout of the entry's `smoothed`) — and
// k_sim_stratum, one workgroup a (stratum, pair of maps), reads two contiguous rows of it.
//
// k_sim_smooth: a workgroup of 256 threads owns the tile of kSimTile x kSimTile cells (i0 + ii, j0 + jj) of one map; only tiles that meet the
// band are launched (tile row bi, tile column bi + d_first + blockIdx.y) and only cells with lo <= j - i <= hi are written.  The tile and its
// halo of h cells on every side, W = kSimTile + 2 h <= 72 rows and columns, are staged in LDS (S, what lies outside the matrix is neither
// loaded nor read); then the row sums T(r, j) = M(r, c0) + M(r, c0 + 1) + ... over the column window of j, in ascending c from the first
// term, once for every staged row r and tile column j: W x 32 sums of at most 2 h + 1 terms, shared by the up to 2 h + 1 cells (i, j) whose
// row window holds r; then X(i, j) = (T(r0, j) + T(r0 + 1, j) + ...) / (double)(rows x cols) in ascending r, one division.  These are the
// operations of include/c3d.h's definition 1 in its order, so the bits are the direct double loop's; no clipped cell is added as a zero
// (a window of -0.0 keeps its sign).  The third phase walks the tile diagonal by diagonal — a wave's lanes are 32 consecutive i of one
// separation and the next — so that the stores of a separation are contiguous in the diagonal-major band, and its reads of T, lane l at
// row r + l, column jj + l, advance by 33 doubles a lane with T's pitch of 32: all 64 banks, no conflict.  LDS: W x W + W x 32 doubles of
// the unit's dynamic array, sized by the launch from h — 16 KiB at h = 0, 24.3 KiB at h = 5, 59 904 bytes at h = 20, always under the 64 KiB a
// launch gets without opting in — so that a small halo does not hold the LDS of the largest: 6 workgroups a CU at h = 5, 2 at h = 20.  A tile reads (32 + 2h)^2 cells for
// 32^2 results: 1.3 times the band at h = 2, 1.7 at h = 5, 5 at h = 20, the halo mostly out of the caches its neighbours filled.
//
// k_sim_stratum: x_i, y_i = the two maps' X(i, i + s), i < N0 = n - s; pair i is kept unless both are 0 (or always, keep_zeros).  Thread t
// brings the pairs t + 256 k in ascending k and an unkept pair brings 0: N as an integer, sum x and sum y through one block_reduce, the
// means by one division each, then the three centred sums through one block_reduce<3>, every product rounded on its own (cmp_rounded:
// no fused form, so Cxx of a map is the same bits whichever side of the pair it stands on).  Then twice, once a map: the rank_keys of the
// kept values, the pad key for unkept pairs and beyond N0, are sorted in the dynamic LDS (str_sort, P = str_slots(N0) 64-bit keys, up to
// 128 KiB), the kept keys are the first N, every kept pair looks its doubled average rank up (str_rank2) and the squares are summed in
// int64; A = N sum a^2 - T^2.  The sort keeps no index.  Launches are grouped by P as k_str_* are (str_launch_classes); the allowance
// for more than 64 KiB is set in str_prepare_unit.  No atomics; a stratum's bytes depend on the two maps' bands and on nothing else.
constexpr int kSimTile = 32;
constexpr int kSimMaxW = kSimTile + 2 * C3D_MAPSIM_MAX_H;          // 72
inline size_t sim_smooth_lds(int h) { return sizeof(double) * (size_t)(kSimTile + 2 * h) * (size_t)(kSimTile + 2 * h + kSimTile); }
static_assert(sizeof(double) * kSimMaxW * (kSimMaxW + kSimTile) <= 64 * 1024, "the smoothing tile fits the dynamic LDS a launch gets without opting in");

__global__ __launch_bounds__(256) void k_sim_smooth(const double* __restrict__ maps, int n, int h, int lo, int hi, int d_first, double* __restrict__ band) {
    const int tid = threadIdx.x, i0 = (int)blockIdx.x * kSimTile, j0 = ((int)blockIdx.x + d_first + (int)blockIdx.y) * kSimTile;
    if (j0 >= n) return;
    const double* const M = maps + (size_t)blockIdx.z * n * n;
    double* const out = band + (size_t)blockIdx.z * (size_t)(hi - lo + 1) * n;
    const int W = kSimTile + 2 * h, rb = i0 - h, cb = j0 - h;
    double* const S = reinterpret_cast<double*>(str_lds);             // W x W: the tile and its halo
    double* const T = S + W * W;                                      // W x kSimTile: the row sums
    for (int rr = tid >> 6; rr < W; rr += 4) {                        // a wave a staged row, 64 columns a step
        const int r = rb + rr;
        if (r < 0 || r >= n) continue;
        for (int cc = tid & 63; cc < W; cc += 64) {
            const int c = cb + cc;
            if (c >= 0 && c < n) S[rr * W + cc] = M[(size_t)r * n + c];
        }
    }
    __syncthreads();
    for (int q = tid; q < W * kSimTile; q += 256) {
        const int rr = q / kSimTile, jj = q - rr * kSimTile, r = rb + rr, j = j0 + jj;
        if (r < 0 || r >= n || j >= n) continue;
        const int c0 = max(0, j - h), c1 = min(n - 1, j + h);
        const double* const row = S + rr * W;
        double t = row[c0 - cb];
        for (int c = c0 + 1; c <= c1; ++c) t += row[c - cb];
        T[rr * kSimTile + jj] = t;
    }
    __syncthreads();
    for (int q = tid; q < (2 * kSimTile - 1) * kSimTile; q += 256) {
        const int ii = q % kSimTile, jj = ii + q / kSimTile - (kSimTile - 1);
        if (jj < 0 || jj >= kSimTile) continue;
        const int i = i0 + ii, j = j0 + jj, s = j - i;
        if (i >= n || j >= n || s < lo || s > hi) continue;
        const int r0 = max(0, i - h), r1 = min(n - 1, i + h), c0 = max(0, j - h), c1 = min(n - 1, j + h);
        double x = T[(r0 - rb) * kSimTile + jj];
        for (int r = r0 + 1; r <= r1; ++r) x += T[(r - rb) * kSimTile + jj];
        out[(size_t)(s - lo) * n + i] = x / (double)((r1 - r0 + 1) * (c1 - c0 + 1));
    }
}

// sum of the squared doubled average ranks of the kept values of v: sorts their keys in t (P slots); red: 256 int64
__device__ __forceinline__ long long sim_rank_squares(const double* __restrict__ v, const double* __restrict__ x, const double* __restrict__ y, int N0, int N, int P,
                                                      bool keep_zeros, unsigned long long* __restrict__ t, long long* __restrict__ red, int tid) {
    __syncthreads();                                                    // t and red may still have readers (the map before this one)
    for (int i = tid; i < P; i += kStrThreads) t[i] = i < N0 && (keep_zeros || !(x[i] == 0.0 && y[i] == 0.0)) ? rank_key(v[i]) : ~0ull;
    __syncthreads();
    str_sort(t, P, tid);
    long long sa = 0;
    for (int i = tid; i < N0; i += kStrThreads) {
        if (!keep_zeros && x[i] == 0.0 && y[i] == 0.0) continue;
        const long long a = str_rank2(t, N, rank_key(v[i]));
        sa += a * a;
    }
    return block_reduce(red, {sa}, tid, RedSum());
}

__global__ __launch_bounds__(kStrThreads) void k_sim_stratum(const double* __restrict__ band, int n, int n_maps, int lo, int hi, int s_first, int P, int keep_zeros,
                                                             double* __restrict__ moments, long long* __restrict__ counts) {
    __shared__ double red[3 * 256];
    __shared__ long long redi[256];
    unsigned long long* const t = reinterpret_cast<unsigned long long*>(str_lds);
    const int tid = threadIdx.x, s = s_first + (int)blockIdx.x, N0 = n - s, S = hi - lo + 1;
    int p, q;
    mapsim_pair((int)blockIdx.y, n_maps, &p, &q);
    const double* const x = band + ((size_t)p * S + (s - lo)) * n;
    const double* const y = band + ((size_t)q * S + (s - lo)) * n;
    const bool keep = keep_zeros != 0;
    long long cnt = 0;
    double sx = 0.0, sy = 0.0;
    for (int i = tid; i < N0; i += kStrThreads) {
        const double a = x[i], b = y[i];
        const bool kept = keep || !(a == 0.0 && b == 0.0);
        cnt += kept ? 1 : 0;
        sx += kept ? a : 0.0;
        sy += kept ? b : 0.0;
    }
    const int N = (int)block_reduce(redi, {cnt}, tid, RedSum());
    block_reduce(red, {sx, sy}, tid, RedSum());
    const double mx = N > 0 ? red[0] / (double)N : 0.0, my = N > 0 ? red[256] / (double)N : 0.0;
    double cxy = 0.0, cxx = 0.0, cyy = 0.0;
    for (int i = tid; i < N0; i += kStrThreads) {
        const double a = x[i], b = y[i];
        const bool kept = keep || !(a == 0.0 && b == 0.0);
        const double dx = a - mx, dy = b - my;
        cxy += kept ? cmp_rounded(dx * dy) : 0.0;
        cxx += kept ? cmp_rounded(dx * dx) : 0.0;
        cyy += kept ? cmp_rounded(dy * dy) : 0.0;
    }
    block_reduce(red, {cxy, cxx, cyy}, tid, RedSum(), true);
    const size_t at = (((size_t)blockIdx.y * S) + (size_t)(s - lo)) * 3;
    if (tid == 0) { moments[at] = red[0]; moments[at + 1] = red[256]; moments[at + 2] = red[512]; }
    const long long saa = sim_rank_squares(x, x, y, N0, N, P, keep, t, redi, tid);
    const long long sbb = sim_rank_squares(y, x, y, N0, N, P, keep, t, redi, tid);
    if (tid == 0) {
        const long long Nl = N, R = Nl * (Nl + 1);
        counts[at] = Nl;
        counts[at + 1] = Nl * saa - R * R;
        counts[at + 2] = Nl * sbb - R * R;
    }
}

// band (n_maps x S x n, S = hi - lo + 1) = the smoothed maps' diagonals lo .. hi at half-width h; cleared here, so that a row's tail is 0
hipError_t launch_mapsim_smooth(const double* maps, int n, int n_maps, int h, int lo, int hi, double* band, hipStream_t s) {
    hipError_t e = hipMemsetAsync(band, 0, sizeof(double) * (size_t)n_maps * (size_t)(hi - lo + 1) * n, s);
    if (e != hipSuccess) return e;
    const int tiles = (n + kSimTile - 1) / kSimTile, d_first = lo / kSimTile, d_last = (hi + kSimTile - 1) / kSimTile;
    hipLaunchKernelGGL(k_sim_smooth, dim3(tiles, d_last - d_first + 1, n_maps), dim3(256), sim_smooth_lds(h), s, maps, n, h, lo, hi, d_first, band);
    return hipGetLastError();
}

// moments, counts (P x S x 3, P = n_maps (n_maps - 1) / 2) = { Cxy, Cxx, Cyy } and { N, A, B } of every pair of maps and stratum of the band
hipError_t launch_mapsim_strata(const double* band, int n, int n_maps, int lo, int hi, bool keep_zeros, double* moments, long long* counts, hipStream_t s) {
    const int pairs = n_maps * (n_maps - 1) / 2;
    str_launch_classes(n, lo, hi, [&](int s_first, int count, int P) {
        hipLaunchKernelGGL(k_sim_stratum, dim3(count, pairs), dim3(kStrThreads), sizeof(unsigned long long) * (size_t)P, s, band, n, n_maps, lo, hi, s_first, P,
                           keep_zeros ? 1 : 0, moments, counts);
    });
    return hipGetLastError();
}
