// c3d_score_insulation.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- insulation profiles and domain boundaries of IF, of a model's distance map and of the consensus (c3d_insulation) ---------------------------
// For every bead the mean of a map over the w x w square that straddles it, its log2 ratio to the row's mean, the strict extrema of that
// profile with their prominences, and the fit of a map's profile to IF's.  The definitions stand in include/c3d.h; what is said here is
// who computes what, and in which order every sum runs.
//
// A map is a band or a model.  IF's band comes from the host, the consensus band from k_ins_band: row a holds the cells (a, a+1 .. a + 2 wmax),
// n x 2 wmax doubles; a model's cells are cmp_dist of its coordinates (or 1.0 / 0.0 for d < cutoff with the contact flag: sums of these
// are integers below 2^53, exact in doubles in any order).  No n x n map exists anywhere.
//
//   k_ins_band       a thread a cell of the consensus band: the pick list's distances in list order from 0.0, divided once by the count
//                    (cpt_mean_dist: k_ens_map's `mean`), or the number of them below cutoff
//   k_ins_squares    the hot kernel.  A workgroup owns one map (blockIdx.y) and kInsTile = 32 consecutive beads.  The squares of a bead are
//                    nested, the square of w the union of the rings r = max(i-a, b-i) = 1..w, ring r holding the 2r - 1 cells
//                    (i-r, i+1 .. i+r) and then (i-r+1 .. i-1, i+r); numbered in that order, ring after ring, cell g of a bead lies in
//                    ring floor(sqrt(g)) + 1 and the square of w is the cells g < w^2.  Thread t adds the cells t, t + 256, ... ascending
//                    into one accumulator a listed window — window k takes the cells g < w_k^2, so its accumulator sees the terms it
//                    would see if it were listed alone — and one block_reduce<NW> a bead closes them: every window of the list out of
//                    one walk over the largest square the bead is inside, w^2 cells and not the sum of the squares.
//                    A model's tile first loads its beads and a halo of wmax on either side into LDS (24 (32 + 2 wmax) bytes) and the
//                    walk computes every cell from them.  STAGED (C3D_INSULATION_STAGE, wmax <= kInsStageMax = 40): the (31 + wmax)^2
//                    cells (a, b) that the tile's squares can touch are computed once each into LDS, 40 KiB at the most, and the walks
//                    read them — neighbouring beads' squares share all but a row and a column, so a distance is otherwise recomputed
//                    up to wmax times.  The same values in the same order: the two forms return the same bytes.  Measured on an
//                    MI355X (profiles/r31_insulation.md) staging does not pay: at 2048 x 20 the call is 0.48 against 0.45 ms at
//                    wmax = 8 and 0.52 against 0.52 ms at 32 — a bead's walk is w^2 / 256 cells a thread and then one block
//                    reduction, which is what a bead costs, and 50 - 64 KiB of LDS leave 2 or 3 workgroups a CU where the plain
//                    form has 8.  So the plain form is the default at every wmax and STAGED is kept for the measurement.
//   k_ins_score      one workgroup a (window, map): sum and count of the valid means (thread t the beads t, t + 256, ... ascending, one
//                    block_reduce<2>), then log2(mean / mbar) a bead
//   k_ins_boundary   a thread a bead: the strict maximum of y = -/+ score and the two walks of its prominence; comparisons, min/max, one
//                    subtraction
//   k_ins_fit        one workgroup a (window, map after IF): count and sums of the beads valid in both rows, the means, the centred sums
//                    (block_reduce<3>), r = sxy / sqrt(sxx syy); the four boundary counts as integers through block_reduce<4>
// Every floating-point sum is per-thread terms in ascending index order closed by block_reduce: no atomics, no prefix sums, and a row's
// arithmetic does not depend on the other maps or windows of the call.
__device__ __forceinline__ double ins_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(256) void k_ins_band(InsJob J) {
    const int W2 = 2 * J.wmax, n = J.n;
    const int idx = blockIdx.x * 256 + threadIdx.x;                   // n * W2 <= 16384 * 256
    if (idx >= n * W2) return;
    const int a = idx / W2, col = idx - a * W2, b = a + 1 + col;
    double v = 0.0;
    if (col >= 1 && b < n) {
        if (J.contact) {
            for (int k = 0; k < J.n_models; ++k) v += cmp_dist(J.xyz + (size_t)J.pick[k] * 3 * n, a, b) < J.cutoff ? 1.0 : 0.0;
        } else {
            v = cpt_mean_dist(J.xyz, n, J.pick, J.n_models, a, b);
        }
    }
    J.band_cons[idx] = v;
}

// ring and cell of g: r = floor(sqrt(g)) + 1 (g < 2^14: the float root is off by one at the most), then (a, b) relative to the bead
__device__ __forceinline__ void ins_cell(int g, int& da, int& db) {
    int r = (int)sqrtf((float)g);
    while (r * r > g) --r;
    while ((r + 1) * (r + 1) <= g) ++r;
    const int c = g - r * r;
    r += 1;
    if (c < r) { da = -r; db = 1 + c; }
    else { da = -r + 1 + (c - r); db = r; }
}

template <int NW, bool STAGED>
__global__ __launch_bounds__(256) void k_ins_squares(InsJob J, double* __restrict__ mean) {
    constexpr int kSide = kInsTile + kInsStageMax - 1;
    __shared__ double red[NW * 256];
    __shared__ double xs[3 * (kInsTile + 2 * C3D_INSULATION_MAX_WINDOW)];
    __shared__ double ds[STAGED ? kSide * kSide : 1];
    const int tid = threadIdx.x, q = blockIdx.y, n = J.n, wmax = J.wmax, W2 = 2 * wmax;
    const int i0 = blockIdx.x * kInsTile, i1 = i0 + kInsTile < n ? i0 + kInsTile : n;     // the tile's beads i0 .. i1 - 1
    const int mi = q - J.has_if;
    const bool is_if = J.has_if && q == 0, is_model = !is_if && mi < J.n_models;
    const double* band = is_if ? J.band_if : J.band_cons;
    const int x0 = i0 - wmax, side = kInsTile + wmax - 1;             // first bead of xs (may lie before the chain); the staged block's side
    if (is_model) {
        const double* x = J.xyz + (size_t)J.pick[mi] * 3 * n;
        const int lo = x0 < 0 ? 0 : x0, hi = i1 - 1 + wmax < n - 1 ? i1 - 1 + wmax : n - 1;
        for (int e = 3 * (lo - x0) + tid; e < 3 * (hi - x0 + 1); e += 256) xs[e] = x[3 * x0 + e];       // 3 x0 + e >= 3 lo >= 0
        __syncthreads();
        if (STAGED) {
            // cell (a, b) at ds[(a - x0) side + (b - i0 - 1)]: a in x0 .. i0 + 30, b in i0 + 1 .. i0 + 31 + wmax
            for (int e = tid; e < side * side; e += 256) {
                const int ra = e / side, rb = e - ra * side, a = x0 + ra, b = i0 + 1 + rb;
                if (a >= 0 && b < n && b - a >= 2 && b - a <= W2) {
                    const double d = cmp_dist(xs, a - x0, b - x0);
                    ds[e] = J.contact ? (d < J.cutoff ? 1.0 : 0.0) : d;
                }
            }
            __syncthreads();
        }
    }
    int w2[NW];
    for (int k = 0; k < NW; ++k) w2[k] = k < J.nw ? J.w[k] * J.w[k] : 0;
    for (int i = i0; i < i1; ++i) {
        const int room = i < n - 1 - i ? i : n - 1 - i;               // the largest window bead i is inside
        int G = 0;
        for (int k = 0; k < NW; ++k)
            if (k < J.nw && J.w[k] <= room) G = w2[k];
        double acc[NW];
        for (int k = 0; k < NW; ++k) acc[k] = 0.0;
        for (int g = tid; g < G; g += 256) {
            int da, db;
            ins_cell(g, da, db);
            const int a = i + da, b = i + db;
            double v;
            if (!is_model) v = band[(size_t)a * W2 + (b - a - 1)];
            else if (STAGED) v = ds[(a - x0) * side + (b - i0 - 1)];
            else {
                const double d = cmp_dist(xs, a - x0, b - x0);
                v = J.contact ? (d < J.cutoff ? 1.0 : 0.0) : d;
            }
#pragma unroll
            for (int k = 0; k < NW; ++k) acc[k] += g < w2[k] ? v : 0.0;
        }
        block_reduce<NW>(red, acc, tid, RedSum(), true);
        if (tid < J.nw) {
            const int w = J.w[tid];
            const double cells = (double)(w * w * (J.contact && !is_if && !is_model ? J.n_models : 1));
            mean[((size_t)q * J.nw + tid) * n + i] = w <= room ? red[tid * 256] / cells : ins_nan();
        }
    }
}

__global__ __launch_bounds__(256) void k_ins_score(int n, const double* __restrict__ mean, double* __restrict__ score) {
    __shared__ double red[2 * 256];
    const int tid = threadIdx.x;
    const size_t row = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * n;
    double v[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const double m = mean[row + i];
        if (m > 0.0) { v[0] += m; v[1] += 1.0; }
    }
    block_reduce<2>(red, v, tid, RedSum());
    const double mbar = red[0] / red[256];
    for (int i = tid; i < n; i += 256) {
        const double m = mean[row + i];
        score[row + i] = m > 0.0 ? log2(m / mbar) : ins_nan();
    }
}

__global__ __launch_bounds__(256) void k_ins_boundary(InsJob J, const double* __restrict__ score, int* __restrict__ boundary, double* __restrict__ strength) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = J.n;
    if (i >= n) return;
    const int q = blockIdx.y / J.nw;
    const bool minima = (J.has_if && q == 0) || J.contact;
    const double* s = score + (size_t)blockIdx.y * n;
    // y = -/+ score; a bead that is not valid has NaN, and every comparison with it is false
    const double yi = minima ? -s[i] : s[i];
    int mark = 0;
    double prom = 0.0;
    if (i >= 1 && i + 1 < n) {
        const double yl = minima ? -s[i - 1] : s[i - 1], yr = minima ? -s[i + 1] : s[i + 1];
        if (yi > yl && yi > yr) {
            double lmin = yi, rmin = yi;
            for (int j = i - 1; j >= 0; --j) {
                const double y = minima ? -s[j] : s[j];
                if (!(y <= yi)) break;
                lmin = fmin(lmin, y);
            }
            for (int j = i + 1; j < n; ++j) {
                const double y = minima ? -s[j] : s[j];
                if (!(y <= yi)) break;
                rmin = fmin(rmin, y);
            }
            mark = 1;
            prom = yi - fmax(lmin, rmin);
        }
    }
    boundary[(size_t)blockIdx.y * n + i] = mark;
    strength[(size_t)blockIdx.y * n + i] = prom;
}

__global__ __launch_bounds__(256) void k_ins_fit(InsJob J, const double* __restrict__ score, const int* __restrict__ boundary, const double* __restrict__ strength,
                                                double min_strength, int tol, double* __restrict__ fit_r, int* __restrict__ fit_counts) {
    __shared__ double red[3 * 256];
    __shared__ int redi[4 * 256];
    const int tid = threadIdx.x, k = blockIdx.x, q = 1 + blockIdx.y, n = J.n;
    const size_t rf = (size_t)k * n, rm = ((size_t)q * J.nw + k) * n;
    const double* F = score + rf;
    const double* S = score + rm;
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const double x = S[i], y = F[i];
        if (x == x && y == y) { v[0] += x; v[1] += y; v[2] += 1.0; }
    }
    block_reduce<3>(red, v, tid, RedSum());
    const double cnt = red[512], mx = red[0] / cnt, my = red[256] / cnt;
    v[0] = v[1] = v[2] = 0.0;
    for (int i = tid; i < n; i += 256) {
        const double x = S[i], y = F[i];
        if (x == x && y == y) {
            const double ex = x - mx, ey = y - my;
            v[0] += ex * ey; v[1] += ex * ex; v[2] += ey * ey;
        }
    }
    block_reduce<3>(red, v, tid, RedSum(), true);
    const double sxy = red[0], sxx = red[256], syy = red[512];
    // counted boundaries (strength >= min_strength) of IF and of the map, and those with a counted one of the other set within tol beads
    int c[4] = {0, 0, 0, 0};
    for (int i = tid; i < n; i += 256) {
        const bool in_f = boundary[rf + i] && strength[rf + i] >= min_strength, in_m = boundary[rm + i] && strength[rm + i] >= min_strength;
        if (!in_f && !in_m) continue;
        const int lo = i - (tol < i ? tol : i), hi = i + (tol < n - 1 - i ? tol : n - 1 - i);
        bool near_f = false, near_m = false;
        for (int j = lo; j <= hi; ++j) {
            near_f = near_f || (boundary[rf + j] && strength[rf + j] >= min_strength);
            near_m = near_m || (boundary[rm + j] && strength[rm + j] >= min_strength);
        }
        c[0] += in_f; c[1] += in_m; c[2] += in_f && near_m; c[3] += in_m && near_f;
    }
    block_reduce<4>(redi, c, tid, RedSum());
    const size_t out = (size_t)(q - 1) * J.nw + k;
    if (tid == 0 && fit_r) fit_r[out] = cnt >= 3.0 && sxx > 0.0 && syy > 0.0 ? sxy / sqrt(sxx * syy) : ins_nan();
    if (tid < 4 && fit_counts) fit_counts[out * 4 + tid] = redi[tid * 256];
}

hipError_t launch_insulation_band(const InsJob& job, hipStream_t s) {
    const unsigned cells = (unsigned)job.n * 2u * (unsigned)job.wmax;
    hipLaunchKernelGGL(k_ins_band, dim3((cells + 255) / 256), dim3(256), 0, s, job);
    return hipGetLastError();
}

template <int NW>
static void ins_launch_squares(const InsJob& job, bool stage, double* mean, hipStream_t s) {
    const dim3 grid((job.n + kInsTile - 1) / kInsTile, job.Q);
    if (stage) hipLaunchKernelGGL((k_ins_squares<NW, true>), grid, dim3(256), 0, s, job, mean);
    else hipLaunchKernelGGL((k_ins_squares<NW, false>), grid, dim3(256), 0, s, job, mean);
}

hipError_t launch_insulation_squares(const InsJob& job, bool stage, double* mean, hipStream_t s) {
    if (job.nw < 1 || job.nw > 8 || job.wmax < 1 || job.wmax > C3D_INSULATION_MAX_WINDOW || (stage && job.wmax > kInsStageMax)) return hipErrorInvalidValue;
    if (job.nw == 1) ins_launch_squares<1>(job, stage, mean, s);
    else if (job.nw == 2) ins_launch_squares<2>(job, stage, mean, s);
    else if (job.nw <= 4) ins_launch_squares<4>(job, stage, mean, s);
    else ins_launch_squares<8>(job, stage, mean, s);
    return hipGetLastError();
}

hipError_t launch_insulation_profile(const InsJob& job, const double* mean, double* score, int* boundary, double* strength, hipStream_t s) {
    hipLaunchKernelGGL(k_ins_score, dim3(job.nw, job.Q), dim3(256), 0, s, job.n, mean, score);
    hipLaunchKernelGGL(k_ins_boundary, dim3((job.n + 255) / 256, job.nw * job.Q), dim3(256), 0, s, job, score, boundary, strength);
    return hipGetLastError();
}

hipError_t launch_insulation_fit(const InsJob& job, const double* score, const int* boundary, const double* strength, double min_strength, int tol,
                                 double* fit_r, int* fit_counts, hipStream_t s) {
    hipLaunchKernelGGL(k_ins_fit, dim3(job.nw, job.Q - 1), dim3(256), 0, s, job, score, boundary, strength, min_strength, tol, fit_r, fit_counts);
    return hipGetLastError();
}
