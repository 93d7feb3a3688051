// c3d_score_loop.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- loop enrichment: the four local-background ratios of a pixel, peaks of IF, listed pixels in every map, aggregate peak analysis (c3d_loops) ----
// The definitions stand in include/c3d.h; what is said here is who computes what, and in which order every sum runs.
//
// A map is a band or a model.  IF's band comes from the host, the consensus band from k_loop_band: row a holds the cells
// (a, a + s_lo .. a + s_hi), n x S doubles, zeros beyond the matrix; a model's cells are cmp_dist of its coordinates.  No n x n map exists.
//
//   k_loop_band      a thread a cell of the consensus band: cpt_mean_dist, k_ens_map's `mean`
//   k_loop_expected  one workgroup a (separation, map): thread t the rows i = t, t + 256, ... ascending, the live cells' sum and count
//                    through one block_reduce<2>, divided once
//   k_loop_scan      the hot kernel, IF only.  A workgroup owns a kLoopTile x kLoopTile tile of pixels in (i, j).  It stages the
//                    (32 + 2w)^2 cells the tile's windows touch in LDS — a cell that is not live, or lies outside the matrix or the band,
//                    is stored as -1, which no IF value is — and E by separation beside them (64 + 4w values).  Thread t owns column
//                    t & 31 and the rows (t >> 5) + 8k, k = 0..3: the 32 lanes of a half-wave read 32 consecutive doubles of one row, the
//                    64 banks once each, whatever the pitch; the pitch is odd so that the two rows of a wave differ in the staging
//                    stores too.  A pixel's walk is loop_walk, the one the list pass runs: the same values in the same order.
//                    It writes `ratio` and, when peaks are wanted, the candidate flag of the pixel.
//   k_loop_nms       a thread a pixel: a candidate stays unless a candidate within `merge` beats it — comparisons only
//   k_loop_rows      a thread a row i: the row's candidates, peaks and inside pixels with a masked end, three integers
//   k_loop_offsets   one workgroup: the integer scan of the rows' peak counts (a thread a run of rows, then the 256 run sums), the report
//   k_loop_write     a thread a row i: its peaks in ascending j at the row's offset, while they fit
//   k_loop_list      a thread a (listed pixel, map): M, E and the four ratios, from the band or, for a model, from coordinates
//   k_loop_closed    one workgroup a map: the two counts of `closed`, integers through block_reduce<2>
//   k_loop_apa       one workgroup a (cell offset, map): thread t the pixels t, t + 256, ... of the list, quotient first, sum and count
//                    through one block_reduce<2>, divided once
//   k_loop_p2ll      a thread a map: the corner's mean row-major, then the quotient
// Every floating-point sum is per-thread terms in a fixed order, closed by block_reduce where more than one thread brings terms: no
// atomics, no prefix sums, and a map's numbers do not depend on the other maps of the call nor a pixel's on the other pixels.
__device__ __forceinline__ double loop_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// where map q takes its cells from: a band (IF's or the consensus') or the coordinates of a picked model
struct LoopSrc {
    const double* band;
    const double* x;
};
__device__ __forceinline__ LoopSrc loop_src(const LoopJob& J, int q) {
    const int mi = q - J.has_if;
    if (J.has_if && q == 0) return {J.band_if, nullptr};
    if (mi >= J.n_models) return {J.band_cons, nullptr};
    return {nullptr, J.xyz + (size_t)J.pick[mi] * 3 * J.n};
}
// M(a, b) of a map, a < b, b - a in s_lo .. s_hi
__device__ __forceinline__ double loop_cell(const LoopJob& J, const LoopSrc& src, int a, int b) {
    return src.band ? src.band[(size_t)a * J.S + (b - a - J.s_lo)] : cmp_dist(src.x, a, b);
}

// The walk of a pixel's (2w + 1)^2 cells, row-major, into the eight accumulators: cell(a, b, m, e) says whether the cell at offset (a, b)
// is live and gives its value and the expected value of its separation.  A cell that is not in a neighbourhood adds +0.0, which
// leaves a sum of non-negative terms as it is, bit for bit.
template <class F>
__device__ __forceinline__ void loop_walk(int p, int w, F&& cell, double (&sm)[4], double (&se)[4]) {
    for (int x = 0; x < 4; ++x) sm[x] = se[x] = 0.0;
    for (int a = -w; a <= w; ++a) {
        const int aa = a < 0 ? -a : a;
        for (int b = -w; b <= w; ++b) {
            double m, e;
            if (!cell(a, b, m, e)) continue;
            const int ab = b < 0 ? -b : b;
            const bool out = aa > p || ab > p;
            const bool c0 = out && a != 0 && b != 0, c1 = out && a >= 1 && b <= -1, c2 = aa <= 1 && ab > p, c3 = ab <= 1 && aa > p;
            sm[0] += c0 ? m : 0.0; se[0] += c0 ? e : 0.0;
            sm[1] += c1 ? m : 0.0; se[1] += c1 ? e : 0.0;
            sm[2] += c2 ? m : 0.0; se[2] += c2 ? e : 0.0;
            sm[3] += c3 ? m : 0.0; se[3] += c3 ? e : 0.0;
        }
    }
}
// r = M / ((SM / SE) E): a quotient, a product, a quotient, each rounded
__device__ __forceinline__ double loop_ratio(double m, double e, double sm, double se) {
    if (sm == 0.0 || se == 0.0) return loop_nan();
    const double bg = sm / se;
    const double ex = bg * e;
    return m / ex;
}

__global__ __launch_bounds__(256) void k_loop_band(LoopJob J) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, cells = (size_t)J.n * J.S;
    if (idx >= cells) return;
    const int a = (int)(idx / J.S), b = a + J.s_lo + (int)(idx - (size_t)a * J.S);
    J.band_cons[idx] = b < J.n ? cpt_mean_dist(J.xyz, J.n, J.pick, J.n_models, a, b) : 0.0;
}

__global__ __launch_bounds__(256) void k_loop_expected(LoopJob J) {
    __shared__ double red[2 * 256];
    const int tid = threadIdx.x, q = blockIdx.y, s = J.s_lo + blockIdx.x, n = J.n;
    const LoopSrc src = loop_src(J, q);
    double v[2] = {0.0, 0.0};
    for (int i = tid; i + s < n; i += 256)
        if (!J.mask[i] && !J.mask[i + s]) { v[0] += loop_cell(J, src, i, i + s); v[1] += 1.0; }
    block_reduce<2>(red, v, tid, RedSum());
    if (tid == 0) J.expected[(size_t)q * J.S + blockIdx.x] = red[256] > 0.0 ? red[0] / red[256] : 0.0;
}

// Tile k of tile row ti starts at column j0 = i0 + min_sep - 31 + 32 k: pixel (i, i + s) of the band lies in exactly one of the tiles
// k = 0 .. (B + 61) / 32, so every (s, i) of the output is written once, the pixels beyond the matrix (i + s > n - 1) included.
__global__ __launch_bounds__(256) void k_loop_scan(LoopJob J, LoopPeakRule rule, double* __restrict__ ratio, unsigned char* __restrict__ cand) {
    constexpr int kSide = kLoopTile + 2 * C3D_LOOP_MAX_WINDOW, kPitch = kSide + 1;
    __shared__ double cells[kSide * kPitch];
    __shared__ double es[2 * kLoopTile + 4 * C3D_LOOP_MAX_WINDOW];
    const int tid = threadIdx.x, n = J.n, w = J.w, S = J.S, B = J.max_sep - J.min_sep + 1;
    const int i0 = blockIdx.x * kLoopTile, j0 = i0 + J.min_sep - (kLoopTile - 1) + kLoopTile * (int)blockIdx.y;
    const int side = kLoopTile + 2 * w, pitch = side | 1, s_hi = J.s_lo + S - 1;
    const int sep0 = (j0 - w) - (i0 + kLoopTile - 1 + w);              // the smallest separation of a staged cell
    for (int e = tid; e < side * side; e += 256) {
        const int ra = e / side, rb = e - ra * side, a = i0 - w + ra, b = j0 - w + rb, s = b - a;
        double v = -1.0;
        if (a >= 0 && b < n && s >= J.s_lo && s <= s_hi && !J.mask[a] && !J.mask[b]) v = J.band_if[(size_t)a * S + (s - J.s_lo)];
        cells[ra * pitch + rb] = v;
    }
    for (int e = tid; e < 2 * kLoopTile + 4 * w; e += 256) {
        const int s = sep0 + e;
        es[e] = s >= J.s_lo && s <= s_hi ? J.expected[s - J.s_lo] : 0.0;
    }
    __syncthreads();
    const int lj = tid & (kLoopTile - 1), j = j0 + lj;
    for (int k = 0; k < 4; ++k) {
        const int li = (tid >> 5) + 8 * k, i = i0 + li, s = j - i;
        if (i >= n || s < J.min_sep || s > J.max_sep) continue;
        double r[4] = {loop_nan(), loop_nan(), loop_nan(), loop_nan()};
        double m = -1.0;
        if (j <= n - 1 && i >= w && j + w <= n - 1) {
            m = cells[(li + w) * pitch + (lj + w)];
            const double e = es[s - sep0];
            if (m >= 0.0 && e != 0.0) {
                double sm[4], se[4];
                const double* at = cells + (li + w) * pitch + (lj + w);
                const double* eat = es + (s - sep0);
                loop_walk(J.p, w, [&](int a, int b, double& cm, double& ce) {
                    cm = at[a * pitch + b];
                    ce = eat[b - a];
                    return cm >= 0.0;
                }, sm, se);
                for (int x = 0; x < 4; ++x) r[x] = loop_ratio(m, e, sm[x], se[x]);
            }
        }
        const size_t out = (size_t)(s - J.min_sep) * n + i;
        if (ratio)
            for (int x = 0; x < 4; ++x) ratio[(size_t)x * B * n + out] = r[x];
        if (cand) cand[out] = r[0] >= rule.thr[0] && r[1] >= rule.thr[1] && r[2] >= rule.thr[2] && r[3] >= rule.thr[3] && m >= rule.min_obs ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_loop_nms(LoopJob J, int merge, const unsigned char* __restrict__ cand, unsigned char* __restrict__ peak) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = J.n, s = J.min_sep + blockIdx.y;
    if (i >= n) return;
    const size_t at = (size_t)blockIdx.y * n + i;
    unsigned char keep = cand[at];
    if (keep) {
        const int j = i + s;
        const double m = J.band_if[(size_t)i * J.S + (s - J.s_lo)];
        for (int di = -merge; di <= merge && keep; ++di)
            for (int dj = -merge; dj <= merge; ++dj) {
                const int i2 = i + di, j2 = j + dj, s2 = j2 - i2;
                if ((di == 0 && dj == 0) || i2 < 0 || i2 >= n || s2 < J.min_sep || s2 > J.max_sep) continue;
                if (!cand[(size_t)(s2 - J.min_sep) * n + i2]) continue;
                const double m2 = J.band_if[(size_t)i2 * J.S + (s2 - J.s_lo)];
                if (m2 > m || (m2 == m && (i2 < i || (i2 == i && j2 < j)))) { keep = 0; break; }
            }
    }
    peak[at] = keep;
}

__global__ __launch_bounds__(256) void k_loop_rows(LoopJob J, const unsigned char* __restrict__ cand, const unsigned char* __restrict__ peak, int* __restrict__ rows) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = J.n;
    if (i >= n) return;
    int c = 0, pk = 0, lost = 0;
    for (int s = J.min_sep; s <= J.max_sep; ++s) {
        const size_t at = (size_t)(s - J.min_sep) * n + i;
        c += cand[at];
        pk += peak[at];
        const int j = i + s;
        if (i >= J.w && j + J.w <= n - 1 && (J.mask[i] || J.mask[j])) ++lost;
    }
    rows[3 * i] = c; rows[3 * i + 1] = pk; rows[3 * i + 2] = lost;
}

__global__ __launch_bounds__(256) void k_loop_offsets(int n, int max_peaks, const int* __restrict__ rows, int* __restrict__ offset, int* __restrict__ report) {
    __shared__ int red[3 * 256];
    __shared__ int runs[256];
    const int tid = threadIdx.x, run = (n + 255) / 256, lo = tid * run, hi = lo + run < n ? lo + run : n;
    int v[3] = {0, 0, 0};
    for (int i = lo; i < hi; ++i) { v[0] += rows[3 * i]; v[1] += rows[3 * i + 1]; v[2] += rows[3 * i + 2]; }
    runs[tid] = v[1];
    block_reduce<3>(red, v, tid, RedSum());
    int off = 0;
    for (int t = 0; t < tid; ++t) off += runs[t];
    for (int i = lo; i < hi; ++i) { offset[i] = off; off += rows[3 * i + 1]; }
    if (tid == 0) {
        const int found = red[256];
        report[0] = red[0]; report[1] = found; report[2] = found < max_peaks ? found : max_peaks; report[3] = red[512];
    }
}

__global__ __launch_bounds__(256) void k_loop_write(LoopJob J, int max_peaks, const unsigned char* __restrict__ peak, const int* __restrict__ offset, int* __restrict__ peaks) {
    const int i = blockIdx.x * 256 + threadIdx.x, n = J.n;
    if (i >= n) return;
    int at = offset[i];
    for (int s = J.min_sep; s <= J.max_sep && at < max_peaks; ++s)
        if (peak[(size_t)(s - J.min_sep) * n + i]) { peaks[2 * at] = i; peaks[2 * at + 1] = i + s; ++at; }
}

__global__ __launch_bounds__(256) void k_loop_list(LoopJob J, const int* __restrict__ list, int L, double* __restrict__ at) {
    const int l = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, n = J.n, w = J.w;
    if (l >= L) return;
    const int i = list[2 * l], j = list[2 * l + 1], s = j - i;
    const LoopSrc src = loop_src(J, q);
    const double* E = J.expected + (size_t)q * J.S - J.s_lo;            // E[separation]
    const double m = loop_cell(J, src, i, j), e = E[s];
    double r[4] = {loop_nan(), loop_nan(), loop_nan(), loop_nan()};
    if (i >= w && j + w <= n - 1 && !J.mask[i] && !J.mask[j] && e != 0.0) {
        double sm[4], se[4];
        loop_walk(J.p, w, [&](int a, int b, double& cm, double& ce) {
            const int ca = i + a, cb = j + b;
            if (J.mask[ca] || J.mask[cb]) return false;
            cm = loop_cell(J, src, ca, cb);
            ce = E[cb - ca];
            return true;
        }, sm, se);
        for (int x = 0; x < 4; ++x) r[x] = loop_ratio(m, e, sm[x], se[x]);
    }
    double* out = at + ((size_t)q * L + l) * 6;
    out[0] = m; out[1] = e;
    for (int x = 0; x < 4; ++x) out[2 + x] = r[x];
}

__global__ __launch_bounds__(256) void k_loop_closed(LoopJob J, int L, const double* __restrict__ at, int* __restrict__ closed) {
    __shared__ int red[2 * 256];
    const int tid = threadIdx.x, q = blockIdx.x;
    const bool above = J.has_if && q == 0;                              // the loop side: > 1 for IF, < 1 for distances
    int v[2] = {0, 0};
    for (int l = tid; l < L; l += 256) {
        const double rd = at[((size_t)q * L + l) * 6 + 2], rl = at[((size_t)q * L + l) * 6 + 3];
        if (rd == rd && rl == rl) {
            ++v[0];
            if (above ? (rd > 1.0 && rl > 1.0) : (rd < 1.0 && rl < 1.0)) ++v[1];
        }
    }
    block_reduce<2>(red, v, tid, RedSum());
    if (tid < 2) closed[2 * q + tid] = red[tid * 256];
}

__global__ __launch_bounds__(256) void k_loop_apa(LoopJob J, const int* __restrict__ list, int L, double* __restrict__ apa) {
    __shared__ double red[2 * 256];
    const int tid = threadIdx.x, q = blockIdx.y, n = J.n, w = J.w, side = 2 * w + 1;
    const int a = (int)blockIdx.x / side - w, b = (int)blockIdx.x % side - w;
    const LoopSrc src = loop_src(J, q);
    const double* E = J.expected + (size_t)q * J.S - J.s_lo;
    double v[2] = {0.0, 0.0};
    for (int l = tid; l < L; l += 256) {
        const int i = list[2 * l], j = list[2 * l + 1];
        if (i < w || j + w > n - 1) continue;
        const int ca = i + a, cb = j + b;
        if (J.mask[ca] || J.mask[cb]) continue;
        const double e = E[cb - ca];
        if (e == 0.0) continue;
        const double t = loop_cell(J, src, ca, cb) / e;
        v[0] += t; v[1] += 1.0;
    }
    block_reduce<2>(red, v, tid, RedSum());
    if (tid == 0) apa[(size_t)q * side * side + blockIdx.x] = red[256] > 0.0 ? red[0] / red[256] : loop_nan();
}

__global__ __launch_bounds__(256) void k_loop_p2ll(int Q, int w, int corner, const double* __restrict__ apa, double* __restrict__ p2ll) {
    const int q = blockIdx.x * 256 + threadIdx.x, side = 2 * w + 1;
    if (q >= Q) return;
    const double* A = apa + (size_t)q * side * side;
    double sum = 0.0;
    for (int a = w - corner + 1; a <= w; ++a)
        for (int b = -w; b <= -w + corner - 1; ++b) sum += A[(a + w) * side + (b + w)];
    const double ll = sum / (double)(corner * corner);
    p2ll[q] = A[w * side + w] / ll;
}

static bool loop_job_ok(const LoopJob& J) {
    return J.n >= 2 && J.w >= 1 && J.w <= C3D_LOOP_MAX_WINDOW && J.p >= 0 && J.p < J.w && J.min_sep >= 2 * J.w + 1 && J.max_sep >= J.min_sep && J.max_sep <= J.n - 1 &&
           J.max_sep - J.min_sep + 1 <= C3D_LOOP_MAX_BAND && J.s_lo == J.min_sep - 2 * J.w && J.S >= 1 && J.s_lo + J.S - 1 <= J.n - 1 && J.Q >= 1;
}

hipError_t launch_loop_expected(const LoopJob& job, hipStream_t s) {
    if (!loop_job_ok(job)) return hipErrorInvalidValue;
    if (job.consensus) {
        const size_t cells = (size_t)job.n * job.S;
        hipLaunchKernelGGL(k_loop_band, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, job);
    }
    hipLaunchKernelGGL(k_loop_expected, dim3(job.S, job.Q), dim3(256), 0, s, job);
    return hipGetLastError();
}

hipError_t launch_loop_scan(const LoopJob& job, const LoopPeakRule& rule, double* ratio, unsigned char* cand, hipStream_t s) {
    if (!loop_job_ok(job) || !job.has_if) return hipErrorInvalidValue;
    const int B = job.max_sep - job.min_sep + 1;
    hipLaunchKernelGGL(k_loop_scan, dim3((job.n + kLoopTile - 1) / kLoopTile, (B + 2 * kLoopTile - 3) / kLoopTile + 1), dim3(256), 0, s, job, rule, ratio, cand);
    return hipGetLastError();
}

hipError_t launch_loop_peaks(const LoopJob& job, int merge, int max_peaks, const unsigned char* cand, unsigned char* peak, int* rows, int* offset, int* peaks, int* report,
                             hipStream_t s) {
    if (!loop_job_ok(job) || !job.has_if || merge < 0 || merge > job.w || max_peaks < 0) return hipErrorInvalidValue;
    const int B = job.max_sep - job.min_sep + 1;
    const unsigned nb = (job.n + 255) / 256;
    hipLaunchKernelGGL(k_loop_nms, dim3(nb, B), dim3(256), 0, s, job, merge, cand, peak);
    hipLaunchKernelGGL(k_loop_rows, dim3(nb), dim3(256), 0, s, job, cand, peak, rows);
    hipLaunchKernelGGL(k_loop_offsets, dim3(1), dim3(256), 0, s, job.n, max_peaks, rows, offset, report);
    if (max_peaks > 0) hipLaunchKernelGGL(k_loop_write, dim3(nb), dim3(256), 0, s, job, max_peaks, peak, offset, peaks);
    return hipGetLastError();
}

hipError_t launch_loop_list(const LoopJob& job, const int* list, int L, double* at, int* closed, hipStream_t s) {
    if (!loop_job_ok(job) || L < 0 || L > C3D_LOOP_MAX_LIST) return hipErrorInvalidValue;
    if (L > 0) hipLaunchKernelGGL(k_loop_list, dim3((L + 255) / 256, job.Q), dim3(256), 0, s, job, list, L, at);
    hipLaunchKernelGGL(k_loop_closed, dim3(job.Q), dim3(256), 0, s, job, L, at, closed);
    return hipGetLastError();
}

hipError_t launch_loop_apa(const LoopJob& job, const int* list, int L, int corner, double* apa, double* p2ll, hipStream_t s) {
    if (!loop_job_ok(job) || L < 0 || L > C3D_LOOP_MAX_LIST || corner < 1 || corner > job.w) return hipErrorInvalidValue;
    const int side = 2 * job.w + 1;
    hipLaunchKernelGGL(k_loop_apa, dim3(side * side, job.Q), dim3(256), 0, s, job, list, L, apa);
    hipLaunchKernelGGL(k_loop_p2ll, dim3((job.Q + 255) / 256), dim3(256), 0, s, job.Q, job.w, corner, apa, p2ll);
    return hipGetLastError();
}
