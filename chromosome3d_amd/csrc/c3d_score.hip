// c3d_score.hip — K6: assessment and Spearman scoring of every replica on the device (gfx950), so that
// ranking needs no read-back of coordinates.
//   count_satisfied_tbl_rows / sum_noe_dev   chromosome3D.pl:447-485, 581-600 (distances as "%.3f" text)
//   Spearman(IF_ij, d_ij), |i-j| >= range     spearman_IF_pdb.pl:42-70 (average ranks, d as "%.3f")
// The reference reads coordinates back from "%8.3f" PDB text and prints distances with "%.3f": both
// roundings are reproduced exactly with the fma-residual rule (round_milli), so distances are integers in
// thousandths of an Angstrom and their average ranks come from a histogram — no sort:
//   k_score_round   xr = round3(x) in fp64
//   k_score_hist    histogram of dq = round3(|xr_i - xr_j|) over ordered pairs |i-j| >= range (int atomics)
//   k_score_scan    exclusive prefix of the histogram (one workgroup per replica)
//   k_score_corr    sum (ra - ma)(rb - mb), sum (rb - mb)^2 with rb = below[dq] + (cnt[dq] + 1)/2, and the
//                   satisfied / sum-of-deviation tallies over the restrained pairs; per-block fp64 partials
// The IF ranks ra (one N x N fp64 matrix per input matrix) come from the host (c3d::if_pair_ranks) or, for large symmetric matrices, from
// the device (k_rank_*: a key-only bitonic sort of the upper triangle and two binary searches per pair; option device_ranks).
// A call whose models do not fit the fixed histogram is scored again by launch_score_wide with a histogram sized from k_score_bbox.
// The models of a run against one another (c3d_compare_replicas: k_cmp_*) sort their own distances with the same network; k_sup_* put them
// in one frame (c3d_superpose_replicas, c3d_rmsd_table); k_ens_* describe the ensemble itself: the mean, spread and contact frequency of
// every pair distance over the models, and the rank correlation of those maps with IF (c3d_ensemble_map, c3d_ensemble_score).
// k_geo_* measure a model (the reference's clash count, nearest partners, chain envelope: c3d_geometry_replicas) and k_sep_* the distance
// against the genomic separation over the models (c3d_separation_profile).
#include "c3d_internal.h"

namespace c3d {

__device__ __forceinline__ long long round_milli_dev(double d) {
    const double p = d * 1000.0;
    const double err = fma(d, 1000.0, -p);
    double r = rint(p);
    const double diff = p - r;
    if (diff == 0.5 || diff == -0.5) {
        if (err > 0) r = floor(p) + 1.0;
        else if (err < 0) r = floor(p);
    }
    return (long long)r;
}

__global__ __launch_bounds__(256) void k_score_round(const float* __restrict__ xin, int n, int npad, double* __restrict__ xr) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n
    if (q >= 3 * n) return;
    const int comp = q / n, i = q - comp * n;
    xr[((size_t)rep * 3 + comp) * n + i] = (double)round_milli_dev((double)xin[((size_t)rep * 3 + comp) * npad + i]) / 1000.0;
}

__device__ __forceinline__ unsigned pair_dq(const double* __restrict__ xr, int n, int i, int j, unsigned nbins, int* overflow) {
    const double dx = xr[i] - xr[j], dy = xr[n + i] - xr[n + j], dz = xr[2 * n + i] - xr[2 * n + j];
    const long long q = round_milli_dev(sqrt(dx * dx + dy * dy + dz * dz));
    if (q >= (long long)nbins) { *overflow = 1; return nbins - 1; }
    return (unsigned)q;
}

__global__ __launch_bounds__(256) void k_score_hist(const double* __restrict__ xr_all, int n, int range, unsigned nbins,
                                                   unsigned* __restrict__ hist_all, int* __restrict__ overflow) {
    const int i = blockIdx.x, rep = blockIdx.y;
    const double* xr = xr_all + (size_t)rep * 3 * n;
    unsigned* hist = hist_all + (size_t)rep * nbins;
    for (int j = threadIdx.x; j < n; j += 256) {
        const int sep = i > j ? i - j : j - i;
        if (sep < range) continue;
        atomicAdd(&hist[pair_dq(xr, n, i, j, nbins, overflow)], 1u);
    }
}

// exclusive prefix sum of hist -> below (one workgroup per replica, 1024 threads, sequential chunks)
__global__ __launch_bounds__(1024) void k_score_scan(const unsigned* __restrict__ hist_all, unsigned nbins,
                                                    unsigned* __restrict__ below_all) {
    __shared__ unsigned part[1024];
    const int rep = blockIdx.x, tid = threadIdx.x;
    const unsigned* hist = hist_all + (size_t)rep * nbins;
    unsigned* below = below_all + (size_t)rep * nbins;
    const unsigned per = (nbins + 1023u) / 1024u;
    const unsigned lo = tid * per, hi = min(lo + per, nbins);
    unsigned s = 0;
    for (unsigned v = lo; v < hi; ++v) s += hist[v];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned run = 0;
        for (int k = 0; k < 1024; ++k) { const unsigned t = part[k]; part[k] = run; run += t; }
    }
    __syncthreads();
    unsigned run = part[tid];
    for (unsigned v = lo; v < hi; ++v) { below[v] = run; run += hist[v]; }
}

// partial[rep][row][0..3] = { sum (ra-ma)(rb-mb), sum (rb-mb)^2, satisfied (as double), sum_dev }
__global__ __launch_bounds__(256) void k_score_corr(const double* __restrict__ xr_all, const float* __restrict__ tgt,
                                                   const double* __restrict__ rankA, int n, int npad, int range, int min_sep,
                                                   unsigned nbins, const unsigned* __restrict__ hist_all,
                                                   const unsigned* __restrict__ below_all, double ma, double mb, double relax,
                                                   double* __restrict__ partial, int* __restrict__ overflow) {
    __shared__ double red[4][256];
    const int i = blockIdx.x, rep = blockIdx.y, tid = threadIdx.x;
    const double* xr = xr_all + (size_t)rep * 3 * n;
    const unsigned* hist = hist_all + (size_t)rep * nbins;
    const unsigned* below = below_all + (size_t)rep * nbins;
    double sab = 0, sbb = 0, sat = 0, dev = 0;
    for (int j = tid; j < n; j += 256) {
        const int sep = i > j ? i - j : j - i;
        if (sep == 0) continue;
        const unsigned dq = pair_dq(xr, n, i, j, nbins, overflow);
        if (sep >= range && rankA) {
            const double rb = (double)below[dq] + 0.5 * ((double)hist[dq] + 1.0);
            const double a = rankA[(size_t)i * n + j] - ma, b = rb - mb;
            sab += a * b;
            sbb += b * b;
        }
        const float tv = tgt[(size_t)i * npad + j];
        if (j > i && sep >= min_sep && tv > 0.0f) {
            const double t = (double)lrintf(tv * 10.0f) / 10.0;     // the tbl's "%.2f" value, exactly t10/10
            const double d = (double)dq / 1000.0;
            if (d < t + 0.0 + relax) sat += 1.0;
            if (d < t - 0.0 - relax) sat -= 1.0;
            if (d > t + 0.0 + 0.2) dev += d - (t + 0.0);
            if (d < t - 0.0 - 0.2) dev += (t - 0.0) - d;
        }
    }
    red[0][tid] = sab; red[1][tid] = sbb; red[2][tid] = sat; red[3][tid] = dev;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) for (int c = 0; c < 4; ++c) red[c][tid] += red[c][tid + s];
        __syncthreads();
    }
    if (tid < 4) partial[((size_t)rep * n + i) * 4 + tid] = red[tid][0];
}

// ---- models wider than the fixed histogram --------------------------------------------------------------------------------------------
// box[rep][comp][0..1] = min, max of the rounded coordinates of a replica
__global__ __launch_bounds__(256) void k_score_bbox(const double* __restrict__ xr_all, int n, double* __restrict__ box) {
    __shared__ double lo[256], hi[256];
    const int rep = blockIdx.x, comp = blockIdx.y, tid = threadIdx.x;
    const double* x = xr_all + ((size_t)rep * 3 + comp) * n;
    double a = x[0], b = x[0];
    for (int i = tid; i < n; i += 256) { a = fmin(a, x[i]); b = fmax(b, x[i]); }
    lo[tid] = a; hi[tid] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { lo[tid] = fmin(lo[tid], lo[tid + s]); hi[tid] = fmax(hi[tid], hi[tid + s]); }
        __syncthreads();
    }
    if (tid == 0) { box[(rep * 3 + comp) * 2] = lo[0]; box[(rep * 3 + comp) * 2 + 1] = hi[0]; }
}

hipError_t launch_score_bbox(const double* xr, int n, int nrep, double* box, hipStream_t s) {
    hipLaunchKernelGGL(k_score_bbox, dim3(nrep, 3), dim3(256), 0, s, xr, n, box);
    return hipGetLastError();
}

// histogram, prefix and sums for `nrep` replicas whose rounded coordinates xr and sums `partial` start at the first of them, with `nbins`
// bins per replica; `overflow` is only ever raised (the caller clears it once for all batches)
hipError_t launch_score_wide(const double* xr, const float* tgt, const double* rankA, int n, int npad, int nrep, int range, int min_sep,
                             unsigned nbins, double ma, double mb, double relax, unsigned* hist, unsigned* below, double* partial,
                             int* overflow, hipStream_t s) {
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned) * (size_t)nbins * nrep, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_hist, dim3(n, nrep), dim3(256), 0, s, xr, n, range, nbins, hist, overflow);
    hipLaunchKernelGGL(k_score_scan, dim3(nrep), dim3(1024), 0, s, hist, nbins, below);
    hipLaunchKernelGGL(k_score_corr, dim3(n, nrep), dim3(256), 0, s, xr, tgt, rankA, n, npad, range, min_sep, nbins, hist, below, ma,
                       mb, relax, partial, overflow);
    return hipGetLastError();
}

// the first pass of every call: all replicas, rounded coordinates first, the fixed histogram
hipError_t launch_score(const float* xin, const float* tgt, const double* rankA, int n, int npad, int nrep, int range, int min_sep,
                        unsigned nbins, double ma, double mb, double relax, double* xr, unsigned* hist, unsigned* below,
                        double* partial, int* overflow, hipStream_t s) {
    hipError_t e = hipMemsetAsync(overflow, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_score_round, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, xin, n, npad, xr);
    return launch_score_wide(xr, tgt, rankA, n, npad, nrep, range, min_sep, nbins, ma, mb, relax, hist, below, partial, overflow, s);
}

// ---- IF ranks on the device -----------------------------------------------------------------------------------------------------------
// The average ranks of c3d::if_pair_ranks for a symmetric matrix: the multiset in which every upper-triangle value |i-j| >= range appears
// twice; a tie group at sorted half-list positions k..e has rank k + e + 1.5.  Equal keys are interchangeable, so the keys alone are
// sorted (order_key of c3d_host.cpp; -0.0 takes the key of +0.0, which the host's value comparison ties it with) and every pair finds
// its group's bounds by binary search.  The sort is a bitonic network over `slots` keys (a power of two >= kRankTile, padded with the
// largest key): the strides below kRankTile run in LDS (32 KiB a workgroup), the others one pass over global memory each.
__device__ __forceinline__ unsigned long long rank_key(double d) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    if ((u << 1) == 0) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// first key of row i in the key array: rows 0..i-1 hold w, w-1, ... keys (w = n - range)
__device__ __forceinline__ size_t rank_row_offset(int i, int w) { return (size_t)i * w - (size_t)i * (i - 1) / 2; }

__global__ __launch_bounds__(256) void k_rank_keys(const double* __restrict__ M, int n, int range, unsigned long long* __restrict__ keys,
                                                  size_t mh, size_t slots, int* __restrict__ asym) {
    const int i = blockIdx.x, tid = threadIdx.x;
    if (i + range < n) {
        unsigned long long* row = keys + rank_row_offset(i, n - range);
        for (int j = i + range + tid; j < n; j += 256) {
            const double a = M[(size_t)i * n + j];
            if (a != M[(size_t)j * n + i]) *asym = 1;
            row[j - i - range] = rank_key(a);
        }
    }
    for (size_t p = mh + (size_t)i * 256 + tid; p < slots; p += (size_t)gridDim.x * 256) keys[p] = ~0ull;
}

// one tile of kRankTile keys: the network's stages size_first..size_last, each from stride min(size, kRankTile) / 2 down
__global__ __launch_bounds__(1024) void k_rank_sort_tile(unsigned long long* __restrict__ keys, size_t size_first, size_t size_last) {
    __shared__ unsigned long long t[kRankTile];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * kRankTile;
    for (int p = tid; p < kRankTile; p += 1024) t[p] = keys[base + p];
    __syncthreads();
    for (size_t size = size_first; size <= size_last; size <<= 1) {
        for (unsigned stride = (unsigned)(size < (size_t)kRankTile ? size : (size_t)kRankTile) >> 1; stride > 0; stride >>= 1) {
            for (unsigned p = tid; p < kRankTile / 2; p += 1024) {
                const unsigned lo = p & (stride - 1), a = ((p - lo) << 1) | lo, b = a | stride;
                const bool up = ((base + a) & size) == 0;
                const unsigned long long x = t[a], y = t[b];
                if ((x > y) == up) { t[a] = y; t[b] = x; }
            }
            __syncthreads();
        }
    }
    for (int p = tid; p < kRankTile; p += 1024) keys[base + p] = t[p];
}

// one compare-exchange pass of stage `size` at `stride` >= kRankTile over slots / 2 pairs
__global__ __launch_bounds__(256) void k_rank_sort_step(unsigned long long* __restrict__ keys, size_t size, size_t stride) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t lo = p & (stride - 1), a = ((p - lo) << 1) | lo, b = a | stride;
    const bool up = (a & size) == 0;
    const unsigned long long x = keys[a], y = keys[b];
    if ((x > y) == up) { keys[a] = y; keys[b] = x; }
}

// first position in keys[0..mh) whose key is not below `key`
__device__ __forceinline__ size_t rank_lower_bound(const unsigned long long* __restrict__ keys, size_t lo, size_t hi, unsigned long long key) {
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// M holds the matrix on entry and the ranks on exit: the thread of (i, j), i < j, is the only reader of (i, j) and the only writer of
// (i, j) and (j, i); pairs inside the band |i-j| < range get 0 as in the host's rank matrix
__global__ __launch_bounds__(256) void k_rank_assign(double* __restrict__ M, int n, int range, const unsigned long long* __restrict__ keys, size_t mh) {
    const int i = blockIdx.x;
    for (int j = i + threadIdx.x; j < n; j += 256) {
        double r = 0.0;
        if (j - i >= range) {
            const unsigned long long key = rank_key(M[(size_t)i * n + j]);
            const size_t k = rank_lower_bound(keys, 0, mh, key);
            const size_t e = key == ~0ull ? mh : rank_lower_bound(keys, k, mh, key + 1);     // one past the group
            r = ((double)k + (double)(e - 1)) + 1.5;
        }
        M[(size_t)i * n + j] = r;
        M[(size_t)j * n + i] = r;
    }
}

// out[i] = sum over j, |i-j| >= range, of (rank(i, j) - ma)^2, summed in a fixed order
__global__ __launch_bounds__(256) void k_rank_saa(const double* __restrict__ M, int n, int range, double ma, double* __restrict__ out) {
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double s = 0;
    for (int j = tid; j < n; j += 256) {
        const int sep = i > j ? i - j : j - i;
        if (sep < range) continue;
        const double d = M[(size_t)i * n + j] - ma;
        s += d * d;
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[i] = red[0];
}

hipError_t launch_if_rank_keys(const double* M, int n, int range, unsigned long long* keys, size_t mh, size_t slots, int* asym, hipStream_t s) {
    hipError_t e = hipMemsetAsync(asym, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rank_keys, dim3(n), dim3(256), 0, s, M, n, range, keys, mh, slots, asym);
    return hipGetLastError();
}

// the network over `slots` keys: what launch_if_rank_sort and launch_compare_ranks both sort with
static void launch_rank_sort_network(unsigned long long* keys, size_t slots, hipStream_t s) {
    const unsigned tiles = (unsigned)(slots / kRankTile), step_blocks = (unsigned)(slots / 2 / 256);
    hipLaunchKernelGGL(k_rank_sort_tile, dim3(tiles), dim3(1024), 0, s, keys, (size_t)2, (size_t)kRankTile);
    for (size_t size = 2 * (size_t)kRankTile; size <= slots; size <<= 1) {
        for (size_t stride = size >> 1; stride >= (size_t)kRankTile; stride >>= 1)
            hipLaunchKernelGGL(k_rank_sort_step, dim3(step_blocks), dim3(256), 0, s, keys, size, stride);
        hipLaunchKernelGGL(k_rank_sort_tile, dim3(tiles), dim3(1024), 0, s, keys, size, size);
    }
}

hipError_t launch_if_rank_sort(double* M, int n, int range, unsigned long long* keys, size_t mh, size_t slots, double ma, double* saa_rows,
                               hipStream_t s) {
    launch_rank_sort_network(keys, slots, s);
    hipLaunchKernelGGL(k_rank_assign, dim3(n), dim3(256), 0, s, M, n, range, keys, mh);
    hipLaunchKernelGGL(k_rank_saa, dim3(n), dim3(256), 0, s, M, n, range, ma, saa_rows);
    return hipGetLastError();
}

// ---- the models of a run against one another (c3d_compare_replicas) -----------------------------------------------------------------------
// c3d_model_similarity for every ordered pair of K models at once: the Spearman coefficient of the i<j distances and the RMS difference of
// those distances after scaling the first model's by the ratio of the mean distances.  A model is n x 3 doubles, xyz interleaved (a
// replica's floats widened by k_cmp_coords).  Per model: the keys of its m = n(n-1)/2 distances are sorted with the network above and every
// pair finds its tie group's bounds k..e, of which k + e is kept (32 bits; average rank = (k + e) / 2 + 1, centred rank = (k + e - (m - 1)) / 2,
// both exact); the same pass sums the distances per row.  Then one pass over the pairs forms both K x K tables: a workgroup takes sixteen
// models a and sixteen models b, one thread an entry, and walks its chunk of the pairs in tiles of kCmpPairs staged in LDS; the per-chunk
// sums are added in chunk order by k_cmp_table_sum.  No atomics anywhere: the same coordinates give the same bits.
//
// The distance has the bits of the host's: ((ux ux) + uy uy) + uz uz with every operation rounded on its own, then sqrt.  This unit is
// compiled with -ffp-contract=fast, which lets the instruction selector fuse any product into the sum that uses it whatever a pragma says
// of the source (and makes __dmul_rn / __dadd_rn plain * and +): each product therefore passes through an empty asm statement, which
// costs no instruction and leaves the selector a register, not a multiplication, to add.
__device__ __forceinline__ double cmp_rounded(double t) {
    asm("" : "+v"(t));
    return t;
}
__device__ __forceinline__ double cmp_dist(const double* __restrict__ x, int i, int j) {
    const double ux = x[3 * i] - x[3 * j], uy = x[3 * i + 1] - x[3 * j + 1], uz = x[3 * i + 2] - x[3 * j + 2];
    double q = cmp_rounded(ux * ux);
    q += cmp_rounded(uy * uy);
    q += cmp_rounded(uz * uz);
    return sqrt(q);
}
// scale * da - db as the host rounds it: the product first
__device__ __forceinline__ double cmp_scaled_diff(double scale, double da, double db) { return cmp_rounded(scale * da) - db; }

constexpr int kCmpPairs = 64;        // pairs of a staged tile (kCmpModels models a side: c3d_internal.h)

__global__ __launch_bounds__(256) void k_cmp_coords(const float* __restrict__ xin, int n, int npad, double* __restrict__ xyz) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n, as the output is laid out
    if (q >= 3 * n) return;
    const int i = q / 3, comp = q - 3 * i;
    xyz[(size_t)rep * 3 * n + q] = (double)xin[((size_t)rep * 3 + comp) * npad + i];
}

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
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) rowsum[i] = red[0];
}

// sums[k] = sum of model k's distances: its n row sums, in a fixed order
__global__ __launch_bounds__(256) void k_cmp_model_sum(const double* __restrict__ rowsum, int n, double* __restrict__ sums) {
    __shared__ double red[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double s = 0;
    for (int i = tid; i < n; i += 256) s += rowsum[(size_t)k * n + i];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
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
    const int tid = threadIdx.x, la = tid >> 4, lb = tid & 15;
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
    const int a = q / K, b = q - a * K, nb = (K + kCmpModels - 1) / kCmpModels;
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
    hipLaunchKernelGGL(k_cmp_coords, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, xin, n, npad, xyz);
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
    const int nb = (K + kCmpModels - 1) / kCmpModels, chunks = compare_table_chunks(m, K);
    const size_t per_chunk = compare_chunk_pairs(m, K);
    hipLaunchKernelGGL(k_cmp_model_sum, dim3(K), dim3(256), 0, s, rowsum, n, sums);
    hipLaunchKernelGGL(k_cmp_table, dim3(chunks, nb, nb), dim3(256), 0, s, xyz, ke, sums, n, K, m, per_chunk, partial);
    hipLaunchKernelGGL(k_cmp_table_sum, dim3((K * K + 255) / 256), dim3(256), 0, s, partial, K, chunks, table);
    return hipGetLastError();
}

// ---- the models of a run in one frame (c3d_superpose_replicas, c3d_rmsd_table) --------------------------------------------------------------
// Coordinate space, where k_cmp_* above work in distance space.  A model is n x 3 doubles, xyz interleaved, centred in place on its centroid
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

__global__ __launch_bounds__(256) void k_sup_gather64(const double* __restrict__ X, int n, int np, double* __restrict__ xyz) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n, as the output is laid out
    if (q >= 3 * n) return;
    const int i = q / 3, comp = q - 3 * i;
    xyz[(size_t)rep * 3 * n + q] = X[((size_t)rep * 3 + comp) * np + i];
}

// cent[k] = the centroid of model k; the model is centred on it in place
__global__ __launch_bounds__(256) void k_sup_centre(double* __restrict__ xyz, int n, double* __restrict__ cent) {
    __shared__ double red[3][256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double* x = xyz + (size_t)k * 3 * n;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int i = tid; i < n; i += 256) { s0 += x[3 * i]; s1 += x[3 * i + 1]; s2 += x[3 * i + 2]; }
    red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) for (int c = 0; c < 3; ++c) red[c][tid] += red[c][tid + w];
        __syncthreads();
    }
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
    const int tid = threadIdx.x, la = tid >> 4, lb = tid & 15;
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
    const int la = q / KB, b = q - la * KB, a = a0 + la, nbB = (KB + kCmpModels - 1) / kCmpModels;
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
    const int tid = threadIdx.x, la = tid >> 4, lb = tid & 15, a = a0 + la, b = blockIdx.y * kCmpModels + lb;
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
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) dev[k] = red[0];
}

// the fitted models become the replicas' coordinates: the beads 0..n-1 of the fp32 SoA (pad beads untouched), or of both fp64 buffers
__global__ __launch_bounds__(256) void k_sup_store32(const double* __restrict__ fitted, int n, int npad, float* __restrict__ X) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n
    if (q >= 3 * n) return;
    const int comp = q / n, i = q - comp * n;
    X[((size_t)rep * 3 + comp) * npad + i] = (float)fitted[((size_t)rep * n + i) * 3 + comp];
}
__global__ __launch_bounds__(256) void k_sup_store64(const double* __restrict__ fitted, int n, int np, double* __restrict__ X0, double* __restrict__ X1) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n
    if (q >= 3 * n) return;
    const int comp = q / n, i = q - comp * n;
    const double v = fitted[((size_t)rep * n + i) * 3 + comp];
    X0[((size_t)rep * 3 + comp) * np + i] = v;
    X1[((size_t)rep * 3 + comp) * np + i] = v;
}

hipError_t launch_superpose_gather64(const double* X, int n, int np, int nrep, double* xyz, hipStream_t s) {
    hipLaunchKernelGGL(k_sup_gather64, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, X, n, np, xyz);
    return hipGetLastError();
}

hipError_t launch_superpose_centre(double* xyz, int n, int K, double* cent, hipStream_t s) {
    hipLaunchKernelGGL(k_sup_centre, dim3(K), dim3(256), 0, s, xyz, n, cent);
    return hipGetLastError();
}

hipError_t launch_superpose_fit(const double* A, int KA, const double* B, int KB, int n, int ident, bool mirror, const int* fixed, double* partial,
                                double* cov, double* fit, int* mirrored, double* res, hipStream_t s) {
    const int chunks = superpose_chunks(n), nbB = (KB + kCmpModels - 1) / kCmpModels;
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
    hipLaunchKernelGGL(k_sup_store32, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, fitted, n, npad, X);
    return hipGetLastError();
}

hipError_t launch_superpose_store64(const double* fitted, int n, int np, int nrep, double* X0, double* X1, hipStream_t s) {
    hipLaunchKernelGGL(k_sup_store64, dim3((3 * n + 255) / 256, nrep), dim3(256), 0, s, fitted, n, np, X0, X1);
    return hipGetLastError();
}

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

__device__ __forceinline__ double ens_dist(double ux, double uy, double uz) {
    double q = cmp_rounded(ux * ux);
    q += cmp_rounded(uy * uy);
    q += cmp_rounded(uz * uz);
    return sqrt(q);
}

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
                const double d = ens_dist(rx[a] - cx[b], ry[a] - cy[b], rz[a] - cz[b]);
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

// out[i] = sum over j, |i-j| >= range, of (A(i, j) - ma)(B(i, j) - ma) for two rank matrices of the same pairs, k_rank_saa's order
__global__ __launch_bounds__(256) void k_ens_corr(const double* __restrict__ A, const double* __restrict__ B, int n, int range, double ma,
                                                 double* __restrict__ out) {
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double s = 0;
    for (int j = tid; j < n; j += 256) {
        const int sep = i > j ? i - j : j - i;
        if (sep < range) continue;
        s += (A[(size_t)i * n + j] - ma) * (B[(size_t)i * n + j] - ma);
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[i] = red[0];
}

hipError_t launch_ensemble_map(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact,
                               hipStream_t s) {
    const unsigned nt = (unsigned)ensemble_tiles(n);
    hipLaunchKernelGGL(k_ens_map, dim3(nt, nt), dim3(256), 0, s, xyz, n, pick, Kp, cutoff, mean, sd, contact);
    return hipGetLastError();
}

hipError_t launch_ensemble_corr(const double* A, const double* B, int n, int range, double ma, double* rows, hipStream_t s) {
    hipLaunchKernelGGL(k_ens_corr, dim3(n), dim3(256), 0, s, A, B, n, range, ma, rows);
    return hipGetLastError();
}

// ---- a model's geometry (c3d_geometry_replicas) ------------------------------------------------------------------------------------------------
// Per model: the reference's clash count (chromosome3D.pl:693-714: pairs no further apart than a cutoff), every bead's share of it and its
// nearest counted partner, the model's extent, and the chain envelope (bond and i,i+2 mean / sd, radius of gyration).  A model is n x 3
// doubles, xyz interleaved; d is ens_dist's sum and square root, so its bits are the host's.
//
// k_geo_pairs: a workgroup of 256 threads owns kGeoTile = 64 row beads of one model (blockIdx.x the row block, blockIdx.y the model) and
// walks ALL columns in staged blocks of 64, a thread a 4 x 4 grid of pairs a block, rows ty + 16 a and columns tx + 16 b as in k_ens_map.
// Every pair is thus evaluated from both sides — d(i, j) and d(j, i) have the same bits — which doubles the square roots and makes a row
// bead's count, minimum and maximum complete inside its workgroup: the sixteen threads of a row meet in LDS, nothing is added across
// workgroups and there is no global atomic.  Counts are integers, minima and maxima have no order: the results are exact.
// k_geo_model: one workgroup a model.  The per-bead counts are added (integers) and halved, the per-bead maxima give the extent, and the
// chain sums are taken as k_sup_centre takes its: thread t adds the terms t, t + 256, ... and the 256 partial sums meet in a fixed tree, an
// order that follows from n alone.  Every sd is the two-pass form: the mean first, then the squared deviations in a second walk.
constexpr int kGeoTile = 64;

__global__ __launch_bounds__(256) void k_geo_pairs(const double* __restrict__ xyz, int n, double cutoff, int sep, int* __restrict__ bead_clashes,
                                                  double* __restrict__ nearest, double* __restrict__ furthest) {
    __shared__ double R[3][kGeoTile], Cc[3][kGeoTile];
    __shared__ double smin[kGeoTile][17], smax[kGeoTile][17];
    __shared__ int scnt[kGeoTile][17];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.x * kGeoTile;
    const double* x = xyz + (size_t)blockIdx.y * 3 * n;
    for (int q = tid; q < 3 * kGeoTile; q += 256) {
        const int p = q / 3, comp = q - 3 * p;
        R[comp][p] = i0 + p < n ? x[(size_t)3 * i0 + q] : 0.0;
    }
    __syncthreads();
    double rx[4], ry[4], rz[4], mn[4], mx[4];
    int cnt[4];
    for (int a = 0; a < 4; ++a) {
        rx[a] = R[0][ty + 16 * a]; ry[a] = R[1][ty + 16 * a]; rz[a] = R[2][ty + 16 * a];
        mn[a] = __builtin_inf(); mx[a] = 0.0; cnt[a] = 0;
    }
    for (int j0 = 0; j0 < n; j0 += kGeoTile) {
        __syncthreads();                                     // the block before this one has been read
        for (int q = tid; q < 3 * kGeoTile; q += 256) {
            const int p = q / 3, comp = q - 3 * p;
            Cc[comp][p] = j0 + p < n ? x[(size_t)3 * j0 + q] : 0.0;
        }
        __syncthreads();
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tx + 16 * b;
            const double cx = Cc[0][tx + 16 * b], cy = Cc[1][tx + 16 * b], cz = Cc[2][tx + 16 * b];
            for (int a = 0; a < 4; ++a) {
                const int i = i0 + ty + 16 * a, gap = i > j ? i - j : j - i;
                const double d = ens_dist(rx[a] - cx, ry[a] - cy, rz[a] - cz);
                const bool inside = i < n && j < n, counted = inside && gap >= sep;
                cnt[a] += counted && d <= cutoff ? 1 : 0;
                mn[a] = counted && d < mn[a] ? d : mn[a];
                mx[a] = inside && d > mx[a] ? d : mx[a];
            }
        }
    }
    for (int a = 0; a < 4; ++a) { scnt[ty + 16 * a][tx] = cnt[a]; smin[ty + 16 * a][tx] = mn[a]; smax[ty + 16 * a][tx] = mx[a]; }
    __syncthreads();
    if (tid < kGeoTile && i0 + tid < n) {
        int c = 0;
        double lo = __builtin_inf(), hi = 0.0;
        for (int t = 0; t < 16; ++t) {
            c += scnt[tid][t];
            lo = smin[tid][t] < lo ? smin[tid][t] : lo;
            hi = smax[tid][t] > hi ? smax[tid][t] : hi;
        }
        const size_t o = (size_t)blockIdx.y * n + i0 + tid;
        bead_clashes[o] = c; nearest[o] = lo; furthest[o] = hi;
    }
}

// the 256 threads' partial sums in one fixed tree; every thread gets the total
__device__ __forceinline__ double geo_block_sum(double* red, double s, int tid) {
    __syncthreads();                                         // the readers of the sum before this one
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}
// mean and population sd of the n - gap distances d(i, i + gap): two walks over the same terms
__device__ __forceinline__ void geo_chain_stats(double* red, const double* __restrict__ x, int n, int gap, int tid, double* mean, double* sd) {
    const double terms = (double)(n - gap);
    double s = 0;
    for (int i = tid; i + gap < n; i += 256) s += cmp_dist(x, i, i + gap);
    const double mu = geo_block_sum(red, s, tid) / terms;
    double v = 0;
    for (int i = tid; i + gap < n; i += 256) {
        const double e = cmp_dist(x, i, i + gap) - mu;
        v += e * e;
    }
    *mean = mu;
    *sd = sqrt(geo_block_sum(red, v, tid) / terms);
}

__global__ __launch_bounds__(256) void k_geo_model(const double* __restrict__ xyz, int n, const int* __restrict__ bead_clashes,
                                                  const double* __restrict__ furthest, long long* __restrict__ clashes, double* __restrict__ chain) {
    __shared__ double red[256];
    __shared__ long long redc[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const double* x = xyz + (size_t)k * 3 * n;
    long long c = 0;
    double hi = 0.0;
    for (int i = tid; i < n; i += 256) {
        c += bead_clashes[(size_t)k * n + i];
        const double f = furthest[(size_t)k * n + i];
        hi = f > hi ? f : hi;
    }
    redc[tid] = c; red[tid] = hi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { redc[tid] += redc[tid + w]; red[tid] = red[tid + w] > red[tid] ? red[tid + w] : red[tid]; }
        __syncthreads();
    }
    const long long both_sides = redc[0];
    const double extent = red[0];
    double f[C3D_GEOMETRY_FIELDS];
    geo_chain_stats(red, x, n, 1, tid, &f[0], &f[1]);
    geo_chain_stats(red, x, n, 2, tid, &f[2], &f[3]);
    double s0 = 0, s1 = 0, s2 = 0;
    for (int i = tid; i < n; i += 256) { s0 += x[3 * i]; s1 += x[3 * i + 1]; s2 += x[3 * i + 2]; }
    const double c0 = geo_block_sum(red, s0, tid) / (double)n, c1 = geo_block_sum(red, s1, tid) / (double)n, c2 = geo_block_sum(red, s2, tid) / (double)n;
    double g = 0;
    for (int i = tid; i < n; i += 256) {
        const double u0 = x[3 * i] - c0, u1 = x[3 * i + 1] - c1, u2 = x[3 * i + 2] - c2;
        g += u0 * u0 + u1 * u1 + u2 * u2;
    }
    f[4] = sqrt(geo_block_sum(red, g, tid) / (double)n);
    f[5] = extent;
    if (tid == 0) {
        clashes[k] = both_sides / 2;
        for (int q = 0; q < C3D_GEOMETRY_FIELDS; ++q) chain[(size_t)C3D_GEOMETRY_FIELDS * k + q] = f[q];
    }
}

hipError_t launch_geometry(const double* xyz, int n, int K, double cutoff, int sep, int* bead_clashes, double* nearest, double* furthest,
                           long long* clashes, double* chain, hipStream_t s) {
    hipLaunchKernelGGL(k_geo_pairs, dim3((n + kGeoTile - 1) / kGeoTile, K), dim3(256), 0, s, xyz, n, cutoff, sep, bead_clashes, nearest, furthest);
    hipLaunchKernelGGL(k_geo_model, dim3(K), dim3(256), 0, s, xyz, n, bead_clashes, furthest, clashes, chain);
    return hipGetLastError();
}

// ---- distance against genomic separation (c3d_separation_profile) -------------------------------------------------------------------------------
// For every separation s: mean, population sd and contact share of the (n - s) Kp distances d_k(i, i + s) over the picked models — the
// diagonal averages of k_ens_map's matrices without the matrices.  The sum of one s runs along a diagonal, so a thread owns a separation:
// a workgroup of 256 threads takes kSepBlock = 64 separations s0 .. s0 + 63 and walks i in chunks of 64.  For a chunk at i0 it stages, for a
// block of kSepModels = 8 models, the 64 beads i0 .. i0 + 63 and the 127 beads i0 + s0 .. i0 + s0 + 126 they pair with (191 beads x 3 x 8
// models = 36 672 bytes, with the sums' meeting place 40 768, of the 64 KiB a launch gets without opting in); wave q of the four takes
// the beads i0 + 16 q .. i0 + 16 q + 15 and lane l the separation s0 + l: the row bead is one LDS address for the whole wave, the partners
// are consecutive doubles.  The grid is ceil(n / 64) workgroups and the diagonals near s = 0 are the longest: at 16384 beads that is one
// workgroup a CU with the first ones finishing last, about a fifth of k_geo_pairs' pair rate (profiles/r22_geometry.txt).  A thread keeps
// its sum (and its 64-bit contact count) in registers across all chunks and models — chunks ascending, models in list order within a chunk —
// and the four waves' sums of a separation are added in wave order at the end: an order fixed by n and Kp, no atomics.  The sd needs the
// finished mean of the whole diagonal, so it is a second launch of the same walk (SECOND) that sums squared deviations from mean[s].
// s = 0 needs no special case: d(i, i) = 0 gives mean 0, sd 0 and, 0 being < every accepted cutoff, contact 1.
constexpr int kSepBlock = 64;
constexpr int kSepModels = 8;
constexpr int kSepBeads = 3 * kSepBlock - 1;                 // 64 row beads, then 127 partners

template <bool SECOND>
__global__ __launch_bounds__(256) void k_sep_profile(const double* __restrict__ xyz, int n, const int* __restrict__ pick, int Kp, double cutoff,
                                                    double* __restrict__ mean, double* __restrict__ out) {
    __shared__ double lds[kSepModels][3][kSepBeads];
    __shared__ double red[4][kSepBlock];
    __shared__ long long redc[4][kSepBlock];
    const int tid = threadIdx.x, ls = tid & (kSepBlock - 1), q = tid >> 6;
    const int s0 = blockIdx.x * kSepBlock, s = s0 + ls;
    const double mu = SECOND && s < n ? mean[s] : 0.0;
    double acc = 0;
    long long cnt = 0;
    for (int i0 = 0; i0 + s0 < n; i0 += kSepBlock)
        for (int m0 = 0; m0 < Kp; m0 += kSepModels) {
            const int mc = Kp - m0 < kSepModels ? Kp - m0 : kSepModels;
            __syncthreads();                                 // the block before this one has been read
            // lds[m][comp][p] = coordinate comp of bead (p < 64 ? i0 + p : i0 + s0 + p - 64) of model pick[m0 + m]; 0 beyond bead n - 1
            for (int w = tid; w < mc * 3 * kSepBeads; w += 256) {
                const int m = w / (3 * kSepBeads), e = w - m * (3 * kSepBeads), p = e / 3, comp = e - 3 * p;
                const int bead = p < kSepBlock ? i0 + p : i0 + s0 + p - kSepBlock;
                lds[m][comp][p] = bead < n ? xyz[(size_t)pick[m0 + m] * 3 * n + (size_t)3 * bead + comp] : 0.0;
            }
            __syncthreads();
            for (int m = 0; m < mc; ++m)
                for (int t = 0; t < 16; ++t) {
                    const int ii = 16 * q + t;
                    if (i0 + ii + s >= n) break;             // the partner is past the chain's end, and so are those of the beads after ii
                    const double d = ens_dist(lds[m][0][ii] - lds[m][0][kSepBlock + ii + ls], lds[m][1][ii] - lds[m][1][kSepBlock + ii + ls],
                                              lds[m][2][ii] - lds[m][2][kSepBlock + ii + ls]);
                    if (!SECOND) {
                        acc += d;
                        cnt += d < cutoff ? 1 : 0;
                    } else {
                        const double e = d - mu;
                        acc += e * e;
                    }
                }
        }
    red[q][ls] = acc; redc[q][ls] = cnt;
    __syncthreads();
    if (q == 0 && s < n) {
        const double total = ((red[0][ls] + red[1][ls]) + red[2][ls]) + red[3][ls];
        const double terms = (double)((long long)(n - s) * Kp);
        if (!SECOND) {
            mean[s] = total / terms;
            if (out) out[s] = (double)(((redc[0][ls] + redc[1][ls]) + redc[2][ls]) + redc[3][ls]) / terms;
        } else {
            out[s] = sqrt(total / terms);
        }
    }
}

hipError_t launch_separation_profile(const double* xyz, int n, const int* pick, int Kp, double cutoff, double* mean, double* sd, double* contact,
                                     hipStream_t s) {
    const dim3 grid((n + kSepBlock - 1) / kSepBlock);
    hipLaunchKernelGGL(k_sep_profile<false>, grid, dim3(256), 0, s, xyz, n, pick, Kp, cutoff, mean, contact);
    if (sd) hipLaunchKernelGGL(k_sep_profile<true>, grid, dim3(256), 0, s, xyz, n, pick, Kp, cutoff, mean, sd);
    return hipGetLastError();
}

hipError_t preload_score_unit() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_score_round));
}

}  // namespace c3d
