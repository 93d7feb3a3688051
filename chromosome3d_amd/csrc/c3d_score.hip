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
//
// The unit, one translation unit and one code object (UNIT_SCORE, preload_score_unit):
//   c3d_score_core.h          what the families share: the block reduction every fixed-order sum goes through, "%.3f" rounding, the pair
//                             distance, the sort keys and their network, the two layouts of a model's coordinates
//   c3d_score.hip             k_score_*  K6 scoring (above)                          k_rank_*  the IF ranks, and k_row_corr
//   c3d_score_compare.inc     k_cmp_*    the models of a run against one another, in distance space (c3d_compare_replicas)
//   c3d_score_superpose.inc   k_sup_*    the models in one frame (c3d_superpose_replicas, c3d_rmsd_table)
//   c3d_score_ensemble.inc    k_ens_*    mean, spread and contact frequency of every pair distance over the models, and the rank correlation
//                             of those maps with IF (c3d_ensemble_map, c3d_ensemble_score)
//   c3d_score_geometry.inc    k_geo_*    a model's clash count, nearest partners and chain envelope (c3d_geometry_replicas);
//                             k_sep_*    the distance against the genomic separation (c3d_separation_profile)
//   c3d_score_stratified.inc  k_str_*    IF against model distance inside every genomic separation: one LDS sort a (stratum, model) and
//                             integer sums (c3d_stratified_score)
//   c3d_score_bead.inc        k_bead_*   the same ranking inside every row of IF — a Spearman coefficient a bead — and the reference's
//                             restraint tallies a bead (c3d_bead_scores)
//   c3d_score_access.inc      k_access   a bead's exposed surface: a neighbour search in LDS feeding point-in-sphere tests (c3d_accessibility)
//   c3d_score_compartment.inc k_cpt_*    compartment eigenvectors: the O/E map of IF, a model or the consensus, and orthogonal iteration on the
//                             correlation of its rows through matrix-vector products with the map (c3d_compartments)
//   c3d_score_insulation.inc  k_ins_*    insulation profiles and domain boundaries: a banded all-pairs sum a bead, the tile's distances staged
//                             in LDS, every window out of one walk over nested squares (c3d_insulation)
//   c3d_score_balance.inc     k_bal_*    the input side: a raw contact matrix balanced by ICE, VC or sqrt-VC, one streaming matrix-vector pass
//                             a round, the stop decided on the device (c3d_balance_matrix)
//   c3d_score_loop.inc        k_loop_*   loop enrichment: a pixel's four local-background ratios out of one walk over its window, IF's tiles
//                             staged in LDS, peaks by exact suppression, listed pixels in every map and their pile-up (c3d_loops)
//   c3d_score_entangle.inc    k_ent_*    entanglement: the Gauss integral of every pair of chain segments as two atan2, summed a segment, a
//                             model and a pair of domains — writhe, average crossing number, linking (c3d_entanglement)
//   c3d_score_mapsim.inc      k_sim_*    the input side: two contact maps against one another, HiCRep's stratum-adjusted coefficient — a clipped box
//                             mean over the band staged in LDS, then a masked Pearson and two LDS sorts a (stratum, pair) (c3d_map_similarity)
#include "c3d_score_core.h"

namespace c3d {

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
    block_reduce(&red[0][0], {sab, sbb, sat, dev}, tid, RedSum());
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
    block_reduce(lo, {a}, tid, RedMin());
    block_reduce(hi, {b}, tid, RedMax());
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

// out[i] = sum over j, |i-j| >= range, of (A(i, j) - ma)(B(i, j) - ma) for two rank matrices of the same pairs, summed in a fixed order.
// The IF side's sum of squares is the case A = B: (M - ma)(M - ma) has the bits of d * d.
__global__ __launch_bounds__(256) void k_row_corr(const double* __restrict__ A, const double* __restrict__ B, int n, int range, double ma,
                                                 double* __restrict__ out) {
    __shared__ double red[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    double s = 0;
    for (int j = tid; j < n; j += 256) {
        const int sep = i > j ? i - j : j - i;
        if (sep < range) continue;
        s += (A[(size_t)i * n + j] - ma) * (B[(size_t)i * n + j] - ma);
    }
    block_reduce(red, {s}, tid, RedSum());
    if (tid == 0) out[i] = red[0];
}

hipError_t launch_if_rank_keys(const double* M, int n, int range, unsigned long long* keys, size_t mh, size_t slots, int* asym, hipStream_t s) {
    hipError_t e = hipMemsetAsync(asym, 0, sizeof(int), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rank_keys, dim3(n), dim3(256), 0, s, M, n, range, keys, mh, slots, asym);
    return hipGetLastError();
}

hipError_t launch_if_rank_sort(double* M, int n, int range, unsigned long long* keys, size_t mh, size_t slots, double ma, double* saa_rows,
                               hipStream_t s) {
    launch_rank_sort_network(keys, slots, s);
    hipLaunchKernelGGL(k_rank_assign, dim3(n), dim3(256), 0, s, M, n, range, keys, mh);
    hipLaunchKernelGGL(k_row_corr, dim3(n), dim3(256), 0, s, M, M, n, range, ma, saa_rows);
    return hipGetLastError();
}

#include "c3d_score_compare.inc"
#include "c3d_score_superpose.inc"
#include "c3d_score_ensemble.inc"
#include "c3d_score_geometry.inc"
#include "c3d_score_stratified.inc"
#include "c3d_score_bead.inc"
#include "c3d_score_access.inc"
#include "c3d_score_compartment.inc"
#include "c3d_score_insulation.inc"
#include "c3d_score_balance.inc"
#include "c3d_score_loop.inc"
#include "c3d_score_entangle.inc"
#include "c3d_score_mapsim.inc"

// loads the unit's code object on the current device and gives the k_str_*, k_sim_stratum and k_bead_* kernels their dynamic-LDS allowance (c3d_gate.cpp "code objects":
// once per device, never beside a launch)
hipError_t preload_score_unit() {
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k_score_round));
    if (e != hipSuccess) return e;
    const hipError_t es = str_prepare_unit();
    return es == hipSuccess ? bead_prepare_unit() : es;
}

}  // namespace c3d
