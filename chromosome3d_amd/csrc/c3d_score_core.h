// c3d_score_core.h — what the kernel families of the scoring unit share (c3d_score.hip and its c3d_score_*.inc): the block reduction, the
// "%.3f" rounding, the pair distance, the sort keys and their network, and the two layouts of a model's coordinates.  Device code only.
#pragma once
#include "c3d_internal.h"

namespace c3d {

// ---- the block reduction ------------------------------------------------------------------------------------------------------------------
// Every "fixed tree" of this unit is this one.  A workgroup of 256 threads, C values a thread; value c of thread t goes to red[c * 256 + t]
// (red: C x 256 of T in LDS) and the levels run at strides w = 128, 64, ... 1:
//     if (t < w) red[t] = op(red[t], red[t + w])        with the operands in that order, the C values of a level one after the other
// with one barrier after the stores and one after every level, so that every thread may read the results — red[c * 256] — afterwards, and
// block_reduce returns the first of them.  `lead` puts a barrier before the stores: for a caller whose red still has readers (the sum
// before this one).  The order of every sum follows from the thread that brought each term and from nothing else: no atomics, the same
// terms give the same bits on every call.  That promise, made in the comment of every family, rests on this function.
struct RedSum { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct RedMin { __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); } };
struct RedMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };
struct RedGreater { __device__ __forceinline__ double operator()(double a, double b) const { return b > a ? b : a; } };

template <int C, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T* red, const T (&v)[C], int tid, Op op, bool lead = false) {
    if (lead) __syncthreads();
    for (int c = 0; c < C; ++c) red[c * 256 + tid] = v[c];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) for (int c = 0; c < C; ++c) red[c * 256 + tid] = op(red[c * 256 + tid], red[c * 256 + tid + w]);
        __syncthreads();
    }
    return red[0];
}

// ---- "%.3f" ---------------------------------------------------------------------------------------------------------------------------------
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

// ---- the distance of two beads of a model ---------------------------------------------------------------------------------------------------
// The distance has the bits of the host's: ((ux ux) + uy uy) + uz uz with every operation rounded on its own, then sqrt.  This unit is
// compiled with -ffp-contract=fast, which lets the instruction selector fuse any product into the sum that uses it whatever a pragma says
// of the source (and makes __dmul_rn / __dadd_rn plain * and +): each product therefore passes through an empty asm statement, which
// costs no instruction and leaves the selector a register, not a multiplication, to add.
__device__ __forceinline__ double cmp_rounded(double t) {
    asm("" : "+v"(t));
    return t;
}
__device__ __forceinline__ double dist3(double ux, double uy, double uz) {
    double q = cmp_rounded(ux * ux);
    q += cmp_rounded(uy * uy);
    q += cmp_rounded(uz * uz);
    return sqrt(q);
}
// beads i and j of a model of n x 3 doubles, xyz interleaved
__device__ __forceinline__ double cmp_dist(const double* __restrict__ x, int i, int j) {
    return dist3(x[3 * i] - x[3 * j], x[3 * i + 1] - x[3 * j + 1], x[3 * i + 2] - x[3 * j + 2]);
}

// ---- sort keys and their network (the IF ranks and the models' distance ranks) ---------------------------------------------------------------
__device__ __forceinline__ unsigned long long rank_key(double d) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    if ((u << 1) == 0) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// first key of row i in the key array: rows 0..i-1 hold w, w-1, ... keys (w = n - range)
__device__ __forceinline__ size_t rank_row_offset(int i, int w) { return (size_t)i * w - (size_t)i * (i - 1) / 2; }

// first position in keys[0..mh) whose key is not below `key`
__device__ __forceinline__ size_t rank_lower_bound(const unsigned long long* __restrict__ keys, size_t lo, size_t hi, unsigned long long key) {
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(1024) void k_rank_sort_tile(unsigned long long* __restrict__ keys, size_t size_first, size_t size_last);
__global__ __launch_bounds__(256) void k_rank_sort_step(unsigned long long* __restrict__ keys, size_t size, size_t stride);

// the network over `slots` keys (kernels: c3d_score.hip): what launch_if_rank_sort and launch_compare_ranks both sort with
static void launch_rank_sort_network(unsigned long long* keys, size_t slots, hipStream_t s) {
    const unsigned tiles = (unsigned)(slots / kRankTile), step_blocks = (unsigned)(slots / 2 / 256);
    hipLaunchKernelGGL(k_rank_sort_tile, dim3(tiles), dim3(1024), 0, s, keys, (size_t)2, (size_t)kRankTile);
    for (size_t size = 2 * (size_t)kRankTile; size <= slots; size <<= 1) {
        for (size_t stride = size >> 1; stride >= (size_t)kRankTile; stride >>= 1)
            hipLaunchKernelGGL(k_rank_sort_step, dim3(step_blocks), dim3(256), 0, s, keys, size, stride);
        hipLaunchKernelGGL(k_rank_sort_tile, dim3(tiles), dim3(1024), 0, s, keys, size, size);
    }
}

// ---- the two layouts of a model set ----------------------------------------------------------------------------------------------------------
// The state keeps a replica as [3][np] (floats, or doubles on a precision-64 context); the model-set families read a model as n x 3 doubles,
// xyz interleaved.  k_models_gather: state -> models, every value as it is (a float widened); k_models_scatter: models -> beads 0..n-1 of the
// state (pad beads untouched), a double narrowed to T, into X0 and, unless it is null, X1 (both fp64 buffers).
template <typename T>
__global__ __launch_bounds__(256) void k_models_gather(const T* __restrict__ X, int n, int np, double* __restrict__ xyz) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n, as the output is laid out
    if (q >= 3 * n) return;
    const int i = q / 3, comp = q - 3 * i;
    xyz[(size_t)rep * 3 * n + q] = (double)X[((size_t)rep * 3 + comp) * np + i];
}
template <typename T>
__global__ __launch_bounds__(256) void k_models_scatter(const double* __restrict__ xyz, int n, int np, T* __restrict__ X0, T* __restrict__ X1) {
    const int rep = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;    // over 3*n
    if (q >= 3 * n) return;
    const int comp = q / n, i = q - comp * n;
    const T v = (T)xyz[((size_t)rep * n + i) * 3 + comp];
    X0[((size_t)rep * 3 + comp) * np + i] = v;
    if (X1) X1[((size_t)rep * 3 + comp) * np + i] = v;
}

}  // namespace c3d
