// c3d_score_stratified.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- IF against model distance inside every genomic separation (c3d_stratified_score) ---------------------------------------------------------
// Stratum s holds the N = n - s pairs (i, i + s).  Inside it IF and the "%.3f" distance are ranked on their own and the DOUBLED average
// ranks a_i, b_i = #{smaller} + #{not larger} + 1 are integers, so the stratum's three sums
//     C = N sum a b - T^2,   A = N sum a^2 - T^2,   B = N sum b^2 - T^2,   T = N (N + 1)
// are exact in 64 bits (4 N^4 < 2.9e17 at N = 16383): no summation order, no tolerance, no atomics.  The host divides (c3d_analysis.cpp).
//
// k_str_if, one workgroup a stratum: the N rank_keys of IF(i, i + s) — 64-bit, padded with the largest key to P = str_slots(N) — are sorted
// in LDS, every element finds its tie group's bounds k, e by two binary searches (as k_rank_assign does) and a_i = k + e + 1 goes, as
// uint32, into a packed diagonal-major array (stratum lo first; str_offset) with sum a^2 beside it.  IF(i + s, i) is read once to hold the
// matrix to its symmetry; a mismatch raises flags[0], a non-finite value flags[1] (plain stores of 1: every writer writes the same).
// flags[3]: the ranks of a stratum did not add up to N (N + 1), which no input can cause.
// The diagonal of a row-major matrix is read uncoalesced, three times a stratum (both triangles, then the upper one again for the lookup:
// the sort keeps no index, and at N = 16383 the keys fill the LDS); not staged, see DESIGN.md K6.
// k_str_model, one workgroup a (stratum, model): the N distances are recomputed from the gathered model (cmp_dist: the host's bits) and
// rounded (round_milli_dev) to uint32 thousandths — 50 000 A is 5e7, the pad 0xFFFFFFFF, anything wider or not a number raises flags[2] —
// sorted in LDS, b_i looked up, a_i read, and sum a b and sum b^2 go through block_reduce in int64.  Thread 0 writes C, A, B.
//
// The network (str_sort) is bitonic over P keys, P a power of two >= kStrMinSlots, kStrThreads = 256 threads.  A stage's strides >= kStrChunk
// = 4 keys are LDS passes in which a thread moves 16-byte vectors (4 keys of 32 bits, 2 of 64: ds_read_b128 / ds_write_b128, a quarter or
// half of the LDS instructions of a key-at-a-time pass); its strides 2 and 1 run in registers on the 4 consecutive keys a thread loads
// as 16 or 32 bytes, so the passes a textbook network pays a two-way bank conflict for at every access (strides 1 and 2) have none and
// cost one barrier, not two.  What is left: the vector passes at strides 4 .. 32 keys, where a wave's vectors are not contiguous, are
// conflicted (not profiled).  A thread owns more than one comparator vector from P = 4096 (32-bit) or 2048 (64-bit) keys on, more than
// one chunk from P = 2048.  Only the set of sorted keys matters to the result, so none of this changes a bit of it.
// Launches are grouped by P (str_launch_classes): the strata with N in (P / 2, P] are one launch with P keys of dynamic LDS, so a short
// stratum does not hold the LDS of the longest.  Above 64 KiB (less the reduction's static scratch) a launch needs the allowance
// preload_score_unit sets when the unit loads.
constexpr int kStrThreads = 256;
constexpr int kStrChunk = 4;
constexpr int kStrMinSlots = 8;
constexpr unsigned kStrPad32 = 0xFFFFFFFFu;
constexpr long long kStrFarthest = 50000000;                 // thousandths of an A: the limit of c3d_score_replicas and of the host twin

__host__ __device__ inline int str_slots(int N) {
    int P = kStrMinSlots;
    while (P < N) P <<= 1;
    return P;
}
// where stratum s begins in the packed array of a_i: strata lo .. s - 1 hold n - lo, n - lo - 1, ... values
__host__ __device__ inline size_t str_offset(int s, int lo, int n) {
    return (size_t)(s - lo) * (size_t)n - ((size_t)s * (size_t)(s - 1) / 2 - (size_t)lo * (size_t)(lo - 1) / 2);
}

template <typename K>
__device__ __forceinline__ void str_cx(K& x, K& y, bool up) {
    if ((x > y) == up) { const K t = x; x = y; y = t; }
}
template <typename K>
struct alignas(16) StrVec { K k[16 / sizeof(K)]; };

template <typename K>
__device__ __forceinline__ void str_sort(K* __restrict__ t, int P, int tid) {
    constexpr int V = 16 / sizeof(K);
    static_assert(V <= kStrChunk && kStrMinSlots >= 2 * kStrChunk, "a vector lies inside one side of every LDS pass's comparators");
    for (int size = kStrChunk; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride >= kStrChunk; stride >>= 1) {
            for (int q = tid; q < P / 2 / V; q += kStrThreads) {
                const int p = q * V, lo = p & (stride - 1), a = ((p - lo) << 1) | lo, b = a | stride;
                const bool up = (a & size) == 0;
                StrVec<K> x = *reinterpret_cast<const StrVec<K>*>(t + a), y = *reinterpret_cast<const StrVec<K>*>(t + b);
                for (int v = 0; v < V; ++v) str_cx(x.k[v], y.k[v], up);
                *reinterpret_cast<StrVec<K>*>(t + a) = x;
                *reinterpret_cast<StrVec<K>*>(t + b) = y;
            }
            __syncthreads();
        }
        for (int c = tid; c < P / kStrChunk; c += kStrThreads) {
            K* const w = t + kStrChunk * c;
            StrVec<K> x[kStrChunk / V];
            for (int v = 0; v < kStrChunk / V; ++v) x[v] = reinterpret_cast<const StrVec<K>*>(w)[v];
            K k0 = x[0].k[0], k1 = x[1 / V].k[1 % V], k2 = x[2 / V].k[2 % V], k3 = x[3 / V].k[3 % V];
            if (size == kStrChunk) { str_cx(k0, k1, true); str_cx(k2, k3, false); }       // the stage of size 2
            const bool up = ((kStrChunk * c) & size) == 0;
            str_cx(k0, k2, up); str_cx(k1, k3, up);
            str_cx(k0, k1, up); str_cx(k2, k3, up);
            x[0].k[0] = k0; x[1 / V].k[1 % V] = k1; x[2 / V].k[2 % V] = k2; x[3 / V].k[3 % V] = k3;
            for (int v = 0; v < kStrChunk / V; ++v) reinterpret_cast<StrVec<K>*>(w)[v] = x[v];
        }
        __syncthreads();
    }
}

// first position in t[lo..hi) whose key is not below `key`
template <typename K>
__device__ __forceinline__ int str_lower_bound(const K* __restrict__ t, int lo, int hi, K key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (t[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the doubled average rank of `key` among the N sorted keys t[0..N): #{smaller} + #{not larger} + 1.  No key of a stratum is the largest
// value of K (a pad; such an IF is not finite and such a distance too far, and both are refused), so key + 1 does not wrap.
template <typename K>
__device__ __forceinline__ long long str_rank2(const K* __restrict__ t, int N, K key) {
    const int k = str_lower_bound(t, 0, N, key);
    const int e = str_lower_bound(t, k, N, (K)(key + 1));
    return (long long)k + (long long)e + 1;
}

extern __shared__ __align__(16) unsigned char str_lds[];

__global__ __launch_bounds__(kStrThreads) void k_str_if(const double* __restrict__ IF, int n, int lo, int s_first, int P, unsigned* __restrict__ a_out,
                                                        long long* __restrict__ saa, int* __restrict__ flags) {
    __shared__ long long red[2 * 256];
    unsigned long long* const t = reinterpret_cast<unsigned long long*>(str_lds);
    const int tid = threadIdx.x, s = s_first + blockIdx.x, N = n - s;
    for (int i = tid; i < P; i += kStrThreads) {
        unsigned long long key = ~0ull;
        if (i < N) {
            const double v = IF[(size_t)i * n + i + s], w = IF[(size_t)(i + s) * n + i];
            if (!(v == w)) flags[0] = 1;
            if (!(fabs(v) <= 1.7976931348623157e308) || !(fabs(w) <= 1.7976931348623157e308)) flags[1] = 1;
            key = rank_key(v);
        }
        t[i] = key;
    }
    __syncthreads();
    str_sort(t, P, tid);
    unsigned* const a_row = a_out + str_offset(s, lo, n);
    long long sa = 0, s1 = 0;
    for (int i = tid; i < N; i += kStrThreads) {
        const long long a = str_rank2(t, N, rank_key(IF[(size_t)i * n + i + s]));
        a_row[i] = (unsigned)a;
        sa += a * a;
        s1 += a;
    }
    // The doubled average ranks of N values add up to N (N + 1) whatever the ties: the stratum checks its own sort and lookup, and
    // flags[3] is an internal error on the host.  (It also keeps this reduction an instantiation of its own: sharing k_geo_model's
    // one-value int64 one changes the order in which the compiler inlines it there, and with it two instructions of that kernel.)
    block_reduce(red, {sa, s1}, tid, RedSum());
    if (tid == 0) {
        saa[s - lo] = red[0];
        if (red[256] != (long long)N * (N + 1)) flags[3] = 1;       // (also beside flags[1]: a NaN's key may be the pad's; the host names [1] first)
    }
}

// the "%.3f" distance of beads i, j in thousandths; *far: it is beyond kStrFarthest or not a number (the key is then kStrFarthest)
__device__ __forceinline__ unsigned str_dist_key(const double* __restrict__ x, int i, int j, bool* far) {
    const double d = cmp_dist(x, i, j);
    long long q = kStrFarthest + 1;
    if (d < 60000.0) q = round_milli_dev(d);
    if (q > kStrFarthest) { *far = true; q = kStrFarthest; }
    return (unsigned)q;
}

__global__ __launch_bounds__(kStrThreads) void k_str_model(const double* __restrict__ xyz, int n, int lo, int s_first, int P, const unsigned* __restrict__ a_in,
                                                           const long long* __restrict__ saa, long long* __restrict__ sums, int* __restrict__ flags) {
    __shared__ long long red[2 * 256];
    unsigned* const t = reinterpret_cast<unsigned*>(str_lds);
    const int tid = threadIdx.x, s = s_first + blockIdx.x, k = blockIdx.y, N = n - s;
    const double* x = xyz + (size_t)k * 3 * n;
    bool far = false;
    for (int i = tid; i < P; i += kStrThreads) t[i] = i < N ? str_dist_key(x, i, i + s, &far) : kStrPad32;
    if (far) flags[2] = 1;
    __syncthreads();
    str_sort(t, P, tid);
    const unsigned* const a_row = a_in + str_offset(s, lo, n);
    long long sab = 0, sbb = 0;
    for (int i = tid; i < N; i += kStrThreads) {
        const long long b = str_rank2(t, N, str_dist_key(x, i, i + s, &far));
        sab += (long long)a_row[i] * b;
        sbb += b * b;
    }
    block_reduce(red, {sab, sbb}, tid, RedSum());
    if (tid == 0) {
        const long long Nl = N, T = Nl * (Nl + 1);
        long long* const out = sums + ((size_t)k * n + s) * C3D_STRATUM_FIELDS;
        out[0] = Nl * red[0] - T * T;
        out[1] = Nl * saa[s - lo] - T * T;
        out[2] = Nl * red[256] - T * T;
    }
}

// calls f(s_first, count, P) for every group of strata lo <= s <= hi that sort P keys: N = n - s in (P / 2, P], or 1 .. kStrMinSlots
template <typename F>
static void str_launch_classes(int n, int lo, int hi, F f) {
    for (int s = lo; s <= hi;) {
        const int P = str_slots(n - s);
        const int n_last = P == kStrMinSlots ? 1 : P / 2 + 1;        // the shortest stratum of this class
        const int s_last = n - n_last < hi ? n - n_last : hi;
        f(s, s_last - s + 1, P);
        s = s_last + 1;
    }
}

hipError_t launch_stratified_if(const double* IF, int n, int lo, int hi, unsigned* a, long long* saa, int* flags, hipStream_t s) {
    hipError_t e = hipMemsetAsync(flags, 0, sizeof(int) * kStrFlags, s);
    if (e != hipSuccess) return e;
    str_launch_classes(n, lo, hi, [&](int s_first, int count, int P) {
        hipLaunchKernelGGL(k_str_if, dim3(count), dim3(kStrThreads), sizeof(unsigned long long) * (size_t)P, s, IF, n, lo, s_first, P, a, saa, flags);
    });
    return hipGetLastError();
}

hipError_t launch_stratified_models(const double* xyz, int n, int K, int lo, int hi, const unsigned* a, const long long* saa, long long* sums, int* flags,
                                    hipStream_t s) {
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(long long) * C3D_STRATUM_FIELDS * (size_t)n * K, s);
    if (e != hipSuccess) return e;
    str_launch_classes(n, lo, hi, [&](int s_first, int count, int P) {
        hipLaunchKernelGGL(k_str_model, dim3(count, K), dim3(kStrThreads), sizeof(unsigned) * (size_t)P, s, xyz, n, lo, s_first, P, a, saa, sums, flags);
    });
    return hipGetLastError();
}

// the dynamic LDS of the longest stratum a context accepts (16384 keys): set once when the unit loads (preload_score_unit), never beside a launch
// (k_sim_stratum: c3d_score_mapsim.inc, the same network over two maps' smoothed values)
__global__ void k_sim_stratum(const double* __restrict__ band, int n, int n_maps, int lo, int hi, int s_first, int P, int keep_zeros, double* __restrict__ moments,
                              long long* __restrict__ counts);
static hipError_t str_prepare_unit() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_str_if), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned long long) * 16384));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_str_model), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned) * 16384));
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sim_stratum), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned long long) * 16384));
    return e;
}
