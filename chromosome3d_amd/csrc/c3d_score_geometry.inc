// c3d_score_geometry.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- a model's geometry (c3d_geometry_replicas) ------------------------------------------------------------------------------------------------
// Per model: the reference's clash count (chromosome3D.pl:693-714: pairs no further apart than a cutoff), every bead's share of it and its
// nearest counted partner, the model's extent, and the chain envelope (bond and i,i+2 mean / sd, radius of gyration).  A model is n x 3
// doubles, xyz interleaved; d is dist3's sum and square root, so its bits are the host's.
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
                const double d = dist3(rx[a] - cx, ry[a] - cy, rz[a] - cz);
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

// mean and population sd of the n - gap distances d(i, i + gap): two walks over the same terms
__device__ __forceinline__ void geo_chain_stats(double* red, const double* __restrict__ x, int n, int gap, int tid, double* mean, double* sd) {
    const double terms = (double)(n - gap);
    double s = 0;
    for (int i = tid; i + gap < n; i += 256) s += cmp_dist(x, i, i + gap);
    const double mu = block_reduce(red, {s}, tid, RedSum(), true) / terms;
    double v = 0;
    for (int i = tid; i + gap < n; i += 256) {
        const double e = cmp_dist(x, i, i + gap) - mu;
        v += e * e;
    }
    *mean = mu;
    *sd = sqrt(block_reduce(red, {v}, tid, RedSum(), true) / terms);
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
    const long long both_sides = block_reduce(redc, {c}, tid, RedSum());
    const double extent = block_reduce(red, {hi}, tid, RedGreater());
    double f[C3D_GEOMETRY_FIELDS];
    geo_chain_stats(red, x, n, 1, tid, &f[0], &f[1]);
    geo_chain_stats(red, x, n, 2, tid, &f[2], &f[3]);
    double s0 = 0, s1 = 0, s2 = 0;
    for (int i = tid; i < n; i += 256) { s0 += x[3 * i]; s1 += x[3 * i + 1]; s2 += x[3 * i + 2]; }
    const double c0 = block_reduce(red, {s0}, tid, RedSum(), true) / (double)n, c1 = block_reduce(red, {s1}, tid, RedSum(), true) / (double)n, c2 = block_reduce(red, {s2}, tid, RedSum(), true) / (double)n;
    double g = 0;
    for (int i = tid; i < n; i += 256) {
        const double u0 = x[3 * i] - c0, u1 = x[3 * i + 1] - c1, u2 = x[3 * i + 2] - c2;
        g += u0 * u0 + u1 * u1 + u2 * u2;
    }
    f[4] = sqrt(block_reduce(red, {g}, tid, RedSum(), true) / (double)n);
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
                    const double d = dist3(lds[m][0][ii] - lds[m][0][kSepBlock + ii + ls], lds[m][1][ii] - lds[m][1][kSepBlock + ii + ls],
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
