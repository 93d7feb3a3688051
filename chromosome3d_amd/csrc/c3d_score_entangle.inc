// c3d_score_entangle.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- entanglement of a model (c3d_entanglement) ---------------------------------------------------------------------------------------------
// The Gauss double integral over two straight segments s and t of a chain is the signed solid angle, over 4 pi, of the planar parallelogram
// {p_t - p_s} seen from the origin; it is split into the triangles (a, b, c) and (a, d, b) of the four bead-to-bead vectors
//     a = x[t] - x[s]    c = x[t+1] - x[s]    d = x[t] - x[s+1]    b = x[t+1] - x[s+1]
// and a triangle's solid angle is Van Oosterom and Strackee's 2 atan2(u . (v x w), |u||v||w| + (u.v)|w| + (u.w)|v| + (v.w)|u|).  ent_pair
// returns atan2_1 + atan2_2, that is 2 pi g(s, t): the sums below are divided by 2 pi once, at their end.  The four lengths (dist3: the
// host's bits), a . b and the normal m = a x b are formed once and serve both triangles: a . (b x c) = c . m and a . (d x b) = -(d . m),
// the triple product turned, which is zero with the definition's whenever one of the four vectors is.  Under a mirror (one coordinate
// negated) both numerators change sign exactly and the denominators keep their bits, whatever the compiler contracts; atan2 is odd in its
// first argument, so the signed sums negate bit for bit and the absolute ones stay.  A triangle with numerator 0 and denominator 0 gives 0.
//
// k_ent_pairs: k_geo_pairs' tiling.  A workgroup of 256 threads owns kEntTile = 64 row segments of one model (blockIdx.x the row block,
// blockIdx.y the model) and walks the column segments in staged blocks of 64 — 65 beads, as segments share beads — a thread a 4 x 4 grid of
// pairs a block, rows ty + 16 a and columns tx + 16 b.  Every pair is evaluated from both sides (g(s, t) and g(t, s) agree to rounding
// only), so a row segment's two sums are complete inside its workgroup: a thread adds its counted pairs in the order of the walk (column
// blocks ascending, b, then a), the sixteen threads of a row meet in LDS and are added in index order.  Only the column blocks that hold a
// counted pair of the tile are walked, which follows from n, min_sep and max_sep; uncounted pairs add nothing (not a zero).
// k_ent_model: one workgroup a model; thread t adds the rows t, t + 256, ... and the 256 partial sums meet in block_reduce's tree.
// k_ent_table: one workgroup a (model, p, q >= p) block of the domain table; thread t takes the block's pairs t, t + 256, ... in row-major
// order (s in domain p, t in domain q), block_reduce closes the sum, and the workgroup writes (p, q) and (q, p): symmetric bit for bit.
// No floating-point atomics anywhere: every sum's order follows from n, min_sep, max_sep and bounds.
constexpr int kEntTile = 64;
constexpr double kEntTwoPi = 6.283185307179586476925286766559;

__device__ __forceinline__ double ent_half_angle(double num, double den) { return (num == 0.0 && den == 0.0) ? 0.0 : atan2(num, den); }

// 2 pi g(s, t) for the row segment p0 -> p1 and the column segment q0 -> q1
__device__ __forceinline__ double ent_pair(double p0x, double p0y, double p0z, double p1x, double p1y, double p1z, double q0x, double q0y, double q0z,
                                           double q1x, double q1y, double q1z) {
    const double ax = q0x - p0x, ay = q0y - p0y, az = q0z - p0z;
    const double cx = q1x - p0x, cy = q1y - p0y, cz = q1z - p0z;
    const double dx = q0x - p1x, dy = q0y - p1y, dz = q0z - p1z;
    const double bx = q1x - p1x, by = q1y - p1y, bz = q1z - p1z;
    const double la = dist3(ax, ay, az), lb = dist3(bx, by, bz), lc = dist3(cx, cy, cz), ld = dist3(dx, dy, dz);
    const double mx = ay * bz - az * by, my = az * bx - ax * bz, mz = ax * by - ay * bx;       // a x b
    const double ab = ax * bx + ay * by + az * bz;
    const double ac = ax * cx + ay * cy + az * cz, bc = bx * cx + by * cy + bz * cz;
    const double ad = ax * dx + ay * dy + az * dz, db = dx * bx + dy * by + dz * bz;
    const double num1 = cx * mx + cy * my + cz * mz;                                            // a . (b x c)
    const double num2 = -(dx * mx + dy * my + dz * mz);                                         // a . (d x b)
    const double den1 = la * lb * lc + ab * lc + ac * lb + bc * la;
    const double den2 = la * ld * lb + ad * lb + ab * ld + db * la;
    return ent_half_angle(num1, den1) + ent_half_angle(num2, den2);
}

__global__ __launch_bounds__(256) void k_ent_pairs(const double* __restrict__ xyz, int n, int min_sep, int max_sep, double* __restrict__ seg_writhe,
                                                  double* __restrict__ seg_acn) {
    __shared__ double R[3][kEntTile + 1], Cc[3][kEntTile + 1];
    __shared__ double sw[kEntTile][17], sa[kEntTile][17];
    const int S = n - 1;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int i0 = blockIdx.x * kEntTile;
    const double* x = xyz + (size_t)blockIdx.y * 3 * n;
    for (int q = tid; q < 3 * (kEntTile + 1); q += 256) {
        const int p = q / 3, comp = q - 3 * p;
        R[comp][p] = i0 + p < n ? x[(size_t)3 * i0 + q] : 0.0;
    }
    __syncthreads();
    double r0x[4], r0y[4], r0z[4], r1x[4], r1y[4], r1z[4], w[4], ac[4];
    for (int a = 0; a < 4; ++a) {
        r0x[a] = R[0][ty + 16 * a]; r0y[a] = R[1][ty + 16 * a]; r0z[a] = R[2][ty + 16 * a];
        r1x[a] = R[0][ty + 16 * a + 1]; r1y[a] = R[1][ty + 16 * a + 1]; r1z[a] = R[2][ty + 16 * a + 1];
        w[a] = 0.0; ac[a] = 0.0;
    }
    // the columns a row of this tile can count lie in i0 - max_sep .. i0 + 63 + max_sep
    const int first = i0 - max_sep > 0 ? (i0 - max_sep) / kEntTile * kEntTile : 0;
    const int last = i0 + kEntTile - 1 + max_sep < S - 1 ? i0 + kEntTile - 1 + max_sep : S - 1;
    for (int j0 = first; j0 <= last; j0 += kEntTile) {
        // a block that lies wholly inside the tile's own band |s - t| < min_sep holds no counted pair (the walk's order skips it as a whole)
        if (j0 + kEntTile - 1 - i0 < min_sep && i0 + kEntTile - 1 - j0 < min_sep) continue;
        __syncthreads();                                     // the block before this one has been read
        for (int q = tid; q < 3 * (kEntTile + 1); q += 256) {
            const int p = q / 3, comp = q - 3 * p;
            Cc[comp][p] = j0 + p < n ? x[(size_t)3 * j0 + q] : 0.0;
        }
        __syncthreads();
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tx + 16 * b;
            const double c0x = Cc[0][tx + 16 * b], c0y = Cc[1][tx + 16 * b], c0z = Cc[2][tx + 16 * b];
            const double c1x = Cc[0][tx + 16 * b + 1], c1y = Cc[1][tx + 16 * b + 1], c1z = Cc[2][tx + 16 * b + 1];
            for (int a = 0; a < 4; ++a) {
                const int i = i0 + ty + 16 * a, gap = i > j ? i - j : j - i;
                if (i < S && j < S && gap >= min_sep && gap <= max_sep) {
                    const double g = ent_pair(r0x[a], r0y[a], r0z[a], r1x[a], r1y[a], r1z[a], c0x, c0y, c0z, c1x, c1y, c1z);
                    w[a] += g;
                    ac[a] += fabs(g);
                }
            }
        }
    }
    for (int a = 0; a < 4; ++a) { sw[ty + 16 * a][tx] = w[a]; sa[ty + 16 * a][tx] = ac[a]; }
    __syncthreads();
    if (tid < kEntTile && i0 + tid < S) {
        double tw = 0.0, ta = 0.0;
        for (int t = 0; t < 16; ++t) { tw += sw[tid][t]; ta += sa[tid][t]; }
        const size_t o = (size_t)blockIdx.y * S + i0 + tid;
        seg_writhe[o] = tw / kEntTwoPi; seg_acn[o] = ta / kEntTwoPi;
    }
}

__global__ __launch_bounds__(256) void k_ent_model(const double* __restrict__ seg_writhe, const double* __restrict__ seg_acn, int S, double* __restrict__ writhe,
                                                  double* __restrict__ acn) {
    __shared__ double red[2 * 256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double w = 0.0, a = 0.0;
    for (int s = tid; s < S; s += 256) { w += seg_writhe[(size_t)k * S + s]; a += seg_acn[(size_t)k * S + s]; }
    block_reduce<2>(red, {w, a}, tid, RedSum());
    if (tid == 0) { writhe[k] = red[0]; acn[k] = red[256]; }
}

// blockIdx.x = q, blockIdx.y = p, blockIdx.z = the model; the workgroups below the diagonal have nothing to do
__global__ __launch_bounds__(256) void k_ent_table(const double* __restrict__ xyz, int n, int min_sep, int max_sep, const int* __restrict__ bounds, int D,
                                                  double* __restrict__ link, double* __restrict__ link_abs) {
    __shared__ double red[2 * 256];
    const int q = blockIdx.x, p = blockIdx.y, k = blockIdx.z, tid = threadIdx.x;
    if (q < p) return;
    const double* x = xyz + (size_t)k * 3 * n;
    const int s0 = bounds[p], t0 = bounds[q], rows = bounds[p + 1] - s0, cols = bounds[q + 1] - t0;
    double w = 0.0, a = 0.0;
    // p < q: the nearest pair of the block is bounds[q] against bounds[p + 1] - 1; a block wholly beyond max_sep is walked by nobody
    if (p == q || t0 - (s0 + rows - 1) <= max_sep) {
        const long long pairs = (long long)rows * cols;
        for (long long e = tid; e < pairs; e += 256) {
            const int s = s0 + (int)(e / cols), t = t0 + (int)(e % cols), gap = s > t ? s - t : t - s;
            if (gap < min_sep || gap > max_sep) continue;
            const double g = ent_pair(x[3 * s], x[3 * s + 1], x[3 * s + 2], x[3 * s + 3], x[3 * s + 4], x[3 * s + 5], x[3 * t], x[3 * t + 1], x[3 * t + 2],
                                      x[3 * t + 3], x[3 * t + 4], x[3 * t + 5]);
            w += g;
            a += fabs(g);
        }
    }
    block_reduce<2>(red, {w, a}, tid, RedSum());
    if (tid == 0) {
        const double lw = red[0] / kEntTwoPi, la = red[256] / kEntTwoPi;
        const size_t base = (size_t)k * D * D;
        link[base + (size_t)p * D + q] = lw; link[base + (size_t)q * D + p] = lw;
        link_abs[base + (size_t)p * D + q] = la; link_abs[base + (size_t)q * D + p] = la;
    }
}

hipError_t launch_entangle_rows(const double* xyz, int n, int K, int min_sep, int max_sep, double* seg_writhe, double* seg_acn, double* writhe, double* acn,
                                hipStream_t s) {
    const int S = n - 1;
    hipLaunchKernelGGL(k_ent_pairs, dim3((S + kEntTile - 1) / kEntTile, K), dim3(256), 0, s, xyz, n, min_sep, max_sep, seg_writhe, seg_acn);
    hipLaunchKernelGGL(k_ent_model, dim3(K), dim3(256), 0, s, seg_writhe, seg_acn, S, writhe, acn);
    return hipGetLastError();
}

hipError_t launch_entangle_table(const double* xyz, int n, int K, int min_sep, int max_sep, const int* bounds, int D, double* link, double* link_abs,
                                 hipStream_t s) {
    hipLaunchKernelGGL(k_ent_table, dim3(D, D, K), dim3(256), 0, s, xyz, n, min_sep, max_sep, bounds, D, link, link_abs);
    return hipGetLastError();
}
