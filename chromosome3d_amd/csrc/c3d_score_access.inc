// c3d_score_access.inc — one kernel family of the scoring unit: included once by c3d_score.hip, inside namespace c3d (shared helpers: c3d_score_core.h)
// ---- a bead's exposed surface (c3d_accessibility) -----------------------------------------------------------------------------------------------
// Shrake-Rupley over uniform spheres.  Every bead of a model is a sphere of radius R = radius + probe that carries P points x_i + R u_p; a
// point is buried when it lies strictly inside the sphere of another bead of the model, and exposed[k n + i] counts the points of bead i
// that are not.  In the arithmetic of the definition (include/c3d.h): c = x_i + R u_p a component as one product and one sum, e = c - x_j,
// buried iff ((ex ex) + ey ey) + ez ez < R2 with R2 = R R, every product through cmp_rounded so that nothing is fused; j = i is left out by
// index, so a second bead at the same coordinates does bury.  The counts are integers and a point's fate has no order: no floating-point
// sum, two calls return the same bytes, and the integers are those of a host loop over all j.
//
// k_access: a workgroup of 256 threads owns kAccTile = 16 row beads of one model (blockIdx.x the tile, blockIdx.y the model) and walks the
// model's columns in super-blocks of kAccSuper = 1024 beads, staged in LDS with coalesced loads as k_geo_pairs stages its blocks.  A
// super-block is two passes with a barrier between them:
//   (a) neighbours: thread t takes the columns t, t + 256, t + 512, t + 768 of the super-block and tests each against the 16 rows; a column
//       that can bury a point of row a (the bound below) has its offset in the super-block appended, as 16 bits, to the list of row a in LDS
//       through that row's integer counter in LDS.  The order of a list depends on the run; what is read from it does not.  A list holds
//       1024 offsets, a whole super-block: it cannot overflow and there is no second path.
//   (b) points: the sixteen threads tid >> 4 == a of row a share its points, thread lane l the points l, l + 16, ... (at most 64 of them at
//       P = C3D_ACCESS_MAX_POINTS = 1024: one bit each of a 64-bit register mask that lives across the super-blocks).  A point that is not
//       yet buried is formed and tested against the row's list until one bead buries it.
// After the last super-block a thread counts its points whose bit is clear and the sixteen counts of a row meet in an LDS integer.
// LDS: 32 KiB of lists + 24 KiB of columns + the tile and the counters = 57 856 bytes, static, under the 64 KiB a launch gets without opting
// in: the points are NOT staged (24 KiB more at P = 1024) but read from global memory where a point is formed — 24 P bytes that every
// workgroup of the launch reads, so they stay in the caches.  Two workgroups fit the 160 KiB of a CU.
//
// The neighbour bound.  Pass (a) keeps j for row i when d2 = ((ux ux) + uy uy) + uz uz <= keep2, u = x_i - x_j, keep2 = 4 R2 (1 + 2^-20)
// formed once on the host.  Why a column that is NOT kept buries no point of the row, under the entry's limits |x| < 1e6 (flags[0] is raised
// for a coordinate outside, and the entry refuses the call), 0.01 <= R <= 1e5 and | |u_p|^2 - 1 | <= 1e-9:
//   - a difference of two doubles is rounded once, so d2 = D^2 (1 + h) with D the true distance and |h| < 2^-50 (five roundings of positive
//     terms); R2 and keep2 carry three roundings more.  d2 > keep2 therefore gives D > 2 R (1 + 2^-21.1), that is D - 2 R > 0.9 R 2^-20.
//   - the exact point c* = x_i + R u_p lies within R |u_p| <= R (1 + 6e-10) of x_i, so |c* - x_j| >= D - R |u_p| > R (1 + 0.9 2^-20 - 6e-10).
//   - the computed e differs from c* - x_j by the roundings of R u (<= 2^-37 A, |R u| < 2^17), of the sum (<= 2^-33 A, |c| < 2^21) and of the
//     difference (<= 2^-35 A while D <= 4 R, |e| < 2^19; a bead further away than 4 R is 3 R from every point and needs no bound):
//     under 2^-32 A a component, 4.1e-10 A in norm, which is at most 4.1e-8 R at R >= 0.01.  So |e| > R (1 + 8.5e-7 - 6e-10 - 4.1e-8)
//     > R (1 + 8e-7),
//   - and the computed sum of squares, |e|^2 (1 + h') with |h'| < 2^-50, exceeds R^2 (1 + 1.6e-6) (1 - 2^-50) > R^2 (1 + 2^-52) >= R2:
//     the strict comparison fails, the point is not buried by j.  A kept j is tested with the definition's own arithmetic, so keeping too
//     many costs time only.  A coordinate that is not a number gives d2 = NaN, not kept, and a sum that is not < R2: the same outcome.
constexpr int kAccTile = 16;
constexpr int kAccSuper = 1024;

__global__ __launch_bounds__(256) void k_access(const double* __restrict__ xyz, int n, const double* __restrict__ pts, int P, double R, double R2, double keep2,
                                               int* __restrict__ exposed, int* __restrict__ flags) {
    __shared__ double Cc[3][kAccSuper];
    __shared__ unsigned short list[kAccTile][kAccSuper];
    __shared__ double T[3][kAccTile];
    __shared__ int fill[kAccTile], open[kAccTile];
    const int tid = threadIdx.x, row = tid >> 4, lane = tid & 15;
    const int i0 = blockIdx.x * kAccTile, i = i0 + row;
    const double* x = xyz + (size_t)blockIdx.y * 3 * n;
    if (tid < 3 * kAccTile) {
        const int p = tid / 3, comp = tid - 3 * p;
        T[comp][p] = i0 + p < n ? x[(size_t)3 * i0 + tid] : 0.0;
    }
    if (tid < kAccTile) open[tid] = 0;
    unsigned long long buried = 0;                           // bit m: point lane + 16 m of row `row`
    bool outside = false;
    for (int j0 = 0; j0 < n; j0 += kAccSuper) {
        __syncthreads();                                     // the super-block before this one has been read (the first time: T is there)
        if (tid < kAccTile) fill[tid] = 0;
        for (int q = tid; q < 3 * kAccSuper; q += 256) {
            const int p = q / 3, comp = q - 3 * p;
            const double v = j0 + p < n ? x[(size_t)3 * j0 + q] : 0.0;
            outside = outside || !(fabs(v) < 1e6);
            Cc[comp][p] = v;
        }
        __syncthreads();
        // (a) the neighbours of the 16 rows among this super-block's columns
        for (int b = 0; b < kAccSuper / 256; ++b) {
            const int c = tid + 256 * b, j = j0 + c;
            if (j >= n) break;
            const double cx = Cc[0][c], cy = Cc[1][c], cz = Cc[2][c];
            for (int a = 0; a < kAccTile; ++a) {
                const double ux = T[0][a] - cx, uy = T[1][a] - cy, uz = T[2][a] - cz;
                double d2 = cmp_rounded(ux * ux);
                d2 += cmp_rounded(uy * uy);
                d2 += cmp_rounded(uz * uz);
                if (i0 + a < n && i0 + a != j && d2 <= keep2) list[a][atomicAdd(&fill[a], 1)] = (unsigned short)c;
            }
        }
        __syncthreads();
        // (b) the row's points that are still open, against the row's list
        const int members = fill[row];
        if (i < n && members > 0) {
            const double tx = T[0][row], ty = T[1][row], tz = T[2][row];
            for (int m = 0, p = lane; p < P; ++m, p += 16) {
                if ((buried >> m) & 1ull) continue;
                const double px = tx + cmp_rounded(R * pts[(size_t)3 * p]);
                const double py = ty + cmp_rounded(R * pts[(size_t)3 * p + 1]);
                const double pz = tz + cmp_rounded(R * pts[(size_t)3 * p + 2]);
                for (int t = 0; t < members; ++t) {
                    const int c = list[row][t];
                    const double ex = px - Cc[0][c], ey = py - Cc[1][c], ez = pz - Cc[2][c];
                    double q = cmp_rounded(ex * ex);
                    q += cmp_rounded(ey * ey);
                    q += cmp_rounded(ez * ez);
                    if (q < R2) { buried |= 1ull << m; break; }
                }
            }
        }
    }
    if (outside) flags[0] = 1;
    if (i < n) {
        const int mine = lane < P ? (P - lane + 15) / 16 : 0;      // the points lane, lane + 16, ... below P
        atomicAdd(&open[row], mine - __popcll(buried));
    }
    __syncthreads();
    if (tid < kAccTile && i0 + tid < n) exposed[(size_t)blockIdx.y * n + i0 + tid] = open[tid];
}

hipError_t launch_accessibility(const double* xyz, int n, int K, const double* points, int P, double R, double R2, double keep2, int* exposed, int* flags,
                                hipStream_t s) {
    hipLaunchKernelGGL(k_access, dim3((n + kAccTile - 1) / kAccTile, K), dim3(256), 0, s, xyz, n, points, P, R, R2, keep2, exposed, flags);
    return hipGetLastError();
}
