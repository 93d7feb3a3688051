// c3d_f64_step_body.inc — the body of the fp64 step kernel, included by its two entry points (c3d_f64.hip):
//   k64_step          C3D_F64_CHUNKED 0: the replica's coordinates staged whole in LDS, rows and columns read from there
//   k64_step_chunked  C3D_F64_CHUNKED 1: columns staged CHUNK at a time in two LDS buffers, the row side (a row's own coordinates, its
//                     chain neighbours, x0 of the update) from global memory; the copy is LDS-DMA (global_load_lds)
// Everything else — the scalar prologue, the order of every sum, the chain butterfly, the row update, the tile sums — is one text.
// C3D_F64_LBFGS 1 makes the same text the body of k64_lbfgs_eval / k64_lbfgs_eval_chunked: staging, pair loop, row reduction and chain terms
// are these lines (the force has k64_step's bits); the scalar prologue and the row finish are the L-BFGS evaluation's (c3d_lbfgs_eval_body.inc
// in doubles: F to vout, y = F_prev - F into the ring, the Q dot products per row, the tile sums in the fixed 8-row tree).
// C3D_F64_EVAL 1 makes it the body of k64_eval_forces / k64_eval_forces_chunked (c3d_eval_f64): the same staging, pair loop, row reduction,
// FOLD multiply and chain terms, no scalar prologue at all (no sums, no FIRE state, no ring), and the row finish is "lanes 0 and 1 store F
// of their row" into fout [nrep][3][np].  Nothing of the solve is read but xin and T, nothing is written but fout.
    extern __shared__ __attribute__((aligned(16))) double sm64[];
    const int tile = blockIdx.x, rep = rep_base + blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = m.n, np = m.np;
    const size_t roff = (size_t)rep * 3 * np;
#if !C3D_F64_CHUNKED
    double* xs = sm64;
    double* ys = sm64 + np;
    double* zs = sm64 + 2 * np;
    double* rowq = sm64 + 3 * np;                       // [kTileRows][4]
    const double *rx = xs, *ry = ys, *rz = zs;          // the row side: a row's own coordinates, its chain neighbours
    // ---- stage the replica's coordinates; the previous step's sums meanwhile ----
    for (int b = 2 * tid; b < 3 * np; b += 2 * kBlock64) *reinterpret_cast<double2*>(sm64 + b) = *reinterpret_cast<const double2*>(xin + roff + b);
#else
    // two buffers [3][CHUNK] of columns, chunk c in buffer c & 1; the row side comes from global memory
    double* rowq = sm64 + 6 * CHUNK;                    // [kTileRows][4]
    const double *rx = xin + roff, *ry = rx + np, *rz = ry + np;
    // chunk c = columns CHUNK c .. min(CHUNK (c + 1), np) - 1 (a multiple of 128: a wave's 16-byte copies are all inside or all outside)
    auto copy = [&](int c) {
        const int c0 = CHUNK * c, cnt = min(CHUNK, np - c0);
        double* dst = sm64 + (c & 1) * 3 * CHUNK;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double* s = rx + (size_t)k * np + c0;
            double* d = dst + k * CHUNK;
#ifndef C3D_F64_PLAIN_COPY
            // LDS-DMA: no register round trip; LDS address = the wave's base + 16 lane (c3d_step_core.h lds_dma_copy)
            for (int b = 2 * tid; b < cnt; b += 2 * kBlock64)
                __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(s + b),
                                                 (void __attribute__((address_space(3)))*)(d + (b - 2 * lane)), 16, 0, 0);
#else       // (measurement build: plain loads and ds_write)
            for (int b = 2 * tid; b < cnt; b += 2 * kBlock64) *reinterpret_cast<double2*>(d + b) = *reinterpret_cast<const double2*>(s + b);
#endif
        }
    };
    // ---- start the copy of the first chunk; the previous step's sums meanwhile ----
    copy(0);
#endif
    // ---- loads whose latency would otherwise be exposed later leave now: the first targets of this wave's rows, the velocities of the two
    //      rows it finishes ----
    const int row0 = tile * kTileRows + wave * kRows64;
    const int ra = min(row0, n - 1), rb = min(row0 + 1, n - 1);
    const double* Ta = T + (size_t)ra * np + lane;
    const double* Tb = T + (size_t)rb * np + lane;
    double ta0 = Ta[0], ta1 = Ta[64], tb0 = Tb[0], tb1 = Tb[64];        // np >= 128: in bounds whatever n is
    const int row = row0 + lane;
#if !C3D_F64_EVAL
    double v0x = 0, v0y = 0, v0z = 0;
#endif
#if C3D_F64_EVAL
    // (forces only: no scalar prologue)
#elif C3D_F64_LBFGS
    // ---- the ring of this step (kind 9 = a stage's first step: no pair yet); v0 = the previous evaluation's force, read from vin ----
    constexpr int Q = kLbfgsQ;
    const bool first = p.kind == kLbfgsFirst;
    int mem = mem0, nxt = 0;
    if (!first) {      // (clamped into the ring whatever the state holds: a stage always begins with kind 9, which sets it)
        mem = min(max(lsin[rep].mem, 1), kLbfgsMaxPairs);
        nxt = min(max(lsin[rep].head, 0), mem - 1) + 1;
        if (nxt == mem) nxt = 0;
    }
#if !C3D_F64_CHUNKED
    if (lane < kRows64 && row < n && !first) {
        const size_t ix = roff + row;
        v0x = vin[ix]; v0y = vin[ix + np]; v0z = vin[ix + 2 * np];
    }
#endif
#else
#if !C3D_F64_CHUNKED
    if (lane < kRows64 && row < n && !kind_has_no_velocity(p.kind)) {
        const double* vsrc = p.kind == kMdBegin ? vinit : vin;
        const size_t ix = roff + row;
        v0x = vsrc[ix]; v0y = vsrc[ix + np]; v0z = vsrc[ix + 2 * np];
    }
#endif
    // ---- the replica's scalars of this step: ONE wave forms them (the sums of 57 tiles through four butterflies, six fp64 divisions and
    //      a square root are ~400 instruction slots — as much as two thirds of a wave's pair loop) and leaves them in LDS before the
    //      barrier everybody waits at anyway ----
    double* scal = rowq + 4 * kTileRows;                // [8] lam, cm0, cm1, cm2, keep, mix, dt, (unused)
    FireState64 st;
    st.dt = fp.dt_start; st.alpha = fp.alpha_start; st.npos = 0; st.pad = 0;
    if (wave == 0 && kind_continues_state(p.kind)) st = sin[rep];        // (asked for here, used after the sums have arrived)
    if (wave == 0) {
        const bool needs = kind_reads_sums(p.kind);
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        if (needs) {
            const double* pp = pin + (size_t)rep * m.ntiles * 4;
            for (int t = lane; t < m.ntiles; t += 64) { s0 += pp[4 * t]; s1 += pp[4 * t + 1]; s2 += pp[4 * t + 2]; s3 += pp[4 * t + 3]; }
            s0 = wave_sum64(s0); s1 = wave_sum64(s1); s2 = wave_sum64(s2); s3 = wave_sum64(s3);
        }
#define C3D_F64_STATE_OUT if (tile == 0 && lane == 0) sout[rep] = st;
#include "c3d_f64_scalars.inc"                  // the controller: lam, cm0 .. cm2, keep, mix, st from s0 .. s3 (one text with k64_step_scalars)
#undef C3D_F64_STATE_OUT
        if (lane == 0) { scal[0] = lam; scal[1] = cm0; scal[2] = cm1; scal[3] = cm2; scal[4] = keep; scal[5] = mix; scal[6] = st.dt; }
    }
#endif   // the mode's prologue
#if C3D_F64_CHUNKED
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's part of chunk 0 has landed; the barrier: everybody's
#endif
    __syncthreads();

    // ---- pair forces of this wave's two rows ----
    double fxa = 0, fya = 0, fza = 0, fxb = 0, fyb = 0, fzb = 0;
    const double R2 = p.R2;
    const double wr4 = p.wr4;
    if (p.kind != kMdBegin) {
        const double xa = rx[ra], ya = ry[ra], za = rz[ra], xb = rx[rb], yb = ry[rb], zb = rz[rb];
        // (FOLD: the pair terms carry the repel weight relative to the NOE weight, the row sums get the NOE weight below)
        const double nws4p = FOLD ? 1.0 : p.nws4, wr4p = FOLD ? p.wq : wr4;
        // Columns: two per lane and pass (j, j + 64) over the first n & ~127 of them, the next two in flight while these two compute; then
        // ONE column per lane if 64 or more are left, then the last n % 64 columns — both rows of the wave in one pass where they fit
        // (lane = (row, column)).  No lane evaluates a padding column pair by pair any more (455 beads: 15 pair terms per lane, not 16);
        // a lane without a column takes the padding bead n (1e4 A away, no target: an exact zero).
        const int nmain = n & ~127;
#if !C3D_F64_CHUNKED
        const double *cxs = xs, *cys = ys, *czs = zs;       // the columns after the main loop: the staged arrays
        constexpr int jo = 0;
        if (nmain > 0) {
            for (int j = lane; j < nmain; j += 128) {
                const int jn = j + 128 < nmain ? 128 : 0;       // the last pass re-reads itself (in bounds)
                Ta += jn; Tb += jn;
                const double na0 = Ta[0], na1 = Ta[64], nb0 = Tb[0], nb1 = Tb[64];
                const double x0 = xs[j], y0 = ys[j], z0 = zs[j], x1 = xs[j + 64], y1 = ys[j + 64], z1 = zs[j + 64];
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, ta0, xa, ya, za, x0, y0, z0, fxa, fya, fza);
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, tb0, xb, yb, zb, x0, y0, z0, fxb, fyb, fzb);
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, ta1, xa, ya, za, x1, y1, z1, fxa, fya, fza);
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, tb1, xb, yb, zb, x1, y1, z1, fxb, fyb, fzb);
                ta0 = na0; ta1 = na1; tb0 = nb0; tb1 = nb1;
            }
        }
#else
        // The main loop's passes in the same ascending order, chunk by chunk (CHUNK is a multiple of 128: a pass never straddles two); the
        // accumulators and the prefetched targets run straight across.  Before chunk c is computed the copy of chunk c + 1 starts into the
        // other buffer, which every wave left at the barrier that ended chunk c - 1: one barrier per chunk.  cl = the chunk that holds the
        // columns after the main loop and, where a lane is left without a column (n % 64 != 0), the padding bead n: they lie in the same
        // 64-column block, so in the same chunk; all of them are below np.
        const int cl = ((n & 63) ? n : n - 1) / CHUNK;
#pragma nounroll
        for (int c = 0;; ++c) {
            if (c < cl) copy(c + 1);
            const double* bx = sm64 + (c & 1) * 3 * CHUNK;
            const int jb = CHUNK * c, jend = min(jb + CHUNK, nmain);
#pragma nounroll
            for (int j = jb + lane; j < jend; j += 128) {
                const int jn = j + 128 < nmain ? 128 : 0;       // the last pass re-reads itself (in bounds)
                Ta += jn; Tb += jn;
                const double na0 = Ta[0], na1 = Ta[64], nb0 = Tb[0], nb1 = Tb[64];
                const double* q = bx + (j - jb);
                const double x0 = q[0], y0 = q[CHUNK], z0 = q[2 * CHUNK], x1 = q[64], y1 = q[CHUNK + 64], z1 = q[2 * CHUNK + 64];
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, ta0, xa, ya, za, x0, y0, z0, fxa, fya, fza);
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, tb0, xb, yb, zb, x0, y0, z0, fxb, fyb, fzb);
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, ta1, xa, ya, za, x1, y1, z1, fxa, fya, fza);
                pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, tb1, xb, yb, zb, x1, y1, z1, fxb, fyb, fzb);
                ta0 = na0; ta1 = na1; tb0 = nb0; tb1 = nb1;
            }
            if (c == cl) break;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const double *cxs = sm64 + (cl & 1) * 3 * CHUNK, *cys = cxs + CHUNK, *czs = cys + CHUNK;   // the last chunk, its first column jo
        const int jo = CHUNK * cl;
#endif
        const double* Tra = T + (size_t)ra * np;
        const double* Trb = T + (size_t)rb * np;
        int c0 = nmain;
        if (n - c0 >= 64) {
            const int j = c0 + lane;
            const double x0 = cxs[j - jo], y0 = cys[j - jo], z0 = czs[j - jo];
            pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, Tra[j], xa, ya, za, x0, y0, z0, fxa, fya, fza);
            pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, Trb[j], xb, yb, zb, x0, y0, z0, fxb, fyb, fzb);
            c0 += 64;
        }
        const int left = n - c0;                             // 0 .. 63 columns
        if (left > 0 && 2 * left <= 64) {
            const bool second = lane >= left;                // lanes [0, left): row a; [left, 2 left): row b; beyond: the padding bead
            const int c = lane - (second ? left : 0);
            const int j = c < left ? c0 + c : n;
            const double xr = second ? xb : xa, yr = second ? yb : ya, zr = second ? zb : za;
            double tx = 0, ty = 0, tz = 0;
            pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, (second ? Trb : Tra)[j], xr, yr, zr, cxs[j - jo], cys[j - jo], czs[j - jo], tx, ty, tz);
            if (second) { fxb += tx; fyb += ty; fzb += tz; } else { fxa += tx; fya += ty; fza += tz; }
        } else if (left > 0) {
            const int j = lane < left ? c0 + lane : n;
            const double x0 = cxs[j - jo], y0 = cys[j - jo], z0 = czs[j - jo];
            pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, Tra[j], xa, ya, za, x0, y0, z0, fxa, fya, fza);
            pair64<POT, GEN, FOLD>(m, nws4p, wr4p, R2, Trb[j], xb, yb, zb, x0, y0, z0, fxb, fyb, fzb);
        }
    }
#if C3D_F64_EVAL
#elif C3D_F64_CHUNKED && C3D_F64_LBFGS
    if (lane < kRows64 && row < n && !first) {          // (here, not ahead of the pair loop: as the velocities of k64_step_chunked below)
        const size_t ix = roff + row;
        v0x = vin[ix]; v0y = vin[ix + np]; v0z = vin[ix + 2 * np];
    }
#elif C3D_F64_CHUNKED
    // (the velocities of the two rows the wave finishes are asked for here, not ahead of the pair loop: held across the chunk loop, the
    //  six registers were one more than the kernel has at five waves a SIMD)
    if (lane < kRows64 && row < n && !kind_has_no_velocity(p.kind)) {
        const double* vsrc = p.kind == kMdBegin ? vinit : vin;
        const size_t ix = roff + row;
        v0x = vsrc[ix]; v0y = vsrc[ix + np]; v0z = vsrc[ix + 2 * np];
    }
#endif
    double Fx = reduce_rows64(fxa, fxb, lane), Fy = reduce_rows64(fya, fyb, lane), Fz = reduce_rows64(fza, fzb, lane);
    if constexpr (FOLD) { Fx *= p.nws4; Fy *= p.nws4; Fz *= p.nws4; }
    // chain terms: lane 4 r + nb evaluates neighbour nb (offsets -2, -1, +1, +2) of row row0 + r; quad sum; to lane r
    {
        const int r = (lane >> 2) & 1, nb = lane & 3;
        double cx = 0, cy = 0, cz = 0;
        if (lane < 8 && p.kind != kMdBegin) chain64(m, p, wr4, R2, rx, ry, rz, row0 + r, nb < 2 ? nb - 2 : nb - 1, cx, cy, cz);
        cx += dpp_mov64<0xB1>(cx); cy += dpp_mov64<0xB1>(cy); cz += dpp_mov64<0xB1>(cz);
        cx += dpp_mov64<0x4E>(cx); cy += dpp_mov64<0x4E>(cy); cz += dpp_mov64<0x4E>(cz);
        const double ox = dpp_mov64<0x12C>(cx), oy = dpp_mov64<0x12C>(cy), oz = dpp_mov64<0x12C>(cz);   // row_ror:12 = lane + 4
        if (lane == 0) { Fx += cx; Fy += cy; Fz += cz; }
        if (lane == 1) { Fx += ox; Fy += oy; Fz += oz; }
    }
#if C3D_F64_EVAL
    // ---- lanes 0, 1 store F of their row ----
    (void)rowq;
    if (lane < kRows64 && row < n) {
        const size_t ix = roff + row;
        fout[ix] = Fx; fout[ix + np] = Fy; fout[ix + 2 * np] = Fz;
    }
#elif C3D_F64_LBFGS
    // ---- lanes 0, 1 finish one row each: F, y into ring slot nxt, the row's Q products (layout: c3d_internal.h "L-BFGS stage") ----
    if (lane < kRows64) {
        double* q = rowq + Q * (wave * kRows64 + lane);
        for (int k = 0; k < Q; ++k) q[k] = 0.0;
        if (row < n) {
            const size_t ix = roff + row, iy = ix + np, iz = iy + np;
            vout[ix] = Fx; vout[iy] = Fy; vout[iz] = Fz;
            q[Q - 3] = fma(Fx, Fx, fma(Fy, Fy, Fz * Fz));
            if (!first) {
                double* hs = hist + (size_t)rep * lbfgs_hist_floats(np) + row;             // slot j, component c: + (3 j + c) np
                double* hy = hs + (size_t)3 * kLbfgsMaxPairs * np;
                const double yx = v0x - Fx, yy = v0y - Fy, yz = v0z - Fz;
                double* yn = hy + (size_t)3 * nxt * np;
                yn[0] = yx; yn[np] = yy; yn[2 * np] = yz;
                const double* sn = hs + (size_t)3 * nxt * np;
                const double sx = sn[0], sy = sn[np], sz = sn[2 * np];
                q[Q - 4] = fma(sx, sx, fma(sy, sy, sz * sz));
#pragma unroll
                for (int j = 0; j < kLbfgsMaxPairs; ++j) {
                    if (j >= mem) break;
                    double ax, ay, az, bx, by, bz;
                    if (j == nxt) { ax = sx; ay = sy; az = sz; bx = yx; by = yy; bz = yz; }
                    else {
                        const double* a = hs + (size_t)3 * j * np;
                        const double* b = hy + (size_t)3 * j * np;
                        ax = a[0]; ay = a[np]; az = a[2 * np]; bx = b[0]; by = b[np]; bz = b[2 * np];
                    }
                    q[4 * j + 0] = fma(Fx, ax, fma(Fy, ay, Fz * az));
                    q[4 * j + 1] = fma(Fx, bx, fma(Fy, by, Fz * bz));
                    q[4 * j + 2] = fma(ax, yx, fma(ay, yy, az * yz));
                    q[4 * j + 3] = fma(bx, yx, fma(by, yy, bz * yz));
                }
            }
        }
    }
    __syncthreads();
    if (tid < Q) part[((size_t)rep * m.ntiles + tile) * Q + tid] = row_sum8_64(rowq + tid, Q);     // tile sums, the fixed 8-row tree
#else
    // ---- lanes 0, 1 finish one row each (the CPU restatement's update, c3o_md_step / c3o_fire_step) ----
    const double lam = scal[0], cm0 = scal[1], cm1 = scal[2], cm2 = scal[3], keep = scal[4], mix = scal[5];
    st.dt = scal[6];
    double q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    if (lane < kRows64 && row < n) {
        const size_t ix = roff + row, iy = ix + np, iz = iy + np;
        const double x0 = rx[row], y0 = ry[row], z0 = rz[row];
#include "c3d_f64_row_finish.inc"               // the update: xn, vn, q0 .. q3 (one text with k64_row_finish)
        xout[ix] = xn; xout[iy] = yn; xout[iz] = zn;
        vout[ix] = vx; vout[iy] = vy; vout[iz] = vz;
    }
    if (lane < kRows64) { double* q = rowq + 4 * (wave * kRows64 + lane); q[0] = q0; q[1] = q1; q[2] = q2; q[3] = q3; }
    __syncthreads();
    if (tid < 4) {                                      // tile sums, fixed tree ((q0+q1)+(q2+q3))+((q4+q5)+(q6+q7))
        const double* q = rowq + tid;
        pout[((size_t)rep * m.ntiles + tile) * 4 + tid] = ((q[0] + q[4]) + (q[8] + q[12])) + ((q[16] + q[20]) + (q[24] + q[28]));
    }
#endif   // the mode's row finish
