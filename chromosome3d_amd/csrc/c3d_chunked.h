// c3d_chunked.h — the chunked-column form of the three per-step kernels: k_step_chunked, k_lbfgs_eval_chunked, k_eval_forces_chunked.
// Included by c3d_device.hip only: the kernels live in that unit's code object (no unit of their own).
//
// The staged kernels (k_step, k_lbfgs_eval, k_eval_forces) copy a replica's whole coordinate array, 3 npad floats, into LDS before the
// pair loop: at most the 64 KB a launch gets without opting in, n <= 5120.  Here a workgroup keeps TWO LDS buffers of 3 CHUNK floats
// and walks the columns chunk by chunk: before it computes chunk c it starts the copy of chunk c + 1 into the other buffer (LDS-DMA,
// lds_dma_copy), one barrier per chunk (ColsChunked::enter).  The pair loop is tile_forces' own, block for block in the same order, the
// accumulators and the target pipeline running straight across chunk boundaries; only where a column's coordinates are read changes.
// The row side — a row's own coordinates, its chain neighbours at +-2, finish_row's position — comes from global memory (a replica's
// coordinates sit in L2 anyway).  So a row's force, and everything after it, has the same bits as from the staged form, and the LDS a
// workgroup takes is sized by CHUNK and the tile, never by n.
//
// Only layouts without a narrow last block (DevModel::wl == 4, nleft == 0: every n > 1024) have a chunked form: the per-step kernels'
// NC = false instantiations.  column_chunk_for (c3d_internal.h) decides; the staged form serves the rest.
#pragma once

namespace c3d {

// the column source of tile_forces_cols in the chunked form (see ColsStaged, c3d_step_core.h).  buf = LDS [2][3][CHUNK], src = the
// replica's coordinates in global memory [3][npad]; BLOCK = threads of the workgroup
template <int CHUNK, int BLOCK>
struct ColsChunked {
    static constexpr bool kStaged = false;
    static constexpr int BPC = CHUNK / 256;          // column blocks per chunk
    static_assert(CHUNK % 256 == 0 && (BPC & (BPC - 1)) == 0, "CHUNK: a power of two times 256 columns");
    float* buf;
    const float* src;
    int npad, tid;
    bool dma;
    // chunk c (columns CHUNK c .. min(CHUNK (c + 1), npad) - 1: a multiple of 256, as lds_dma_copy wants) into buffer c & 1
    __device__ __forceinline__ void copy(int c) const {
        const int c0 = CHUNK * c, cnt = min(CHUNK, npad - c0);
        float* dst = buf + (c & 1) * 3 * CHUNK;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* s = src + (size_t)k * npad + c0;
            float* d = dst + k * CHUNK;
            if (dma) {   // lds_dma_copy's instructions (a call of it from here changed the address arithmetic of the staged kernels' calls)
                const int lane = tid & 63;
                for (int b = 4 * tid; b < cnt; b += 4 * BLOCK)
                    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(s + b),
                                                     (void __attribute__((address_space(3)))*)(d + (b - 4 * lane)), 16, 0, 0);
            } else for (int b = 4 * tid; b < cnt; b += 4 * BLOCK) *reinterpret_cast<float4*>(d + b) = *reinterpret_cast<const float4*>(s + b);
        }
    }
    // top of column block jb: at the first block of chunk c > 0 wait for chunk c (this wave's copies: vmcnt; everyone's: the barrier,
    // which also means every wave is done with chunk c - 1), then start chunk c + 1 into the buffer chunk c - 1 leaves free.  Chunk 0
    // was started by the kernel's prologue and made visible by its barrier.
    __device__ __forceinline__ void enter(int jb) const {
        if (jb & (BPC - 1)) return;
        const int c = jb / BPC;
        if (c > 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        if (CHUNK * (c + 1) < npad) copy(c + 1);
    }
    __device__ __forceinline__ void load(int jb, int lane, float4& xj, float4& yj, float4& zj) const {
        const float* b = buf + ((jb / BPC) & 1) * 3 * CHUNK + 256 * (jb & (BPC - 1)) + 4 * lane;
        xj = *reinterpret_cast<const float4*>(b);
        yj = *reinterpret_cast<const float4*>(b + CHUNK);
        zj = *reinterpret_cast<const float4*>(b + 2 * CHUNK);
    }
};

// ---------------------------------------------------------------------------------------------
// k_step in the chunked form (NC = false).  Written out beside k_step rather than folded into it: k_step's machine code stays what it
// was.  Differences: LDS = the two chunk buffers | rowq | the scalars' hand-over; the prologue starts chunk 0 instead of the whole
// array; the row side reads xin.
// ---------------------------------------------------------------------------------------------
template <int POT, bool GEN, int RPW, int TR, bool WIDE, int CHUNK>
__global__ __launch_bounds__(64 * TR / RPW) __attribute__((amdgpu_waves_per_eu(WIDE ? 4 : 1))) void k_step_chunked(
    const float* __restrict__ pin, const float* __restrict__ xin, const float* __restrict__ tgt,
    const float* __restrict__ vin, const float* __restrict__ vinit, const FireState* __restrict__ sin,
    float* __restrict__ xout, float* __restrict__ vout, float* __restrict__ pout, FireState* __restrict__ sout,
    const DevModel m, const DevStep p, const DevFire fp) {
    constexpr bool NC = false;
    constexpr int WAVES = TR / RPW;
    constexpr int BLOCK = 64 * WAVES;
    constexpr int TILES = TR / kTileRows;
    static_assert(TR % kTileRows == 0 && TILES >= 1 && TILES <= 2, "a workgroup owns one or two 8-row tiles");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    {   // (k_step: the kernel arguments beyond the preloaded ones, fetched at once)
        const auto ka = __builtin_amdgcn_kernarg_segment_ptr();
        unsigned t0, t1, t2, t3;
        asm volatile("s_load_dword %0, %4, 0x40\n\ts_load_dword %1, %4, 0x80\n\ts_load_dword %2, %4, 0xc0\n\ts_load_dword %3, %4, 0x100\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(ka) : "memory");
    }
    int tile, rep;
    if (!block_to_tile(m, tile, rep)) return;
    tile *= TILES;
    if (tile >= m.ntiles) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npad = m.npad;
    float* rowq = smem + 6 * CHUNK;             // [TR][4] per-row contributions to the replica sums
    const size_t roff = (size_t)rep * 3 * npad;
    const float* xs = xin + roff;               // the row side, from global memory
    const float* ys = xs + npad;
    const float* zs = ys + npad;
    const ColsChunked<CHUNK, BLOCK> cols{smem, xs, npad, tid, m.stage_dma != 0};
    const int row0 = tile * kTileRows + wave * RPW;
    const int row = row0 + lane;
    const bool fin_lane = lane < RPW;
    const bool finisher = fin_lane && row < m.n;
    const size_t ix = roff + row, iy = ix + npad, iz = iy + npad;
    const bool needs_partials = p.kind == 0 || p.kind == 1 || p.kind == 2 || p.kind == 5;

    cols.copy(0);
    const float4* pp = reinterpret_cast<const float4*>(pin) + (size_t)rep * m.ntiles;
    float4 q0 = make_float4(0, 0, 0, 0);
    if (needs_partials && lane < m.ntiles && (!WIDE || !C3D_SHARE_SCALARS || wave == 0)) q0 = pp[lane];
    float4 tv[RPW];
    if (p.kind != 4) {
        if (pair_targets_in_use<POT, GEN, RPW, NC>(m)) pair_targets_prefetch(m, row0, lane, 0, tv);
        else tile_prefetch<RPW, NC>(m, tgt, row0, lane, 0, tv);
    }
    float vx0 = 0.0f, vy0 = 0.0f, vz0 = 0.0f;
    if (finisher && p.kind != 3 && p.kind != 6) {
        const float* vsrc = p.kind == 4 ? vinit : vin;
        vx0 = vsrc[ix]; vy0 = vsrc[iy]; vz0 = vsrc[iz];
    }
    FireState st;
    st.dt = fp.dt_start; st.alpha = fp.alpha_start; st.npos = 0; st.pad = 0;
    if (p.kind == 2 || p.kind == 5) st = sin[rep];
    constexpr bool SHARE = WIDE && C3D_SHARE_SCALARS;
    float* const scb = rowq + 4 * TR;           // [12]: StepScalars (6) + FireState (4)
    const bool sums_here = !SHARE || wave == 0;
    float4 psum = make_float4(0, 0, 0, 0);
    if (needs_partials && sums_here) {
        psum.x += q0.x; psum.y += q0.y; psum.z += q0.z; psum.w += q0.w;
        for (int t = lane + 64; t < m.ntiles; t += 64) {
            const float4 q = pp[t];
            psum.x += q.x; psum.y += q.y; psum.z += q.z; psum.w += q.w;
        }
    }
    StepScalars sc;
    sc.lam = 1.0f; sc.cmx = sc.cmy = sc.cmz = 0.0f; sc.keep = 0.0f; sc.mix = 0.0f;
    if (sums_here) {
        if (needs_partials) psum = wave_sum4(psum);
        sc = step_scalars(m, p, fp, psum, st);
        if ((p.kind == 2 || p.kind == 3 || p.kind == 5 || p.kind == 6) && tile == 0 && tid == 0) sout[rep] = st;
        if constexpr (SHARE) {
            if (lane == 0) {
                scb[0] = sc.lam; scb[1] = sc.cmx; scb[2] = sc.cmy; scb[3] = sc.cmz; scb[4] = sc.keep; scb[5] = sc.mix;
                scb[6] = st.dt; scb[7] = st.alpha; reinterpret_cast<int*>(scb)[8] = st.npos; reinterpret_cast<int*>(scb)[9] = st.pad;
            }
        }
    }
    __syncthreads();
    if constexpr (SHARE) {
        if (!sums_here) {
            sc.lam = scb[0]; sc.cmx = scb[1]; sc.cmy = scb[2]; sc.cmz = scb[3]; sc.keep = scb[4]; sc.mix = scb[5];
            st.dt = scb[6]; st.alpha = scb[7]; st.npos = reinterpret_cast<const int*>(scb)[8]; st.pad = reinterpret_cast<const int*>(scb)[9];
        }
    }

    float Fx = 0.0f, Fy = 0.0f, Fz = 0.0f;
    if (p.kind != 4) tile_forces_cols<POT, GEN, RPW, NC, true, WIDE>(m, p, tgt, xs, ys, zs, cols, row0, lane, tv, Fx, Fy, Fz);

    float4 q = make_float4(0, 0, 0, 0);
    if (finisher) {
        float vx, vy, vz, xn, yn, zn;
        finish_row(m, p, fp, sc, st, Fx, Fy, Fz, xs[row], ys[row], zs[row], vx0, vy0, vz0, xn, yn, zn, vx, vy, vz, q);
        xout[ix] = xn; xout[iy] = yn; xout[iz] = zn;
        vout[ix] = vx; vout[iy] = vy; vout[iz] = vz;
    }
    if (fin_lane) reinterpret_cast<float4*>(rowq)[row - tile * kTileRows] = q;
    __syncthreads();
    if (tid < TILES && tile + tid < m.ntiles)
        reinterpret_cast<float4*>(pout)[(size_t)rep * m.ntiles + tile + tid] = tile_sum8(reinterpret_cast<const float4*>(rowq) + kTileRows * tid);
}

// ---------------------------------------------------------------------------------------------
// k_lbfgs_eval in the chunked form (NC = false): the same differences as k_step_chunked
// ---------------------------------------------------------------------------------------------
template <int POT, bool GEN, int RPW, int TR, bool WIDE, int CHUNK>
__global__ __launch_bounds__(64 * TR / RPW) __attribute__((amdgpu_waves_per_eu(WIDE ? 4 : 1))) void k_lbfgs_eval_chunked(
    const float* __restrict__ xin, const float* __restrict__ tgt, const float* __restrict__ fprev, float* __restrict__ fout,
    float* __restrict__ hist, float* __restrict__ part, const LbfgsState* __restrict__ sin, const DevModel m, const DevStep p,
    const int mem0) {
    constexpr bool NC = false;
    constexpr int WAVES = TR / RPW;
    constexpr int BLOCK = 64 * WAVES;
    constexpr int TILES = TR / kTileRows;
    constexpr int Q = kLbfgsQ;
    static_assert(TR % kTileRows == 0 && TILES >= 1 && TILES <= 2, "a workgroup owns one or two 8-row tiles");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int tile, rep;
    if (!block_to_tile(m, tile, rep)) return;
    tile *= TILES;
    if (tile >= m.ntiles) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npad = m.npad;
    float* rowq = smem + 6 * CHUNK;             // [TR][Q]
    const size_t roff = (size_t)rep * 3 * npad;
    const float* xs = xin + roff;
    const float* ys = xs + npad;
    const float* zs = ys + npad;
    const ColsChunked<CHUNK, BLOCK> cols{smem, xs, npad, tid, m.stage_dma != 0};
    const int row0 = tile * kTileRows + wave * RPW;
    const int row = row0 + lane;
    const bool fin_lane = lane < RPW;
    const bool finisher = fin_lane && row < m.n;

    cols.copy(0);
    float4 tv[RPW];
    if (pair_targets_in_use<POT, GEN, RPW, NC>(m)) pair_targets_prefetch(m, row0, lane, 0, tv);
    else tile_prefetch<RPW, NC>(m, tgt, row0, lane, 0, tv);
    const bool first = p.kind == 9;
    int mem = mem0, nxt = 0;
    if (!first) {
        mem = min(max(sin[rep].mem, 1), kLbfgsMaxPairs);
        nxt = min(max(sin[rep].head, 0), mem - 1) + 1;
        if (nxt == mem) nxt = 0;
    }
    float fpx = 0.0f, fpy = 0.0f, fpz = 0.0f;
    const size_t ix = roff + row, iy = ix + npad, iz = iy + npad;
    if (finisher && !first) { fpx = fprev[ix]; fpy = fprev[iy]; fpz = fprev[iz]; }
    __syncthreads();

    float Fx = 0.0f, Fy = 0.0f, Fz = 0.0f;
    tile_forces_cols<POT, GEN, RPW, NC, true, WIDE>(m, p, tgt, xs, ys, zs, cols, row0, lane, tv, Fx, Fy, Fz);

    if (fin_lane) {
        float* q = rowq + (row - tile * kTileRows) * Q;
        for (int k = 0; k < Q; ++k) q[k] = 0.0f;
        if (finisher) {
            fout[ix] = Fx; fout[iy] = Fy; fout[iz] = Fz;
            q[Q - 3] = fmaf(Fx, Fx, fmaf(Fy, Fy, Fz * Fz));
            if (!first) {
                float* hs = hist + (size_t)rep * lbfgs_hist_floats(npad) + row;
                float* hy = hs + (size_t)3 * kLbfgsMaxPairs * npad;
                const float yx = fpx - Fx, yy = fpy - Fy, yz = fpz - Fz;
                float* yn = hy + (size_t)3 * nxt * npad;
                yn[0] = yx; yn[npad] = yy; yn[2 * npad] = yz;
                const float* sn = hs + (size_t)3 * nxt * npad;
                const float sx = sn[0], sy = sn[npad], sz = sn[2 * npad];
                q[Q - 4] = fmaf(sx, sx, fmaf(sy, sy, sz * sz));
#pragma unroll
                for (int j = 0; j < kLbfgsMaxPairs; ++j) {
                    if (j >= mem) break;
                    float ax, ay, az, bx, by, bz;
                    if (j == nxt) { ax = sx; ay = sy; az = sz; bx = yx; by = yy; bz = yz; }
                    else {
                        const float* a = hs + (size_t)3 * j * npad;
                        const float* b = hy + (size_t)3 * j * npad;
                        ax = a[0]; ay = a[npad]; az = a[2 * npad]; bx = b[0]; by = b[npad]; bz = b[2 * npad];
                    }
                    q[4 * j + 0] = fmaf(Fx, ax, fmaf(Fy, ay, Fz * az));
                    q[4 * j + 1] = fmaf(Fx, bx, fmaf(Fy, by, Fz * bz));
                    q[4 * j + 2] = fmaf(ax, yx, fmaf(ay, yy, az * yz));
                    q[4 * j + 3] = fmaf(bx, yx, fmaf(by, yy, bz * yz));
                }
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < TILES * Q; t += BLOCK) {
        const int tt = t / Q, k = t - tt * Q;
        if (tile + tt < m.ntiles) part[((size_t)rep * m.ntiles + tile + tt) * Q + k] = row_sum8(rowq + tt * kTileRows * Q + k, Q);
    }
}

// ---------------------------------------------------------------------------------------------
// the forces hook in the chunked form (NC = false; ERPW and PACKED as in k_eval_forces)
// ---------------------------------------------------------------------------------------------
template <int POT, bool GEN, int ERPW, bool PACKED, int CHUNK>
__global__ __launch_bounds__(64 * kTileRows / ERPW) void k_eval_forces_chunked(const DevModel m, const DevStep p,
                                                               const float* __restrict__ tgt, const float* __restrict__ xin,
                                                               float* __restrict__ fout) {
    constexpr int BLOCK = 64 * kTileRows / ERPW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int tile, rep;
    if (!block_to_tile(m, tile, rep)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npad = m.npad;
    const size_t roff = (size_t)rep * 3 * npad;
    const float* xs = xin + roff;
    const ColsChunked<CHUNK, BLOCK> cols{smem, xs, npad, tid, m.stage_dma != 0};
    const int row0 = tile * kTileRows + wave * ERPW;
    float4 tv[ERPW];
    tile_prefetch<ERPW, false>(m, tgt, row0, lane, 0, tv);
    cols.copy(0);
    __syncthreads();
    float Fx, Fy, Fz;
    tile_forces_cols<POT, GEN, ERPW, false, PACKED, false>(m, p, tgt, xs, xs + npad, xs + 2 * npad, cols, row0, lane, tv, Fx, Fy, Fz);
    const int row = row0 + lane;
    if (lane < ERPW && row < m.n) {
        fout[roff + row] = Fx;
        fout[roff + npad + row] = Fy;
        fout[roff + 2 * npad + row] = Fz;
    }
}

// ---------------------------------------------------------------------------------------------
// launchers (called by launch_step / launch_lbfgs_eval / launch_eval_forces when the form says chunked)
// ---------------------------------------------------------------------------------------------
template <class F> hipError_t with_chunk(int chunk, F&& f) {
    switch (chunk) {
        case 256: return f(int_c<256>{});
        case 1024: return f(int_c<1024>{});
        case 2048: return f(int_c<2048>{});
        default: return hipErrorInvalidValue;
    }
}
static size_t chunk_lds_bytes(int chunk, size_t extra_floats) { return sizeof(float) * ((size_t)6 * chunk + extra_floats); }

hipError_t launch_step_chunked(const DevModel& m, const DevStep& p, const DevFire& fp, const DevBuffers& b, int par, const StepForm& f,
                                      hipStream_t s) {
    const int q = par ^ 1;
    return with_chunk(f.chunk, [&](auto CH) {
        if (f.wide) {
            constexpr int TR = 2 * kTileRows;
            const int nwg = (m.ntiles + 1) / 2;
            hipLaunchKernelGGL((k_step_chunked<4, false, 4, TR, true, CH>), dim3(8, m.nrep_g, (nwg + 7) / 8), dim3(64 * TR / 4),
                               chunk_lds_bytes(CH, 4 * TR + 12), s,
                               b.P[par], b.X[par], b.tgt, b.V[par], b.Vinit, b.S[par], b.X[q], b.V[q], b.P[q], b.S[q], m, p, fp);
            return hipGetLastError();
        }
        return with_pot(f.pot, [&](auto POT) { return with_bool(f.gen, [&](auto GEN) { return with_rpw(f.rpw, [&](auto RPW) {
            hipLaunchKernelGGL((k_step_chunked<POT, GEN, RPW, kTileRows, false, CH>), grid_blocks(m), dim3(64 * kTileRows / RPW),
                               chunk_lds_bytes(CH, 4 * kTileRows + 12), s,
                               b.P[par], b.X[par], b.tgt, b.V[par], b.Vinit, b.S[par], b.X[q], b.V[q], b.P[q], b.S[q], m, p, fp);
            return hipGetLastError();
        }); }); });
    });
}

hipError_t launch_lbfgs_eval_chunked(const DevModel& m, const DevStep& p, const DevBuffers& b, const LbfgsBuffers& lb, int par, int mem,
                                            const StepForm& f, hipStream_t s) {
    const int q = par ^ 1;
    return with_chunk(f.chunk, [&](auto CH) {
        if (f.wide) {
            constexpr int TR = 2 * kTileRows;
            const int nwg = (m.ntiles + 1) / 2;
            hipLaunchKernelGGL((k_lbfgs_eval_chunked<4, false, 4, TR, true, CH>), dim3(8, m.nrep_g, (nwg + 7) / 8), dim3(64 * TR / 4),
                               chunk_lds_bytes(CH, (size_t)kLbfgsQ * TR), s, b.X[par], b.tgt, b.V[par], b.V[q], lb.hist, lb.part, lb.S[par], m, p, mem);
            return hipGetLastError();
        }
        return with_pot(f.pot, [&](auto POT) { return with_bool(f.gen, [&](auto GEN) { return with_rpw(f.rpw, [&](auto RPW) {
            hipLaunchKernelGGL((k_lbfgs_eval_chunked<POT, GEN, RPW, kTileRows, false, CH>), grid_blocks(m), dim3(64 * kTileRows / RPW),
                               chunk_lds_bytes(CH, (size_t)kLbfgsQ * kTileRows), s, b.X[par], b.tgt, b.V[par], b.V[q], lb.hist, lb.part, lb.S[par], m, p, mem);
            return hipGetLastError();
        }); }); });
    });
}

hipError_t launch_eval_forces_chunked(const DevModel& m, const DevStep& p, const DevBuffers& b, int parity, float* Fout, bool general_tail,
                                             int rows_per_wave, int chunk, hipStream_t s) {
    const dim3 g = grid_blocks(m);
    return with_chunk(chunk, [&](auto CH) { return with_pot(m.noe_pot, [&](auto POT) { return with_bool(general_tail, [&](auto GEN) {
        if constexpr (POT == 4 && !GEN)
            if (rows_per_wave == 2 || rows_per_wave == -2) return with_bool(rows_per_wave == 2, [&](auto PACKED) {
                hipLaunchKernelGGL((k_eval_forces_chunked<4, false, 2, PACKED, CH>), g, dim3(64 * kTileRows / 2), chunk_lds_bytes(CH, 0), s, m, p,
                                   b.tgt, b.X[parity], Fout);
                return hipGetLastError();
            });
        hipLaunchKernelGGL((k_eval_forces_chunked<POT, GEN, 4, true, CH>), g, dim3(kEvalBlock), chunk_lds_bytes(CH, 0), s, m, p, b.tgt, b.X[parity], Fout);
        return hipGetLastError();
    }); }); });
}

}  // namespace c3d
