// c3d_lbfgs_eval_body.inc — the statement list of the L-BFGS evaluation, included as the body of both of its entry points (c3d_lbfgs.h):
// k_lbfgs_eval (COLS = ColsStaged) and k_lbfgs_eval_chunked (COLS = ColsChunked<CHUNK, BLOCK>, NC = false).  The forms differ only in
// the `COLS::kStaged` branches; why a text and not a function: c3d_step_body.inc.
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
    const size_t roff = (size_t)rep * 3 * npad;
    const float* xs = COLS::kStaged ? smem : xin + roff;     // the row side: LDS (staged) or global memory (chunked)
    const float* ys = COLS::kStaged ? smem + npad : xs + npad;
    const float* zs = COLS::kStaged ? smem + 2 * npad : ys + npad;
    float* rowq = smem + COLS::lds_floats(npad);    // [TR][Q]
    const COLS cols{smem, xs, npad, tid, m.stage_dma != 0};
    const int row0 = tile * kTileRows + wave * RPW;
    const int row = row0 + lane;
    const bool fin_lane = lane < RPW;
    const bool finisher = fin_lane && row < m.n;

    if constexpr (COLS::kStaged) {
        if (m.stage_dma) lds_dma_copy<BLOCK>(xin + roff, smem, 3 * npad, tid);
        else for (int b = 4 * tid; b < 3 * npad; b += 4 * BLOCK) *reinterpret_cast<float4*>(smem + b) = *reinterpret_cast<const float4*>(xin + roff + b);
    } else cols.copy(0);
    float4 tv[RPW];
    if (pair_targets_in_use<POT, GEN, RPW, NC>(m)) pair_targets_prefetch(m, row0, lane, 0, tv);
    else tile_prefetch<RPW, NC>(m, tgt, row0, lane, 0, tv);
    const bool first = p.kind == kLbfgsFirst;
    int mem = mem0, nxt = 0;
    if (!first) {      // (clamped into the ring whatever the state holds: a stage always begins with kind 9, which sets it)
        mem = min(max(sin[rep].mem, 1), kLbfgsMaxPairs);
        nxt = min(max(sin[rep].head, 0), mem - 1) + 1;
        if (nxt == mem) nxt = 0;
    }
    float fpx = 0.0f, fpy = 0.0f, fpz = 0.0f;
    const size_t ix = roff + row, iy = ix + npad, iz = iy + npad;
    if (finisher && !first) { fpx = fprev[ix]; fpy = fprev[iy]; fpz = fprev[iz]; }
    __syncthreads();

    float Fx = 0.0f, Fy = 0.0f, Fz = 0.0f;
    tile_forces<POT, GEN, RPW, NC, true, WIDE>(m, p, tgt, xs, ys, zs, cols, row0, lane, tv, Fx, Fy, Fz);

    if (fin_lane) {
        float* q = rowq + (row - tile * kTileRows) * Q;
        for (int k = 0; k < Q; ++k) q[k] = 0.0f;
        if (finisher) {
            fout[ix] = Fx; fout[iy] = Fy; fout[iz] = Fz;
            q[Q - 3] = fmaf(Fx, Fx, fmaf(Fy, Fy, Fz * Fz));
            if (!first) {
                float* hs = hist + (size_t)rep * lbfgs_hist_floats(npad) + row;            // slot j, component c: + (3 j + c) npad
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
