// c3d_eval_forces_body.inc — the statement list of the forces hook, included as the body of both of its entry points (c3d_device.hip):
// k_eval_forces (COLS = ColsStaged: a plain copy of the whole array into LDS) and k_eval_forces_chunked (COLS = ColsChunked).  Why a
// text and not a function: c3d_step_body.inc.
    constexpr int BLOCK = 64 * kTileRows / ERPW;
    constexpr bool NC = COLS::kStaged;          // (the chunked form exists for NC = false only)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int tile, rep;
    if (!block_to_tile(m, tile, rep)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npad = m.npad;
    const size_t roff = (size_t)rep * 3 * npad;
    const float* xs = COLS::kStaged ? smem : xin + roff;
    const COLS cols{smem, xs, npad, tid, m.stage_dma != 0};
    const int row0 = tile * kTileRows + wave * ERPW;
    float4 tv[ERPW];
    tile_prefetch<ERPW, NC>(m, tgt, row0, lane, 0, tv);
    if constexpr (COLS::kStaged) {
        for (int b = tid; b < 3 * npad; b += BLOCK) smem[b] = xin[roff + b];
    } else cols.copy(0);
    __syncthreads();
    float Fx, Fy, Fz;
    tile_forces<POT, GEN, ERPW, NC, PACKED, false>(m, p, tgt, xs, xs + npad, xs + 2 * npad, cols, row0, lane, tv, Fx, Fy, Fz);
    const int row = row0 + lane;
    if (lane < ERPW && row < m.n) {
        fout[roff + row] = Fx;
        fout[roff + npad + row] = Fy;
        fout[roff + 2 * npad + row] = Fz;
    }
