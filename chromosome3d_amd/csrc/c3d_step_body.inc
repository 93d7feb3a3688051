// c3d_step_body.inc — the statement list of the per-step kernel, included as the body of both of its entry points (c3d_device.hip):
// k_step (COLS = ColsStaged) and k_step_chunked (COLS = ColsChunked<CHUNK, BLOCK>, NC = false).  The entry point supplies the
// template parameters, the kernel arguments, COLS and NC.  The forms differ only in the `COLS::kStaged` branches: where the coordinates
// sit in LDS, where the row side reads from, the prologue copy and the C3D_STAMP diagnostics.
//
// A text, not a __device__ function: a function boundary, even one always inlined, changes the order in which the optimiser sees the
// statements, and with it the machine code of every instantiation (tools/isa_compare.py).  For the same reason the row-side pointers
// below keep each form's own address arithmetic and order (the staged form forms roff after the LDS layout, the chunked one before).
    constexpr int WAVES = TR / RPW;
    constexpr int BLOCK = 64 * WAVES;
    constexpr int TILES = TR / kTileRows;       // 8-row tiles of this workgroup
    static_assert(TR % kTileRows == 0 && TILES >= 1 && TILES <= 2, "a workgroup owns one or two 8-row tiles");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if constexpr (COLS::kStaged) C3D_STAMP(6);      // before any kernel argument beyond the preloaded ones is needed
    {   // The 280-byte kernarg block spans five 64-byte lines and the scalar cache is cold at every launch: the
        // compiler fetches the arguments where they are first used, one ~550-cycle miss after the other.  Touch
        // the four lines beyond the preloaded pointers at once; the later loads then hit.
        static_assert(10 * sizeof(void*) + sizeof(DevModel) + sizeof(DevStep) + sizeof(DevFire) >= 0x100 + 4,
                      "the touched offsets must lie inside the explicit kernel arguments");
        static_assert(10 * sizeof(void*) + sizeof(DevModel) + sizeof(DevStep) + sizeof(DevFire) <= 0x140,
                      "a sixth 64-byte line of kernel arguments needs a sixth touch");
        const auto ka = __builtin_amdgcn_kernarg_segment_ptr();
        unsigned t0, t1, t2, t3;
        asm volatile("s_load_dword %0, %4, 0x40\n\ts_load_dword %1, %4, 0x80\n\ts_load_dword %2, %4, 0xc0\n\ts_load_dword %3, %4, 0x100\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3) : "s"(ka) : "memory");
    }
    int tile, rep;
    if (!block_to_tile(m, tile, rep)) return;   // (tile = the workgroup's number among those of its replica)
    tile *= TILES;                              // its first 8-row tile
    if (tile >= m.ntiles) return;
    if constexpr (COLS::kStaged) C3D_STAMP(0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npad = m.npad;
    // the row side: LDS (staged) or the replica's coordinates in global memory (chunked)
    const float* xs = COLS::kStaged ? smem : xin + (size_t)rep * 3 * npad;
    const float* ys = COLS::kStaged ? smem + npad : xs + npad;
    const float* zs = COLS::kStaged ? smem + 2 * npad : ys + npad;
    float* rowq = smem + COLS::lds_floats(npad);    // [TR][4] per-row contributions to the replica sums
    const size_t roff = (size_t)rep * 3 * npad;
    const COLS cols{smem, xs, npad, tid, m.stage_dma != 0};
    const int row0 = tile * kTileRows + wave * RPW;
    const int row = row0 + lane;                // the row this lane finishes (lanes < RPW only)
    const bool fin_lane = lane < RPW;
    const bool finisher = fin_lane && row < m.n;
    const size_t ix = roff + row, iy = ix + npad, iz = iy + npad;
    // (kind_reads_sums, and below kind_has_no_velocity, kind_continues_state, kind_stores_state of c3d_step_kinds.h, written out: as calls they
    // change k_step's machine code)
    const bool needs_partials = p.kind == kMdCouple || p.kind == kMdRescale || p.kind == kFire || p.kind == kTwoPoint;

    // ---- 1. every independent global load is issued before anything waits -------------------
    if constexpr (COLS::kStaged) {
        if (m.stage_dma) lds_dma_copy<BLOCK>(xin + roff, smem, 3 * npad, tid);
        else for (int b = 4 * tid; b < 3 * npad; b += 4 * BLOCK) *reinterpret_cast<float4*>(smem + b) = *reinterpret_cast<const float4*>(xin + roff + b);
    } else cols.copy(0);
    // the first partial-sum entry of every lane is only ISSUED here: adding it up right away would park the wave
    // on this cold load before the target and velocity loads below are even on their way
    const float4* pp = reinterpret_cast<const float4*>(pin) + (size_t)rep * m.ntiles;
    float4 q0 = make_float4(0, 0, 0, 0);
    if (needs_partials && lane < m.ntiles && (!WIDE || !C3D_SHARE_SCALARS || wave == 0)) q0 = pp[lane];      // (wave 0 alone forms the replica sums, below)
    float4 tv[RPW];
    if (p.kind != kMdBegin) {
        if (pair_targets_in_use<POT, GEN, RPW, NC>(m)) pair_targets_prefetch(m, row0, lane, 0, tv);
        else tile_prefetch<RPW, NC>(m, tgt, row0, lane, 0, tv);
    }
    float vx0 = 0.0f, vy0 = 0.0f, vz0 = 0.0f;
    if (finisher && p.kind != kFireFirst && p.kind != kTwoPointFirst) {
        const float* vsrc = p.kind == kMdBegin ? vinit : vin;
        vx0 = vsrc[ix]; vy0 = vsrc[iy]; vz0 = vsrc[iz];
    }
    FireState st;
    st.dt = fp.dt_start; st.alpha = fp.alpha_start; st.npos = 0; st.pad = 0;
    if (p.kind == kFire || p.kind == kTwoPoint) st = sin[rep];
    // WIDE (large N: hundreds of tile sums): ONE wave of the workgroup forms the replica sums and the step's scalars and hands them to the
    // others through LDS across the barrier that waits for the coordinates anyway — the same values, the same bits (every wave used to
    // derive them for itself: ~90 of a wave's ~2200 VALU instructions per step at N = 2500, three quarters of them redundant)
    constexpr bool SHARE = WIDE && C3D_SHARE_SCALARS;       // (narrow form, N = 455 x 20, same box: 6.92 us per step shared against 6.78 per wave — its
                                                            //  waves would wait at the barrier for a chain they used to run beside their own loads)
    float* const scb = rowq + 4 * TR;           // [12]: StepScalars (6) + FireState (4)
    const bool sums_here = !SHARE || wave == 0;
    float4 psum = make_float4(0, 0, 0, 0);
    if (needs_partials && sums_here) {   // one float4 per tile; ntiles <= 64 for N <= 512
        psum.x += q0.x; psum.y += q0.y; psum.z += q0.z; psum.w += q0.w;
        for (int t = lane + 64; t < m.ntiles; t += 64) {
            const float4 q = pp[t];
            psum.x += q.x; psum.y += q.y; psum.z += q.z; psum.w += q.w;
        }
    }
    if constexpr (COLS::kStaged) C3D_STAMP(1);

    // ---- 2. scalars per wave (no barrier of their own; every wave ends with the same values) -----------------
    StepScalars sc;
    sc.lam = 1.0f; sc.cmx = sc.cmy = sc.cmz = 0.0f; sc.keep = 0.0f; sc.mix = 0.0f;
    if (sums_here) {
        if (needs_partials) psum = wave_sum4(psum);
        sc = step_scalars(m, p, fp, psum, st);
        if ((p.kind == kFire || p.kind == kFireFirst || p.kind == kTwoPoint || p.kind == kTwoPointFirst) && tile == 0 && tid == 0) sout[rep] = st;
        if constexpr (SHARE) {
            if (lane == 0) {
                scb[0] = sc.lam; scb[1] = sc.cmx; scb[2] = sc.cmy; scb[3] = sc.cmz; scb[4] = sc.keep; scb[5] = sc.mix;
                scb[6] = st.dt; scb[7] = st.alpha; reinterpret_cast<int*>(scb)[8] = st.npos; reinterpret_cast<int*>(scb)[9] = st.pad;
            }
        }
    }
    if constexpr (COLS::kStaged) C3D_STAMP(2);
    __syncthreads();
    if constexpr (SHARE) {
        if (!sums_here) {
            sc.lam = scb[0]; sc.cmx = scb[1]; sc.cmy = scb[2]; sc.cmz = scb[3]; sc.keep = scb[4]; sc.mix = scb[5];
            st.dt = scb[6]; st.alpha = scb[7]; st.npos = reinterpret_cast<const int*>(scb)[8]; st.pad = reinterpret_cast<const int*>(scb)[9];
        }
    }
    if constexpr (COLS::kStaged) C3D_STAMP(3);

    // ---- 3. K2: pair forces for this wave's rows ---------------------------------------------
    float Fx = 0.0f, Fy = 0.0f, Fz = 0.0f;
    if (p.kind != kMdBegin) tile_forces<POT, GEN, RPW, NC, true, WIDE>(m, p, tgt, xs, ys, zs, cols, row0, lane, tv, Fx, Fy, Fz);

    if constexpr (COLS::kStaged) C3D_STAMP(4);
    // ---- 4. epilogue: lanes 0..RPW-1 finish one row each --------------------------------------
    float4 q = make_float4(0, 0, 0, 0);   // this lane's contribution to the tile's partial sums
    if (finisher) {
        float vx, vy, vz, xn, yn, zn;
        finish_row(m, p, fp, sc, st, Fx, Fy, Fz, xs[row], ys[row], zs[row], vx0, vy0, vz0, xn, yn, zn, vx, vy, vz, q);
        xout[ix] = xn; xout[iy] = yn; xout[iz] = zn;
        vout[ix] = vx; vout[iy] = vy; vout[iz] = vz;
    }
    // tile partial sums: the fixed tree of tile_sum8 over the eight rows (deterministic, the cluster kernel's order)
    if (fin_lane) reinterpret_cast<float4*>(rowq)[row - tile * kTileRows] = q;
    __syncthreads();
    if (tid < TILES && tile + tid < m.ntiles)
        reinterpret_cast<float4*>(pout)[(size_t)rep * m.ntiles + tile + tid] = tile_sum8(reinterpret_cast<const float4*>(rowq) + kTileRows * tid);
    if constexpr (COLS::kStaged) C3D_STAMP(5);
