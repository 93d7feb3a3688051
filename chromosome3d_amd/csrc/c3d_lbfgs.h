// c3d_lbfgs.h — the L-BFGS stage (kinds 8 / 9) of the per-step path: k_lbfgs_eval and k_lbfgs_move.  Included by c3d_device.hip only:
// the kernels live in that unit's code object (no unit of their own).
//
// One L-BFGS step = two launches per replica group.  The direction needs global sums of the gradient just computed (its projections on
// the stored pairs: tools/minimiser_study.py lbfgs_fixed_step, late = False), and on the per-step path the kernel boundary is the only
// synchronisation between workgroups:
//   k_lbfgs_eval  forces of the rows (tile_forces<>, the choices launch_step makes; staged or chunked, as k_step: the body is
//                 c3d_lbfgs_eval_body.inc), y = F_prev - F into the ring, per-tile sums of
//                 F.s_j, F.y_j, s_j.y, y_j.y, s.s, F.F (c3d_internal.h "L-BFGS stage")
//   k_lbfgs_move  every workgroup of a replica: the tile sums in fp64 in one fixed order, the pair test, the new column of S'Y and Y'Y,
//                 the two triangular solves of the compact form, the descent test (thread 0, LDS); then its rows: the direction
//                 gamma F - sum top_i s_i + gamma sum u_i y_i, the per-bead cap, the move, s into the ring, the tile sums P.
// Fixed unit step, no energy, no line search.  Everything that varies from step to step (ring head, counts) lives on the device: one
// captured graph serves every chunk of a stage.
#pragma once

namespace c3d {

// fixed tree over the 8 rows of a tile (the order of tile_sum8)
__device__ __forceinline__ float row_sum8(const float* q, int stride) {
    return ((q[0] + q[stride]) + (q[2 * stride] + q[3 * stride])) + ((q[4 * stride] + q[5 * stride]) + (q[6 * stride] + q[7 * stride]));
}


template <int POT, bool GEN, int RPW, bool NC, int TR = kTileRows, bool WIDE = false>
__global__ __launch_bounds__(64 * TR / RPW) __attribute__((amdgpu_waves_per_eu(WIDE ? 4 : 1))) void k_lbfgs_eval(
    const float* __restrict__ xin, const float* __restrict__ tgt, const float* __restrict__ fprev, float* __restrict__ fout,
    float* __restrict__ hist, float* __restrict__ part, const LbfgsState* __restrict__ sin, const DevModel m, const DevStep p,
    const int mem0) {
    using COLS = ColsStaged;
#include "c3d_lbfgs_eval_body.inc"
}
template <int POT, bool GEN, int RPW, int TR, bool WIDE, int CHUNK>
__global__ __launch_bounds__(64 * TR / RPW) __attribute__((amdgpu_waves_per_eu(WIDE ? 4 : 1))) void k_lbfgs_eval_chunked(
    const float* __restrict__ xin, const float* __restrict__ tgt, const float* __restrict__ fprev, float* __restrict__ fout,
    float* __restrict__ hist, float* __restrict__ part, const LbfgsState* __restrict__ sin, const DevModel m, const DevStep p,
    const int mem0) {
    constexpr bool NC = false;
    using COLS = ColsChunked<CHUNK, 64 * TR / RPW>;
#include "c3d_lbfgs_eval_body.inc"
}

// rows per workgroup of the move
constexpr int kLbfgsMoveRows = 256;

// c3d_lbfgs_move_row.inc in floats (k_lbfgs_move, k_lbfgs_move_rows): the per-bead cap is finish_row's, max_step v_rsq_f32(d.d).  Where
// d.d is beyond a float with d finite (|d| from 2^63.5 on) v_rsq_f32(inf) = 0 would leave the bead where it is: the root is then taken of
// d 2^-66, whose square a float holds whatever d (a NaN d.d is no cap: the NaN goes on into the move, as in the CPU restatement)
#define C3D_LBFGS_T float
#define C3D_LBFGS_FMA fmaf
#define C3D_LBFGS_CAP                                                                              \
        const float ms2 = fp.max_step * fp.max_step;                                               \
        const float l2 = fmaf(dx, dx, fmaf(dy, dy, dz * dz));                                      \
        float scl = l2 > ms2 ? fp.max_step * __builtin_amdgcn_rsqf(l2) : 1.0f;                     \
        if (l2 == __builtin_huge_valf()) {                                                         \
            const float ex = dx * 0x1p-66f, ey = dy * 0x1p-66f, ez = dz * 0x1p-66f;                \
            scl = fp.max_step * __builtin_amdgcn_rsqf(fmaf(ex, ex, fmaf(ey, ey, ez * ez))) * 0x1p-66f; \
        }                                                                                          \
        dx *= scl; dy *= scl; dz *= scl;

__global__ __launch_bounds__(kLbfgsMoveRows) void k_lbfgs_move(
    const float* __restrict__ xin, float* __restrict__ xout, const float* __restrict__ fcur, float* __restrict__ hist,
    const float* __restrict__ part, float* __restrict__ pout, const LbfgsState* __restrict__ sin, LbfgsState* __restrict__ sout,
    const DevModel m, const DevStep p, const DevFire fp, const int mem0) {
    constexpr int Q = kLbfgsQ, M = kLbfgsMaxPairs;
    __shared__ double sums[Q];
    __shared__ LbfgsState st;
    __shared__ float coef[1 + 2 * M];            // gamma, then a_j (of s_j), b_j (of y_j) by slot
    __shared__ int shi[2];                       // slot mask of the pairs in the direction, slot of the move's s
    __shared__ float dd[kLbfgsMoveRows];
    const int rep = m.rep_base + blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool first = p.kind == kLbfgsFirst;
    // 1. replica sums of the tile partials in fp64: lane l takes tiles l, l + 64, ... in order, then a butterfly (the same order in every
    //    workgroup, whatever the replica group)
    const float* pr = part + (size_t)rep * m.ntiles * Q;
    for (int k = wave; k < Q; k += kLbfgsMoveRows / 64) {
        double a = 0.0;
        for (int t = lane; t < m.ntiles; t += 64) a += (double)pr[(size_t)t * Q + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) sums[k] = a;
    }
    if (!first) {
        const double* src = reinterpret_cast<const double*>(sin + rep);
        double* dst = reinterpret_cast<double*>(&st);
        for (int k = tid; k < (int)(sizeof(LbfgsState) / sizeof(double)); k += kLbfgsMoveRows) dst[k] = src[k];
    }
    __syncthreads();
    // 2. the compact form, serially (a few hundred fp64 operations): c3d_lbfgs_serial.inc, the text the table hook below runs too
    if (tid == 0) {
#define C3D_LBFGS_COEF float
#define C3D_LBFGS_GAMMA0 ((double)(fp.dt_start * fp.dt_start * m.acc))       /* kind 6's first step length */
#include "c3d_lbfgs_serial.inc"
#undef C3D_LBFGS_GAMMA0
#undef C3D_LBFGS_COEF
    }
    __syncthreads();
    // 3. the rows of this workgroup
    const int i = blockIdx.x * kLbfgsMoveRows + tid;
    const int np = m.npad;
    const size_t roff = (size_t)rep * 3 * np;
    float d2 = 0.0f;
    if (i < m.n) {
#include "c3d_lbfgs_move_row.inc"
    }
    dd[tid] = d2;
    __syncthreads();
    // 4. P[parity^1] of this workgroup's tiles: (move.move, F.F of the evaluation, 0, 0) — the exit test reads .y, the finiteness test all
    constexpr int WT = kLbfgsMoveRows / kTileRows;
    const int t = blockIdx.x * WT + tid;
    if (tid < WT && t < m.ntiles)
        reinterpret_cast<float4*>(pout)[(size_t)rep * m.ntiles + t] = make_float4(row_sum8(dd + kTileRows * tid, 1), pr[(size_t)t * Q + Q - 3], 0.0f, 0.0f);
    // 5. the replica's state: one workgroup writes it
    if (blockIdx.x == 0) {
        const double* src = reinterpret_cast<const double*>(&st);
        double* dst = reinterpret_cast<double*>(sout + rep);
        for (int k = tid; k < (int)(sizeof(LbfgsState) / sizeof(double)); k += kLbfgsMoveRows) dst[k] = src[k];
    }
}

// launch_step's form, with the kernel of an L-BFGS evaluation
hipError_t launch_lbfgs_eval(const DevModel& m0, const DevStep& p, const DevBuffers& b, const LbfgsBuffers& lb, int par, int mem,
                             const StepForm& f, hipStream_t s) {
    if (mem < 1 || mem > kLbfgsMaxPairs) return hipErrorInvalidValue;
    const int q = par ^ 1;
    DevModel m = m0;
    m.tgs2 = f.pairs ? b.tgs2 : nullptr;      // (the kernels that read it)
    const int tr = f.wide ? 2 * kTileRows : kTileRows;
    const auto go = [&](auto kernel, int rpw) {
        hipLaunchKernelGGL(kernel, grid_blocks(m, tr / kTileRows), dim3(64 * tr / rpw), step_lds_bytes(m, f.chunk, (size_t)kLbfgsQ * tr), s,
                           b.X[par], b.tgt, b.V[par], b.V[q], lb.hist, lb.part, lb.S[par], m, p, mem);
        return hipGetLastError();
    };
    return with_chunk(f.chunk, [&](auto CH) {
        if (f.wide) {
            if constexpr (CH == 0) return go(k_lbfgs_eval<4, false, 4, false, 2 * kTileRows, true>, 4);
            else return go(k_lbfgs_eval_chunked<4, false, 4, 2 * kTileRows, true, CH>, 4);
        }
        return with_pot(f.pot, [&](auto POT) { return with_bool(f.gen, [&](auto GEN) { return with_rpw(f.rpw, [&](auto RPW) {
            if constexpr (CH == 0) return with_bool(f.nc, [&](auto NC) { return go(k_lbfgs_eval<POT, GEN, RPW, NC>, RPW); });
            else return go(k_lbfgs_eval_chunked<POT, GEN, RPW, kTileRows, false, CH>, RPW);
        }); }); });
    });
}

hipError_t launch_lbfgs_move(const DevModel& m, const DevStep& p, const DevFire& fp, const DevBuffers& b, const LbfgsBuffers& lb, int parity,
                             int mem, hipStream_t s) {
    if (mem < 1 || mem > kLbfgsMaxPairs) return hipErrorInvalidValue;
    const int q = parity ^ 1;
    hipLaunchKernelGGL(k_lbfgs_move, dim3((m.n + kLbfgsMoveRows - 1) / kLbfgsMoveRows, m.nrep_g), dim3(kLbfgsMoveRows), 0, s,
                       b.X[parity], b.X[q], b.V[q], lb.hist, lb.part, b.P[q], lb.S[parity], lb.S[q], m, p, fp, mem);
    return hipGetLastError();
}

// ---- the rows of the move as a table (c3d_debug_lbfgs_move_rows) ---------------------------------------------------------------------
// c3d_lbfgs_move_row.inc — section 3 of k_lbfgs_move — a thread a row over buffers in the kernel's own layouts with np = the rows padded
// to 256: xin, xout, fcur [3][np], hist [s | y][M][3][np]; coef[1 + 2 M], the slot mask and the slot of s are the call's, as they are a
// replica's in the move.  d2out[row] = the bead's move.move.
__global__ void k_lbfgs_move_rows(const DevFire fp, const int rows, const int np, const float* __restrict__ coef_in, const int mask_in,
                                  const int slot, const float* __restrict__ xin, float* __restrict__ xout, const float* __restrict__ fcur,
                                  float* __restrict__ hist, float* __restrict__ d2out) {
    constexpr int M = kLbfgsMaxPairs;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    float coef[1 + 2 * M];
    for (int k = 0; k < 1 + 2 * M; ++k) coef[k] = coef_in[k];
    const int shi[2] = {mask_in, slot};
    const int rep = 0;
    const size_t roff = 0;
    float d2 = 0.0f;
    {
#include "c3d_lbfgs_move_row.inc"
    }
    d2out[i] = d2;
}
#undef C3D_LBFGS_CAP
#undef C3D_LBFGS_FMA
#undef C3D_LBFGS_T
hipError_t launch_lbfgs_move_rows(const DevFire& fp, int rows, int np, const float* coef, int mask, int slot, const float* xin, float* xout,
                                  const float* fcur, float* hist, float* d2, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_move_rows, dim3((rows + 63) / 64), dim3(64), 0, s, fp, rows, np, coef, mask, slot, xin, xout, fcur, hist, d2);
    return hipGetLastError();
}

// ---- the serial section as a table (c3d_debug_lbfgs_direction) ----------------------------------------------------------------------
// c3d_lbfgs_serial.inc — what thread 0 of every workgroup of k_lbfgs_move runs between its barriers — on `rows` independent rows, a
// thread a row: flags[2 r] = first step (kind 9), flags[2 r + 1] = mem0 (1 .. kLbfgsMaxPairs: the entry checks it).  Out: the state the
// step leaves, coef[1 + 2 M] (the floats the rows of the move read, widened) and (slot mask, slot of the move's s).
__global__ void k_lbfgs_direction(const DevModel m, const DevFire fp, const int rows, const double* __restrict__ sums_in,
                                  const LbfgsState* __restrict__ sin, const int* __restrict__ flags, LbfgsState* __restrict__ sout,
                                  double* __restrict__ coef_out, int* __restrict__ shi_out) {
    constexpr int Q = kLbfgsQ, M = kLbfgsMaxPairs;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double sums[Q];
    for (int k = 0; k < Q; ++k) sums[k] = sums_in[(size_t)r * Q + k];
    LbfgsState st = sin[r];
    float coef[1 + 2 * M];
    int shi[2];
    const bool first = flags[2 * r] != 0;
    const int mem0 = flags[2 * r + 1];
    {
#define C3D_LBFGS_COEF float
#define C3D_LBFGS_GAMMA0 ((double)(fp.dt_start * fp.dt_start * m.acc))
#include "c3d_lbfgs_serial.inc"
#undef C3D_LBFGS_GAMMA0
#undef C3D_LBFGS_COEF
    }
    sout[r] = st;
    for (int k = 0; k < 1 + 2 * M; ++k) coef_out[(size_t)r * (1 + 2 * M) + k] = (double)coef[k];
    shi_out[2 * r] = shi[0]; shi_out[2 * r + 1] = shi[1];
}
hipError_t launch_lbfgs_direction(const DevModel& m, const DevFire& fp, int rows, const double* sums, const LbfgsState* in, const int* flags,
                                  LbfgsState* out, double* coef, int* shi, hipStream_t s) {
    hipLaunchKernelGGL(k_lbfgs_direction, dim3((rows + 63) / 64), dim3(64), 0, s, m, fp, rows, sums, in, flags, out, coef, shi);
    return hipGetLastError();
}

}  // namespace c3d
