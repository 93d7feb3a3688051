// c3d_f64.hip — the SA step in fp64 (option "precision" = 64): the reference's precision on the GPU.
//
// The reference's arithmetic is fp64 throughout (Perl, CNS); the product kernels run fp32.  This is the
// same algorithm — same energy model, same lagged sums, same leap-frog / FIRE update (deck :1646-1700, :1729-1782,
// :1790-1803 restated in DESIGN.md section 3) — in fp64, and since round 4 in the per-step kernel's SHAPE (round 3: one wave
// per row over array-of-structures coordinates, a force and an update launch per step, 29.5 us per 20-replica step):
//
//   k64_step   ONE launch per SA step of a replica group.  A workgroup (4 waves) owns kTileRows = 8 consecutive rows of one
//              replica's N x N pair matrix, 2 rows per wave; the replica's coordinates are staged once in LDS as
//              structure-of-arrays doubles (3 x 8 x npad bytes), lanes run along the columns (column 64 k + lane: every
//              target load is one 512-byte line per wave, every coordinate read a conflict-free ds_read_b64), two columns
//              in flight per lane.  1 / d comes from a 23-bit seed (v_rsq_f32) and ONE coupled Newton step that delivers d and
//              1 / d together, each to about 5e-14 relative (sqrt_hrsqrt64 below; 5 fused operations instead of the ~30 of a
//              correctly rounded sqrt and a division); the two
//              rows of a wave are reduced in ONE transposing DPP butterfly on the 32-bit halves.  The row's owner lane
//              adds the chain terms, integrates the row and leaves its contribution to the replica sums; the sums a step
//              needs (kinetic energy, centre-of-mass velocity, FIRE power and norms) are the per-tile partial sums the
//              previous step left, added in a fixed order by every wave — the kernel boundary is the only synchronisation,
//              exactly as in k_step (c3d_device.hip), so the hipGraph replay and the replica groups on two streams of the
//              per-step path carry it unchanged.
//
// It puts a number on what fp32 buys (bench.py prints the f64 line beside the f32 one) and, because the CPU restatement the
// tests hold is the same algorithm in the same precision, it ties the GPU to it over LONG trajectories (fp32 trajectories leave
// any reference after a few hundred chaotic steps; tests/test_gpu_parity.py::test_fp64_path_*).  Targets are 0.1 * t10 formed
// in fp64 from the integer tenths (as the CPU restatement forms them), not the fp32 target matrix.
#include "c3d_internal.h"

namespace c3d {

struct FireState64 {
    double dt, alpha;
    int npos, pad;
};
constexpr double kBoltz64 = 0.0019872, kAccel64 = 418.4;
constexpr int kRows64 = 2;                       // rows per wave
constexpr int kWaves64 = kTileRows / kRows64;    // 4 waves: one tile of 8 rows per workgroup (the fp32 step's tile)
constexpr int kBlock64 = 64 * kWaves64;
constexpr int kColPad64 = 128;                   // columns padded to two per lane
constexpr int kLbfgsMoveRows64 = 256;            // rows per workgroup of k64_lbfgs_move
constexpr double kNoTarget64 = 1.0e300;          // "no restraint" in the target matrix of the fast soft lower side (pair64)

// ---- 64-bit values through the 32-bit cross-lane paths (DPP, permlane swaps): VALU only, no LDS round trip ----------
template <int CTRL>
__device__ __forceinline__ double dpp_mov64(double v) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double xrow_sum64(double v) {    // + the other three 16-lane rows, every lane
    const long long b = __double_as_longlong(v);
    unsigned lo = (unsigned)(b & 0xffffffffll), hi = (unsigned)(b >> 32);
    auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = __longlong_as_double(((long long)h16[0] << 32) | l16[0]) + __longlong_as_double(((long long)h16[1] << 32) | l16[1]);
    const long long c = __double_as_longlong(v);
    lo = (unsigned)(c & 0xffffffffll); hi = (unsigned)(c >> 32);
    auto l32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto h32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __longlong_as_double(((long long)h32[0] << 32) | l32[0]) + __longlong_as_double(((long long)h32[1] << 32) | l32[1]);
}
__device__ __forceinline__ double wave_sum64(double v) {    // total in every lane, fixed tree
    v += dpp_mov64<0xB1>(v);
    v += dpp_mov64<0x4E>(v);
    v += dpp_mov64<0x124>(v);
    v += dpp_mov64<0x128>(v);
    return xrow_sum64(v);
}
// a0 / a1: this lane's partial sums for the wave's two rows; returns, in every lane l, the wave total of row (l & 1)
__device__ __forceinline__ double reduce_rows64(double a0, double a1, int lane) {
    const bool odd = lane & 1;
    double k = odd ? a1 : a0;
    const double s = odd ? a0 : a1;
    k += dpp_mov64<0xB1>(s);
    k += dpp_mov64<0x4E>(k);
    k += dpp_mov64<0x124>(k);
    k += dpp_mov64<0x128>(k);
    return xrow_sum64(k);
}

// d = sqrt(r2) and h = 1 / (2 d) together: a 23-bit seed + ONE coupled Newton step (Goldschmidt form).  With the seed's relative error
// e (v_rsq_f32's ulp and the rounding of r2 to float: |e| <= 1.5 x 2^-23 = 1.8e-7), g = sqrt(r2) (1 + e) and h = (1 + e) / (2 sqrt(r2)),
// so r = 1/2 - g h = -e - e^2 / 2 and g (1 + r) = sqrt(r2) (1 - 1.5 e^2): d and h come out within 1.5 e^2 = 4.8e-14 relative, some
// 200 double ulps, not "an ulp or two" — measured pair by pair in tests/test_gpu_pair_table.py (profiles/r34_pair_table.md).  Under the
// suite's fp64 force cap (1e-11 of a row's scale) that is two hundred times inside; against a pair's OWN force near d = T it is
// unbounded in relative terms (the force is 2 w S (d - T) / d), which is why that table bounds a component by the row's term scales.
// The second step (C3D_F64_TWO_NEWTON, defined by no build) would bring both within an ulp or two at three more fused operations a
// pair.  (r2 >= 1e-30: no denormal, no zero.)
__device__ __forceinline__ void sqrt_hrsqrt64(double r2, double& d, double& h) {
    // 23-bit seeds from the fp32 unit (v_rsq_f64 is no better and no faster), the halving done there too; 1e-30 <= r2 <= 1e9
    const float yf = __builtin_amdgcn_rsqf((float)r2);
    double g = r2 * (double)yf;
    h = (double)(0.5f * yf);
    double r = fma(-g, h, 0.5);
#ifdef C3D_F64_TWO_NEWTON
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-g, h, 0.5);
#endif
    d = fma(g, r, g); h = fma(h, r, h);
}

// 1 / x and sqrt(x) to a rounding or two (fp32 seed, two Newton steps each): the per-workgroup scalars.  The seed is a float's: outside
// 2^-120 <= x < 2^120 (where x and 1 / x are both normal floats) — a sum that underflowed, a zero, a negative number, an infinity, a
// NaN — the operand takes the correctly rounded division / square root instead: a path no sane trajectory enters, but finite doubles
// must not come out as NaN or on the wrong side of a bound (the seed of 1e-40 is inf and the Newton steps make NaN of it; that of 1e40 is
// 0 and stays 0).  The range test is one addition and one unsigned compare on the high word (sign and exponent), and the branch is
// the WAVE's (any lane outside: every lane computes the wide form, each keeps the one its operand asks for): one scalar branch on the
// step kernels' critical path instead of two exec-mask regions (a per-lane branch cost 0.06 us of a 10.1 us step).
__device__ __forceinline__ bool seed_range64(double x) {
    return (unsigned)(__double_as_longlong(x) >> 32) - 0x38700000u < 0x0F000000u;      // biased exponents 903 .. 1142, sign 0
}
__device__ __forceinline__ double rcp64(double x) {
    double y = (double)__builtin_amdgcn_rcpf((float)x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    const bool wide = !seed_range64(x);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(wide) != 0, 0)) y = wide ? 1.0 / x : y;
    return y;
}
__device__ __forceinline__ double sqrt64(double x) {
    const double y = (double)__builtin_amdgcn_rsqf((float)x);
    double g = x * y, h = 0.5 * y;
    double r = fma(-g, h, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-g, h, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    g = fma(fma(-g, g, x), h, g);                   // one more correction of g alone
    const bool wide = !seed_range64(x);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(wide) != 0, 0)) g = wide ? __builtin_sqrt(x) : g;      // (0 -> 0, NaN -> NaN: the CPU restatement's sqrt)
    return g;
}

// The per-bead cap's scale max_step / |d| beyond the seed's range.  sqrt_hrsqrt64 seeds from a float: for d.d >= 2^128 the seed is 0, the
// Newton steps keep 0, and a bead the CPU restatement moves by max_step would stay where it is.  A capped d.d outside seed_range64 takes the
// correctly rounded max_step / sqrt(d.d) — the CPU restatement's own two operations — behind the wave's branch, as rcp64 does (the users:
// c3d_f64_row_finish.inc, the rows of k64_lbfgs_move).  capped = the cap acted on this lane; scl = the seeded scale (1 where it did not).
__device__ __forceinline__ double cap_scale_wide64(double d2, bool capped, double max_step, double scl) {
    const bool wide = capped && !seed_range64(d2);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(wide) != 0, 0)) scl = wide ? max_step / __builtin_sqrt(d2) : scl;
    return scl;
}

// HALF of dE/dDelta of the NOE term without S and w.  GEN = tails with a 1/D^2 part.
template <int POT, bool GEN>
__device__ __forceinline__ double half_noe_grad64(const Model64& m, double delta) {
    if constexpr (!GEN) {      // the force stays at its value at the switch distance: slope 2 rs above, 2 mrs below (POT 3)
        if constexpr (POT == 0) return fmin(fmax(delta, -m.rs), m.rs);
        else if constexpr (POT == 1) return fmin(delta, m.rs);
        else if constexpr (POT == 3) return fmin(fmax(delta, -m.mrs), m.rs);
        else if constexpr (POT == 4) {
            // lower side beyond mrs: dE/dD = 2 mrs^4 / D^3 (soft form, exponent 2, no asymptote) = the lower bound -mrs (mrs / D)^3 of
            // the same clamp; 1 / D from a 23-bit seed (v_rcp_f32) and ONE Newton step: with the seed's relative error e (|e| <= 1.5 x 2^-23)
            // y (2 - D y) = (1 - e^2) / D, 3.2e-14 relative, three times that in the bound (see sqrt_hrsqrt64; C3D_F64_TWO_NEWTON as there)
            // D = |delta| (a free source modifier; round 4, second session: it was max(-delta, mrs)): inside the square part and above the
            // target the bound -mrs^4 / D^3 then lies BELOW delta and does not bind; delta = 0 (or below the fp32 seed's range): the seed is
            // inf, the Newton step NaN, and max(delta, NaN) = delta
            const double D = fabs(delta);
            double y = (double)__builtin_amdgcn_rcpf((float)D);
            double e = fma(-D, y, 1.0);
            y = fma(y, e, y);
#ifdef C3D_F64_TWO_NEWTON
            e = fma(-D, y, 1.0);
            y = fma(y, e, y);
#endif
            return fmin(fmax(delta, (y * y) * (y * m.nmrs4)), m.rs);       // nmrs4 = -mrs^4
        }
        else return delta;
    } else {
        const double ad = fabs(delta);
        const double a2 = ad * ad > 1e-300 ? ad * ad : 1e-300;
        const double up = 0.5 * (m.tail_c - m.tail_b / a2), lo = -0.5 * (m.mtail_c - m.mtail_b / (m.mexp == 2 ? a2 * ad : a2));
        if constexpr (POT == 0) return ad > m.rs ? (delta > 0 ? up : -up) : delta;
        else if constexpr (POT == 1) return delta > m.rs ? up : delta;
        else if constexpr (POT == 3 || POT == 4) return delta > m.rs ? up : (delta < -m.mrs ? lo : delta);
        else return delta;
    }
}

// One pair term of a row against column j (T = 0.1 * t10 where restrained, else 0; pad columns sit 1e4 A away with T = 0).
// Straight-line code, no branch around the square root (a branch serialises the four pair terms a lane has in flight):
//   NOE    -w S g(d - T) / d = nws4 * (g / 2) * h,  nws4 = -4 w S where restrained else 0, h = 1 / (2 d)
//   repel  on EVERY column: 4 w_vdw k_rep max(0, R2 - r2); the self term has dx = 0, the |i-j| < rep_sep neighbours are taken
//          back out with the chain terms (chain64)
// FOLD (fast soft lower side only): the row's sum is formed WITHOUT the NOE weight — nws4 = 1 here, wr4 = the repel weight divided by the NOE
// weight — and multiplied by it once per row (k64_step): one multiplication less per pair term.  Needs a non-zero NOE weight.
template <int POT, bool GEN, bool FOLD = false>
__device__ __forceinline__ void pair64(const Model64& m, double nws4, double wr4, double R2, double T, double xi, double yi, double zi,
                                       double xj, double yj, double zj, double& fx, double& fy, double& fz) {
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    // The guard against r2 = 0 (the self term; the CPU restatement clamps at 1e-12, which no pair of distinct beads ever reaches) rides in the
    // fma chain: 1e-30 is below half an ulp of any r2 > 1e-14, so every real pair keeps its bits, and the self term stays finite (x 0 = 0).
    const double r2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, 1e-30)));
    double d, h;
    sqrt_hrsqrt64(r2, d, h);
    double wn = nws4;
    // no restraint: T = 0 and the weight is switched off — except for the fast soft lower side (POT 4), where such a pair carries
    // T = kNoTarget64 = 1e300 instead: a pair that far inside its "target" feels exactly nothing (D = 1e300: the fp32 seed of 1 / D is 0, the
    // Newton steps keep it, the bound is -0, the force +0), which saves the compare and the two selects of every pair term
    if constexpr (!(POT == 4 && !GEN)) wn = T > 0.0 ? nws4 : 0.0;
    double cn = half_noe_grad64<POT, GEN>(m, d - T) * h;
    if constexpr (!(FOLD && POT == 4 && !GEN)) cn = wn * cn;
    const double coef = fma(wr4, fmax(R2 - r2, 0.0), cn);
    fx = fma(coef, dx, fx); fy = fma(coef, dy, fy); fz = fma(coef, dz, fz);
}

// pseudo-bond (i,i+-1) and pseudo-angle (i,i+-2) terms of `row` against neighbour row + off
__device__ __forceinline__ void chain64(const Model64& m, const Step64& p, double wr4, double R2, const double* xs, const double* ys,
                                        const double* zs, int row, int off, double& cx, double& cy, double& cz) {
    cx = cy = cz = 0.0;
    const int jn = row + off, sep = off < 0 ? -off : off;
    if (row >= m.n || jn < 0 || jn >= m.n) return;
    const double dx = xs[row] - xs[jn], dy = ys[row] - ys[jn], dz = zs[row] - zs[jn];
    const double r2 = fmax(fma(dx, dx, fma(dy, dy, dz * dz)), 1e-12);
    double d, h;
    sqrt_hrsqrt64(r2, d, h);                          // h = 1 / (2 d)
    double coef = 0.0;
    if (sep == 1) coef = p.kb4 * (d - m.b0) * h;
    else if (m.k_ang > 0 && (m.ang_mode == 1 || r2 < p.a0sq)) coef = p.ka4 * (d - m.a0) * h;
    if (sep < m.rep_sep) coef -= wr4 * fmax(R2 - r2, 0.0);      // the pair loop applied the repel term to every column
    cx = coef * dx; cy = coef * dy; cz = coef * dz;
}

// P: [nrep][ntiles][4] per-tile sums of the previous step — MD kinds: (sum v^2, sum vx, vy, vz); FIRE: (v.F, F.F, v.v, 0)
template <int POT, bool GEN, bool FOLD = false>
__global__ __launch_bounds__(kBlock64) __attribute__((amdgpu_waves_per_eu(5))) void k64_step(const Model64 m, const Step64 p, const Fire64 fp, const int rep_base,
                                                    const double* __restrict__ T, const double* __restrict__ xin,
                                                    const double* __restrict__ vin, const double* __restrict__ vinit,
                                                    const double* __restrict__ pin, const FireState64* __restrict__ sin,
                                                    double* __restrict__ xout, double* __restrict__ vout, double* __restrict__ pout,
                                                    FireState64* __restrict__ sout) {
#define C3D_F64_CHUNKED 0
#define C3D_F64_LBFGS 0
#define C3D_F64_EVAL 0
#include "c3d_f64_step_body.inc"
#undef C3D_F64_EVAL
#undef C3D_F64_LBFGS
#undef C3D_F64_CHUNKED
}

// The same step with the columns staged CHUNK at a time (two LDS buffers of 3 CHUNK doubles: 24 KB at CHUNK 512, 48 KB at 1024, whatever n is) and the row
// side read from global memory: every n up to 16384, in k64_step's bits (the same passes in the same order).
template <int POT, bool GEN, bool FOLD, int CHUNK>
__global__ __launch_bounds__(kBlock64) __attribute__((amdgpu_waves_per_eu(5))) void k64_step_chunked(const Model64 m, const Step64 p, const Fire64 fp, const int rep_base,
                                                    const double* __restrict__ T, const double* __restrict__ xin,
                                                    const double* __restrict__ vin, const double* __restrict__ vinit,
                                                    const double* __restrict__ pin, const FireState64* __restrict__ sin,
                                                    double* __restrict__ xout, double* __restrict__ vout, double* __restrict__ pout,
                                                    FireState64* __restrict__ sout) {
    static_assert(CHUNK % 128 == 0, "a pass of the two-column main loop (j, j + 64, stride 128) never straddles a chunk");
#define C3D_F64_CHUNKED 1
#define C3D_F64_LBFGS 0
#define C3D_F64_EVAL 0
#include "c3d_f64_step_body.inc"
#undef C3D_F64_EVAL
#undef C3D_F64_LBFGS
#undef C3D_F64_CHUNKED
}

// ---- the L-BFGS stage (kinds 9 / 8) in fp64: the twins of k_lbfgs_eval and k_lbfgs_move (c3d_lbfgs.h), two launches a step ----------
// fixed tree over the 8 rows of a tile (row_sum8's order)
__device__ __forceinline__ double row_sum8_64(const double* q, int stride) {
    return ((q[0] + q[stride]) + (q[2 * stride] + q[3 * stride])) + ((q[4 * stride] + q[5 * stride]) + (q[6 * stride] + q[7 * stride]));
}

// The evaluation: k64_step's forces of a tile's rows (the same body text: staging, passes, sums and chain terms in its order, so its bits),
// then vout = F, y = vin - F (vin = the previous evaluation's force) into ring slot nxt of hist, and the tile's kLbfgsQ sums into part.
// hist [nrep][2: s, y][kLbfgsMaxPairs][3][np], part [nrep][ntiles][kLbfgsQ], both doubles.
template <int POT, bool GEN, bool FOLD = false>
__global__ __launch_bounds__(kBlock64) __attribute__((amdgpu_waves_per_eu(5))) void k64_lbfgs_eval(const Model64 m, const Step64 p, const int rep_base,
                                                    const double* __restrict__ T, const double* __restrict__ xin,
                                                    const double* __restrict__ vin, double* __restrict__ vout,
                                                    double* __restrict__ hist, double* __restrict__ part,
                                                    const LbfgsState* __restrict__ lsin, const int mem0) {
#define C3D_F64_CHUNKED 0
#define C3D_F64_LBFGS 1
#define C3D_F64_EVAL 0
#include "c3d_f64_step_body.inc"
#undef C3D_F64_EVAL
#undef C3D_F64_LBFGS
#undef C3D_F64_CHUNKED
}
template <int POT, bool GEN, bool FOLD, int CHUNK>
__global__ __launch_bounds__(kBlock64) __attribute__((amdgpu_waves_per_eu(5))) void k64_lbfgs_eval_chunked(const Model64 m, const Step64 p, const int rep_base,
                                                    const double* __restrict__ T, const double* __restrict__ xin,
                                                    const double* __restrict__ vin, double* __restrict__ vout,
                                                    double* __restrict__ hist, double* __restrict__ part,
                                                    const LbfgsState* __restrict__ lsin, const int mem0) {
    static_assert(CHUNK % 128 == 0, "a pass of the two-column main loop (j, j + 64, stride 128) never straddles a chunk");
#define C3D_F64_CHUNKED 1
#define C3D_F64_LBFGS 1
#define C3D_F64_EVAL 0
#include "c3d_f64_step_body.inc"
#undef C3D_F64_EVAL
#undef C3D_F64_LBFGS
#undef C3D_F64_CHUNKED
}

// c3d_lbfgs_move_row.inc in doubles (k64_lbfgs_move, k64_lbfgs_move_rows): the per-bead cap with 1 / |d| as k64_step's clamp forms it,
// beyond the seed's range included (cap_scale_wide64)
#define C3D_LBFGS_T double
#define C3D_LBFGS_FMA fma
#define C3D_LBFGS_CAP                                                                              \
        const double l2 = fma(dx, dx, fma(dy, dy, dz * dz));                                       \
        if (l2 > fp.max_step * fp.max_step) {                                                      \
            double len, hh;                                                                        \
            sqrt_hrsqrt64(l2, len, hh);                                                            \
            hh = fma(fma(-len, hh, 0.5), hh, hh);                                                  \
            const double scl = cap_scale_wide64(l2, true, fp.max_step, fp.max_step * (hh + hh));   \
            dx *= scl; dy *= scl; dz *= scl;                                                       \
        }
// The move: k_lbfgs_move in doubles.  Every workgroup of a replica forms the replica sums of the tile partials in one fixed order (lane l
// takes tiles l, l + 64, ..., then the butterfly), thread 0 the compact form (pair test, gamma, the two triangular solves, the descent test
// with memory drop); then its rows: direction, the per-bead cap at max_step, the move, s into the ring; P = (move.move, F.F, 0, 0) per tile.
__global__ __launch_bounds__(kLbfgsMoveRows64) void k64_lbfgs_move(const Model64 m, const Step64 p, const Fire64 fp, const int rep_base,
                                                                   const double* __restrict__ xin, double* __restrict__ xout,
                                                                   const double* __restrict__ fcur, double* __restrict__ hist,
                                                                   const double* __restrict__ part, double* __restrict__ pout,
                                                                   const LbfgsState* __restrict__ sin, LbfgsState* __restrict__ sout,
                                                                   const int mem0) {
    constexpr int Q = kLbfgsQ, M = kLbfgsMaxPairs, ROWS = kLbfgsMoveRows64;
    __shared__ double sums[Q];
    __shared__ LbfgsState st;
    __shared__ double coef[1 + 2 * M];           // gamma, then a_j (of s_j), b_j (of y_j) by slot
    __shared__ int shi[2];                       // slot mask of the pairs in the direction, slot of the move's s
    __shared__ double dd[ROWS];
    const int rep = rep_base + blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool first = p.kind == kLbfgsFirst;
    // 1. replica sums of the tile partials: the same order in every workgroup, whatever the replica group
    const double* pr = part + (size_t)rep * m.ntiles * Q;
    for (int k = wave; k < Q; k += ROWS / 64) {
        double a = 0.0;
        for (int t = lane; t < m.ntiles; t += 64) a += pr[(size_t)t * Q + k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if (lane == 0) sums[k] = a;
    }
    if (!first) {
        const double* src = reinterpret_cast<const double*>(sin + rep);
        double* dst = reinterpret_cast<double*>(&st);
        for (int k = tid; k < (int)(sizeof(LbfgsState) / sizeof(double)); k += ROWS) dst[k] = src[k];
    }
    __syncthreads();
    // 2. the compact form, serially: c3d_lbfgs_serial.inc, k_lbfgs_move's text
    if (tid == 0) {
#define C3D_LBFGS_COEF double
#define C3D_LBFGS_GAMMA0 (fp.dt_start * fp.dt_start * p.kacc)                /* kind 6's first step length in k64_step */
#include "c3d_lbfgs_serial.inc"
#undef C3D_LBFGS_GAMMA0
#undef C3D_LBFGS_COEF
    }
    __syncthreads();
    // 3. the rows of this workgroup
    const int i = blockIdx.x * ROWS + tid;
    const int np = m.np;
    const size_t roff = (size_t)rep * 3 * np;
    double d2 = 0.0;
    if (i < m.n) {
#include "c3d_lbfgs_move_row.inc"
    }
    dd[tid] = d2;
    __syncthreads();
    // 4. P[parity^1] of this workgroup's tiles: (move.move, F.F of the evaluation, 0, 0) — where k64_export and the exit test look
    constexpr int WT = ROWS / kTileRows;
    const int t = blockIdx.x * WT + tid;
    if (tid < WT && t < m.ntiles) {
        double* po = pout + ((size_t)rep * m.ntiles + t) * 4;
        po[0] = row_sum8_64(dd + kTileRows * tid, 1); po[1] = pr[(size_t)t * Q + Q - 3]; po[2] = 0.0; po[3] = 0.0;
    }
    // 5. the replica's state: one workgroup writes it
    if (blockIdx.x == 0) {
        const double* src = reinterpret_cast<const double*>(&st);
        double* dst = reinterpret_cast<double*>(sout + rep);
        for (int k = tid; k < (int)(sizeof(LbfgsState) / sizeof(double)); k += ROWS) dst[k] = src[k];
    }
}

// ---- the forces hook of a precision-64 context (c3d_eval_f64): k64_step's force, nothing else ----------
// The same body text once more (C3D_F64_EVAL): staging, chunk pipeline, passes, reduce_rows64, the FOLD multiply and the chain butterfly
// are k64_step's lines, so F has the bits of the force k64_step and k64_lbfgs_eval integrate.  fout [nrep][3][np] is a buffer of the
// context's own (never the velocity slot); p.kind is 3 (no kind-4 "no force" step here).
template <int POT, bool GEN, bool FOLD = false>
__global__ __launch_bounds__(kBlock64) __attribute__((amdgpu_waves_per_eu(5))) void k64_eval_forces(const Model64 m, const Step64 p, const int rep_base,
                                                    const double* __restrict__ T, const double* __restrict__ xin,
                                                    double* __restrict__ fout) {
#define C3D_F64_CHUNKED 0
#define C3D_F64_LBFGS 0
#define C3D_F64_EVAL 1
#include "c3d_f64_step_body.inc"
#undef C3D_F64_EVAL
#undef C3D_F64_LBFGS
#undef C3D_F64_CHUNKED
}
template <int POT, bool GEN, bool FOLD, int CHUNK>
__global__ __launch_bounds__(kBlock64) __attribute__((amdgpu_waves_per_eu(5))) void k64_eval_forces_chunked(const Model64 m, const Step64 p, const int rep_base,
                                                    const double* __restrict__ T, const double* __restrict__ xin,
                                                    double* __restrict__ fout) {
    static_assert(CHUNK % 128 == 0, "a pass of the two-column main loop (j, j + 64, stride 128) never straddles a chunk");
#define C3D_F64_CHUNKED 1
#define C3D_F64_LBFGS 0
#define C3D_F64_EVAL 1
#include "c3d_f64_step_body.inc"
#undef C3D_F64_EVAL
#undef C3D_F64_LBFGS
#undef C3D_F64_CHUNKED
}

// k_energy (c3d_device.hip) over the fp64 coordinates and the fp64 targets T [n][np] (Angstrom; "no restraint" is 0, or kNoTarget64 where the
// fast soft lower side runs): unweighted energies (noe x S, bond + angle, repel x k_rep) of a replica, eout [nrep][4].  One workgroup per
// replica; thread t takes rows t, t + 256, ... and the pairs j > i in ascending order, the 256 partial sums meet in one fixed LDS tree: two
// calls return the same bits.  Square roots are the correctly rounded ones (this is not a hot path); rep_r2 = (repel_s r0_rep)^2 in double.
__global__ __launch_bounds__(256) void k64_energy(const Model64 m, const double rep_r2, const double* __restrict__ T,
                                                 const double* __restrict__ xin, double* __restrict__ eout) {
    __shared__ double red[3][256];
    const int rep = blockIdx.x, tid = threadIdx.x, np = m.np;
    const double* x = xin + (size_t)rep * 3 * np;
    const double* y = x + np;
    const double* z = y + np;
    double e_noe = 0, e_bond = 0, e_rep = 0;
    const double rs = m.rs, c = m.tail_c, b = m.tail_b;
    const double a = rs * rs - b / rs - c * rs;
    // lower side of potentials 3 / 4: E = ma + mb / D^mexp + mc D beyond mrs (Model64::mtail_b is the force's coefficient: mb x mexp)
    const bool pot3 = m.noe_pot == 3 || m.noe_pot == 4;
    const double mrs = m.mrs, mc = m.mtail_c, mb = m.mexp == 2 ? 0.5 * m.mtail_b : m.mtail_b;
    const double ma = mrs * mrs - (m.mexp == 2 ? mb / (mrs * mrs) : mb / mrs) - mc * mrs;
    const double a0sq = m.a0 * m.a0;
    for (int i = tid; i < m.n; i += 256) {
        const double xi = x[i], yi = y[i], zi = z[i];
        const double* Ti = T + (size_t)i * np;
        for (int j = i + 1; j < m.n; ++j) {
            const double dx = xi - x[j], dy = yi - y[j], dz = zi - z[j];
            double r2 = dx * dx + dy * dy + dz * dz;
            if (r2 < 1e-12) r2 = 1e-12;
            const double t = Ti[j];
            const int sep = j - i;
            if (t > 0 && t < 0.5 * kNoTarget64) {
                const double delta = sqrt(r2) - t, ad = fabs(delta);
                bool soft;
                if (m.noe_pot == 0) soft = ad > rs; else if (m.noe_pot == 1 || pot3) soft = delta > rs; else soft = false;
                if (pot3 && delta < -mrs) e_noe += ma + (m.mexp == 2 ? mb / (ad * ad) : mb / ad) + mc * ad;
                else e_noe += soft ? (a + b / ad + c * ad) : delta * delta;
            }
            if (sep == 1) { const double dl = sqrt(r2) - m.b0; e_bond += m.k_bond * dl * dl; }
            if (sep == 2 && m.k_ang > 0 && (m.ang_mode == 1 || r2 < a0sq)) { const double dl = sqrt(r2) - m.a0; e_bond += m.k_ang * dl * dl; }
            if (sep >= m.rep_sep && r2 < rep_r2) { const double q = rep_r2 - r2; e_rep += q * q; }
        }
    }
    red[0][tid] = e_noe * m.s_noe; red[1][tid] = e_bond; red[2][tid] = e_rep * m.k_rep;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { red[0][tid] += red[0][tid + s]; red[1][tid] += red[1][tid + s]; red[2][tid] += red[2][tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { eout[rep * 4 + 0] = red[0][0]; eout[rep * 4 + 1] = red[1][0]; eout[rep * 4 + 2] = red[2][0]; eout[rep * 4 + 3] = 0; }
}

// T[i][j] = 0.1 * t10 where a restraint exists (|i-j| >= min_sep, t10 > 0), else 0; np columns per row
__global__ __launch_bounds__(256) void k64_targets(int n, int np, int min_sep, double none, const int32_t* __restrict__ t10, double* __restrict__ T) {
    const int i = blockIdx.x;
    for (int j = threadIdx.x; j < np; j += 256) {
        double v = none;
        if (j < n) {
            const int sep = j > i ? j - i : i - j;
            const int32_t t = t10[(size_t)i * n + j];
            if (sep >= min_sep && t > 0) v = 0.1 * t;
        }
        T[(size_t)i * np + j] = v;
    }
}

// t10[i][j] = t10[j][i] = the tenths of restraint k (a list with every pair once: no two threads write the same element)
__global__ __launch_bounds__(256) void k64_tenths(int n, int R, const int32_t* __restrict__ ri, const int32_t* __restrict__ rj,
                                                 const int32_t* __restrict__ rt10, int32_t* __restrict__ t10) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= R) return;
    const int i = ri[k], j = rj[k];
    if (i < 0 || j < 0 || i >= n || j >= n) return;
    t10[(size_t)i * n + j] = rt10[k];
    t10[(size_t)j * n + i] = rt10[k];
}

// fp32 SoA buffers [nrep][3][npad] <-> fp64 SoA state [nrep][3][np] (the solver's read-back, energies and scoring work on the fp32 copy)
__global__ __launch_bounds__(256) void k64_import(int n, int npad, int np, const float* __restrict__ Xf, double* __restrict__ X0,
                                                 double* __restrict__ X1, double* __restrict__ V0, double* __restrict__ V1) {
    const int rep = blockIdx.x;
    for (int k = threadIdx.x; k < 3 * np; k += 256) {
        const int c = k / np, i = k - c * np;
        // pad beads far away and apart from each other (repel and NOE terms vanish), as in the fp32 layout
        const double x = i < n ? (double)Xf[((size_t)rep * 3 + c) * npad + i] : (double)kPadCoord * (c + 1) + 16.0 * (i - n);
        X0[(size_t)rep * 3 * np + k] = x; X1[(size_t)rep * 3 * np + k] = x;
        V0[(size_t)rep * 3 * np + k] = 0.0; V1[(size_t)rep * 3 * np + k] = 0.0;
    }
}
__global__ __launch_bounds__(256) void k64_export(int n, int npad, int np, int ntiles, const double* __restrict__ X, const double* __restrict__ V,
                                                 const double* __restrict__ P, float* __restrict__ Xf, float* __restrict__ Vf, float* __restrict__ Pf) {
    const int rep = blockIdx.x;
    for (int k = threadIdx.x; k < 3 * n; k += 256) {
        const int c = k / n, i = k - c * n;
        Xf[((size_t)rep * 3 + c) * npad + i] = (float)X[((size_t)rep * 3 + c) * np + i];
        Vf[((size_t)rep * 3 + c) * npad + i] = (float)V[((size_t)rep * 3 + c) * np + i];
    }
    // the per-tile sums go where the host looks for them (max RMS force of the minimiser, finiteness)
    for (int t = threadIdx.x; t < 4 * ntiles; t += 256) Pf[(size_t)rep * ntiles * 4 + t] = (float)P[(size_t)rep * ntiles * 4 + t];
}

// ---- host side ---------------------------------------------------------------------------------------
int cols64(int n) { return (n + kColPad64 - 1) / kColPad64 * kColPad64; }
size_t fire_state64_bytes() { return sizeof(FireState64); }

// The builders of the kernel arguments (c3d_internal.h): the only place a derived fp64 parameter is formed.
Model64 model64(const DevModel& d, const c3d_model& h) {
    Model64 m;
    m.n = d.n; m.np = cols64(d.n); m.ntiles = d.ntiles;
    m.min_sep = h.min_sep; m.rep_sep = d.rep_sep; m.ang_mode = d.ang_mode; m.mexp = h.msoexp == 2 ? 2 : 1;
    m.s_noe = h.s_noe; m.rs = h.rswitch;
    m.tail_c = (double)h.asym * m.rs; m.tail_b = (m.tail_c - 2.0 * m.rs) * m.rs * m.rs;
    // lower side beyond mrs: dE/dD = mtail_c - mtail_b / D^(mexp + 1)
    m.mrs = h.mrswitch; m.mtail_c = h.masym; m.mtail_b = (m.mtail_c - 2.0 * m.mrs) * m.mrs * m.mrs * (m.mexp == 2 ? m.mrs : 1.0);
    m.nmrs4 = -(m.mrs * m.mrs) * (m.mrs * m.mrs);
    // the device potential that runs (form64 reads it); a potential 4 whose doubles are not the fast form's would run as 3 (cannot happen)
    m.noe_pot = d.noe_pot == 4 && !(m.mexp == 2 && m.mtail_c == 0.0 && m.tail_b == 0.0 && m.tail_c == 2.0 * m.rs) ? 3 : device_pot(d.noe_pot);
    m.k_bond = h.k_bond; m.b0 = h.b0; m.k_ang = h.k_ang; m.a0 = h.a0; m.r0_rep = h.r0_rep; m.k_rep = h.k_rep; m.mass = h.mass; m.fbeta = h.fbeta;
    { const int ndf = 3 * d.n - 3; m.t_fac = m.mass / kAccel64 / ((ndf > 0 ? ndf : 1) * kBoltz64); m.inv_n = 1.0 / d.n; }
    return m;
}
Step64 step64(const Model64& m, int kind, double dt, double w_all, double w_vdw, double repel_s, double t_bath) {
    Step64 p;
    p.kind = kind; p.dt = dt; p.w_all = w_all; p.w_vdw = w_vdw; p.repel_s = repel_s; p.t_bath = t_bath;
    p.R2 = (p.repel_s * m.r0_rep) * (p.repel_s * m.r0_rep);
    p.wr4 = p.w_vdw * m.k_rep * 4.0;
    p.nws4 = -4.0 * p.w_all * m.s_noe;
    p.wq = p.nws4 != 0.0 ? p.wr4 / p.nws4 : 0.0;
    p.acc = p.dt * kAccel64 / m.mass;
    p.kb4 = -p.w_all * 4.0 * m.k_bond; p.ka4 = -p.w_all * 4.0 * m.k_ang;
    p.kacc = kAccel64 / m.mass;
    p.a0sq = m.a0 * m.a0;
    return p;
}
Fire64 fire64(const c3d_fire_params& f) {
    Fire64 fp;
    fp.dt_start = f.dt_start; fp.dt_max = f.dt_max; fp.f_inc = f.f_inc; fp.f_dec = f.f_dec; fp.alpha_start = f.alpha_start;
    fp.f_alpha = f.f_alpha; fp.max_step = f.max_step; fp.n_min = f.n_min;
    return fp;
}

// The one runtime -> template dispatch of the force kernels (k64_step, k64_lbfgs_eval, k64_eval_forces and their chunked forms): fn is
// called with POT, GEN, FOLD, CHUNK as integral constants, CHUNK 0 = staged, else one of the instantiated set (column_chunk64_valid).
// The general forms have no potential-4 kernel (form64 never asks for one), and FOLD exists for the fast soft lower side only.
template <class Fn> static hipError_t with_form64(const Form64& f, Fn&& fn) {
    return with_pot(f.pot, [&](auto P) {
        return with_bool(f.gen, [&](auto G) {
            return with_bool(f.fold, [&](auto F) {
                constexpr int POT = G && P == 4 ? 2 : P;
                constexpr bool FOLD = F && POT == 4 && !G;
                switch (f.chunk) {
                    case 0: return fn(int_c<POT>{}, G, bool_c<FOLD>{}, int_c<0>{});
                    case 256: return fn(int_c<POT>{}, G, bool_c<FOLD>{}, int_c<256>{});
                    case 512: return fn(int_c<POT>{}, G, bool_c<FOLD>{}, int_c<512>{});
                    case 1024: return fn(int_c<POT>{}, G, bool_c<FOLD>{}, int_c<1024>{});
                    default: return hipErrorInvalidValue;
                }
            });
        });
    });
}
// doubles of LDS the columns take: the replica's three coordinate rows staged whole, or two buffers of 3 CHUNK
static size_t cols_lds64(const Model64& m, int chunk) { return chunk ? (size_t)6 * chunk : (size_t)3 * m.np; }

hipError_t launch_step64(const DevModel& d, const Model64& m, const Step64& p, const Fire64& fp, const Form64& f, const Buffers64& b, int parity,
                         hipStream_t s) {
    const int q = parity ^ 1;
    const dim3 grid(d.ntiles, d.nrep_g), blk(kBlock64);
    const size_t lds = sizeof(double) * (cols_lds64(m, f.chunk) + 4 * kTileRows + 8);
    FireState64* sin = reinterpret_cast<FireState64*>(b.S[parity]);
    FireState64* sout = reinterpret_cast<FireState64*>(b.S[q]);
    return with_form64(f, [&](auto POT, auto GEN, auto FOLD, auto CHUNK) {
        if constexpr (CHUNK == 0)
            hipLaunchKernelGGL((k64_step<POT, GEN, FOLD>), grid, blk, lds, s, m, p, fp, d.rep_base, b.T, b.X[parity], b.V[parity], b.Vinit, b.P[parity],
                               sin, b.X[q], b.V[q], b.P[q], sout);
        else
            hipLaunchKernelGGL((k64_step_chunked<POT, GEN, FOLD, CHUNK>), grid, blk, lds, s, m, p, fp, d.rep_base, b.T, b.X[parity], b.V[parity], b.Vinit,
                               b.P[parity], sin, b.X[q], b.V[q], b.P[q], sout);
        return hipGetLastError();
    });
}
// The kernel of an L-BFGS evaluation in the step's form (staged up to 2560 beads, chunked beyond or where f64_column_chunk asks): reads
// X[parity] and the previous force V[parity], writes the force V[parity^1], ring slot and tile sums
hipError_t launch_lbfgs_eval64(const DevModel& d, const Model64& m, const Step64& p, const Form64& f, const Buffers64& b, const LbfgsBuffers64& lb,
                               int parity, int mem, hipStream_t s) {
    if (mem < 1 || mem > kLbfgsMaxPairs) return hipErrorInvalidValue;
    const int q = parity ^ 1;
    const dim3 grid(d.ntiles, d.nrep_g), blk(kBlock64);
    const size_t lds = sizeof(double) * (cols_lds64(m, f.chunk) + (size_t)kLbfgsQ * kTileRows);
    return with_form64(f, [&](auto POT, auto GEN, auto FOLD, auto CHUNK) {
        if constexpr (CHUNK == 0)
            hipLaunchKernelGGL((k64_lbfgs_eval<POT, GEN, FOLD>), grid, blk, lds, s, m, p, d.rep_base, b.T, b.X[parity], b.V[parity], b.V[q], lb.hist,
                               lb.part, lb.S[parity], mem);
        else
            hipLaunchKernelGGL((k64_lbfgs_eval_chunked<POT, GEN, FOLD, CHUNK>), grid, blk, lds, s, m, p, d.rep_base, b.T, b.X[parity], b.V[parity], b.V[q],
                               lb.hist, lb.part, lb.S[parity], mem);
        return hipGetLastError();
    });
}
// the move that follows it: X[parity] -> X[parity^1], P[parity^1], the state S[parity] -> S[parity^1]
hipError_t launch_lbfgs_move64(const DevModel& d, const Model64& m, const Step64& p, const Fire64& fp, const Buffers64& b, const LbfgsBuffers64& lb,
                               int parity, int mem, hipStream_t s) {
    if (mem < 1 || mem > kLbfgsMaxPairs) return hipErrorInvalidValue;
    const int q = parity ^ 1;
    hipLaunchKernelGGL(k64_lbfgs_move, dim3((d.n + kLbfgsMoveRows64 - 1) / kLbfgsMoveRows64, d.nrep_g), dim3(kLbfgsMoveRows64), 0, s, m, p, fp,
                       d.rep_base, b.X[parity], b.X[q], b.V[q], lb.hist, lb.part, b.P[q], lb.S[parity], lb.S[q], mem);
    return hipGetLastError();
}
// The rows of k64_lbfgs_move as a table (c3d_debug_lbfgs_move_rows on a precision-64 context): k_lbfgs_move_rows in doubles.
__global__ void k64_lbfgs_move_rows(const Fire64 fp, const int rows, const int np, const double* __restrict__ coef_in, const int mask_in,
                                    const int slot, const double* __restrict__ xin, double* __restrict__ xout, const double* __restrict__ fcur,
                                    double* __restrict__ hist, double* __restrict__ d2out) {
    constexpr int M = kLbfgsMaxPairs;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    double coef[1 + 2 * M];
    for (int k = 0; k < 1 + 2 * M; ++k) coef[k] = coef_in[k];
    const int shi[2] = {mask_in, slot};
    const int rep = 0;
    const size_t roff = 0;
    double d2 = 0.0;
    {
#include "c3d_lbfgs_move_row.inc"
    }
    d2out[i] = d2;
}
#undef C3D_LBFGS_CAP
#undef C3D_LBFGS_FMA
#undef C3D_LBFGS_T
hipError_t launch_lbfgs_move_rows64(const Fire64& fp, int rows, int np, const double* coef, int mask, int slot, const double* xin, double* xout,
                                    const double* fcur, double* hist, double* d2, hipStream_t s) {
    hipLaunchKernelGGL(k64_lbfgs_move_rows, dim3((rows + 63) / 64), dim3(64), 0, s, fp, rows, np, coef, mask, slot, xin, xout, fcur, hist, d2);
    return hipGetLastError();
}
// The serial section of k64_lbfgs_move as a table (c3d_debug_lbfgs_direction on a precision-64 context): k_lbfgs_direction in doubles.
__global__ void k64_lbfgs_direction(const Step64 p, const Fire64 fp, const int rows, const double* __restrict__ sums_in,
                                    const LbfgsState* __restrict__ sin, const int* __restrict__ flags, LbfgsState* __restrict__ sout,
                                    double* __restrict__ coef_out, int* __restrict__ shi_out) {
    constexpr int Q = kLbfgsQ, M = kLbfgsMaxPairs;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double sums[Q];
    for (int k = 0; k < Q; ++k) sums[k] = sums_in[(size_t)r * Q + k];
    LbfgsState st = sin[r];
    double coef[1 + 2 * M];
    int shi[2];
    const bool first = flags[2 * r] != 0;
    const int mem0 = flags[2 * r + 1];
    {
#define C3D_LBFGS_COEF double
#define C3D_LBFGS_GAMMA0 (fp.dt_start * fp.dt_start * p.kacc)
#include "c3d_lbfgs_serial.inc"
#undef C3D_LBFGS_GAMMA0
#undef C3D_LBFGS_COEF
    }
    sout[r] = st;
    for (int k = 0; k < 1 + 2 * M; ++k) coef_out[(size_t)r * (1 + 2 * M) + k] = coef[k];
    shi_out[2 * r] = shi[0]; shi_out[2 * r + 1] = shi[1];
}
hipError_t launch_lbfgs_direction64(const Step64& p, const Fire64& fp, int rows, const double* sums, const LbfgsState* in, const int* flags,
                                    LbfgsState* out, double* coef, int* shi, hipStream_t s) {
    hipLaunchKernelGGL(k64_lbfgs_direction, dim3((rows + 63) / 64), dim3(64), 0, s, p, fp, rows, sums, in, flags, out, coef, shi);
    return hipGetLastError();
}
// The controller of k64_step as a table (c3d_debug_step_scalars_f64): c3d_f64_scalars.inc — the text wave 0 of every k64_step workgroup
// runs on the replica's sums — a thread a row, on (psum[4], FireState64) as given whatever the kind.  out [rows][6] = lam, cm0 .. cm2, keep, mix.
__global__ void k64_step_scalars(const Model64 m, const Step64 p, const Fire64 fp, const int rows, const double* __restrict__ psum,
                                 const FireState64* __restrict__ sin, double* __restrict__ out, FireState64* __restrict__ sout) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const double s0 = psum[4 * (size_t)r], s1 = psum[4 * (size_t)r + 1], s2 = psum[4 * (size_t)r + 2], s3 = psum[4 * (size_t)r + 3];
    FireState64 st = sin[r];
    {
#define C3D_F64_STATE_OUT
#include "c3d_f64_scalars.inc"
#undef C3D_F64_STATE_OUT
        double* o = out + 6 * (size_t)r;
        o[0] = lam; o[1] = cm0; o[2] = cm1; o[3] = cm2; o[4] = keep; o[5] = mix;
    }
    sout[r] = st;
}
hipError_t launch_step_scalars64(const Model64& m, const Step64& p, const Fire64& fp, int rows, const double* psum, const void* in, double* scalars,
                                 void* out, hipStream_t s) {
    hipLaunchKernelGGL(k64_step_scalars, dim3((rows + 63) / 64), dim3(64), 0, s, m, p, fp, rows, psum, static_cast<const FireState64*>(in), scalars,
                       static_cast<FireState64*>(out));
    return hipGetLastError();
}
// The row update of k64_step as a table (c3d_debug_row_finish_f64): c3d_f64_row_finish.inc — the text lanes 0 and 1 of every k64_step wave
// run on their row — a thread a row.  in [rows][16] = x0[3], v0[3], F[3], lam, cm0 .. cm2, keep, mix, st.dt; out [rows][10] = xn[3], vn[3], q0 .. q3.
__global__ void k64_row_finish(const Step64 p, const Fire64 fp, const int rows, const double* __restrict__ in, double* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const double* a = in + kRowFinish64In * (size_t)r;
    const double x0 = a[0], y0 = a[1], z0 = a[2], v0x = a[3], v0y = a[4], v0z = a[5], Fx = a[6], Fy = a[7], Fz = a[8];
    const double lam = a[9], cm0 = a[10], cm1 = a[11], cm2 = a[12], keep = a[13], mix = a[14];
    FireState64 st;
    st.dt = a[15]; st.alpha = 0.0; st.npos = 0; st.pad = 0;
    double q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    {
#include "c3d_f64_row_finish.inc"
        double* o = out + kRowFinish64Out * (size_t)r;
        o[0] = xn; o[1] = yn; o[2] = zn; o[3] = vx; o[4] = vy; o[5] = vz; o[6] = q0; o[7] = q1; o[8] = q2; o[9] = q3;
    }
}
hipError_t launch_row_finish64(const Step64& p, const Fire64& fp, int rows, const double* in, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k64_row_finish, dim3((rows + 63) / 64), dim3(64), 0, s, p, fp, rows, in, out);
    return hipGetLastError();
}
// c3d_eval_f64's force in the step's form (p of kind 3), X[parity] -> Fout
hipError_t launch_eval_forces64(const DevModel& d, const Model64& m, const Step64& p, const Form64& f, const Buffers64& b, int parity, double* Fout,
                                hipStream_t s) {
    const dim3 grid(d.ntiles, d.nrep_g), blk(kBlock64);
    const size_t lds = sizeof(double) * cols_lds64(m, f.chunk);
    return with_form64(f, [&](auto POT, auto GEN, auto FOLD, auto CHUNK) {
        if constexpr (CHUNK == 0) hipLaunchKernelGGL((k64_eval_forces<POT, GEN, FOLD>), grid, blk, lds, s, m, p, d.rep_base, b.T, b.X[parity], Fout);
        else hipLaunchKernelGGL((k64_eval_forces_chunked<POT, GEN, FOLD, CHUNK>), grid, blk, lds, s, m, p, d.rep_base, b.T, b.X[parity], Fout);
        return hipGetLastError();
    });
}
hipError_t launch_energy64(const DevModel& d, const Model64& m, double rep_r2, const Buffers64& b, int parity, double* Eout, hipStream_t s) {
    hipLaunchKernelGGL(k64_energy, dim3(d.nrep), dim3(256), 0, s, m, rep_r2, b.T, b.X[parity], Eout);
    return hipGetLastError();
}
hipError_t launch_targets64(const Model64& m, const Form64& f, const int32_t* t10, double* T, hipStream_t s) {
    const double none = (f.pot == 4 && !f.gen) ? kNoTarget64 : 0.0;        // what pair64 of the kernel that will run expects
    hipLaunchKernelGGL(k64_targets, dim3(m.n), dim3(256), 0, s, m.n, m.np, m.min_sep, none, t10, T);
    return hipGetLastError();
}
hipError_t launch_tenths64(int n, int R, const int32_t* ri, const int32_t* rj, const int32_t* rt10, int32_t* t10, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    hipLaunchKernelGGL(k64_tenths, dim3((R + 255) / 256), dim3(256), 0, s, n, R, ri, rj, rt10, t10);
    return hipGetLastError();
}
hipError_t launch_import64(const DevModel& d, const float* Xf, const Buffers64& b, hipStream_t s) {
    hipLaunchKernelGGL(k64_import, dim3(d.nrep), dim3(256), 0, s, d.n, d.npad, cols64(d.n), Xf, b.X[0], b.X[1], b.V[0], b.V[1]);
    return hipGetLastError();
}
hipError_t launch_export64(const DevModel& d, const Buffers64& b, int parity, float* Xf, float* Vf, float* Pf, hipStream_t s) {
    hipLaunchKernelGGL(k64_export, dim3(d.nrep), dim3(256), 0, s, d.n, d.npad, cols64(d.n), d.ntiles, b.X[parity], b.V[parity], b.P[parity], Xf, Vf, Pf);
    return hipGetLastError();
}

hipError_t preload_f64_unit() {
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&k64_import));
}

}  // namespace c3d
