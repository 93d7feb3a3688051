// c3d_debug.cpp — host unit of libc3d.so: the table test hooks (c3d.h, "Test hook") of the step controller, the row update and the L-BFGS
// move — c3d_debug_step_scalars, c3d_debug_row_finish, their _f64 twins, c3d_debug_lbfgs_direction, c3d_debug_lbfgs_move_rows.  Each runs
// the text a step kernel runs on a table of rows and touches nothing of the solve: its refusals, its launch, its unpacking.  The model,
// the FIRE values and the step are built by the functions every launch uses (dev_model, dev_fire, dev_step; model64, fire64, step64), so a
// table also covers what the host folds into them (acc, kacc, t_fac, inv_n).
// (c3d_debug_tear16 and the stamp readers stay in c3d_api.cpp, the two rank hooks in c3d_analysis.cpp with that unit's scratch types.)
#include "c3d_ctx.h"

using namespace c3d::host;

namespace {
// A device table for the length of a hook, on the context's stream: `count` elements uploaded from a host pointer, or zero-filled;
// downloaded to a host pointer.  The hook synchronises the stream after its last download.
template <class T>
struct DevTable : DevTmp<T> {
    size_t bytes = 0;
    int upload(c3d_ctx* c, size_t count, const T* src) {
        HIP_TRY(hipMalloc(&this->p, bytes = sizeof(T) * count));
        HIP_TRY(hipMemcpyAsync(this->p, src, bytes, hipMemcpyHostToDevice, c->stream));
        return C3D_OK;
    }
    int zeros(c3d_ctx* c, size_t count) {
        HIP_TRY(hipMalloc(&this->p, bytes = sizeof(T) * count));
        HIP_TRY(hipMemsetAsync(this->p, 0, bytes, c->stream));
        return C3D_OK;
    }
    int download(c3d_ctx* c, T* dst) const {
        HIP_TRY(hipMemcpyAsync(dst, this->p, bytes, hipMemcpyDeviceToHost, c->stream));
        return C3D_OK;
    }
};
// a table call: its failure is the entry's
#define TABLE_TRY(expr) do { if (const int rc__ = (expr)) return rc__; } while (0)

// a controller state as the step-scalar hooks take and return it: (dt, alpha) pairs and npos, row by row
template <class State, class F>
void pack_states(std::vector<State>& st, const F* state_in, const int32_t* npos_in) {
    for (size_t r = 0; r < st.size(); ++r) st[r] = State{state_in[2 * r], state_in[2 * r + 1], npos_in[r], 0};
}
template <class State, class F>
void unpack_states(const std::vector<State>& st, F* state_out, int32_t* npos_out) {
    for (size_t r = 0; r < st.size(); ++r) { state_out[2 * r] = st[r].dt; state_out[2 * r + 1] = st[r].alpha; npos_out[r] = st[r].npos; }
}
}  // namespace

// Test hook: step_scalars<true> on a table of rows (c3d.h).
extern "C" int c3d_debug_step_scalars(c3d_ctx* c, int kind, float dt, float t_bath, int rows, const float* psum, const float* state_in,
                                      const int32_t* npos_in, float* scalars, float* state_out, int32_t* npos_out) {
    if (!c || !psum || !state_in || !npos_in || !scalars || !state_out || !npos_out || rows < 1 || rows > (1 << 20))
        return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars: bad arguments");
    if (!(kind == 0 || kind == 1 || kind == 2 || kind == 3 || kind == 5 || kind == 6))
        return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars: kind is 0, 1, 2, 3, 5 or 6");
    if (c->n < 1) return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars: set the targets first (the bead count enters the temperature)");
    C3D_ENTRY(c, unit_bit(UNIT_SYM));
    const size_t n = (size_t)rows;
    std::vector<c3d::FireState> st(n);
    pack_states(st, state_in, npos_in);
    DevTable<float> d_psum, d_out;
    DevTable<c3d::FireState> d_in, d_st;
    TABLE_TRY(d_psum.upload(c, 4 * n, psum));
    TABLE_TRY(d_in.upload(c, n, st.data()));
    TABLE_TRY(d_out.zeros(c, 6 * n));
    TABLE_TRY(d_st.zeros(c, n));
    LAUNCH_TRY("step scalars launch", c3d::launch_step_scalars(dev_model(c), dev_step(c, kind, dt, 1.0f, 1.0f, 0.85f, t_bath), dev_fire(c), rows,
                                                               d_psum.p, d_in.p, d_out.p, d_st.p, c->stream));
    TABLE_TRY(d_out.download(c, scalars));
    TABLE_TRY(d_st.download(c, st.data()));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unpack_states(st, state_out, npos_out);
    return C3D_OK;
}

// Test hook: finish_row on a table of rows (c3d.h) — the row update that consumes c3d_debug_step_scalars' scalars, under the same
// DevModel / DevStep / DevFire (acc = 418.4 / mass and max_step as the host holds them; the kernel forms dt acc itself).
extern "C" int c3d_debug_row_finish(c3d_ctx* c, int kind, float dt, int rows, const float* in, float* out) {
    if (!c || !in || !out) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish: bad arguments");
    if (rows < 1 || rows > (1 << 20)) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish: rows is 1 .. 2^20");
    if (kind < 0 || kind > 6) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish: kind is 0, 1, 2, 3, 4, 5 or 6");
    if (c->n < 1) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish: set the targets first (the model is built for a bead count)");
    C3D_ENTRY(c, unit_bit(UNIT_SYM));
    DevTable<float> d_in, d_out;
    TABLE_TRY(d_in.upload(c, C3D_ROW_FINISH_IN * (size_t)rows, in));
    TABLE_TRY(d_out.zeros(c, C3D_ROW_FINISH_OUT * (size_t)rows));
    LAUNCH_TRY("row finish launch", c3d::launch_row_finish(dev_model(c), dev_step(c, kind, dt, 1.0f, 1.0f, 0.85f, 0.0f), dev_fire(c), rows, d_in.p,
                                                           d_out.p, c->stream));
    TABLE_TRY(d_out.download(c, out));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

// Test hooks: the fp64 controller (c3d_f64_scalars.inc) and the fp64 row update (c3d_f64_row_finish.inc) on tables of rows (c3d.h).
// The stage weights of the Step64 (1, 1, 0.85) enter neither text.
namespace {
struct FireRow64 { double dt, alpha; int32_t npos, pad; };       // a FireState64 (c3d_f64.hip) as the host packs it
bool f64_table_kind(int kind, bool row_finish) {
    return kind == 0 || kind == 1 || kind == 2 || kind == 3 || kind == 5 || kind == 6 || (row_finish && kind == 4);
}
}  // namespace
extern "C" int c3d_debug_step_scalars_f64(c3d_ctx* c, int kind, double dt, double t_bath, int rows, const double* psum, const double* state_in,
                                          const int32_t* npos_in, double* scalars, double* state_out, int32_t* npos_out) {
    if (!c || !psum || !state_in || !npos_in || !scalars || !state_out || !npos_out)
        return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars_f64: bad arguments");
    if (rows < 1 || rows > (1 << 20)) return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars_f64: rows is 1 .. 2^20");
    if (!f64_table_kind(kind, false)) return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars_f64: kind is 0, 1, 2, 3, 5 or 6");
    if (c->precision != 64) return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars_f64: the context's precision is not 64");
    if (c->n < 1) return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars_f64: set the targets first (the bead count enters the temperature)");
    if (sizeof(FireRow64) != c3d::fire_state64_bytes()) return fail(C3D_ERR_INVALID, "c3d_debug_step_scalars_f64: the state's layout is not the one this entry packs");
    C3D_ENTRY(c, unit_bit(UNIT_F64));
    const size_t n = (size_t)rows;
    std::vector<FireRow64> st(n);
    pack_states(st, state_in, npos_in);
    DevTable<double> d_psum, d_out;
    DevTable<FireRow64> d_in, d_st;
    TABLE_TRY(d_psum.upload(c, 4 * n, psum));
    TABLE_TRY(d_in.upload(c, n, st.data()));
    TABLE_TRY(d_out.zeros(c, 6 * n));
    TABLE_TRY(d_st.zeros(c, n));
    const c3d::Model64 m64 = c3d::model64(dev_model(c), c->model);
    LAUNCH_TRY("fp64 step scalars launch", c3d::launch_step_scalars64(m64, c3d::step64(m64, kind, dt, 1.0, 1.0, 0.85, t_bath), c3d::fire64(c->fire), rows,
                                                                     d_psum.p, d_in.p, d_out.p, d_st.p, c->stream));
    TABLE_TRY(d_out.download(c, scalars));
    TABLE_TRY(d_st.download(c, st.data()));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unpack_states(st, state_out, npos_out);
    return C3D_OK;
}
static_assert(C3D_ROW_FINISH_IN == c3d::kRowFinish64In && C3D_ROW_FINISH_OUT == c3d::kRowFinish64Out, "c3d.h states the row table's sizes");
extern "C" int c3d_debug_row_finish_f64(c3d_ctx* c, int kind, double dt, int rows, const double* in, double* out) {
    if (!c || !in || !out) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish_f64: bad arguments");
    if (rows < 1 || rows > (1 << 20)) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish_f64: rows is 1 .. 2^20");
    if (!f64_table_kind(kind, true)) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish_f64: kind is 0, 1, 2, 3, 4, 5 or 6");
    if (c->precision != 64) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish_f64: the context's precision is not 64");
    if (c->n < 1) return fail(C3D_ERR_INVALID, "c3d_debug_row_finish_f64: set the targets first (the model is built for a bead count)");
    C3D_ENTRY(c, unit_bit(UNIT_F64));
    DevTable<double> d_in, d_out;
    TABLE_TRY(d_in.upload(c, C3D_ROW_FINISH_IN * (size_t)rows, in));
    TABLE_TRY(d_out.zeros(c, C3D_ROW_FINISH_OUT * (size_t)rows));
    const c3d::Model64 m64 = c3d::model64(dev_model(c), c->model);
    LAUNCH_TRY("fp64 row finish launch", c3d::launch_row_finish64(c3d::step64(m64, kind, dt, 1.0, 1.0, 0.85, 0.0), c3d::fire64(c->fire), rows, d_in.p,
                                                                 d_out.p, c->stream));
    TABLE_TRY(d_out.download(c, out));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return C3D_OK;
}

// Test hook: the serial section of the L-BFGS move (c3d_lbfgs_serial.inc) on a table of rows (c3d.h) — k_lbfgs_direction, or
// k64_lbfgs_direction on a precision-64 context.  The first step's gamma is formed from what the host folds into the model (acc, kacc).
static_assert(C3D_LBFGS_MAX_PAIRS == c3d::kLbfgsMaxPairs && C3D_LBFGS_SUMS == c3d::kLbfgsQ, "c3d.h states the L-BFGS stage's sizes");
static_assert(sizeof(c3d::LbfgsState) == 4 * sizeof(int32_t) + C3D_LBFGS_STATE_DOUBLES * sizeof(double), "LbfgsState is 4 ints, then doubles");
extern "C" int c3d_debug_lbfgs_direction(c3d_ctx* c, int rows, const double* sums, const int32_t* state_int_in, const double* state_dbl_in,
                                         const int32_t* first, const int32_t* mem0, int32_t* state_int_out, double* state_dbl_out,
                                         double* coef, int32_t* mask_slot) {
    if (!c || !sums || !state_int_in || !state_dbl_in || !first || !mem0 || !state_int_out || !state_dbl_out || !coef || !mask_slot ||
        rows < 1 || rows > (1 << 16))
        return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_direction: bad arguments");
    for (int r = 0; r < rows; ++r)
        if (mem0[r] < 1 || mem0[r] > c3d::kLbfgsMaxPairs) return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_direction: mem0 is 1 .. 8 (lbfgs_memory)");
    if (c->n < 1) return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_direction: set the targets first (the model is built for a bead count)");
    const bool f64 = c->precision == 64;
    C3D_ENTRY(c, f64 ? unit_bit(UNIT_F64) : 0u);
    constexpr int ND = C3D_LBFGS_STATE_DOUBLES, NC = C3D_LBFGS_COEFS;
    const size_t n = (size_t)rows;
    std::vector<c3d::LbfgsState> st(n);
    std::vector<int> flags(2 * n);
    for (int r = 0; r < rows; ++r) {
        c3d::LbfgsState& s = st[r];
        s.cnt = state_int_in[4 * r]; s.head = state_int_in[4 * r + 1]; s.mem = state_int_in[4 * r + 2]; s.resets = state_int_in[4 * r + 3];
        memcpy(reinterpret_cast<char*>(&s) + 4 * sizeof(int32_t), state_dbl_in + (size_t)ND * r, sizeof(double) * ND);     // gamma, SY, YY
        flags[2 * r] = first[r] != 0; flags[2 * r + 1] = mem0[r];
    }
    DevTable<double> d_sums, d_coef;
    DevTable<c3d::LbfgsState> d_in, d_out;
    DevTable<int> d_flags, d_shi;
    TABLE_TRY(d_sums.upload(c, C3D_LBFGS_SUMS * n, sums));
    TABLE_TRY(d_in.upload(c, n, st.data()));
    TABLE_TRY(d_flags.upload(c, 2 * n, flags.data()));
    TABLE_TRY(d_coef.zeros(c, NC * n));
    TABLE_TRY(d_out.zeros(c, n));
    TABLE_TRY(d_shi.zeros(c, 2 * n));
    if (f64) {
        const c3d::Model64 m64 = c3d::model64(dev_model(c), c->model);
        LAUNCH_TRY("fp64 L-BFGS direction launch", c3d::launch_lbfgs_direction64(c3d::step64(m64, c3d::kLbfgsFirst, 0.0, 1.0, 1.0, 0.85, 0.0), c3d::fire64(c->fire), rows,
                                                                                 d_sums.p, d_in.p, d_flags.p, d_out.p, d_coef.p, d_shi.p, c->stream));
    } else {
        LAUNCH_TRY("L-BFGS direction launch", c3d::launch_lbfgs_direction(dev_model(c), dev_fire(c), rows, d_sums.p, d_in.p, d_flags.p, d_out.p,
                                                                          d_coef.p, d_shi.p, c->stream));
    }
    TABLE_TRY(d_coef.download(c, coef));
    TABLE_TRY(d_out.download(c, st.data()));
    TABLE_TRY(d_shi.download(c, flags.data()));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int r = 0; r < rows; ++r) {
        const c3d::LbfgsState& s = st[r];
        state_int_out[4 * r] = s.cnt; state_int_out[4 * r + 1] = s.head; state_int_out[4 * r + 2] = s.mem; state_int_out[4 * r + 3] = s.resets;
        memcpy(state_dbl_out + (size_t)ND * r, reinterpret_cast<const char*>(&s) + 4 * sizeof(int32_t), sizeof(double) * ND);
        mask_slot[2 * r] = flags[2 * r]; mask_slot[2 * r + 1] = flags[2 * r + 1];
    }
    return C3D_OK;
}

// Test hook: the rows of the L-BFGS move (c3d_lbfgs_move_row.inc) on a table of rows (c3d.h) — k_lbfgs_move_rows, or k64_lbfgs_move_rows
// on a precision-64 context.  The host lays the rows out as the move kernels find them: x, F [3][np], the ring [s | y][8][3][np] with np
// the rows padded to 256; columns beyond the rows hold zeros and are not run.
namespace {
template <class T, class Launch>
int lbfgs_move_rows(c3d_ctx* c, int rows, const double* coef, int slot, const double* in, double* out, const char* what, Launch&& launch) {
    constexpr int M = c3d::kLbfgsMaxPairs, NC = C3D_LBFGS_COEFS;
    const int np = (rows + 255) / 256 * 256;
    const size_t nh = c3d::lbfgs_hist_floats(np);
    std::vector<T> hx(3 * (size_t)np, T(0)), hf(3 * (size_t)np, T(0)), hh(nh, T(0)), hc(NC), hd((size_t)np);
    for (int k = 0; k < NC; ++k) hc[k] = (T)coef[k];
    for (int r = 0; r < rows; ++r) {
        const double* a = in + (size_t)C3D_LBFGS_MOVE_ROW_IN * r;
        for (int k = 0; k < 3; ++k) {
            hx[(size_t)k * np + r] = (T)a[k]; hf[(size_t)k * np + r] = (T)a[3 + k];
            for (int j = 0; j < M; ++j) {
                hh[((size_t)3 * j + k) * np + r] = (T)a[6 + 3 * j + k];                       // s_j
                hh[((size_t)3 * (M + j) + k) * np + r] = (T)a[6 + 3 * M + 3 * j + k];         // y_j
            }
        }
    }
    DevTable<T> d_x, d_xo, d_f, d_h, d_c, d_d;
    TABLE_TRY(d_x.upload(c, hx.size(), hx.data()));
    TABLE_TRY(d_f.upload(c, hf.size(), hf.data()));
    TABLE_TRY(d_h.upload(c, nh, hh.data()));
    TABLE_TRY(d_c.upload(c, NC, hc.data()));
    TABLE_TRY(d_xo.zeros(c, hx.size()));
    TABLE_TRY(d_d.zeros(c, (size_t)np));
    if (const hipError_t e = launch(np, d_c.p, d_x.p, d_xo.p, d_f.p, d_h.p, d_d.p); e != hipSuccess)
        return fail(C3D_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    TABLE_TRY(d_xo.download(c, hx.data()));
    TABLE_TRY(d_h.download(c, hh.data()));
    TABLE_TRY(d_d.download(c, hd.data()));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int next = (slot + 1) % M;
    for (int r = 0; r < rows; ++r) {
        double* o = out + (size_t)C3D_LBFGS_MOVE_ROW_OUT * r;
        for (int k = 0; k < 3; ++k) {
            o[k] = (double)hx[(size_t)k * np + r];
            o[3 + k] = (double)hh[((size_t)3 * slot + k) * np + r];
            o[6 + k] = (double)hh[((size_t)3 * next + k) * np + r];
        }
        o[9] = (double)hd[r];
    }
    return C3D_OK;
}
}  // namespace
extern "C" int c3d_debug_lbfgs_move_rows(c3d_ctx* c, int rows, const double* coef, int mask, int slot, const double* in, double* out) {
    if (!c || !coef || !in || !out) return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_move_rows: bad arguments");
    if (rows < 1 || rows > (1 << 16)) return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_move_rows: rows is 1 .. 2^16");
    if (mask < 0 || mask > 255) return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_move_rows: mask is 0 .. 255");
    if (slot < 0 || slot >= c3d::kLbfgsMaxPairs) return fail(C3D_ERR_INVALID, "c3d_debug_lbfgs_move_rows: slot is 0 .. 7");
    const bool f64 = c->precision == 64;
    C3D_ENTRY(c, f64 ? unit_bit(UNIT_F64) : 0u);
    if (f64)
        return lbfgs_move_rows<double>(c, rows, coef, slot, in, out, "fp64 L-BFGS move rows launch",
                                       [&](int np, const double* dc, const double* x, double* xo, const double* f, double* h, double* d) {
                                           return c3d::launch_lbfgs_move_rows64(c3d::fire64(c->fire), rows, np, dc, mask, slot, x, xo, f, h, d, c->stream);
                                       });
    return lbfgs_move_rows<float>(c, rows, coef, slot, in, out, "L-BFGS move rows launch",
                                  [&](int np, const float* dc, const float* x, float* xo, const float* f, float* h, float* d) {
                                      return c3d::launch_lbfgs_move_rows(dev_fire(c), rows, np, dc, mask, slot, x, xo, f, h, d, c->stream);
                                  });
}
