// c3d_lbfgs_move_row.inc — one row of an L-BFGS move: the direction gamma F + sum a_j s_j + sum b_j y_j over the slot mask, the per-bead
// cap at max_step, the move, s into ring slot shi[1], the bead's move.move.  One text, four users: the rows of k_lbfgs_move and
// k_lbfgs_move_rows (c3d_lbfgs.h), of k64_lbfgs_move and k64_lbfgs_move_rows (c3d_f64.hip; the *_rows kernels: a thread a row of a
// table, c3d_debug_lbfgs_move_rows).  A ring slot outside the mask is not read: it holds stale or never-written memory.
// The includer defines C3D_LBFGS_T (float / double), C3D_LBFGS_FMA (fmaf / fma) and C3D_LBFGS_CAP, the statements that cap (dx, dy, dz).
// In:  i (the row), np (columns of a coordinate), roff (the replica's offset in x / F), rep, M, coef[1 + 2 M], shi[2], fp, xin, fcur, hist.
// Out: xout, ring slot shi[1] of hist, d2 (the includer's).
        const size_t ix = roff + i, iy = ix + np, iz = iy + np;
        const C3D_LBFGS_T c = coef[0];
        C3D_LBFGS_T dx = c * fcur[ix], dy = c * fcur[iy], dz = c * fcur[iz];
        C3D_LBFGS_T* hs = hist + (size_t)rep * lbfgs_hist_floats(np) + i;
        C3D_LBFGS_T* hy = hs + (size_t)3 * M * np;
        const int mask = shi[0];
#pragma unroll
        for (int j = 0; j < M; ++j) {
            if (!(mask & (1 << j))) continue;
            const C3D_LBFGS_T a = coef[1 + j], b = coef[1 + M + j];
            const C3D_LBFGS_T* s = hs + (size_t)3 * j * np;
            const C3D_LBFGS_T* y = hy + (size_t)3 * j * np;
            dx = C3D_LBFGS_FMA(a, s[0], C3D_LBFGS_FMA(b, y[0], dx));
            dy = C3D_LBFGS_FMA(a, s[np], C3D_LBFGS_FMA(b, y[np], dy));
            dz = C3D_LBFGS_FMA(a, s[2 * np], C3D_LBFGS_FMA(b, y[2 * np], dz));
        }
        C3D_LBFGS_CAP
        xout[ix] = xin[ix] + dx; xout[iy] = xin[iy] + dy; xout[iz] = xin[iz] + dz;
        C3D_LBFGS_T* sn = hs + (size_t)3 * shi[1] * np;
        sn[0] = dx; sn[np] = dy; sn[2 * np] = dz;
        d2 = C3D_LBFGS_FMA(dx, dx, C3D_LBFGS_FMA(dy, dy, dz * dz));
