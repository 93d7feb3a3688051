// c3d_lbfgs_serial.inc — the serial section of an L-BFGS move: what one thread runs between the two barriers of k_lbfgs_move (c3d_lbfgs.h)
// and k64_lbfgs_move (c3d_f64.hip), and what k_lbfgs_direction / k64_lbfgs_direction run a thread a row (c3d_debug_lbfgs_direction).
// One text, so that the table tests hold the statements the production kernels run; a body and not a function, because a function
// boundary has changed machine code in this project before (c3d_step_body.inc).
//
// The includer provides
//   C3D_LBFGS_COEF     the type of coef[] (float in the fp32 kernels, double in the fp64 ones): the only difference between the precisions
//   C3D_LBFGS_GAMMA0   the first step's gamma, a double: kind 6's first length dt_start^2 acc as the precision's step kernel forms it
//   Q, M               kLbfgsQ, kLbfgsMaxPairs
//   first, mem0        kind 9 (the stage's first step), the option lbfgs_memory (1 .. M)
//   sums[Q]            doubles: slot j: (F.s_j, F.y_j, s_j.y, y_j.y) at 4j, then s.s, F.F (c3d_internal.h "L-BFGS stage")
//   st                 the LbfgsState of the previous step (not read when first), left as this step's
//   coef[1 + 2 M]      out: gamma, then a_j (of s_j), b_j (of y_j) by slot, 0 for a slot outside the direction
//   shi[2]             out: slot mask of the pairs in the direction, slot of the move's s
// A state out of range on input is clamped first: mem to [1, M], head to [0, mem - 1], cnt to [0, mem].
        if (first) {
            st.cnt = 0; st.mem = mem0; st.head = mem0 - 1; st.resets = 0;
            st.gamma = C3D_LBFGS_GAMMA0;
        } else {
            st.mem = min(max(st.mem, 1), M);
            st.head = min(max(st.head, 0), st.mem - 1);
            st.cnt = min(max(st.cnt, 0), st.mem);
            const int mem = st.mem;
            const int nx = st.head + 1 == mem ? 0 : st.head + 1;
            const double sy = sums[4 * nx + 2], yy = sums[4 * nx + 3], ss = sums[Q - 4];
            if (sy > 1e-12 * sqrt(ss * yy)) {
                st.head = nx;
                st.cnt = min(st.cnt + 1, mem);
                for (int i = 0; i < st.cnt; ++i) {
                    int sl = nx - i; if (sl < 0) sl += mem;
                    st.SY[sl][nx] = sums[4 * sl + 2];
                    st.YY[sl][nx] = sums[4 * sl + 3];
                    st.YY[nx][sl] = sums[4 * sl + 3];
                }
                st.gamma = sy / yy;
            } else {
                st.cnt = 0;
                st.resets += 1;
                st.gamma *= 2.0;
            }
            st.gamma = fmin(fmax(st.gamma, 1e-7), 1e2);
        }
        const int mem = st.mem, cnt = st.cnt;
        const double g = st.gamma, ff = sums[Q - 3];
        int sl[M];
        double ps[M], py[M], u[M], w[M], top[M];
        for (int i = 0; i < cnt; ++i) {                  // age order: i = 0 the oldest pair
            int k = st.head - (cnt - 1) + i; if (k < 0) k += mem;
            sl[i] = k;
            ps[i] = -sums[4 * k];                        // S'g, Y'g with g = -F
            py[i] = -sums[4 * k + 1];
        }
        for (int i = cnt - 1; i >= 0; --i) {             // R u = S'g, R = upper triangle of S'Y
            double a = ps[i];
            for (int j = i + 1; j < cnt; ++j) a -= st.SY[sl[i]][sl[j]] * u[j];
            u[i] = a / st.SY[sl[i]][sl[i]];
        }
        for (int i = 0; i < cnt; ++i) {                  // w = (D + gamma Y'Y) u - gamma Y'g
            double a = st.SY[sl[i]][sl[i]] * u[i];
            for (int j = 0; j < cnt; ++j) a += g * st.YY[sl[i]][sl[j]] * u[j];
            w[i] = a - g * py[i];
        }
        for (int i = 0; i < cnt; ++i) {                  // R' top = w
            double a = w[i];
            for (int j = 0; j < i; ++j) a -= st.SY[sl[j]][sl[i]] * top[j];
            top[i] = a / st.SY[sl[i]][sl[i]];
        }
        // d = -H g = gamma F - sum top_i s_i + gamma sum u_i y_i;  F.d > 0 or the memory goes
        double fd = g * ff;
        for (int i = 0; i < cnt; ++i) fd += top[i] * ps[i] - g * u[i] * py[i];
        int mask = 0;
        for (int j = 0; j < 2 * M; ++j) coef[1 + j] = (C3D_LBFGS_COEF)0.0;
        if (fd > 0.0) {
            for (int i = 0; i < cnt; ++i) {
                coef[1 + sl[i]] = (C3D_LBFGS_COEF)(-top[i]); coef[1 + M + sl[i]] = (C3D_LBFGS_COEF)(g * u[i]); mask |= 1 << sl[i];
            }
        } else {
            st.cnt = 0;
            st.resets += 1;
        }
        coef[0] = (C3D_LBFGS_COEF)g;
        shi[0] = mask;
        shi[1] = st.head + 1 == mem ? 0 : st.head + 1;   // where this move's s goes: the slot the next evaluation completes
