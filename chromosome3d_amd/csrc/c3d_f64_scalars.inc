// c3d_f64_scalars.inc — the fp64 step controller: the statements that turn a replica's four sums of the previous evaluation and its
// FIRE / two-point state into the scalars of this step.  One text, two users (c3d_f64.hip): wave 0 of every k64_step / k64_step_chunked
// workgroup (c3d_f64_step_body.inc, after its four wave_sum64 calls) and k64_step_scalars, a thread a row (c3d_debug_step_scalars_f64).
// In:  m (Model64), p (Step64), fp (Fire64), s0 .. s3 (the sums), st (FireState64).
// Out: lam, cm0, cm1, cm2, keep, mix (declared here) and st as the step leaves it.
// C3D_F64_STATE_OUT: the includer's store of st, at the place a kind that carries state has finished with it.
        // (reciprocals and square roots by seed + two Newton steps, the constant factors folded on the host: the correctly rounded
        //  divisions and sqrt of the straightforward form are ~230 dependent fp64 operations — a microsecond on every workgroup's
        //  critical path, more than the launch boundary hides; these are a rounding or two away from them)
        double lam = 1.0, cm0 = 0, cm1 = 0, cm2 = 0, keep = 0.0, mix = 0.0;
        if (p.kind == kMdCouple || p.kind == kMdRescale) {
            double tprev = m.t_fac * s0;                // mass / kAccel / (ndf kBoltz) * sum v^2
            if (tprev < 1e-2) tprev = 1e-2;
            const double ratio = p.t_bath * rcp64(tprev);
            if (p.kind == kMdCouple) { double l2 = 1.0 + p.dt * m.fbeta * (ratio - 1.0); if (l2 < 0) l2 = 0; lam = sqrt64(l2); }
            else lam = sqrt64(ratio);
            cm0 = s1 * m.inv_n; cm1 = s2 * m.inv_n; cm2 = s3 * m.inv_n;
        } else if (kind_is_fire(p.kind)) {
            if (s0 > 0) {                               // power of the previous evaluation positive (kind 3: sums are 0)
                keep = 1.0 - st.alpha;
                mix = st.alpha * sqrt64(s2 * rcp64(s1 > 1e-30 ? s1 : 1e-30));
                if (st.npos > fp.n_min) { st.dt = st.dt * fp.f_inc < fp.dt_max ? st.dt * fp.f_inc : fp.dt_max; st.alpha *= fp.f_alpha; }
                st.npos += 1;
            } else {
                st.alpha = fp.alpha_start; st.dt *= fp.f_dec; st.npos = 0;
            }
            C3D_F64_STATE_OUT
        } else if (kind_is_two_point(p.kind)) {        // two-point step size, the length one evaluation late (c3o_bb_step): lam = previous length, mix = this one
            const int k = p.kind == kTwoPointFirst ? 0 : st.npos;
            const double a_prev = st.dt;
            double a = a_prev;
            if (k == 0) a = fp.dt_start * fp.dt_start * p.kacc;
            else if (k >= 2) {
                if (s0 > 0) a = (k & 1) ? s0 * rcp64(s2) : s3 * rcp64(s0);
                else a = 2.0 * a_prev;
                if (!(a >= 1e-7)) a = 1e-7;
                if (a > 1e2) a = 1e2;
            }
            lam = a_prev; mix = a;
            st.dt = a; st.npos = k + 1;
            C3D_F64_STATE_OUT
        }
