// c3d_f64_row_finish.inc — one row's update in fp64 (the CPU restatement's c3o_md_step / c3o_fire_step / c3o_bb_step per bead): from the
// row's coordinates, velocities, force and the step's scalars to its new coordinates, velocities and its contribution to the four sums
// the next step reads.  One text, two users (c3d_f64.hip): lanes 0 and 1 of every wave of k64_step / k64_step_chunked
// (c3d_f64_step_body.inc) and k64_row_finish, a thread a row (c3d_debug_row_finish_f64).
// In:  p (Step64), fp (Fire64), x0, y0, z0, v0x, v0y, v0z, Fx, Fy, Fz, lam, cm0, cm1, cm2, keep, mix, st.dt.
// Out: xn, yn, zn, vx, vy, vz (declared here), q0 .. q3 (the includer's, zero on entry).
        double vx, vy, vz, xn, yn, zn;
        if (p.kind == kMdBegin) {                       // MD begin: Maxwell velocities, no move
            vx = v0x; vy = v0y; vz = v0z; xn = x0; yn = y0; zn = z0;
            q0 = vx * vx + vy * vy + vz * vz; q1 = vx; q2 = vy; q3 = vz;
        } else if (p.kind == kMdCouple || p.kind == kMdRescale) {
            const double acc = p.acc;
            vx = lam * (v0x - cm0) + acc * Fx; vy = lam * (v0y - cm1) + acc * Fy; vz = lam * (v0z - cm2) + acc * Fz;
            xn = x0 + p.dt * vx; yn = y0 + p.dt * vy; zn = z0 + p.dt * vz;
            q0 = vx * vx + vy * vy + vz * vz; q1 = vx; q2 = vy; q3 = vz;
        } else if (p.kind == kTwoPoint || p.kind == kTwoPointFirst) {       // (kind_is_two_point written out: as a call it changes k64_row_finish's machine code)
            const double ms2 = fp.max_step * fp.max_step;
            auto clamp_scale = [&](double d2) {
                double scl = 1.0;
                if (d2 > ms2) { double dd, hh; sqrt_hrsqrt64(d2, dd, hh); hh = fma(fma(-dd, hh, 0.5), hh, hh); scl = fp.max_step * (hh + hh); }
                return cap_scale_wide64(d2, d2 > ms2, fp.max_step, scl);
            };
            q1 = Fx * Fx + Fy * Fy + Fz * Fz;
            if (p.kind == kTwoPoint) {
                double sx = lam * v0x, sy = lam * v0y, sz = lam * v0z;
                const double scp = clamp_scale(sx * sx + sy * sy + sz * sz);
                sx *= scp; sy *= scp; sz *= scp;
                const double yx = v0x - Fx, yy = v0y - Fy, yz = v0z - Fz;
                q0 = sx * yx + sy * yy + sz * yz; q2 = yx * yx + yy * yy + yz * yz; q3 = sx * sx + sy * sy + sz * sz;
            }
            const double dxs = mix * Fx, dys = mix * Fy, dzs = mix * Fz;
            const double scl = clamp_scale(dxs * dxs + dys * dys + dzs * dzs);
            xn = x0 + scl * dxs; yn = y0 + scl * dys; zn = z0 + scl * dzs;
            vx = Fx; vy = Fy; vz = Fz;
        } else {
            q0 = v0x * Fx + v0y * Fy + v0z * Fz; q1 = Fx * Fx + Fy * Fy + Fz * Fz; q2 = v0x * v0x + v0y * v0y + v0z * v0z;
            const double acc = st.dt * p.kacc;
            vx = keep * v0x + mix * Fx; vy = keep * v0y + mix * Fy; vz = keep * v0z + mix * Fz;
            vx += acc * Fx; vy += acc * Fy; vz += acc * Fz;
            const double dxs = st.dt * vx, dys = st.dt * vy, dzs = st.dt * vz;
            const double d2 = dxs * dxs + dys * dys + dzs * dzs;
            double scl = 1.0;
            if (d2 > fp.max_step * fp.max_step) { double dd, hh; sqrt_hrsqrt64(d2, dd, hh); hh = fma(fma(-dd, hh, 0.5), hh, hh); scl = fp.max_step * (hh + hh); }
            scl = cap_scale_wide64(d2, d2 > fp.max_step * fp.max_step, fp.max_step, scl);
            xn = x0 + scl * dxs; yn = y0 + scl * dys; zn = z0 + scl * dzs;
        }
