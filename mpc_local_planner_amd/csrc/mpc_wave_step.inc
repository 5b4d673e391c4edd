// mpc_wave_step.inc: the lane-parallel passes after a factorisation: slack / dual steps and fraction-to-boundary, acceptance, initial point, seeds, kept multipliers -- part of struct IpmWave (mpc_wave.hpp includes this file inside the struct's body; not a translation unit of its own).

    // ---------------------------------------------------------------- parallel post-processing of the step
    struct Fwd { T hdz, clam, dz2, dphi, a_p, a_d, dzmax, nunu; bool finite; };

    // fraction to the boundary: alpha = min(1, tau / max_i(-dval_i / val_i)).  The pass collects the largest ratio -dval / val (with the reciprocals of the slacks
    // it holds anyway; one reciprocal per multiplier) and divides ONCE after the wave reduction, instead of one IEEE division per row and bound.
    __device__ __forceinline__ void ftb_ratio(T ival, T dval, T& r) const { r = t_max(r, -dval * ival); }
    __device__ __forceinline__ T ftb_alpha(T r, T tau) const { return r > tau ? tau / r : T(1); }

    // REC (the fused step pass, kernels with kFusedPasses; meaningful where trial_fast_ok(): one grid point per lane): the pass also leaves in `tr` what trial_setup() would
    // collect next -- the controls, slacks and their steps it has just loaded and computed (the same expressions: -(row_val + s) - row_jdz), the bounds --, so that the line
    // search starts without another pass over the same LDS words.
    template <bool REC>
    __device__ __forceinline__ Fwd post_pass(T dd, const T nu[3], T tau, TrialRegs& tr) const {
        MPC_PHASE_LANE
        const int n = L.n;
        const T d = SCL(SC_D);
        T hdz = T(0), clam = T(0), dz2 = T(0), dphi = T(0), r_p = T(0), r_d = T(0), dzmax = T(0);
        if constexpr (REC) {
            trial_setup_states(tr, lane);
            for (int j = 0; j < 2; ++j) { tr.ulb[j] = P.u_lb[j]; tr.uub[j] = P.u_ub[j]; tr.u[j] = tr.du[j] = T(0); }
            for (int q = 0; q < 4; ++q) { tr.on[q] = false; tr.s[q] = T(1); tr.ds[q] = T(0); }
        }
        if (lane == 0) {
            if (dtf()) {
                T dl = d - P.dt_lb, du = P.dt_ub - d;
                T pl = SCL(SC_PDL), pu = SCL(SC_PDU);
                const T idl = t_rcp(dl), idu = t_rcp(du);
                T gb = -mu * idl + mu * idu;
                hdz += gb * dd; dphi += gb * dd;
                ftb_ratio(idl, dd, r_p); ftb_ratio(idu, -dd, r_p);
                ftb_ratio(t_rcp(pl), mu * idl - pl - (pl * idl) * dd, r_d);
                ftb_ratio(t_rcp(pu), mu * idu - pu + (pu * idu) * dd, r_d);
                dz2 += dd * dd; dzmax = t_max(dzmax, t_abs(dd));
            }
            if (mintime()) { hdz += T(n - 1) * dd; dphi += T(n - 1) * dd; }
            if (ball()) {
                const T jdz = ball_jdz(), s = SCL(SC_TS), y = SCL(SC_TY), res = SCL(SC_TG) + s;
                const T is = t_rcp(s);
                const T sig = y * is, ybar = mu * is + sig * res;
                const T ds = -res - jdz, dy = ybar + sig * jdz - y;
                hdz += ybar * jdz;
                dphi -= (mu * is) * ds;
                ftb_ratio(is, ds, r_p);
                ftb_ratio(t_rcp(y), dy, r_d);
            }
        }
        for (int k = lane; k < n; k += kWave) {
            if (k < n - 1) {
                for (int j = 0; j < 2; ++j) {
                    T u = F(L.U, j, k), du_ = F(L.DU, j, k);
                    T dl = u - P.u_lb[j], du = P.u_ub[j] - u;
                    T pl = F(L.PL, j, k), pu = F(L.PU, j, k);
                    const T idl = t_rcp(dl), idu = t_rcp(du);
                    T gbar = mu * idu - mu * idl + (quad() ? T(2) * P.R[j] * u * (intf() ? d : T(1)) : T(0));   // barrier (+ objective) gradient wrt u
                    if (costx() && quad()) gbar += T(2) * P.Ro * F(L.U, 1 - j, k) * (intf() ? d : T(1));
                    hdz += gbar * du_; dphi += gbar * du_;
                    ftb_ratio(idl, du_, r_p); ftb_ratio(idu, -du_, r_p);
                    ftb_ratio(t_rcp(pl), mu * idl - pl - (pl * idl) * du_, r_d);
                    ftb_ratio(t_rcp(pu), mu * idu - pu + (pu * idu) * du_, r_d);
                    dz2 += du_ * du_; dzmax = t_max(dzmax, t_abs(du_));
                    if constexpr (REC) { tr.u[j] = u; tr.du[j] = du_; }
                }
                for (int i = 0; i < 3; ++i) {
                    clam += C_(i, k) * F(L.LAMN, i, k);        // (a non-finite multiplier makes this sum non-finite: tested below)
                }
                if (intf()) {       // d/ddt of the integral-form stage cost
                    const T xd0 = F(L.X, 0, k) - xf[0], xd1 = F(L.X, 1, k) - xf[1], xd2 = normalize_theta(F(L.X, 2, k) - xf[2]);
                    const T v = F(L.U, 0, k), w = F(L.U, 1, k);
                    T sc = P.Q[0] * xd0 * xd0 + P.Q[1] * xd1 * xd1 + P.Q[2] * xd2 * xd2 + P.R[0] * v * v + P.R[1] * w * w;
                    if (costx()) {
                        const T xd[3] = {xd0, xd1, xd2};
                        sc += offquad(P.Qo, xd) + T(2) * P.Ro * v * w;
                        if (k == 0 && P.trapz) sc -= T(0.5) * fullquad(P.Q, P.Qo, xd);
                    }
                    hdz += sc * dd; dphi += sc * dd;
                }
            }
            if (k >= 1) {
                T vg[3] = {T(0), T(0), T(0)};
                if (via() && k < n - 1) { T vv; via_terms(k, F(L.X, 0, k), F(L.X, 1, k), F(L.X, 2, k), vv, vg); }
                T gxo[3] = {T(0), T(0), T(0)};         // cost variants: what the off-diagonal weights / the trapezoid term add to the gradient wrt x_k
                if (costx()) {
                    if (k < n - 1) {
                        if (quad()) {
                            const T xd[3] = {F(L.X, 0, k) - xf[0], F(L.X, 1, k) - xf[1], normalize_theta(F(L.X, 2, k) - xf[2])};
                            offmul(P.Qo, xd, gxo);
                            for (int i = 0; i < 3; ++i) gxo[i] *= T(2) * (intf() ? d : T(1));
                        }
                    } else {
                        T xdT[3], y3[3]; xd_final(T(0), xdT);
                        if (hasqf()) { offmul(P.Qfo, xdT, y3); for (int i = 0; i < 3; ++i) gxo[i] += T(2) * y3[i]; }
                        if (P.trapz) {
                            offmul(P.Qo, xdT, y3);
                            for (int i = 0; i < 3; ++i) gxo[i] += d * (P.Q[i] * xdT[i] + y3[i]);
                            const T sc = T(0.5) * fullquad(P.Q, P.Qo, xdT);
                            hdz += sc * dd; dphi += sc * dd;
                        }
                    }
                }
                for (int i = 0; i < 3; ++i) {
                    if (k < n - 1 || !fx(i)) {
                        T dx = F(L.DX, i, k);
                        dz2 += dx * dx; dzmax = t_max(dzmax, t_abs(dx));
                        T g = vg[i];
                        if (quad() && k < n - 1) { T xd = F(L.X, i, k) - xf[i]; if (i == 2) xd = normalize_theta(xd); g = T(2) * P.Q[i] * xd * (intf() ? d : T(1)); }
                        else if (k == n - 1 && hasqf()) { T xd = F(L.X, i, k) - xf[i]; if (i == 2) xd = normalize_theta(xd); g += T(2) * P.Qf[i] * xd; }
                        g += gxo[i];
                        hdz += g * dx; dphi += g * dx;
                    }
                }
            }
            for (int q = 0; q < 4; ++q) {
                if (!row_on(k, q)) continue;
                T jdz = row_jdz(k, q, dd);
                T s = F(L.SR, q, k), y = F(L.YR, q, k);
                T res = row_val(L.U, d, k, q) + s;
                const T is = t_rcp(s);
                T sig = y * is;
                T ybar = mu * is + sig * res;
                T ds = -res - jdz;
                T dy = ybar + sig * jdz - y;
                hdz += ybar * jdz;
                dphi -= (mu * is) * ds;
                ftb_ratio(is, ds, r_p);
                ftb_ratio(t_rcp(y), dy, r_d);
                if constexpr (REC) { tr.on[q] = true; tr.s[q] = s; tr.ds[q] = ds; }
            }
            if (nM() > 0 && k >= 1 && k < n - 1) {
                for (int m0 = 0; m0 < nM(); m0 += kRowGroup) {
                RowCache oc;
                ob_load<false>(m0, k, oc);
#pragma unroll
                for (int jm = 0; jm < kRowGroup; ++jm) {
                    const int m = m0 + jm;
                    if (m >= nM()) break;
                    if (oi(m, k) < 0) continue;
                    const T jdz = obst_jdz(k, m, oc.ax[jm], oc.ay[jm]);
                    const T s = F(L.OS, m, k), y = F(L.OY, m, k);
                    if (erho > T(0)) {      // restoration mode: elastic row; the step of e is kept for the trials and the accept pass
                        const T ee = OE_(0, m, k);
                        T ds, de, dy, ybar;
                        elastic_steps(s, y, oc.g[jm], ee, jdz, ds, de, dy, ybar);
                        OE_(1, m, k) = de;
                        hdz += ybar * jdz;
                        dphi += -(mu * t_rcp(s)) * ds - (mu * t_rcp(ee)) * de + erho * de;
                        ftb_ratio(t_rcp(s), ds, r_p); ftb_ratio(t_rcp(ee), de, r_p);
                        ftb_ratio(t_rcp(y), dy, r_d); ftb_ratio(t_rcp(erho - y), -dy, r_d);
                        continue;
                    }
                    const T res = oc.g[jm] + s;
                    const T is = t_rcp(s);
                    const T sig = y * is;
                    const T ybar = mu * is + sig * res;
                    const T ds = -res - jdz;
                    const T dy = ybar + sig * jdz - y;
                    hdz += ybar * jdz;
                    dphi -= (mu * is) * ds;
                    ftb_ratio(is, ds, r_p);
                    ftb_ratio(t_rcp(y), dy, r_d);
                }
                }
            }
        }
        Fwd o;
        if constexpr (kBatchedReductions) {
            T ra[4] = {hdz, clam, r_p, r_d}, rb[3] = {dz2, dphi, dzmax};      // (sums and maxima mixed in each batch, as in kkt_pass)
            wave_reduce_n<OpSum, OpSum, OpMax, OpMax>(ra);
            wave_reduce_n<OpSum, OpSum, OpMax>(rb);
            o.hdz = ra[0]; o.clam = ra[1]; o.dz2 = rb[0]; o.dphi = rb[1];
            o.a_p = ftb_alpha(ra[2], tau); o.a_d = ftb_alpha(ra[3], tau); o.dzmax = rb[2];
        } else {
        o.hdz = wave_sum(hdz); o.clam = wave_sum(clam); o.dz2 = wave_sum(dz2); o.dphi = wave_sum(dphi);
        o.a_p = ftb_alpha(wave_max(r_p), tau); o.a_d = ftb_alpha(wave_max(r_d), tau); o.dzmax = wave_max(dzmax);
        }
        o.nunu = T(0);
        for (int i = 0; i < 3; ++i) if (fx(i)) o.nunu += nu[i] * nu[i];
        o.finite = t_finite(o.hdz) && t_finite(o.dz2) && t_finite(o.clam);
        return o;
    }

    // ---------------------------------------------------------------- trial point / acceptance (parallel)
    __device__ __forceinline__ void accept(T alpha, T a_d) const {
        MPC_PHASE_LANE
        const int n = L.n;
        const T kS = T(MPC_LIT(1e10)), ikS = LL ? T(MPC_LIT(1.0 / 1e10)) : T(1) / kS;      // (LL is fp64 only: the quotient as the compiler folds it)
        const T d_old = SCL(SC_D), dd = SCL(SC_DD), d_new = d_old + (dtf_sum() ? alpha * dd : T(0));
        // phase 1: everything that reads the OLD point
        T sn[4], yn[4];
        // Chunks of 64 grid points are visited from the END of the horizon: a rate row k reads the OLD u_{k-1}, which belongs to the
        // previous chunk when k is a multiple of 64, so that chunk must not have been overwritten yet (n > 64: configs 3 and 5).
        for (int k = ((n - 1) / kWave) * kWave + lane; k >= 0; k -= kWave) {
            const bool act = k < n;
            if (act) {
            for (int q = 0; q < 4; ++q) {
                if (!row_on(k, q)) continue;
                T s = F(L.SR, q, k), y = F(L.YR, q, k);
                T res = row_val(L.U, d_old, k, q) + s;
                T jdz = row_jdz(k, q, dd);
                const T is = t_rcp(s);
                T sig = y * is;
                T ds = -res - jdz;
                T dy = mu * is + sig * res + sig * jdz - y;
                sn[q] = s + alpha * ds;
                T yv = y + a_d * dy;
                const T musn = mu * t_rcp(sn[q]);
                yn[q] = t_min(t_max(yv, musn * ikS), kS * musn);
            }
            if (nM() > 0 && k >= 1 && k < n - 1) {
                for (int m0 = 0; m0 < nM(); m0 += kRowGroup) {
                RowCache oc;
                ob_load<false>(m0, k, oc);
#pragma unroll
                for (int jm = 0; jm < kRowGroup; ++jm) {
                    const int m = m0 + jm;
                    if (m >= nM()) break;
                    if (oi(m, k) < 0) continue;
                    const T jdz = obst_jdz(k, m, oc.ax[jm], oc.ay[jm]);
                    const T s = F(L.OS, m, k), y = F(L.OY, m, k);
                    const T res = oc.g[jm] + s;
                    const T is = t_rcp(s);
                    const T sig = y * is;
                    if (erho > T(0)) {      // restoration mode: slack, elastic variable and multiplier of the elastic row; the same safeguards for e and its multiplier rho - y
                        const T ee = OE_(0, m, k);
                        T ds, de, dy, ybar;
                        elastic_steps(s, y, oc.g[jm], ee, jdz, ds, de, dy, ybar);
                        const T so = s + alpha * ds, eo = ee + alpha * de;
                        T yo = y + a_d * dy;
                        const T muso = mu * t_rcp(so), mueo = mu * t_rcp(eo);
                        yo = t_min(t_max(yo, muso * ikS), kS * muso);
                        yo = t_min(t_max(yo, erho - kS * mueo), erho - mueo * ikS);
                        F(L.OS, m, k) = so; F(L.OY, m, k) = yo; OE_(0, m, k) = eo;
                        continue;
                    }
                    const T so = s + alpha * (-res - jdz);
                    T yo = y + a_d * (mu * is + sig * res + sig * jdz - y);
                    const T muso = mu * t_rcp(so);
                    yo = t_min(t_max(yo, muso * ikS), kS * muso);
                    F(L.OS, m, k) = so; F(L.OY, m, k) = yo;
                }
                }
            }
            }
            sync();      // all lanes of this chunk have read their neighbours' old controls
            if (act) {
            for (int q = 0; q < 4; ++q) if (row_on(k, q)) { F(L.SR, q, k) = sn[q]; F(L.YR, q, k) = yn[q]; }
            if (k < n - 1) {
                for (int j = 0; j < 2; ++j) {
                    T u = F(L.U, j, k), du_ = F(L.DU, j, k);
                    T dl = u - P.u_lb[j], du = P.u_ub[j] - u;
                    T pl = F(L.PL, j, k), pu = F(L.PU, j, k);
                    const T idl = t_rcp(dl), idu = t_rcp(du);
                    T pln = pl + a_d * (mu * idl - pl - (pl * idl) * du_);
                    T pun = pu + a_d * (mu * idu - pu + (pu * idu) * du_);
                    T un = ut(j, k, alpha);
                    const T mdl = mu * t_rcp(un - P.u_lb[j]), mdu = mu * t_rcp(P.u_ub[j] - un);
                    F(L.PL, j, k) = t_min(t_max(pln, mdl * ikS), kS * mdl);
                    F(L.PU, j, k) = t_min(t_max(pun, mdu * ikS), kS * mdu);
                    F(L.U, j, k) = un;
                }
                for (int i = 0; i < 3; ++i) {
                    T lo = F(L.LAM, i, k);
                    F(L.LAM, i, k) = lo + alpha * (F(L.LAMN, i, k) - lo);
                }
            }
            for (int i = 0; i < 3; ++i) F(L.X, i, k) = xt(i, k, alpha);
            }
        }
        if (lane == 0) {
            if (dtf()) {
                T dl = d_old - P.dt_lb, du = P.dt_ub - d_old;
                T pl = SCL(SC_PDL), pu = SCL(SC_PDU);
                const T idl = t_rcp(dl), idu = t_rcp(du);
                T pln = pl + a_d * (mu * idl - pl - (pl * idl) * dd);
                T pun = pu + a_d * (mu * idu - pu + (pu * idu) * dd);
                const T mdl = mu * t_rcp(d_new - P.dt_lb), mdu = mu * t_rcp(P.dt_ub - d_new);
                SCL(SC_PDL) = t_min(t_max(pln, mdl * ikS), kS * mdl);
                SCL(SC_PDU) = t_min(t_max(pun, mdu * ikS), kS * mdu);
            }
            SCL(SC_D) = d_new;
            if (ball()) {        // from the caches of the OLD point (value, gradient) and the step
                const T jdz = ball_jdz(), s = SCL(SC_TS), y = SCL(SC_TY), res = SCL(SC_TG) + s, is = t_rcp(s), sig = y * is;
                const T so = s + alpha * (-res - jdz);
                T yo = y + a_d * (mu * is + sig * res + sig * jdz - y);
                const T muso = mu * t_rcp(so);
                yo = t_min(t_max(yo, muso * ikS), kS * muso);
                SCL(SC_TS) = so; SCL(SC_TY) = yo;
            }
        }
    }

    // ---------------------------------------------------------------- initial point (parallel)
    __device__ __forceinline__ void cold_start() const {
        const int n = L.n;
        const T dth = normalize_theta(xf[2] - x0[2]);
        for (int k = lane; k < n; k += kWave) {
            T fr = T(k) / T(n - 1);
            T xk[3];
            if (k == 0) { xk[0] = x0[0]; xk[1] = x0[1]; xk[2] = x0[2]; }
            else if (k == n - 1) { xk[0] = xf[0]; xk[1] = xf[1]; xk[2] = xf[2]; }
            else {
                xk[0] = x0[0] + fr * (xf[0] - x0[0]);
                xk[1] = x0[1] + fr * (xf[1] - x0[1]);
                xk[2] = normalize_theta(x0[2] + fr * dth);
            }
            for (int i = 0; i < 3; ++i) F(L.X, i, k) = xk[i];
            if (k < n - 1) { F(L.U, 0, k) = T(0); F(L.U, 1, k) = T(0); }
        }
        if (lane == 0) SCL(SC_D) = P.dt_ref;
    }

    // initial vertex values of candidate kind `kind` (mpc_candidate_kind; MPC_CAND_REFERENCE is cold_start() / the caller's guess):
    // positions on the straight line as in cold_start(); heading = direction of travel, turned by pi when the goal lies behind the start
    // pose (initializeSequences without xinit, full_discretization_grid_base_se2.cpp:136-190), + pi for the *_REVERSE kinds; the BLEND kinds
    // turn from the start heading into that direction over the first m grid points and into the goal heading over the last m.
    // Kinds 5..8 (HERMITE_FF / _RR / _FR / _RF): positions on the cubic Hermite curve between the two poses, end tangents along the headings scaled by
    // tscale * |goal - start| and signed by the driving direction at that end; heading = tangent direction (+ pi where the robot drives backwards:
    // the first half of the horizon takes the start's direction, the second half the goal's).
    __device__ __forceinline__ void seed_start(int kind, T tscale = T(2)) const {
        const int n = L.n;
        const T ddx = xf[0] - x0[0], ddy = xf[1] - x0[1];
        if (kind >= 5) {
            const T sg0 = (kind == 5 || kind == 7) ? T(1) : T(-1), sg1 = (kind == 5 || kind == 8) ? T(1) : T(-1);
            const T dd = sqrt(ddx * ddx + ddy * ddy);
            T s0_, c0_, s1_, c1_;
            t_sincos(x0[2], &s0_, &c0_);
            t_sincos(xf[2], &s1_, &c1_);
            const T m0x = sg0 * tscale * dd * c0_, m0y = sg0 * tscale * dd * s0_, m1x = sg1 * tscale * dd * c1_, m1y = sg1 * tscale * dd * s1_;
            for (int k = lane; k < n; k += kWave) {
                const T t = T(k) / T(n - 1), t2 = t * t, t3 = t2 * t;
                const T h00 = T(2) * t3 - T(3) * t2 + T(1), h10 = t3 - T(2) * t2 + t, h01 = T(-2) * t3 + T(3) * t2, h11 = t3 - t2;
                const T g00 = T(6) * t2 - T(6) * t, g10 = T(3) * t2 - T(4) * t + T(1), g01 = T(-6) * t2 + T(6) * t, g11 = T(3) * t2 - T(2) * t;
                T xk[3];
                if (k == 0) { xk[0] = x0[0]; xk[1] = x0[1]; xk[2] = x0[2]; }
                else if (k == n - 1) { xk[0] = xf[0]; xk[1] = xf[1]; xk[2] = xf[2]; }
                else {
                    xk[0] = h00 * x0[0] + h10 * m0x + h01 * xf[0] + h11 * m1x;
                    xk[1] = h00 * x0[1] + h10 * m0y + h01 * xf[1] + h11 * m1y;
                    const T tx = g00 * x0[0] + g10 * m0x + g01 * xf[0] + g11 * m1x, ty = g00 * x0[1] + g10 * m0y + g01 * xf[1] + g11 * m1y;
                    T th = t_atan2(ty, tx);
                    if ((2 * k < n - 1 ? sg0 : sg1) < T(0)) th = normalize_theta(th + T(3.14159265358979323846));
                    xk[2] = th;
                }
                for (int i = 0; i < 3; ++i) F(L.X, i, k) = xk[i];
                if (k < n - 1) { F(L.U, 0, k) = T(0); F(L.U, 1, k) = T(0); }
            }
            if (lane == 0) SCL(SC_D) = P.dt_ref;
            return;
        }
        T orient = t_atan2(ddy, ddx);
        T s0, c0;
        t_sincos(x0[2], &s0, &c0);
        if (ddx * c0 + ddy * s0 < T(0)) orient = normalize_theta(orient + T(3.14159265358979323846));
        if (kind == 2 || kind == 4) orient = normalize_theta(orient + T(3.14159265358979323846));
        const bool blend = kind >= 3;
        int m = P.cand_blend;
        if (m > (n - 1) / 2) m = (n - 1) / 2;
        const T d0 = normalize_theta(orient - x0[2]), df = normalize_theta(orient - xf[2]);
        for (int k = lane; k < n; k += kWave) {
            const T fr = T(k) / T(n - 1);
            T xk[3];
            if (k == 0) { xk[0] = x0[0]; xk[1] = x0[1]; xk[2] = x0[2]; }
            else if (k == n - 1) { xk[0] = xf[0]; xk[1] = xf[1]; xk[2] = xf[2]; }
            else {
                xk[0] = x0[0] + fr * ddx;
                xk[1] = x0[1] + fr * ddy;
                xk[2] = orient;
                if (blend && k < m) xk[2] = normalize_theta(x0[2] + (T(k) / T(m)) * d0);
                if (blend && n - 1 - k < m) xk[2] = normalize_theta(xf[2] + (T(n - 1 - k) / T(m)) * df);
            }
            for (int i = 0; i < 3; ++i) F(L.X, i, k) = xk[i];
            if (k < n - 1) { F(L.U, 0, k) = T(0); F(L.U, 1, k) = T(0); }
        }
        if (lane == 0) SCL(SC_D) = P.dt_ref;
    }

    // ---- multipliers kept in the handle between control cycles (dual_warm_start).  Block layout (doubles): [0] grid size, [1] pi_dt lower,
    //      [2] pi_dt upper, [3] terminal-ball multiplier, then the LDS word ranges LAM (3 NS), YR (4 NS), PL (2 NS), PU (2 NS) verbatim: mpc::dual_words(NS) doubles.
    __device__ __forceinline__ void store_duals(double* blk) const {
        const int NS = L.NS;
        if (lane == 0) { blk[0] = double(L.n); blk[1] = double(SCL(SC_PDL)); blk[2] = double(SCL(SC_PDU)); blk[3] = ball() ? double(SCL(SC_TY)) : 0.0; }
        for (int e = lane; e < 3 * NS; e += kWave) blk[4 + e] = double(sm[L.LAM + e]);
        for (int e = lane; e < 4 * NS; e += kWave) blk[4 + 3 * NS + e] = double(sm[L.YR + e]);
        for (int e = lane; e < 2 * NS; e += kWave) { blk[4 + 7 * NS + e] = double(sm[L.PL + e]); blk[4 + 9 * NS + e] = double(sm[L.PU + e]); }
    }
    // every inequality multiplier max(previous, mu0 / slack) (the slacks and mu0 / slack were just set by init_point), lam as it was
    __device__ __forceinline__ void load_duals(const double* blk) const {
        const int n = L.n, NS = L.NS;
        for (int k = lane; k < n; k += kWave) {
            if (k < n - 1) {
                for (int i = 0; i < 3; ++i) F(L.LAM, i, k) = T(blk[4 + i * NS + k]);
                for (int j = 0; j < 2; ++j) {
                    F(L.PL, j, k) = t_max(F(L.PL, j, k), T(blk[4 + 7 * NS + j * NS + k]));
                    F(L.PU, j, k) = t_max(F(L.PU, j, k), T(blk[4 + 9 * NS + j * NS + k]));
                }
            }
            for (int q = 0; q < 4; ++q) if (row_on(k, q)) F(L.YR, q, k) = t_max(F(L.YR, q, k), T(blk[4 + 3 * NS + q * NS + k]));
        }
        if (lane == 0) {
            if (dtf()) { SCL(SC_PDL) = t_max(SCL(SC_PDL), T(blk[1])); SCL(SC_PDU) = t_max(SCL(SC_PDU), T(blk[2])); }
            if (ball()) SCL(SC_TY) = t_max(SCL(SC_TY), T(blk[3]));
        }
    }

    __device__ __forceinline__ void init_point() {
        MPC_PHASE_LANE
        const int n = L.n;
        if (lane == 0) {
            for (int i = 0; i < 3; ++i) {
                F(L.X, i, 0) = x0[i];
                if (fx(i)) F(L.X, i, n - 1) = xf[i];
            }
            if (!dtf()) SCL(SC_D) = P.dt_ref;
        }
        sync();
        // seed controls from the state guess when every control is zero
        T nz = T(0);
        for (int k = lane; k < n - 1; k += kWave) nz += (F(L.U, 0, k) != T(0) || F(L.U, 1, k) != T(0)) ? T(1) : T(0);
        nz = wave_sum(nz);
        const T d0 = SCL(SC_D);
        if (nz == T(0)) {
            for (int k = lane; k < n - 1; k += kWave) {
                T dx = F(L.X, 0, k + 1) - F(L.X, 0, k), dy = F(L.X, 1, k + 1) - F(L.X, 1, k);
                T dth = normalize_theta(F(L.X, 2, k + 1) - F(L.X, 2, k));
                T s, c;
                t_sincos(F(L.X, 2, k), &s, &c);
                T v = (dx * c + dy * s) / d0;
                v = t_min(t_max(v, P.u_lb[0]), P.u_ub[0]);
                T rate = dth / d0, w;
                if (MODEL == MODEL_UNICYCLE) w = rate;
                else {
                    T vv = t_abs(v) > T(1e-3) ? v : (v >= T(0) ? T(1e-3) : T(-1e-3));
                    if (MODEL == MODEL_SIMPLE_CAR) w = t_atan(P.p0 * rate / vv);
                    else if (MODEL == MODEL_SIMPLE_CAR_FRONT) w = t_asin(t_min(T(1), t_max(T(-1), P.p0 * rate / vv)));
                    else { T sb = t_min(T(1), t_max(T(-1), P.p0 * rate / vv)); w = t_atan(t_tan(t_asin(sb)) * (P.p1 + P.p0) / P.p0); }
                }
                w = t_min(t_max(w, P.u_lb[1]), P.u_ub[1]);
                F(L.U, 0, k) = v; F(L.U, 1, k) = w;
            }
            sync();
            // ... and keep the seeded controls inside the control-rate rows, as the reference's u = 0 start is (every row but the first): increments clamped to
            // rate_seed_frac x the rate limits forward from u_prev, then backward from the final row (against u_ref = 0).  A seed that jumps violates the rows it
            // crosses: their slacks start at the 1e-2 floor with a residual and the fraction-to-boundary rule pins the first iterations.  Lane j walks control j.
            if (lane < 2 && ron(lane) && ron(2 + lane)) {
                const int j = lane;
                const T fr = Algo<T>::rate_seed_frac, lo = P.rate_lim[j] * d0 * fr, hi = P.rate_lim[2 + j] * d0 * fr;
                T prev = F(L.U, j, 0);
                if (row0_on) { const T up_ = j ? uprev[1] : uprev[0]; prev = t_min(t_max(prev, up_ + P.rate_lim[j] * dtprev * fr), up_ + P.rate_lim[2 + j] * dtprev * fr); F(L.U, j, 0) = prev; }
                for (int k = 1; k < n - 1; ++k) { prev = t_min(t_max(F(L.U, j, k), prev + lo), prev + hi); F(L.U, j, k) = prev; }
                T nxt = T(0);
                for (int k = n - 2; k >= 0; --k) { nxt = t_min(t_max(F(L.U, j, k), nxt - hi), nxt - lo); F(L.U, j, k) = nxt; }
            }
        }
        sync();
        for (int k = lane; k < n - 1; k += kWave)
            for (int j = 0; j < 2; ++j) F(L.U, j, k) = push_interior(F(L.U, j, k), P.u_lb[j], P.u_ub[j]);
        if (lane == 0 && dtf()) SCL(SC_D) = push_interior(SCL(SC_D), P.dt_lb, P.dt_ub);
        sync();
        if (nM() > 0) { rows_dropped = associate_obstacles(); sync(); }
        if (via()) { associate_via_points(); sync(); }
        const bool dual_ok = dual_in != nullptr && warm_guess && (int)dual_in[0] == n;       // same grid size as the solve that left the multipliers
        mu = dual_ok ? P.mu_init_dual : (warm_guess ? P.mu_init_warm : P.mu_init); rho = T(0); delta_last = T(0); fail0 = false;
        const T d = SCL(SC_D);
        for (int k = lane; k < n; k += kWave) {
            for (int q = 0; q < 4; ++q) {
                T s = T(1), y = T(0);
                if (row_on(k, q)) { s = t_max(-row_val(L.U, d, k, q), Algo<T>::slack_push); y = mu / s; }
                F(L.SR, q, k) = s; F(L.YR, q, k) = y;
            }
            if (nM() > 0) {
                const T px = F(L.X, 0, k), py = F(L.X, 1, k);
                for (int m = 0; m < nM(); ++m) {
                    T s = T(1), y = T(0), g, a3[3], hk, h3[3];
                    if (k >= 1 && k < n - 1) {
                        if (obst_row3(k, m, px, py, F(L.X, 2, k), g, a3, hk, h3, d)) { s = t_max(-g, Algo<T>::clearance_slack_push); y = mu / s; }
                    } else set_oi(m, k, -1);
                    F(L.OS, m, k) = s; F(L.OY, m, k) = y;
                }
            }
            if (k < n - 1) {
                for (int j = 0; j < 2; ++j) {
                    T u = F(L.U, j, k);
                    F(L.PL, j, k) = mu / (u - P.u_lb[j]);
                    F(L.PU, j, k) = mu / (P.u_ub[j] - u);
                }
                for (int i = 0; i < 3; ++i) F(L.LAM, i, k) = T(0);
            }
        }
        if (lane == 0) {
            SCL(SC_PDL) = dtf() ? mu / (d - P.dt_lb) : T(0);
            SCL(SC_PDU) = dtf() ? mu / (P.dt_ub - d) : T(0);
            if (ball()) {
                T a[3];
                const T s = t_max(-ball_eval(T(0), a), Algo<T>::slack_push);
                SCL(SC_TS) = s; SCL(SC_TY) = mu / s;
            }
        }
        sync();
        if (dual_ok) { load_duals(dual_in); sync(); }
    }

