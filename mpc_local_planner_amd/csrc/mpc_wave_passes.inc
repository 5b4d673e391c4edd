// mpc_wave_passes.inc: the lane-parallel passes before a factorisation: point evaluation, line-search trials, KKT error + stage records, condensed barrier terms -- part of struct IpmWave (mpc_wave.hpp includes this file inside the struct's body; not a translation unit of its own).

    // ---------------------------------------------------------------- point evaluation (parallel)
    // trig cache + c_k for the point (XB, UB, d); returns wave-reduced sum|c|, objective
    __device__ __forceinline__ void eval_point(T d, T& theta_c, T& fobj, T alpha = T(0), bool trial = false) const {
        MPC_PHASE_LANE
        const int n = L.n;
        const T al = trial ? alpha : T(0);
        T th = T(0), fo = T(0);
        // clearance rows (non-linear): |g(x_k) + s| with the trial slack s + alpha*ds
        if (nM() > 0) {
            for_each_row([&](int k, int m) {
                if (oi(m, k) < 0) return;
                T og = T(0), oax = T(0), oay = T(0);
                if (trial) { og = OB_(0, m, k); oax = OB_(1, m, k); oay = OB_(2, m, k); }      // (the values at the current point, cached by kkt_pass: on their way while the distance is worked out)
                const T px = xt(0, k, al), py = xt(1, k, al), pth = fpline() ? xt(2, k, al) : T(0);
                T g, a3[3], hk, h3[3];
                obst_row3(k, m, px, py, pth, g, a3, hk, h3, d);
                T s = F(L.OS, m, k);
                if (erho > T(0)) {      // restoration mode: g + s - e with the trial values of both, + rho e in the objective
                    const T ee = OE_(0, m, k), de = trial ? T(OE_(1, m, k)) : T(0);
                    if (trial) s += alpha * (-(og + s - ee) - obst_jdz(k, m, oax, oay) + de);
                    const T et = ee + (trial ? alpha * de : T(0));
                    th += t_abs(g + s - et);
                    fo += erho * et;
                    return;
                }
                if (trial) s += alpha * (-(og + s) - obst_jdz(k, m, oax, oay));
                th += t_abs(g + s);
            });
        }
        for (int k = lane; k < n - 1; k += kWave) {
            T xk[3] = {xt(0, k, al), xt(1, k, al), xt(2, k, al)};
            T xn[3] = {xt(0, k + 1, al), xt(1, k + 1, al), xt(2, k + 1, al)};
            T v = ut(0, k, al), w = ut(1, k, al);
            T tr[4], tr2[2], f[3];
            model_trig_colloc<T, MODEL, kLocalLiterals>(P, colloc(), xk[2], v, w, d, tr, tr2);
            colloc_f<T, MODEL>(P, colloc(), tr, tr2, v, w, f);
            T c0 = d * f[0] - (xn[0] - xk[0]);
            T c1 = d * f[1] - (xn[1] - xk[1]);
            T c2 = d * f[2] - normalize_theta(xn[2] - xk[2]);
            for (int i = 0; i < NTRB; ++i) F(L.TRIG, i, k) = tr[i];
            if (colloc() == COLLOC_CN) { F(L.TRIG, NTRB, k) = tr2[0]; F(L.TRIG, NTRB + 1, k) = tr2[1]; }
            C_(0, k) = c0; C_(1, k) = c1; C_(2, k) = c2;
            th += t_abs(c0) + t_abs(c1) + t_abs(c2);
            if (quad()) {
                T xd0 = xk[0] - xf[0], xd1 = xk[1] - xf[1], xd2 = normalize_theta(xk[2] - xf[2]);
                fo += (P.Q[0] * xd0 * xd0 + P.Q[1] * xd1 * xd1 + P.Q[2] * xd2 * xd2 + P.R[0] * v * v + P.R[1] * w * w) * (intf() ? d : T(1));
                if (costx()) {
                    const T xd[3] = {xd0, xd1, xd2};
                    fo += (offquad(P.Qo, xd) + T(2) * P.Ro * v * w) * (intf() ? d : T(1));
                    if (k == 0 && P.trapz) fo -= T(0.5) * d * fullquad(P.Q, P.Qo, xd);
                }
            }
            if (via()) { T vv, vg[3]; via_terms(k, xk[0], xk[1], xk[2], vv, vg); fo += vv; }
        }
        if (lane == 0) {
            if (mintime()) fo += T(n - 1) * d;
            if (costx()) fo += final_cost_extra(al, d);
            if (hasqf()) {       // the terminal cost does not depend on the stage cost's type (src/controller.cpp:641-672)
                for (int i = 0; i < 3; ++i) if (!fx(i)) {
                    T xd = xt(i, n - 1, al) - xf[i];
                    if (i == 2) xd = normalize_theta(xd);
                    fo += P.Qf[i] * xd * xd;
                }
            }
            if (ball()) { T a[3]; th += t_abs(ball_eval(al, a) + ball_slack(alpha, trial)); }
        }
        if constexpr (kBatchedReductions) {
            T r2[2] = {th, fo};
            wave_reduce_n<OpSum, OpSum>(r2);
            theta_c = r2[0]; fobj = r2[1];
        } else {
        theta_c = wave_sum(th);
        fobj = wave_sum(fo);
        }
    }

    // sum of barrier logs at the current (alpha = 0) or trial point; wave-reduced
    __device__ __forceinline__ T barrier_logs(T d, T alpha, bool trial, T dd) const {
        MPC_PHASE_LANE
        const int n = L.n;
        LogAccT acc;
        for (int k = lane; k < n; k += kWave) {
            if (k < n - 1) {
                for (int j = 0; j < 2; ++j) { T u = ut(j, k, trial ? alpha : T(0)); acc.mul(u - P.u_lb[j]); acc.mul(P.u_ub[j] - u); }
            }
            for (int q = 0; q < 4; ++q) {
                if (!row_on(k, q)) continue;
                T s = F(L.SR, q, k);
                if (trial) s += alpha * (-(row_val(L.U, SCL(SC_D), k, q) + s) - row_jdz(k, q, dd));
                acc.mul(s);
            }
            if (nM() > 0 && k >= 1 && k < n - 1) {
                for (int m0 = 0; m0 < nM(); m0 += kRowGroup) {
                RowCache oc;
                if (trial) ob_load<false>(m0, k, oc);
#pragma unroll
                for (int jm = 0; jm < kRowGroup; ++jm) {
                    const int m = m0 + jm;
                    if (m >= nM()) break;
                    if (oi(m, k) < 0) continue;
                    T s = F(L.OS, m, k);
                    if (erho > T(0)) {
                        const T ee = OE_(0, m, k), de = trial ? T(OE_(1, m, k)) : T(0);
                        if (trial) s += alpha * (-(oc.g[jm] + s - ee) - obst_jdz(k, m, oc.ax[jm], oc.ay[jm]) + de);
                        acc.mul(s); acc.mul(ee + (trial ? alpha * de : T(0)));
                        continue;
                    }
                    if (trial) s += alpha * (-(oc.g[jm] + s) - obst_jdz(k, m, oc.ax[jm], oc.ay[jm]));
                    acc.mul(s);
                }
                }
            }
        }
        if (lane == 0 && dtf()) { acc.mul(d - P.dt_lb); acc.mul(P.dt_ub - d); }
        if (lane == 0 && ball()) acc.mul(ball_slack(alpha, trial));
        return wave_sum(acc.value());
    }

    // ---------------------------------------------------------------- line-search trials, register-resident fast path
    // (n <= 64, no clearance rows: one interval / one rate row per lane).  Everything a trial needs that does not depend on the
    // step length is pulled into registers once per iteration; a trial is then ~300 instructions with no LDS reads.  Same
    // arithmetic as eval_point() + barrier_logs() at (alpha, trial = true).
    struct TrialRegs {
        T xk[3], dxk[3], xn[3], dxn[3], u[2], du[2], s[4], ds[4];
        T ulb[2], uub[2], dt_lb, dt_ub, nm1;      // (the quadratic weights are read from the problem record when needed: ten registers less across the line search)
        bool stage, on[4], quad, mint, dtf;
        int k;
    };
    // kFusedPasses: the kernels whose launches can qualify (decided at compile time); such a kernel's post_pass() leaves TrialRegs filled from what it holds anyway
    // (the fused step pass), trial_setup() stays the separate pass of the others
    static constexpr bool kFusedPasses = EXT == 0 && !GS && !W2 && !OBST && !(sizeof(T) == 8 && NTRB > 3);
    // (a fixed layout of at most 64 grid points per record decides it at compile time -- no instance of such a handle has more points than the record --: the headline
    //  instantiation does not carry the generic trial path)
    __device__ __forceinline__ bool trial_fast_ok() const { if constexpr (NSC > 0 && NSC <= kWave) return kFusedPasses; else return kFusedPasses && L.n <= kWave; }      // (a kernel with clearance-row code only runs for handles that have rows)      // (the extended instantiations and the fp64 bicycle / front-wheel models keep those registers for what they add: no scratch memory anywhere)
    // the part of the set-up that no other pass holds: the switches, and the lane's interval (x_k, x_k+1 and their steps)
    __device__ __forceinline__ void trial_setup_states(TrialRegs& r, int k) const {
        const int n = L.n;
        r.k = k; r.stage = k < n - 1;
        r.quad = quad(); r.mint = mintime(); r.dtf = dtf(); r.nm1 = T(n - 1);
        r.dt_lb = P.dt_lb; r.dt_ub = P.dt_ub;
        for (int i = 0; i < 3; ++i) {
            r.xk[i] = r.dxk[i] = r.xn[i] = r.dxn[i] = T(0);
            if (r.stage) {
                r.xk[i] = F(L.X, i, k); r.xn[i] = F(L.X, i, k + 1);
                if (k > 0) r.dxk[i] = F(L.DX, i, k);
                if (k + 1 < n - 1 || !fx(i)) r.dxn[i] = F(L.DX, i, k + 1);
            }
        }
    }
    __device__ __forceinline__ void trial_setup(TrialRegs& r, T dd) const {
        MPC_PHASE_LANE
        const int n = L.n, k = lane;
        const T d = SCL(SC_D);
        trial_setup_states(r, k);
        for (int j = 0; j < 2; ++j) {
            r.ulb[j] = P.u_lb[j]; r.uub[j] = P.u_ub[j];
            r.u[j] = r.stage ? F(L.U, j, k) : T(0); r.du[j] = r.stage ? F(L.DU, j, k) : T(0);
        }
        for (int q = 0; q < 4; ++q) {
            r.on[q] = k < n && row_on(k, q);
            r.s[q] = T(1); r.ds[q] = T(0);
            if (r.on[q]) { const T s = F(L.SR, q, k); r.s[q] = s; r.ds[q] = -(row_val(L.U, d, k, q) + s) - row_jdz(k, q, dd); }
        }
    }
    // kBatchedReductions: the kernels whose passes carry their wave reductions through the DPP steps together (wave_reduce_n) -- the fixed layout's, shape known or not;
    // every other kernel keeps one chain per value, and with it its registers and its text
    static constexpr bool kBatchedReductions = NSC != 0;
    // returns wave-reduced sum|c| (th), objective (fo) and the sum of the barrier logs at z + alpha dz, dt = d
    __device__ __forceinline__ void trial_eval(const TrialRegs& r, T alpha, T d, T& th_out, T& fo_out, T& logs_out) const {
        MPC_PHASE_LANE
        T th = T(0), fo = T(0);
        LogAccT acc;
        if (r.stage) {
            const T x0_ = r.xk[0] + alpha * r.dxk[0], x1_ = r.xk[1] + alpha * r.dxk[1];
            const T x2_ = r.k > 0 ? normalize_theta(r.xk[2] + alpha * r.dxk[2]) : r.xk[2];
            const T n0 = r.xn[0] + alpha * r.dxn[0], n1 = r.xn[1] + alpha * r.dxn[1];
            const T n2 = r.dxn[2] != T(0) ? normalize_theta(r.xn[2] + alpha * r.dxn[2]) : r.xn[2];
            const T v = r.u[0] + alpha * r.du[0], w = r.u[1] + alpha * r.du[1];
            T tr[4], tr2[2], f[3];
            model_trig_colloc<T, MODEL, kLocalLiterals>(P, colloc(), x2_, v, w, d, tr, tr2);
            colloc_f<T, MODEL>(P, colloc(), tr, tr2, v, w, f);
            const T c0 = d * f[0] - (n0 - x0_), c1 = d * f[1] - (n1 - x1_), c2 = d * f[2] - normalize_theta(n2 - x2_);
            for (int i = 0; i < NTRB; ++i) F(L.TRIG, i, r.k) = tr[i];
            if (colloc() == COLLOC_CN) { F(L.TRIG, NTRB, r.k) = tr2[0]; F(L.TRIG, NTRB + 1, r.k) = tr2[1]; }
            C_(0, r.k) = c0; C_(1, r.k) = c1; C_(2, r.k) = c2;
            th = t_abs(c0) + t_abs(c1) + t_abs(c2);
            if (r.quad) {
                const T xd0 = x0_ - xf[0], xd1 = x1_ - xf[1], xd2 = normalize_theta(x2_ - xf[2]);
                fo = (P.Q[0] * xd0 * xd0 + P.Q[1] * xd1 * xd1 + P.Q[2] * xd2 * xd2 + P.R[0] * v * v + P.R[1] * w * w) * (intf() ? d : T(1));
            }
            if (via()) { T vv, vg[3]; via_terms(r.k, x0_, x1_, x2_, vv, vg); fo += vv; }
            acc.mul(v - r.ulb[0]); acc.mul(r.uub[0] - v); acc.mul(w - r.ulb[1]); acc.mul(r.uub[1] - w);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc.mul(r.s[q] + alpha * r.ds[q]);      // rows that are off carry s = 1, ds = 0
        if (lane == 0) {
            if (r.mint) fo += r.nm1 * d;
            if (hasqf()) {
                for (int i = 0; i < 3; ++i) if (!fx(i)) {
                    T xd = xt(i, L.n - 1, alpha) - xf[i];
                    if (i == 2) xd = normalize_theta(xd);
                    fo += P.Qf[i] * xd * xd;
                }
            }
            if (r.dtf) { acc.mul(d - r.dt_lb); acc.mul(r.dt_ub - d); }
            if (ball()) { T a[3]; const T st = ball_slack(alpha, true); th += t_abs(ball_eval(alpha, a) + st); acc.mul(st); }
        }
        if constexpr (kBatchedReductions) {
            T r3[3] = {th, fo, acc.value()};
            wave_reduce_n<OpSum, OpSum, OpSum>(r3);
            th_out = r3[0]; fo_out = r3[1]; logs_out = r3[2];
        } else {
        th_out = wave_sum(th); fo_out = wave_sum(fo); logs_out = wave_sum(acc.value());
        }
    }

    // ---------------------------------------------------------------- KKT error + stage records
    struct Err { T rd, rp, cmin, cmax, csum, sum_mult, sum_bmult, theta; int n_mult, n_bmult; };     // csum: sum of the n_bmult complementarity products

    // Ipopt's scaled optimality error E_mu.  (reciprocals instead of IEEE divisions -- ~100 ticks each for a lone wave --: 1/count is cached with the counts,
    // 1/s_max is a constant, the two scalings are inverted once per call)
    __device__ __forceinline__ T err_value(const Err& e, T mu_t) const {
        const T sd = t_max(Algo<T>::s_max, e.sum_mult * inv_cnt_mult) * (T(1) / Algo<T>::s_max);
        const T sc = t_max(Algo<T>::s_max, e.sum_bmult * inv_cnt_bmult) * (T(1) / Algo<T>::s_max);
        T comp = e.n_bmult > 0 ? t_max(e.cmax - mu_t, mu_t - e.cmin) : T(0);
        return t_max(e.rd * t_rcp(sd), t_max(e.rp, comp * t_rcp(sc)));
    }

    // parallel: KKT error pieces (needs LAM of the neighbours) ; also writes the mu-independent part of STG
    __device__ __forceinline__ Err kkt_pass() const {
        MPC_PHASE_LANE
        const int n = L.n;
        const T d = SCL(SC_D);
        if (nM() > 0) {      // value, gradient and curvature of every clearance row at the current point -> the rows' caches, one (grid point, row) pair per lane
            for_each_row([&](int k, int m) {
                T g, a3[3], hk, h3[3], ad, hd[4];
                if (!obst_row3(k, m, F(L.X, 0, k), F(L.X, 1, k), F(L.X, 2, k), g, a3, hk, h3, d, ad, hd)) return;
                OB_(0, m, k) = g; OB_(1, m, k) = a3[0]; OB_(2, m, k) = a3[1]; OB_(3, m, k) = hk;
                if (fpline() || dynobs()) { OX_(0, m, k) = a3[2]; OX_(1, m, k) = h3[0]; OX_(2, m, k) = h3[1]; OX_(3, m, k) = h3[2]; }
                if (dynturn()) { OX_(4, m, k) = ad; OX_(5, m, k) = hd[0]; OX_(6, m, k) = hd[1]; OX_(7, m, k) = hd[2]; OX_(8, m, k) = hd[3]; }
            });
            sync();
        }
        T rd = T(0), rp = T(0), cmin = T(1e30), cmax = T(0), smult = T(0), sb = T(0), th = T(0), rdd = T(0), cs = T(0);
        int nm = 0, nb = 0;
        for (int k = lane; k < n; k += kWave) {
            T rec[21];
            if (k < n - 1) {
                T lam[3] = {F(L.LAM, 0, k), F(L.LAM, 1, k), F(L.LAM, 2, k)};
                T tr[4] = {F(L.TRIG, 0, k), F(L.TRIG, 1, k), F(L.TRIG, 2, k), NTRB > 3 ? F(L.TRIG, 3, k) : T(0)};
                T tr2[2] = {T(0), T(0)};
                if (colloc() == COLLOC_CN) { tr2[0] = F(L.TRIG, NTRB, k); tr2[1] = F(L.TRIG, NTRB + 1, k); }
                T v = F(L.U, 0, k), w = F(L.U, 1, k);
                // derivatives of the collocation increment D(theta, u, dt) (forward or midpoint differences, mpc_core.hpp::stage_map);
                // gJ[j] = lam' dD/dq_j is what the dual residuals need, Jdt = dD/d dt the dt column of the row
                StageMap<T> sm_;
                stage_map<T, MODEL>(P, colloc(), tr, tr2, v, w, d, lam, sm_);
                T gJ[3];
                for (int j = 0; j < 3; ++j) gJ[j] = lam[0] * sm_.Jq[0][j] + lam[1] * sm_.Jq[1][j] + lam[2] * sm_.Jq[2][j];
                // stage record, mu-independent part: kept in registers and stored at the END of the loop body -- every LDS store
                // forces the loads that follow it in program order to be re-issued and waited for (possible aliasing)
                rec[0] = sm_.Jq[0][0]; rec[1] = sm_.Jq[1][0];
                rec[2] = sm_.Jdt[0]; rec[3] = sm_.Jdt[1]; rec[4] = sm_.Jdt[2];
                for (int a = 0; a < 3; ++a) { rec[5 + a] = sm_.Jq[a][1]; rec[8 + a] = sm_.Jq[a][2]; }
                rec[11] = sm_.Hqq[0][0]; rec[12] = sm_.Hqq[0][1]; rec[13] = sm_.Hqq[0][2];
                rec[14] = sm_.Hqq[1][1]; rec[15] = sm_.Hqq[1][2]; rec[16] = sm_.Hqq[2][2];
                rec[17] = sm_.Hqd[0]; rec[18] = sm_.Hqd[1]; rec[19] = sm_.Hqd[2];
                rec[20] = sm_.Hdd;
                for (int i = 0; i < 3; ++i) {
                    T ci = C_(i, k);
                    rp = t_max(rp, t_abs(ci)); th += t_abs(ci); smult += t_abs(lam[i]);
                }
                nm += 3;
                rdd += lam[0] * sm_.Jdt[0] + lam[1] * sm_.Jdt[1] + lam[2] * sm_.Jdt[2];
                T gx[3] = {T(0), T(0), T(0)}, gu[2] = {T(0), T(0)};
                if (quad()) {
                    T xd[3] = {F(L.X, 0, k) - xf[0], F(L.X, 1, k) - xf[1], normalize_theta(F(L.X, 2, k) - xf[2])};
                    const T w8 = intf() ? d : T(1);
                    for (int i = 0; i < 3; ++i) gx[i] = T(2) * P.Q[i] * xd[i] * w8;
                    gu[0] = T(2) * P.R[0] * v * w8; gu[1] = T(2) * P.R[1] * w * w8;
                    if (intf()) rdd += P.Q[0] * xd[0] * xd[0] + P.Q[1] * xd[1] * xd[1] + P.Q[2] * xd[2] * xd[2] + P.R[0] * v * v + P.R[1] * w * w;
                    if (costx()) {
                        T qo[3]; offmul(P.Qo, xd, qo);
                        for (int i = 0; i < 3; ++i) gx[i] += T(2) * qo[i] * w8;
                        gu[0] += T(2) * P.Ro * w * w8; gu[1] += T(2) * P.Ro * v * w8;
                        if (intf()) rdd += offquad(P.Qo, xd) + T(2) * P.Ro * v * w;
                        if (k == 0 && P.trapz) rdd -= T(0.5) * fullquad(P.Q, P.Qo, xd);
                    }
                }
                if (via()) { T vv; via_terms(k, F(L.X, 0, k), F(L.X, 1, k), F(L.X, 2, k), vv, gx); }
                T osx = T(0), osy = T(0), ost = T(0);
                if (nM() > 0 && k >= 1) {
                    for (int m0 = 0; m0 < nM(); m0 += kRowGroup) {
                    RowCache oc;
                    ob_load<false>(m0, k, oc);
#pragma unroll
                    for (int jm = 0; jm < kRowGroup; ++jm) {
                        const int m = m0 + jm;
                        if (m >= nM()) break;
                        if (oi(m, k) < 0) continue;
                        const T g = oc.g[jm], ax = oc.ax[jm], ay = oc.ay[jm];
                        T a3[3] = {ax, ay, T(0)}, ad = T(0);
                        if (fpline() || dynobs()) a3[2] = OX_(0, m, k);
                        if (dynturn()) ad = OX_(4, m, k);
                        const T s = F(L.OS, m, k), y = F(L.OY, m, k);
                        const T ee = erho > T(0) ? T(OE_(0, m, k)) : T(0);            // restoration mode: the row reads g + s - e = 0
                        const T res = g + s - ee;
                        rp = t_max(rp, t_abs(res)); th += t_abs(res);
                        cmin = t_min(cmin, s * y); cmax = t_max(cmax, s * y); cs += s * y;
                        sb += y; nb += 1;
                        if (erho > T(0)) {      // the elastic variable's own complementarity, e (rho - y); e itself counts as infeasibility of the ORIGINAL row
                            const T ce = ee * (erho - y);
                            cmin = t_min(cmin, ce); cmax = t_max(cmax, ce); cs += ce;
                            sb += erho - y; nb += 1;
                            rp = t_max(rp, ee);
                        }
                        osx += y * ax; osy += y * ay;
                        if (dynturn()) { rdd += y * ad; ost += y * a3[2]; }
                        else if (dynobs()) rdd += y * a3[2]; else ost += y * a3[2];
                    }
                    }
                }
                if (k >= 1) {
                    T r0 = gx[0] + osx + lam[0] - F(L.LAM, 0, k - 1);
                    T r1 = gx[1] + osy + lam[1] - F(L.LAM, 1, k - 1);
                    T r2 = gx[2] + ost + lam[2] + gJ[0] - F(L.LAM, 2, k - 1);
                    rd = t_max(rd, t_max(t_abs(r0), t_max(t_abs(r1), t_abs(r2))));
                }
                for (int j = 0; j < 2; ++j) {
                    T u = j == 0 ? v : w;
                    T pl = F(L.PL, j, k), pu = F(L.PU, j, k);
                    T r = gu[j] + gJ[1 + j] - pl + pu;
                    for (int q = j; q < 4; q += 2) {
                        const T sg = slot_sign<T>(q);
                        if (row_on(k, q)) r += sg * F(L.YR, q, k);
                        if (row_on(k + 1, q)) r -= sg * F(L.YR, q, k + 1);
                    }
                    rd = t_max(rd, t_abs(r));
                    T cl = (u - P.u_lb[j]) * pl, cu = (P.u_ub[j] - u) * pu;
                    cmin = t_min(cmin, t_min(cl, cu)); cmax = t_max(cmax, t_max(cl, cu)); cs += cl + cu;
                    sb += pl + pu; nb += 2;
                }
                if (k == n - 2) {
                    T ta[3] = {T(0), T(0), T(0)}, ty = T(0);
                    if (ball()) {        // terminal l2-ball row: value / gradient cache for the step, residuals
                        const T tg = ball_eval(T(0), ta), ts = SCL(SC_TS);
                        ty = SCL(SC_TY);
                        SCL(SC_TG) = tg; SCL(SC_TA) = ta[0]; SCL(SC_TA + 1) = ta[1]; SCL(SC_TA + 2) = ta[2];
                        rp = t_max(rp, t_abs(tg + ts)); th += t_abs(tg + ts);
                        cmin = t_min(cmin, ts * ty); cmax = t_max(cmax, ts * ty); cs += ts * ty;
                        sb += ty; nb += 1;
                    }
                    T gext[3] = {T(0), T(0), T(0)};
                    if (costx()) {       // off-diagonal terminal cost, trapezoid term of the final state (gradient, and its share of d/d dt)
                        T xdT[3], y3[3]; xd_final(T(0), xdT);
                        if (hasqf()) { offmul(P.Qfo, xdT, y3); for (int i = 0; i < 3; ++i) gext[i] += T(2) * y3[i]; }
                        if (P.trapz) {
                            offmul(P.Qo, xdT, y3);
                            for (int i = 0; i < 3; ++i) gext[i] += d * (P.Q[i] * xdT[i] + y3[i]);
                            rdd += T(0.5) * fullquad(P.Q, P.Qo, xdT);
                        }
                    }
                    for (int i = 0; i < 3; ++i) if (!fx(i)) {
                        T g = gext[i];
                        if (hasqf()) {
                            T xd = F(L.X, i, n - 1) - xf[i];
                            if (i == 2) xd = normalize_theta(xd);
                            g += T(2) * P.Qf[i] * xd;
                        }
                        rd = t_max(rd, t_abs(g + ty * ta[i] - lam[i]));
                    }
                }
            }
            for (int q = 0; q < 4; ++q) {
                if (!row_on(k, q)) continue;
                T s = F(L.SR, q, k), y = F(L.YR, q, k);
                T res = row_val(L.U, d, k, q) + s;
                rp = t_max(rp, t_abs(res)); th += t_abs(res);
                cmin = t_min(cmin, s * y); cmax = t_max(cmax, s * y); cs += s * y;
                sb += y; nb += 1;
                if (k > 0) rdd -= slot_sign<T>(q) * P.rate_lim[q] * y;
            }
            if (k < n - 1) {
                if constexpr (GS) { for (int i = 0; i < 3; ++i) TL_(TE_CC + i, k) = C_(i, k); }      // c_k where the sweeps' pointers live
                S_(0, k) = rec[0]; S_(1, k) = rec[1]; S_(2, k) = T(1);                 // column 2 of Ghat: (a0, a1, 1)
                S_(3, k) = rec[2]; S_(4, k) = rec[3]; S_(5, k) = rec[4];
                for (int a = 0; a < 3; ++a) { S_(6 + a, k) = rec[5 + a]; S_(9 + a, k) = rec[8 + a]; }   // Bx column-major
                // raw (mu-independent) pieces parked in their A slots; stage_barrier_terms() turns them into the combined entries
                S_(RA + A22, k) = rec[11]; S_(RA + A26, k) = rec[12]; S_(RA + A27, k) = rec[13];
                S_(RA + A66, k) = rec[14]; S_(RA + A67, k) = rec[15]; S_(RA + A77, k) = rec[16];
                S_(RA + A25, k) = rec[17]; S_(RA + A56, k) = rec[18]; S_(RA + A57, k) = rec[19]; S_(RA + A55, k) = rec[20];
            }
        }
        if (lane == 0) {
            if (mintime()) rdd += T(n - 1);
            if (dtf()) {
                T pl = SCL(SC_PDL), pu = SCL(SC_PDU);
                rdd += -pl + pu;
                T cl = (d - P.dt_lb) * pl, cu = (P.dt_ub - d) * pu;
                cmin = t_min(cmin, t_min(cl, cu)); cmax = t_max(cmax, t_max(cl, cu)); cs += cl + cu;
                sb += pl + pu; nb += 2;
            }
        }
        Err e;
        if constexpr (kBatchedReductions) {      // the nine reductions in two batches (the registers of a batch's moves stay few), two compare-and-select chains in each:
            T ra[5] = {rdd, rd, rp, cs, sb}, rb[4] = {cmin, cmax, smult, th};      // the sums of a batch stand between a compare and the select that reads its mask
            wave_reduce_n<OpSum, OpMax, OpMax, OpSum, OpSum>(ra);
            wave_reduce_n<OpMin, OpMax, OpSum, OpSum>(rb);
            rdd = ra[0]; e.rd = ra[1]; e.rp = ra[2]; e.csum = ra[3]; e.sum_bmult = ra[4];
            if (dtf()) e.rd = t_max(e.rd, t_abs(rdd));
            e.cmin = rb[0]; e.cmax = rb[1]; e.sum_mult = rb[2] + e.sum_bmult; e.theta = rb[3];
        } else {
        rdd = wave_sum(rdd);
        e.rd = wave_max(rd);
        if (dtf()) e.rd = t_max(e.rd, t_abs(rdd));
        e.rp = wave_max(rp);
        e.cmin = wave_min(cmin);
        e.cmax = wave_max(cmax);
        e.csum = wave_sum(cs);
        e.sum_bmult = wave_sum(sb);
        e.sum_mult = wave_sum(smult) + e.sum_bmult;
        e.theta = wave_sum(th);
        }
        if (nM() == 0 && cnt_bmult >= 0) { e.n_bmult = cnt_bmult; e.n_mult = cnt_mult; }      // without clearance rows the counts never change
        else {
            e.n_bmult = (int)wave_sum((T)nb);
            e.n_mult = (int)wave_sum((T)nm) + e.n_bmult;
            cnt_bmult = e.n_bmult; cnt_mult = e.n_mult;
            inv_cnt_bmult = T(1) / T(e.n_bmult > 0 ? e.n_bmult : 1); inv_cnt_mult = T(1) / T(e.n_mult > 0 ? e.n_mult : 1);
        }
        return e;
    }

    // parallel: combine the raw pieces with the mu-dependent condensed barrier terms into the A-form; record n-1 = final rate rows
    __device__ __forceinline__ void stage_barrier_terms() const {
        MPC_PHASE_LANE
        const int n = L.n;
        const T d = SCL(SC_D);
        const bool quad = this->quad();
        T q2[3] = {T(0), T(0), T(0)}, r2[2] = {T(0), T(0)};
        if (quad) { const T w8 = intf() ? d : T(1); for (int i = 0; i < 3; ++i) q2[i] = T(2) * P.Q[i] * w8; for (int j = 0; j < 2; ++j) r2[j] = T(2) * P.R[j] * w8; }
        for (int k = lane; k < n; k += kWave) {
            StageParts<T> sp;
            sp.h00 = S_(RA + A22, k); sp.h01 = S_(RA + A26, k); sp.h02 = S_(RA + A27, k);
            sp.h11 = S_(RA + A66, k); sp.h12 = S_(RA + A67, k); sp.h22 = S_(RA + A77, k);
            sp.g[0] = S_(RA + A25, k); sp.g[1] = S_(RA + A56, k); sp.g[2] = S_(RA + A57, k);
            sp.hdd = k < n - 1 ? S_(RA + A55, k) : T(0);
            if (EXT && hessm() && k < n - 1) {       // MPC_HESSIAN_CONVEXIFIED: positive semidefinite part of the stage's curvature block (theta, v, w, dt)
                StageMap<T> pm;
                pm.Hqq[0][0] = sp.h00; pm.Hqq[0][1] = pm.Hqq[1][0] = sp.h01; pm.Hqq[0][2] = pm.Hqq[2][0] = sp.h02;
                pm.Hqq[1][1] = sp.h11; pm.Hqq[1][2] = pm.Hqq[2][1] = sp.h12; pm.Hqq[2][2] = sp.h22;
                pm.Hqd[0] = sp.g[0]; pm.Hqd[1] = sp.g[1]; pm.Hqd[2] = sp.g[2]; pm.Hdd = sp.hdd;
                psd_project4(pm, k == 0);
                sp.h00 = pm.Hqq[0][0]; sp.h01 = pm.Hqq[0][1]; sp.h02 = pm.Hqq[0][2]; sp.h11 = pm.Hqq[1][1]; sp.h12 = pm.Hqq[1][2]; sp.h22 = pm.Hqq[2][2];
                sp.g[0] = pm.Hqd[0]; sp.g[1] = pm.Hqd[1]; sp.g[2] = pm.Hqd[2]; sp.hdd = pm.Hdd;
            }
            sp.hx[0] = sp.hx[1] = sp.hx[2] = T(0);
            if (quad && k < n - 1) {
                sp.hx[0] = q2[0] * (F(L.X, 0, k) - xf[0]); sp.hx[1] = q2[1] * (F(L.X, 1, k) - xf[1]);
                sp.hx[2] = q2[2] * normalize_theta(F(L.X, 2, k) - xf[2]);
            }
            sp.sz[0] = sp.sz[1] = sp.gb[0] = sp.gb[1] = T(0);
            if (k < n - 1) {
                for (int j = 0; j < 2; ++j) {
                    T u = F(L.U, j, k);
                    const T idl = t_rcp(u - P.u_lb[j]), idu = t_rcp(P.u_ub[j] - u);      // one reciprocal per bound, shared by all quotients
                    sp.sz[j] = F(L.PL, j, k) * idl + F(L.PU, j, k) * idu;
                    sp.gb[j] = mu * idu - mu * idl + r2[j] * u;
                }
            }
            sp.ss[0] = sp.ss[1] = sp.sl[0] = sp.sl[1] = sp.sll = sp.gy[0] = sp.gy[1] = sp.gyl = T(0);
            for (int q = 0; q < 4; ++q) {
                if (!row_on(k, q)) continue;
                const int j = q & 1;
                const T sg = slot_sign<T>(q), lim = k > 0 ? P.rate_lim[q] : T(0);
                T s = F(L.SR, q, k), y = F(L.YR, q, k);
                const T is = t_rcp(s);
                T sig = y * is;
                T ybar = mu * is + sig * (row_val(L.U, d, k, q) + s);
                sp.ss[j] += sig; sp.sl[j] += sig * lim; sp.sll += sig * lim * lim;
                sp.gy[j] += sg * ybar; sp.gyl += sg * lim * ybar;
            }
            sp.oxx = sp.oxy = sp.oyy = sp.ogx = sp.ogy = T(0);
            if (nM() > 0 && k >= 1 && k < n - 1) {
                for (int m0 = 0; m0 < nM(); m0 += kRowGroup) {
                RowCache oc;
                ob_load<true>(m0, k, oc);
#pragma unroll
                for (int jm = 0; jm < kRowGroup; ++jm) {
                    const int m = m0 + jm;
                    if (m >= nM()) break;
                    if (oi(m, k) < 0) continue;
                    const T s = F(L.OS, m, k), y = F(L.OY, m, k), g = oc.g[jm];
                    const T ax = oc.ax[jm], ay = oc.ay[jm], hk = oc.hk[jm];
                    const T is = t_rcp(s);
                    T sig = y * is;
                    T ybar = mu * is + sig * (g + s);
                    if (erho > T(0)) elastic_condense(s, y, g, T(OE_(0, m, k)), sig, ybar);
                    // hess(g) = -hk (I - a a')
                    sp.oxx += sig * ax * ax - y * hk * (T(1) - ax * ax);
                    sp.oxy += sig * ax * ay + y * hk * ax * ay;
                    sp.oyy += sig * ay * ay - y * hk * (T(1) - ay * ay);
                    sp.ogx += ax * ybar; sp.ogy += ay * ybar;
                    if (fpline()) {
                        const T at = OX_(0, m, k);
                        sp.oxt += sig * ax * at + y * OX_(1, m, k);
                        sp.oyt += sig * ay * at + y * OX_(2, m, k);
                        sp.ott += sig * at * at + y * OX_(3, m, k);
                        sp.ogt += at * ybar;
                    }
                    if (dynturn()) {      // dt parts next to the heading parts: x dt, y dt, theta dt, dt dt
                        const T ad = OX_(4, m, k), at = OX_(0, m, k);
                        sp.cxd[0] += sig * ax * ad + y * OX_(5, m, k);
                        sp.cxd[1] += sig * ay * ad + y * OX_(6, m, k);
                        sp.cxd[2] += sig * at * ad + y * OX_(8, m, k);
                        sp.hdd += sig * ad * ad + y * OX_(7, m, k);
                        sp.gdt += ad * ybar;
                    } else if (dynobs()) {       // dt parts of the rows of dynamic obstacles (zero for the static ones)
                        const T ad = OX_(0, m, k);
                        sp.cxd[0] += sig * ax * ad + y * OX_(1, m, k);
                        sp.cxd[1] += sig * ay * ad + y * OX_(2, m, k);
                        sp.hdd += sig * ad * ad + y * OX_(3, m, k);
                        sp.gdt += ad * ybar;
                    }
                }
                }
            }
            if (intf() && k < n - 1) {       // d/ddt and the mixed second derivatives of  dt * (xd'Q xd + u'R u)
                const T xd0 = F(L.X, 0, k) - xf[0], xd1 = F(L.X, 1, k) - xf[1], xd2 = normalize_theta(F(L.X, 2, k) - xf[2]);
                const T v = F(L.U, 0, k), w = F(L.U, 1, k);
                if (k > 0) { sp.cxd[0] += T(2) * P.Q[0] * xd0; sp.cxd[1] += T(2) * P.Q[1] * xd1; sp.cxd[2] += T(2) * P.Q[2] * xd2; }   // x_0 is not a variable
                sp.cud[0] = T(2) * P.R[0] * v; sp.cud[1] = T(2) * P.R[1] * w;
                sp.gdt += P.Q[0] * xd0 * xd0 + P.Q[1] * xd1 * xd1 + P.Q[2] * xd2 * xd2 + P.R[0] * v * v + P.R[1] * w * w;
            }
            if (via() && k >= 1 && k < n - 1) {
                T vv, vg[3];
                const int m = via_terms(k, F(L.X, 0, k), F(L.X, 1, k), F(L.X, 2, k), vv, vg);
                const T h = T(2) * P.vp_wp * T(m);
                sp.oxx += h; sp.oyy += h; sp.ogx += vg[0]; sp.ogy += vg[1]; sp.hx[2] += vg[2];
            }
            if (costx() && quad && k < n - 1) {       // off-diagonal weights: Hessian slots A01 A02 A12 A67, gradients, dt coupling; trapezoid: x_0's half term
                const T w8 = intf() ? d : T(1);
                const T xd[3] = {F(L.X, 0, k) - xf[0], F(L.X, 1, k) - xf[1], normalize_theta(F(L.X, 2, k) - xf[2])};
                const T v = F(L.U, 0, k), w = F(L.U, 1, k);
                T qo[3]; offmul(P.Qo, xd, qo);
                sp.oxy += T(2) * P.Qo[0] * w8; sp.oxt += T(2) * P.Qo[1] * w8; sp.oyt += T(2) * P.Qo[2] * w8;
                sp.h12 += T(2) * P.Ro * w8;
                for (int i = 0; i < 3; ++i) sp.hx[i] += T(2) * qo[i] * w8;
                sp.gb[0] += T(2) * P.Ro * w * w8; sp.gb[1] += T(2) * P.Ro * v * w8;
                if (intf()) {
                    if (k > 0) for (int i = 0; i < 3; ++i) sp.cxd[i] += T(2) * qo[i];
                    sp.cud[0] += T(2) * P.Ro * w; sp.cud[1] += T(2) * P.Ro * v;
                    sp.gdt += offquad(P.Qo, xd) + T(2) * P.Ro * v * w;
                    if (k == 0 && P.trapz) sp.gdt -= T(0.5) * fullquad(P.Q, P.Qo, xd);
                }
            }
            T A[NADD];
            assemble_adds(sp, q2, r2, A);
#pragma unroll
            for (int i = 0; i < NADDv; ++i) S_(RA + i, k) = A[i];
        }
    }

