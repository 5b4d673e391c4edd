// mpc_wave_solve.inc: the interior-point loop (restoration entry, barrier strategy, regularisation, line search) -- part of struct IpmWave (mpc_wave.hpp includes this file inside the struct's body; not a translation unit of its own).

    // ---------------------------------------------------------------- driver (all lanes, uniform control flow)
    // enters the restoration mode at the current point (the caches of kkt_pass hold the rows' values there); returns what the objective gains: rho x sum of e.
    // dtheta: what the NON-LINEAR part of the infeasibility (theta_c of solve(): sum |c| + sum |g + s - e| at the last accepted point) changes by -- every row's |g + s| with the
    // slack it had leaves, |g + s - e| with the reset slack and the new e (zero, or the floor mu / rho) enters.  Without it the first line search after the entry would
    // take the rows' OLD violation for linear rows' infeasibility and understate every trial merit by rho (1 - alpha) x that amount (ADVICE r05).
    __device__ __forceinline__ T enter_restoration(T& dtheta) {
        const int n = L.n;
        erho = Algo<T>::elastic_rho;
        T esum = T(0), dth = T(0);
        for (int k = lane; k < n - 1; k += kWave) {
            if (k < 1) continue;
            for (int m = 0; m < nM(); ++m) {
                if (oi(m, k) < 0) continue;
                const T g = OB_(0, m, k);
                const T s_old = F(L.OS, m, k);
                const T s = t_max(t_max(-g, Algo<T>::clearance_slack_push), s_old);
                const T ee = t_max(g + s, mu / erho);
                const T y = t_max(t_min(F(L.OY, m, k), T(0.5) * erho), mu / s);
                F(L.OS, m, k) = s; F(L.OY, m, k) = y; OE_(0, m, k) = ee; OE_(1, m, k) = T(0);
                esum += ee;
                dth += t_abs(g + s - ee) - t_abs(g + s_old);
            }
        }
        esum = wave_sum(esum);
        dtheta = wave_sum(dth);
        sync();
        return erho * esum;
    }

    __device__ __forceinline__ SolveStats<T> solve() {
        SolveStats<T> out;
        flags = MPC_SHAPE_FLAGS(P);      // (mpc_core.hpp; SHAPE != 0: the launch plan has held this word to SHAPE, and the accessors of the shape's bits read the constant)
        flags = __builtin_amdgcn_readfirstlane(flags);
        nfix = (int)fx(0) + (int)fx(1) + (int)fx(2);
        row0_on = dtprev != T(0);
        if constexpr (kLocalLiterals) colloc_ = uni_(P.collocation);
        if (iter_cap <= 0) iter_cap = P.max_iter;
        if (lane < 8) sm[L.ZC + lane] = lane == 4 ? T(1) : T(0);      // constant coefficient triples of the sweeps
        if constexpr (GS) {      // ... and their copies where the sweeps' pointers live: the single words, and 0 0 0 1 0 0 in every stage's tile slot (guard tile and spare tiles included)
            if (lane < 8) gw((unsigned)(GlobalStage::ZC + lane)) = lane == 4 ? T(1) : T(0);
            for (int k = lane - GlobalStage::kGuard; k < 4 * GlobalStage::tiles(L.NS) - GlobalStage::kGuard; k += kWave) {
#pragma unroll
                for (int j = 0; j < 6; ++j) TL_(TE_Z + j, k) = j == 3 ? T(1) : T(0);
            }
        }
        if (lane < 12) sm[L.ZI + lane] = lane == 6 ? T(1) : T(0);     // unit vectors / zeros of the partitioned sweep's combine step
        const bool pit = pit_enabled();
        PitLaneConsts plc{};      // fixed layout: the partitioned sweeps' per-lane constants, once per solve (mpc_wave_pit.inc); empty otherwise
        if constexpr (NSC != 0) { if (pit) plc = pit_lane_consts(); }
        init_point();
        U(mu, rho, delta_last); U(x0[0], x0[1], x0[2]); U(xf[0], xf[1], xf[2]); U(uprev[0], uprev[1], dtprev);
        T theta_c, fobj;
        eval_point(SCL(SC_D), theta_c, fobj);
        U(theta_c, fobj);
        sync();
        int it = 0, status = ST_MAX_ITER, n_acc = 0;
        // What the loop reads of the problem record, fetched ONCE and kept in scalar registers: P lives in LDS, so every P.x inside the loop is a ds_read the compiler may not
        // hoist over the passes' LDS stores, waited for on the spot by a lone wave; tol / 10 was an IEEE division of the same two operands in every barrier update.
        const T tol = uni_(P.tol), tol10 = uni_(P.tol / T(10));
        const bool mu_monotone = uni_(P.mu_strategy) == 1;
        const long long max_ticks = uni_(P.max_ticks);
        const long long t_start = max_ticks > 0 ? (long long)wall_clock64() : 0ll;      // mpc_config.max_time_us: this solve's own clock
        const T acc_tol = uni_(P.acc_tol);
        const int acc_it = uni_(P.acc_iter);
        T e0 = T(0), logs_cur = T(0), dc_mu = T(-1), dc_val = T(0);
        T last_alpha = T(0), last_ad = T(0);
        int jam_streak = 0;
        T jam_theta0 = T(0);
        bool endgame = false;
        T mu_max = Algo<T>::mu_max_fact * mu; U(mu_max);
        bool have_logs = false;
        // Ipopt's filter (mpc_config.line_search = MPC_LS_FILTER), all of it in ONE register of the wave: lane f < flt_cap keeps theta of the f-th pair of the current barrier
        // problem, lane flt_cap + f its phi (a ring: the oldest pair is overwritten), lane 32 the infeasibility of the start point, lane 33 the mu the pairs belong to
        const bool filter = uni_(P.line_search) == 1;
        T fstate = T(-1);
        int nfilt = 0, fpos = 0;
        static_assert(Algo<T>::flt_cap == 16, "the filter's pairs sit in DPP rows 0 and 1");
        MPC_PROF_BEGIN
        while (true) {
            Err er;
            MPC_GAP_END(GLUE_BACK_EDGE);
            MPC_MARK("KKT_BEGIN");
            MPC_TICK(KKT, er = kkt_pass());
            U(er.rd, er.rp, er.cmin, er.cmax); U(er.csum, er.sum_mult, er.sum_bmult, er.theta); U(inv_cnt_mult, inv_cnt_bmult);
            MPC_MARK("KKT_END");
            if constexpr (OBST) {
                // RESTORATION for clearance rows that jam (r05; what Ipopt leaves to its restoration phase -- src/controller.cpp:388-421 hands the NLP to Ipopt; restated in
                // the CPU restatements the tests check against; DESIGN.md section 3.3 has the derivation).  A row that starts violated pulls its slack to the boundary within a
                // few iterations; from then on the fraction-to-boundary rule admits steps of 1e-3 and the infeasibility stays where it is.  Detected as elastic_trigger
                // iterations in a row with a primal step limit below elastic_ap while the infeasibility has not fallen below elastic_prog x its value at the start of the
                // streak.  From there on the clearance rows are ELASTIC: g + s - e = 0, e >= 0, + rho e in the objective (the exact l1 penalty of the row's violation).
                // Every row is satisfied again at once -- e takes up the violation, the slack goes back to its start rule --, and rho pushes e to zero as the trajectory
                // moves out of the band.  The mode stays on until the solve ends; e counts as primal infeasibility (kkt_pass), so a solve can only end with e <= tol.
                if (nM() > 0 && erho == T(0) && jam_streak >= Algo<T>::elastic_trigger && er.theta >= Algo<T>::elastic_prog * jam_theta0) {
                    T dth_rows;
                    fobj += enter_restoration(dth_rows);
                    theta_c += dth_rows;
                    rho = T(0); have_logs = false; jam_streak = 0;
                    nfilt = 0; fpos = 0;      // the objective changed: the filter's pairs are of another barrier function
                    er = kkt_pass();
                    U(er.rd, er.rp, er.cmin, er.cmax); U(er.csum, er.sum_mult, er.sum_bmult, er.theta); U(theta_c, fobj, erho);
                }
            }
            e0 = err_value(er, T(0)); U(e0);
            // (t_max / t_min drop a NaN operand: the maxima inside e0 cannot carry one; the sums do -- ADVICE r03)
            if (!t_finite(e0) || !t_finite(er.theta) || !t_finite(er.sum_mult) || !t_finite(er.csum)) { status = ST_NUMERICAL; break; }
            if (e0 <= tol) { status = ST_CONVERGED; break; }
            // Ipopt's acceptable-level stop, counting half: acc_iter iterations in a row at the level acc_tol (mpc_config.acceptable_tol / _iter)
            n_acc = (acc_it > 0 && e0 <= acc_tol) ? n_acc + 1 : 0;
            if (acc_it > 0 && n_acc >= acc_it) { status = ST_CONVERGED; break; }
            if (it >= iter_cap) { status = ST_MAX_ITER; break; }
            if (max_ticks > 0 && (long long)wall_clock64() - t_start > max_ticks) { status = ST_TIME_LIMIT; break; }
            if (win_ptr) {      // hedged candidate: one L2 read per iteration (all lanes, same word)
                const int w = __builtin_amdgcn_readfirstlane(__hip_atomic_load(win_ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                if (w < my_cand) { status = ST_SUPERSEDED; break; }
            }
            if (mu_monotone || endgame) {        // monotone Fiacco-McCormick (Ipopt's own default mu_strategy; the end game of the adaptive one)
                for (int guard = 0; guard < 50; ++guard) {
                    T emu = err_value(er, mu);
                    if (emu <= Algo<T>::kappa_eps * mu && mu > tol10) {
                        mu = t_max(tol10, t_min(Algo<T>::kappa_mu * mu, pow_(mu, Algo<T>::theta_mu)));
                        rho = T(0);
                    } else break;
                }
            } else if (it > 0) {
                // adaptive (the default; what corbo's SolverIpopt is believed to set; the first iteration keeps the start value): mu = sigma x the average complementarity, sigma from the step lengths the
                // LAST iteration achieved -- Mehrotra's (mu_aff / mu)^3 read off the step that was actually taken, no second solve --, never below
                // min(mu, mu_err_floor x E_0) (a barrier far below the optimality error is what stalls the non-convex instances), inside [tol / 10, mu_max_fact x mu_0]
                const T avg = er.csum * inv_cnt_bmult;
                const T a_ = T(1) - t_min(last_alpha, last_ad);
                const T sig = t_min(t_max(a_ * a_ * a_, Algo<T>::sigma_min), T(1));
                T mu_new = t_min(t_max(sig * avg, tol10), mu_max);
                mu_new = t_max(mu_new, t_min(mu, Algo<T>::mu_err_floor * e0));
                if (mu_new <= tol) { mu_new = tol; endgame = true; }      // end game: from mu = tol on the monotone rule takes over (tol -> tol / 10 once the barrier problem is solved to kappa_eps mu): a solve stops at a point of the central path, as with the monotone strategy
                if (mu_new != mu) { mu = mu_new; rho = T(0); }
            }
            U(mu, rho);
            MPC_GAP_END(GLUE_KKT_TO_BARRIER);
            MPC_MARK("BARRIER_BEGIN");
            MPC_TICK(BARRIER_TERMS, stage_barrier_terms(); sync());
            MPC_MARK("BARRIER_END");
            T tau = t_max(Algo<T>::tau_min, T(1) - mu);
            if (mu != dc_mu) { dc_mu = mu; dc_val = nfix > 0 ? Algo<T>::delta_c * pow_(mu, Algo<T>::kappa_c) : T(0); }   // pow() only when mu moved
            U(tau, dc_mu, dc_val);
            const T dc = dc_val;
            T delta = (fail0 && delta_last > T(0)) ? t_max(Algo<T>::delta_min, Algo<T>::kappa_minus * delta_last) : T(0);
            U(delta);
            const bool started_zero = delta == T(0);
            bool ok = false;
            Fwd fw;
            TrialRegs tregs;
            T dd = T(0), nu[3] = {T(0), T(0), T(0)}, curv = T(0);
            for (int ntry = 0; ntry <= 40; ++ntry) {
                bool good, used_pit = false;
                MPC_DBG_PIT_CHECK
                MPC_GAP_END(GLUE_BARRIER_TO_FAC);
                if (pit && mu > pit_floor()) {        // partitioned sweep; a broken-down combine pivot (or a singular stage pivot) falls back to the serial sweep; below pit_floor() the end game takes the serial sweeps
                    int gp_;
                    MPC_TICK(BACKWARD, gp_ = backward_pit(plc, delta, dc, dd, nu); sync());
                    good = used_pit = gp_ > 0;
                    if (gp_ == 0) { MPC_GAP_END(GLUE_BARRIER_TO_FAC); MPC_TICK(BACKWARD, good = backward_dpp(delta, dc, dd, nu); sync()); }
                } else { MPC_TICK(BACKWARD, good = backward_dpp(delta, dc, dd, nu); sync()); }
                MPC_PROF_COUNT(nfac);
                MPC_DBG_NANCHECK_FIELDS
                U(dd, nu[0], nu[1], nu[2]);
                if (good) {
                    MPC_GAP_END(GLUE_BARRIER_TO_FAC);
                    if (used_pit) { MPC_TICK(FORWARD, forward_pit(plc, dd, nu, delta); sync()); }
                    else { MPC_TICK(FORWARD, forward_states(dd, nu, delta); sync()); }
                    MPC_DBG_NANCHECK_STEP
                    MPC_GAP_END(GLUE_BARRIER_TO_FAC);
                    MPC_MARK("POST_BEGIN");
                    MPC_TICK(POST, fw = post_pass<kFusedPasses>(dd, nu, tau, tregs));
                    U(fw.hdz, fw.clam, fw.dz2, fw.dphi); U(fw.a_p, fw.a_d, fw.dzmax, fw.nunu);
                    MPC_MARK("POST_END");
                    good = fw.finite;
                    if (good) {      // the backward sweep has checked the inertia of this factorisation (mpc_core.hpp::riccati_root); the curvature only feeds the penalty update
                        curv = -fw.hdz + fw.clam - dc * fw.nunu; U(curv);
                        ok = true; break;
                    }
                }
                if (delta == T(0)) delta = (delta_last == T(0)) ? Algo<T>::delta_first : t_max(Algo<T>::delta_min, Algo<T>::kappa_minus * delta_last);
                else delta *= (delta_last == T(0)) ? Algo<T>::kappa_plus_first : Algo<T>::kappa_plus;
                U(delta);
                if (delta > Algo<T>::delta_max) break;
            }
            if (!ok) { status = ST_LINSOLVE; break; }
            if constexpr (OBST) {      // the restoration trigger's streak
                if (nM() > 0 && erho == T(0)) {
                    if (fw.a_p < Algo<T>::elastic_ap && er.rp > T(1e-3)) { if (jam_streak == 0) jam_theta0 = er.theta; ++jam_streak; }
                    else jam_streak = 0;
                }
            }
            if (delta > T(0)) delta_last = delta;
            U(delta_last);
            if (started_zero) fail0 = delta > T(0);
            const T theta = er.theta;
            if (!filter && theta > T(0)) {
                T sigma = curv > T(0) ? T(1) : T(0);
                T rho_trial = (fw.dphi + T(0.5) * sigma * curv) / ((T(1) - Algo<T>::rho_frac) * theta);
                if (rho < rho_trial) rho = rho_trial + T(1);
                U(rho);
            }
            T phi0;
            // sum of the barrier logs at the current point: it is the value of the last accepted trial (same point, mu-independent)
            if (!have_logs) { MPC_GAP_END(GLUE_LS_SETUP); MPC_TICK(LOGS0, logs_cur = barrier_logs(SCL(SC_D), T(0), false, dd)); have_logs = true; U(logs_cur); }
            const T rho_ls = filter ? T(0) : rho;       // the filter compares the barrier function itself
            phi0 = fobj - mu * logs_cur + rho_ls * theta;
            T Dm = fw.dphi - rho_ls * theta;
            T theta_rows = theta - theta_c;
            T alpha = fw.a_p;
            U(phi0, Dm, theta_rows, alpha);
            // filter line search, Waechter & Biegler (2006) Algorithm A steps A-5.1 .. A-5.10 without the second-order correction: the shortest step worth trying (eq. 23),
            // the switching condition's two powers (eq. 19; once per iteration), the bounds on theta
            T a_min = T(0), p_ph = T(0), p_th = T(0), theta_max = T(0), theta_min = T(0);
            if (filter) {
                T theta0 = rd_lane(fstate, 32);
                if (theta0 < T(0)) { theta0 = theta; if (lane == 32) fstate = theta; }
                if (mu != rd_lane(fstate, 33)) { nfilt = 0; fpos = 0; if (lane == 33) fstate = mu; }
                theta_max = Algo<T>::flt_thmax * t_max(T(1), theta0); theta_min = Algo<T>::flt_thmin * t_max(T(1), theta0);
                a_min = Algo<T>::flt_gth;
                if (fw.dphi < T(0)) {
                    a_min = t_min(a_min, Algo<T>::flt_gph * theta / (-fw.dphi));
                    if (theta <= theta_min) {      // the two powers of the switching condition are only ever consulted at such a point (below, and here): two pow() a solve's feasible iterations pay, the others do not (a call: 300 instructions each, 3-5 % of an iteration at n = 50)
                        p_ph = pow_cold(-fw.dphi, Algo<T>::flt_sph); p_th = pow_cold(theta, Algo<T>::flt_sth);
                        a_min = t_min(a_min, Algo<T>::flt_delta * p_th / p_ph);
                    }
                }
                a_min = a_min * Algo<T>::flt_gal * fw.a_p;
                theta_max = uni_(theta_max); theta_min = uni_(theta_min); a_min = uni_(a_min); p_ph = uni_(p_ph); p_th = uni_(p_th);      // wave-uniform, live across the trial evaluations: scalar registers in every kernel variant
            }
            bool accepted = false, sw_arm = false;
            const bool fast_trials = trial_fast_ok();
            MPC_GAP_END(GLUE_LS_SETUP);
            MPC_MARK("TSETUP_BEGIN");
            if (fast_trials && !kFusedPasses) { MPC_TICK(TRIAL_SETUP, trial_setup(tregs, dd)); }      // (kFusedPasses: post_pass has filled them)
            MPC_MARK("TSETUP_END");
            T th_t = T(0), f_t = T(0), lg_t = T(0);
            for (int ls = 0; ls < Algo<T>::max_ls; ++ls) {
                if (ls > 0) { alpha *= T(0.5); U(alpha); }
                const bool below = filter && ls > 0 && alpha < a_min;      // below the shortest step worth trying: this trial point is the one taken with an emptied filter
                T phit, tht;
                T d_t = SCL(SC_D) + (dtf_sum() ? alpha * SCL(SC_DD) : T(0)); U(d_t);
                MPC_GAP_END(GLUE_LS_SETUP);
                MPC_MARK("TRIAL_BEGIN");
                if (fast_trials) {
                    MPC_TICK(TRIAL, trial_eval(tregs, alpha, d_t, th_t, f_t, lg_t);
                             tht = th_t + (T(1) - alpha) * theta_rows;
                             phit = f_t - mu * lg_t + rho_ls * tht; sync());
                } else {
                    MPC_TICK(TRIAL, eval_point(d_t, th_t, f_t, alpha, true);
                             tht = th_t + (T(1) - alpha) * theta_rows;
                             lg_t = barrier_logs(d_t, alpha, true, dd);
                             phit = f_t - mu * lg_t + rho_ls * tht; sync());
                }
                MPC_MARK("TRIAL_END");
                MPC_PROF_COUNT(ntrial);
                U(th_t, f_t, lg_t, phit);
                if (!filter) {
                    if (t_finite(phit) && phit - phi0 - Algo<T>::ls_eps * t_abs(phi0) <= Algo<T>::eta_armijo * alpha * Dm) { accepted = true; break; }
                } else {
                    if (below) break;
                    U(tht);
                    bool okf = t_finite(phit) && tht <= theta_max;
                    if (okf) {      // acceptable to every pair of the filter (each pair with its margins, eq. 18 with the filter's theta)
                        const T f_ph = __shfl_xor(fstate, 16);      // lanes 0 .. 15: the phi of their pair
                        const bool dominated = lane < nfilt && !(tht <= (T(1) - Algo<T>::flt_gth) * fstate || phit <= f_ph - Algo<T>::flt_gph * fstate);
                        okf = __builtin_amdgcn_ballot_w64(dominated) == 0ull;
                    }
                    if (okf) {
                        const bool switching = fw.dphi < T(0) && alpha * p_ph > Algo<T>::flt_delta * p_th;
                        if (theta <= theta_min && switching) {      // f-type step: Armijo on the barrier function (eq. 20, round-off relaxed as in section 3.3)
                            if (phit - phi0 - Algo<T>::ls_eps * t_abs(phi0) <= Algo<T>::flt_eta * alpha * fw.dphi) { accepted = true; sw_arm = true; }
                        } else if (tht <= (T(1) - Algo<T>::flt_gth) * theta || phit <= phi0 - Algo<T>::flt_gph * theta) accepted = true;      // sufficient progress against the current point (eq. 18)
                    }
                    if (accepted) break;
                }
            }
            if (filter) {
                if (accepted && !sw_arm) {      // the current point enters the filter (A-7: every step but an f-type one)
                    if (lane == fpos) fstate = theta;
                    if (lane == Algo<T>::flt_cap + fpos) fstate = phi0;
                    fpos = (fpos + 1) & (Algo<T>::flt_cap - 1); nfilt = nfilt < Algo<T>::flt_cap ? nfilt + 1 : Algo<T>::flt_cap;
                }
                if (!accepted) {      // every trial step refused.  Ipopt would enter its restoration phase; here the filter is emptied and the shortest trial step taken
                    nfilt = 0; fpos = 0;
                    accepted = t_finite(f_t) && t_finite(lg_t);
                }
            }
            MPC_DBG_NANCHECK_LS_FAILED
            // Ipopt's acceptable-level stop, refused-step half (tested before the line-search failure: Ipopt answers a failed line search at an
            // acceptable point with success): every trial step refused (or only one below 1e-6 of the fraction-to-boundary step accepted) at a point
            // at the acceptable level: the solve ends here, nothing is moved (the next iteration would compute the same step and refuse it again)
            if (acc_tol > T(0) && (!accepted || alpha < T(1e-6) * fw.a_p) && e0 <= acc_tol) { status = ST_CONVERGED; break; }
            if (!accepted && alpha * fw.dzmax < T(1e-14)) { status = ST_LINESEARCH; break; }
            MPC_DBG_NANCHECK_LS
            MPC_GAP_END(GLUE_TRIAL_TO_ACCEPT);
            MPC_MARK("ACCEPT_BEGIN");
            MPC_TICK(ACCEPT, accept(alpha, fw.a_d); sync());
            MPC_MARK("ACCEPT_END");
            theta_c = th_t; fobj = f_t; logs_cur = lg_t;
            last_alpha = alpha; last_ad = fw.a_d;
            U(theta_c, fobj, logs_cur); U(last_alpha, last_ad);
            ++it;
        }
        MPC_PROF_END
        out.status = status; out.iters = it; out.kkt_error = e0; out.objective = fobj;
        return out;
    }
