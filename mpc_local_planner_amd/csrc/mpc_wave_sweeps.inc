// mpc_wave_sweeps.inc: the serial Riccati sweeps (backward_dpp, forward_states) and the multiplier recurrence -- part of struct IpmWave (mpc_wave.hpp includes this file inside the struct's body; not a translation unit of its own).

    // ---------------------------------------------------------------- backward Riccati sweep
    // terminal value function of the backward sweeps (serial and partitioned), straight into the owning lanes' registers: column c of [P | p | S];
    // a3 / a4 / a5 = this lane's entries of the rows 3..5 of the final rate rows' record (stage n-1: the A slots (i, c) for c in {3, 4, 5, 8})
    __device__ __forceinline__ void terminal_value(T (&V)[6], const int c, const T delta, const T d, const T a3, const T a4, const T a5) const {
        const int n = L.n;
        // condensed terminal l2-ball row: + sigma a a' + 2 y S on the final-state block, + a ybar on its gradient
        T tsig = T(0), tyb = T(0), ty = T(0), ta[3] = {T(0), T(0), T(0)};
        if (ball()) {
            const T ts = SCL(SC_TS), tg = SCL(SC_TG);
            ty = SCL(SC_TY);
            const T its = t_rcp(ts);
            tsig = ty * its; tyb = mu * its + tsig * (tg + ts);
            ta[0] = SCL(SC_TA); ta[1] = SCL(SC_TA + 1); ta[2] = SCL(SC_TA + 2);
        }
        const T tac = c < 3 ? (c == 0 ? ta[0] : (c == 1 ? ta[1] : ta[2])) : T(0);
        // cost variants: off-diagonal terminal weights (Qf, S) and the trapezoid term 0.5 dt xd' Q xd of the final state (x-x, x-dt, gradients)
        T xdT[3] = {T(0), T(0), T(0)}, qT[3] = {T(0), T(0), T(0)};       // qT = Q xd_T (full) when the trapezoid term exists
        if (costx()) { xd_final(T(0), xdT); if (P.trapz) { offmul(P.Qo, xdT, qT); for (int i = 0; i < 3; ++i) qT[i] += P.Q[i] * xdT[i]; } }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (fx(i)) V[i] = c == 9 + i ? T(1) : T(0);
            else {
                T pii = delta, pi_ = T(0);
                if (hasqf()) {
                    T xd = F(L.X, i, n - 1) - xf[i];
                    if (i == 2) xd = normalize_theta(xd);
                    pii += T(2) * P.Qf[i]; pi_ = T(2) * P.Qf[i] * xd;
                }
                if (ball()) { pii += T(2) * ty * P.ball_S[i]; pi_ += ta[i] * tyb; }
                V[i] = c == i ? pii : (c == 8 ? pi_ : T(0));
                if (ball() && c < 3) V[i] += tsig * ta[i] * tac;       // a of a fixed component is 0
                if (costx()) {
                    if (c < 3 && !fx(c)) {         // Hessian entry (i, c) over the free final components
                        const int oi = i + c - 1;  // (0,1) -> 0, (0,2) -> 1, (1,2) -> 2
                        if (c != i) { if (hasqf()) V[i] += T(2) * P.Qfo[oi]; if (ball()) V[i] += T(2) * ty * P.So[oi]; if (P.trapz) V[i] += d * P.Qo[oi]; }
                        else if (P.trapz) V[i] += d * P.Q[i];
                    }
                    if (c == 8) {
                        T y3[3];
                        if (hasqf()) { offmul(P.Qfo, xdT, y3); V[i] += T(2) * y3[i]; }
                        if (P.trapz) V[i] += d * qT[i];
                    }
                    if (c == 5 && P.trapz) V[i] += qT[i];
                }
            }
        }
        {
            const bool t3 = c == 3 || c == 5 || c == 8, t4 = c == 4 || c == 5 || c == 8, t5 = c == 3 || c == 4 || c == 5 || c == 8;
            V[3] = t3 ? a3 : T(0); V[4] = t4 ? a4 : T(0); V[5] = t5 ? a5 : T(0);
            if (costx() && P.trapz) {
                if (c < 3 && !fx(c)) V[5] += c == 0 ? qT[0] : (c == 1 ? qT[1] : qT[2]);
                if (c == 8) V[5] += T(0.5) * (xdT[0] * qT[0] + xdT[1] * qT[1] + xdT[2] * qT[2]);
            }
        }
    }

    __device__ __forceinline__ T fast_rcp(double x) const {
        double r = __builtin_amdgcn_rcp(x);
        r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
        r = __builtin_fma(__builtin_fma(-x, r, 1.0), r, r);
        return r;
    }
    __device__ __forceinline__ T fast_rcp(float x) const { return 1.0f / x; }
    __device__ __forceinline__ static int sign_word(double x) { return __double2hiint(x); }      // the word that holds the sign bit
    __device__ __forceinline__ static int sign_word(float x) { return __float_as_int(x); }

    // ---- register-resident backward sweep: lane c (0..11 of every 16-lane DPP row) owns COLUMN c of the value block
    //      [P | . . | p | S] (6x12) and of Hhat (8x12).  Entries of other columns are fetched with the DP-ALU DPP broadcast
    //      (v_fmac_f64_dpp ... row_newbcast:m), so a stage is ~90 fp64 VALU instructions and NO LDS hand-off; the stage
    //      record (3 coefficients + 8 cost entries per lane) is prefetched from LDS one stage ahead.
    //        T1 = V+ Ghat           T1[i][c] = sum_{m<3} V+[i][m] G[m][c] + V+[i][x(c)]
    //        Hhat = Ghat' T1 + cost Hhat[r][c] = sum_{m<3} G[m][r] T1[m][c] + T1[x(r)][c] + A[r][c]
    //        V = Hhat_xx - Hhat_xu R^-1 Hhat_ux   (R = Hhat[6:8][6:8], closed-form inverse; symmetry: Hhat[i][6] = lane i's Hhat[6][.])
    //      Cost model on gfx950 with one wave per SIMD (scripts/ubench/issue_rate.hip): EVERY instruction, VALU or not, costs
    //      ~4.5 cycles of issue, an LDS write->read hand-off ~115 cycles, s_nop 1 ~8 cycles: the sweep is written to minimise
    //      the instruction count.  The DPP arithmetic lives in four inline-asm blocks per stage (mpc_dpp_blocks.inc, generated
    //      by scripts/gen_dpp_blocks.py): the compiler cannot see a DPP operand inside inline asm and therefore does not insert
    //      the 2 wait states of the VALU-write -> DPP-read hazard; each block opens with s_nop 1 and orders its own instructions.
    __device__ __forceinline__ bool backward_dpp(T delta, T dc, T& dd_out, T nu_out[3]) const {
        MPC_PHASE_LANE
        MPC_LAP_BEGIN(t_lap)
        MPC_MARK("BWD_SETUP_BEGIN");
        const int n = L.n;
        const T d = SCL(SC_D);
        const int ZC = W_ZC();                          // constants 0 0 0 0 1 0 0 0 (written once per solve): (0,0,0) @0, (0,1,0) @3, (1,0,0) @4
        const int c = lane & 15;                    // column owned by this lane (12..15 idle: they carry zeros)
        const bool act = c < 12;
        // coefficient triple of column c: three consecutive words, running pointer (stride 0 for the constant triples).
        // kind: 0 (0,0,0)  1 (1,0,0)  2 (0,1,0)  3 (a0,a1,1)  4 f  5 Bx[:,0]  6 Bx[:,1]  7 c_k   -- columns 0..11, 3 bits each
        constexpr unsigned long long KIND = 1ull | (2ull << 3) | (3ull << 6) | (4ull << 15) | (5ull << 18) | (6ull << 21) | (7ull << 24);
        const int kind = act ? (int)((KIND >> (3 * c)) & 7) : 0;
        // (GS: everything the loop reads is an ENTRY of the stage's tile slot -- the constant triples too --, so a lane's "pointers" are the byte offsets of its entries inside a slot
        //  and do not move; what moves is the wave-uniform offset of the stage's slot, kb in load_stage, which the compiler folds into the scalar base of the loads)
        const int gb = kind < 3 ? ZT_W(kind) : (kind < 7 ? STG_W(3 * (kind - 3)) : CC_W(0));
        const int gsw = kind < 3 ? 0 : (kind < 7 ? STG_S : CC_S);
        const int gs = sw_step(gsw);
        const int ge = kind < 3 ? zt_entry(kind) : (kind < 7 ? 3 * (kind - 3) : TE_CC);      // first entry of the triple in the tile slot
        SwCRef gp;
        if constexpr (GS) gp = (unsigned)(4 * ge) * (unsigned)sizeof(T); else gp = sw(gb + (n - 2) * gsw);
        SwCRef ap[8];
        int as_[8];
        int kl = n - 2;                                 // GS: the stage the next load_stage() reads
        constexpr unsigned long long rows[8] = {stage_add_row(0, EXT), stage_add_row(1, EXT), stage_add_row(2, EXT), stage_add_row(3, EXT),
                                                stage_add_row(4, EXT), stage_add_row(5, EXT), stage_add_row(6, EXT), stage_add_row(7, EXT)};
        const int sh = act ? 5 * c : 60;               // idle lanes: shift the row word out (slot -1)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int slot1 = (int)((rows[r] >> sh) & 31);       // slot + 1, 0 = structurally zero
            as_[r] = sw_step(slot1 ? STG_S : 0);
            if constexpr (GS) ap[r] = (unsigned)(4 * (slot1 ? RA - 1 + slot1 : TE_Z)) * (unsigned)sizeof(T);
            else ap[r] = sw(slot1 ? STG_W(RA - 1 + slot1) + (n - 2) * STG_S : ZC);
        }
        const T ec = (c == 5 || (c >= 8 && c < 12)) ? T(1) : T(0);       // own column enters T1 (dt, p, S)
        const T E3 = c == 6 ? T(1) : T(0), E4 = c == 7 ? T(1) : T(0);     // the u columns pick up the u_prev columns of V+
        const T dA0 = c == 0 ? delta : T(0), dA1 = c == 1 ? delta : T(0), dA2 = c == 2 ? delta : T(0);   // x diagonal, k >= 1
        const T dA6 = c == 6 ? delta : T(0), dA7 = c == 7 ? delta : T(0);                                 // u diagonal
        // negated gains go to GAIN as [nK0 (cols 0..5) | nkappa0 | nKnu0 (3 of 5) | nK1 ... ] : g1 = g0 + NGH; idle lanes hit a dummy pair
        const bool wrG = lane < 12 && c != 6 && c != 7;
        const int g0 = c < 6 ? c : (c == 8 ? 6 : 7 + (c - 9));
        SwRef kp = sw(wrG ? GAIN_W(g0) + (n - 2) * GAIN_S : GAIN_DUMMY_W());      // idle lanes: a dummy pair
        const int ks = sw_step(wrG ? GAIN_S : 0);
        // ---- terminal value function, straight into the owning lanes' registers (rows 3..5: the u_prev / dt entries of the
        //      final rate rows = the A slots (i, c) of stage n-1 for c in {3, 4, 5, 8})
        T V[6];
        if constexpr (GS) { const unsigned kbT = (unsigned)tile_k(n - 1) * (unsigned)sizeof(T); terminal_value(V, c, delta, d, gld(kbT, ap[3]), gld(kbT, ap[4]), gld(kbT, ap[5])); }
        else terminal_value(V, c, delta, d, sw_ld_at(ap[3], as_[3]), sw_ld_at(ap[4], as_[4]), sw_ld_at(ap[5], as_[5]));       // rows 3..5: one stage above the running pointers
        T add_dd0 = T(0), add_qd0 = T(0);
        if (mintime()) add_qd0 += T(n - 1);
        if (dtf()) {
            const T dl = d - P.dt_lb, du = P.dt_ub - d;
            const T idl = fast_rcp(dl), idu = fast_rcp(du);
            add_dd0 = SCL(SC_PDL) * idl + SCL(SC_PDU) * idu + delta;
            add_qd0 += mu * idu - mu * idl;
        }
        const T s05 = c == 5 ? add_dd0 : (c == 8 ? add_qd0 : T(0));       // stage-0 extras of row 5
        T om = T(0), wn[3] = {T(0), T(0), T(0)};
        T worst = T(1);                                                   // min over the stages of |det R| - 1e-14 * scale
        int negc = 0;                                                     // negative eigenvalues of the control pivots = sign changes of (1, R00, det R), summed over the stages
        auto load_stage = [&](T (&g)[3], T (&a)[8]) {                     // reads the stage the running pointers are at, then steps them
            if constexpr (GS) {
                const unsigned kb = (unsigned)tile_k(kl) * (unsigned)sizeof(T);
                g[0] = gld(kb, gp); g[1] = gld(kb, gp + 4u * (unsigned)sizeof(T)); g[2] = gld(kb, gp + 8u * (unsigned)sizeof(T));
#pragma unroll
                for (int r = 0; r < 8; ++r) a[r] = gld(kb, ap[r]);
                --kl;
            } else {
                g[0] = sw_ld(gp, 0); g[1] = sw_ld(gp, 1); g[2] = sw_ld(gp, 2);
                gp -= gs;
#pragma unroll
                for (int r = 0; r < 8; ++r) { a[r] = sw_ld(ap[r]); ap[r] -= as_[r]; }
            }
        };
        auto stage = [&](T dk0, T dk1, T dk2, T s5, T (&G)[3], T (&A)[8], T (&Gn)[3], T (&An)[8]) {
            load_stage(Gn, An);                                           // prefetch of the next stage (k - 1)
            // ---- T1 = V+ Ghat (own column, then the five broadcast columns) and
            //      omega[b] += S+[0][b] c0 + S+[1][b] c1 + S+[2][b] c2  (lanes 9..11; c_k is lane 8's coefficient triple)
            T t[6];
            MPC_DPP_BLOCK_T1
            // ---- Hhat = Ghat' T1 + cost entries (+ regularisation on this lane's diagonal entry)
            T h[8];
            h[0] = (A[0] + dk0) + t[0]; h[1] = (A[1] + dk1) + t[1]; h[2] = (A[2] + dk2) + t[2];
            h[3] = A[3]; h[4] = A[4];
            h[5] = (A[5] + s5) + t[5];
            h[6] = (A[6] + dA6) + t[3]; h[7] = (A[7] + dA7) + t[4];
            MPC_DPP_BLOCK_H
            // ---- Schur complement on the control block
            T R00, R01, R11;
            MPC_DPP_BLOCK_R
            const T r2 = R01 * R01;
            const T det = R00 * R11 - r2;
            worst = t_fmin(worst, t_abs(det) - T(1e-14) * (t_abs(R00 * R11) + r2));   // a NaN determinant poisons V and is caught by the root solve
            { const int s0 = sign_word(R00), s1 = sign_word(det); negc += (int)((unsigned)s0 >> 31) + (int)((unsigned)(s0 ^ s1) >> 31); }
            const T nid = -fast_rcp(det);
            const T nRi00 = R11 * nid, Ri01 = -(R01 * nid), nRi11 = R00 * nid;  // -R^-1 = [nRi00 Ri01; Ri01 nRi11]
            const T nK0 = nRi00 * h[6] + Ri01 * h[7], nK1 = Ri01 * h[6] + nRi11 * h[7];
            sw_st(kp, 0, nK0); sw_st(kp, NGH, nK1);
            kp -= ks;
            // W[a][b] -= Su[:,a]' Knu[:,b] in lane 9+b, omega[a] -= Su[:,a]' kappa in lane 8 (Su[j][a] = Hhat[6+j][9+a]);
            // V = Hhat_xx + Hhat_xu nK   (row i of Hhat[:,6:8] = lane i's Hhat[6:8][.])
            V[0] = h[0]; V[1] = h[1]; V[2] = h[2]; V[3] = h[3]; V[4] = h[4]; V[5] = h[5];
            MPC_DPP_BLOCK_V
        };
        T Ga[3], Aa[8], Gb[3], Ab[8];
        MPC_LAP(bwd_setup, t_lap);
        load_stage(Ga, Aa);
        int k = n - 2;
        if constexpr (GS && !(OBST && MODEL == MODEL_KINEMATIC_BICYCLE)) {      // (that one kernel has no registers left for the third set)
            // records from global memory: TWO stages ahead (three register sets in rotation) -- a stage is ~360 cycles, the first touch of a new cache line of the rows
            // (every 16 stages, all rows at once) an L2 / Infinity-Cache access of up to ~1000; the loads run two stages past stage 0 (into the guard tile)
            T Gc[3], Ac[8];
            load_stage(Gb, Ab);
            for (; k >= 3; k -= 3) {
                stage(dA0, dA1, dA2, T(0), Ga, Aa, Gc, Ac);
                stage(dA0, dA1, dA2, T(0), Gb, Ab, Ga, Aa);
                stage(dA0, dA1, dA2, T(0), Gc, Ac, Gb, Ab);
            }
            if (k == 2) { stage(dA0, dA1, dA2, T(0), Ga, Aa, Gc, Ac); stage(dA0, dA1, dA2, T(0), Gb, Ab, Ga, Aa); stage(T(0), T(0), T(0), s05, Gc, Ac, Gb, Ab); }
            else if (k == 1) { stage(dA0, dA1, dA2, T(0), Ga, Aa, Gc, Ac); stage(T(0), T(0), T(0), s05, Gb, Ab, Ga, Aa); }
            else stage(T(0), T(0), T(0), s05, Ga, Aa, Gc, Ac);
        } else {
        for (; k >= 2; k -= 2) {        // stages k and k-1 (both >= 1): the two register sets swap roles, no copies
            MPC_MARK("MAT_LOOP_BEGIN");
            stage(dA0, dA1, dA2, T(0), Ga, Aa, Gb, Ab);
            stage(dA0, dA1, dA2, T(0), Gb, Ab, Ga, Aa);
            MPC_MARK("MAT_LOOP_END");
        }
        if (k == 1) { stage(dA0, dA1, dA2, T(0), Ga, Aa, Gb, Ab); stage(T(0), T(0), T(0), s05, Gb, Ab, Ga, Aa); }
        else stage(T(0), T(0), T(0), s05, Ga, Aa, Gb, Ab);
        }
        MPC_LAP(bwd_loop, t_lap);
        // row 5 of the value block, omega and the W / omega corrections are gathered with v_readlane (no LDS round trip)
        if (!(rd_lane(worst, 0) > T(0))) return false;
        RicState<T> Vr;
        Vr.neg = __builtin_amdgcn_readlane(negc, 0);
        Vr.P[5][5] = rd_lane(V[5], 5);
        Vr.p[5] = rd_lane(V[5], 8);
        Vr.S[5][0] = rd_lane(V[5], 9); Vr.S[5][1] = rd_lane(V[5], 10); Vr.S[5][2] = rd_lane(V[5], 11);
        Vr.om[0] = rd_lane(om, 9) + rd_lane(wn[0], 8);
        Vr.om[1] = rd_lane(om, 10) + rd_lane(wn[1], 8);
        Vr.om[2] = rd_lane(om, 11) + rd_lane(wn[2], 8);
        {
            // W[a][b] partial lives in lane 9+b as wn[a]; symmetrise; the fixed components carry -delta_c on the diagonal
            const T w00 = rd_lane(wn[0], 9), w01 = rd_lane(wn[0], 10), w02 = rd_lane(wn[0], 11);
            const T w10 = rd_lane(wn[1], 9), w11 = rd_lane(wn[1], 10), w12 = rd_lane(wn[1], 11);
            const T w20 = rd_lane(wn[2], 9), w21 = rd_lane(wn[2], 10), w22 = rd_lane(wn[2], 11);
            Vr.W[0][0] = w00 - (fx(0) ? dc : T(0)); Vr.W[1][1] = w11 - (fx(1) ? dc : T(0)); Vr.W[2][2] = w22 - (fx(2) ? dc : T(0));
            Vr.W[0][1] = Vr.W[1][0] = T(0.5) * (w01 + w10);
            Vr.W[0][2] = Vr.W[2][0] = T(0.5) * (w02 + w20);
            Vr.W[1][2] = Vr.W[2][1] = T(0.5) * (w12 + w21);
        }
        bool okr;      // the (dt, nu) root system (mpc_core.hpp): with the shape known, the form without identity rows and selects
        if constexpr (SHAPE != 0) okr = riccati_root_uniform<((SHAPE >> 3) & 1) != 0, SHAPE & 7>(Vr, dd_out, nu_out) > 0;      // (the same system with its exchanges as uniform branches)
        else okr = riccati_root(Vr, P, dd_out, nu_out) > 0;
        MPC_DBG_ROOT("serial", okr, rd_lane(worst, 0))
        return okr;
    }

    // inclusive suffix sum over the wave (lane i gets sum_{j >= i} v_j): Hillis-Steele inside each 16-lane row with DPP row
    // shifts (row_shl:n = 0x100 + n, out-of-row sources read as 0), then the totals of the higher rows via v_readlane.
    // ~27 VALU instructions and no LDS traffic (the ds_bpermute version was 12 LDS round trips).
    template <int CTRL> __device__ __forceinline__ static double dpp_shl0(double v) {
        int lo = __double2loint(v), hi = __double2hiint(v);
        lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
        hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
        return __hiloint2double(hi, lo);
    }
    template <int CTRL> __device__ __forceinline__ static float dpp_shl0(float v) {
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
    }
    __device__ __forceinline__ T wave_suffix_sum(T v) const {
        v += dpp_shl0<0x101>(v);
        v += dpp_shl0<0x102>(v);
        v += dpp_shl0<0x104>(v);
        v += dpp_shl0<0x108>(v);
        const T r1 = rd_lane(v, 16), r2 = rd_lane(v, 32), r3 = rd_lane(v, 48);
        const T c2 = r3, c1 = r2 + r3, c0 = r1 + c1;
        const int row = lane >> 4;
        return v + (row == 0 ? c0 : (row == 1 ? c1 : (row == 2 ? c2 : T(0))));
    }

    // state recurrence (one component per lane, DPP broadcasts, prefetched coefficients) then multipliers by lane-parallel suffix scans
    __device__ __forceinline__ void forward_states(T dd, const T nu[3], T delta) const {
        MPC_PHASE_LANE
        const int n = L.n;
        // ---- lane-parallel: fold nu and dd into the affine terms so that the serial loop only carries (x, u_prev)
        //      kappa^ = kappa + Knu nu + K[:,5] dd  (stored over kappa),  c^ = c + f dd  (stored in LAMN, rewritten below)
        //      (gains are stored negated: [nK0 (6) | nkappa0 | nKnu0 (3) | nK1 (6) | nkappa1 | nKnu1 (3)])
        for (int k = lane; k < n - 1; k += kWave) {
            // (GS: kappa^ goes to DU -- the loop reads kappa^_k three stages before it writes du_k into the same word -- and c^ to LAMN as in the LDS form: no global store in
            //  this pass, so the barrier behind it does not wait for a trip to memory, and the loop's constant term comes from LDS.  Measured, config 5 in fp64 at B = 1024:
            //  6.04 -> 5.88 ms)
            for (int a = 0; a < 2; ++a) {
                const T kh = G_(NGH * a + 6, k) + (G_(NGH * a + 7, k) * nu[0] + G_(NGH * a + 8, k) * nu[1] + G_(NGH * a + 9, k) * nu[2] + G_(NGH * a + 5, k) * dd);
                if constexpr (GS) F(L.DU, a, k) = kh; else G_(NGH * a + 6, k) = kh;
            }
            for (int i = 0; i < 3; ++i) CH_(i, k) = C_(i, k) + S_(3 + i, k) * dd;
        }
        if (lane == 0) { SCL(SC_DD) = dd; F(L.DX, 0, 0) = T(0); F(L.DX, 1, 0) = T(0); F(L.DX, 2, 0) = T(0); }
        sync();
        // ---- serial recurrence, one COMPONENT per lane: lanes 0..2 carry dx_k, lanes 3,4 carry du_{k-1}; a stage is
        //        s  = cst + sum_j q_j * xi[j]        lanes 3,4: du_k = nkappa^ + nK xi ;  lanes 0..2: dx_k[c] + a_c dx_k[2] + c^_k[c]
        //        xn = s + b0 * s[3] + b1 * s[4]      lanes 0..2: + Bx[c][:] du_k
        //      i.e. 7 DPP-broadcast FMAs; the 8 per-lane coefficients are prefetched one stage ahead through running pointers.
        {
            const int c = lane & 15;
            const int ZC = W_ZC();
            int qw[8], qs[8];        // word index and stride of: cst, q0..q4, b0, b1
#pragma unroll
            for (int j = 0; j < 8; ++j) { qw[j] = ZC; qs[j] = 0; }
            if (c < 3) {
                if constexpr (GS) {      // (entries of the stages' tile slots: one word from stage to stage inside a tile, tile_jump more across a tile boundary -- load_q)
                    const int t0 = tile_k(0);
                    qw[1 + c] = ZC + 4;
                    if (c < 2) { qw[3] = t0 + 4 * c; qs[3] = 1; }
                    qw[6] = t0 + 4 * (6 + c); qs[6] = 1;
                    qw[7] = t0 + 4 * (9 + c); qs[7] = 1;
                } else {
                qw[0] = CH_W(c); qs[0] = 1;
                qw[1 + c] = ZC + 4;                                          // xi[c] itself
                if (c < 2) { qw[3] = STG_W(c); qs[3] = STG_S; }              // a_c * xi[2]
                qw[6] = STG_W(6 + c); qs[6] = STG_S;
                qw[7] = STG_W(9 + c); qs[7] = STG_S;
                }
            } else if (c < 5) {
                const int a = c - 3;
                qw[0] = GAIN_W(NGH * a + 6); qs[0] = GAIN_S;
#pragma unroll
                for (int j = 0; j < 5; ++j) { qw[1 + j] = GAIN_W(NGH * a + j); qs[1 + j] = GAIN_S; }
            }
            SwCRef qp[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { qp[j] = sw(qw[j]); qs[j] = sw_step(qs[j]); }
            // where the result goes: dx_{k+1}[c] / du_k[c-3]; idle lanes write a dummy word of the sweep scratch
            LdsT* op = lds(c < 3 ? L.DX + c * L.NS + 1 : (c < 5 ? L.DU + (c - 3) * L.NS : L.VP + 12));
            const int os = c < 5 ? 1 : 0;
            // GS: what a tile pointer jumps across a tile boundary (on top of its one word), per lane: the pointers 0, 6, 7 of the lanes 0..2 and pointer 3 of the lanes 0, 1 are tile pointers
            const unsigned tjump = (unsigned)(4 * TNT - 4) * (unsigned)sizeof(T);
            const unsigned jl = (GS && c < 3) ? tjump : 0u, jl3 = (GS && c < 2) ? tjump : 0u;
            int kl = 0;                                                   // GS: the stage the next load_q() reads (wave-uniform)
            // GS: the constant term of a stage comes from LDS -- c^_k (LAMN) for the lanes 0..2, kappa^_k (DU) for the lanes 3, 4, a zero for the rest
            const LdsT* q0p = lds(c < 3 ? L.LAMN + c * L.NS : (c < 5 ? L.DU + (c - 3) * L.NS : L.ZC));
            const int q0s = c < 5 ? 1 : 0;
            auto load_q = [&](T (&q)[8]) {
                if constexpr (GS) {
                    q[0] = *q0p; q0p += q0s;
#pragma unroll
                    for (int j = 1; j < 8; ++j) { q[j] = sw_ld(qp[j]); qp[j] += qs[j]; }
                    if (((kl + GlobalStage::kGuard) & 3) == 3) { qp[3] += jl3; qp[6] += jl; qp[7] += jl; }
                    ++kl;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { q[j] = sw_ld(qp[j]); qp[j] += qs[j]; }
                }
            };
            T xi = T(0);
            auto stage = [&](T (&q)[8], T (&qn)[8]) {
                load_q(qn);
                T s = q[0], s2 = T(0), xn;
                MPC_DPP_BLOCK_FWD
                *op = xn; op += os;
                xi = xn;
            };
            MPC_LAP_BEGIN(t_lap)
            if constexpr (GS) {
                // coefficients from global memory: three stages ahead instead of one (a stage is ~250 cycles of work, an L2 hit under load several times that: measured
                // 690 cycles per stage with the one-stage prefetch of the LDS form, profiles/r05_phase_profile_gs.log); four register sets in rotation
                auto comp = [&](T (&q)[8]) {
                    T s = q[0], s2 = T(0), xn;
                    MPC_DPP_BLOCK_FWD
                    *op = xn; op += os;
                    xi = xn;
                };
                T q0[8], q1[8], q2[8], q3[8];
                load_q(q0); load_q(q1); load_q(q2);
                const int cnt = n - 1;
                int k = 0;
                for (; k + 4 <= cnt; k += 4) { load_q(q3); comp(q0); load_q(q0); comp(q1); load_q(q1); comp(q2); load_q(q2); comp(q3); }
                if (k < cnt) comp(q0);
                if (k + 1 < cnt) comp(q1);
                if (k + 2 < cnt) comp(q2);
            } else {
            T qa[8], qb[8];
            load_q(qa);
            int k = 0;
            for (; k + 1 < n - 1; k += 2) {
                MPC_MARK("FWD_LOOP_BEGIN");
                stage(qa, qb); stage(qb, qa);
                MPC_MARK("FWD_LOOP_END");
            }
            if (k < n - 1) stage(qa, qb);
            }
            MPC_LAP(fwd_loop, t_lap);
        }
        multipliers(dd, nu, delta);
    }

    // multipliers of the collocation rows for ALL stages at once, from the primal step in DX / DU (lane-parallel suffix scans); the tail of both
    // forward passes (serial and partitioned)
    __device__ __forceinline__ void multipliers(T dd, const T nu[3], T delta) const {
        MPC_PHASE_LANE
        const int n = L.n;
        MPC_PROF_SCOPE_MULT
        sync();
        const T xi[3] = {F(L.DX, 0, n - 1), F(L.DX, 1, n - 1), F(L.DX, 2, n - 1)};
        // ---- multipliers: lam+_{k-1} = lam+_k + t_k + e_theta (a0_k lam+_k[0] + a1_k lam+_k[1]),  k = n-2 .. 1,
        //      lam+_{n-2} from the terminal condition.  Components 0,1 are plain suffix sums, component 2 a second one.
        T lp[3];
        for (int i = 0; i < 3; ++i) {
            if (fx(i)) lp[i] = nu[i];
            else {
                T g = delta * xi[i];
                if (hasqf()) {
                    T xd = F(L.X, i, n - 1) - xf[i];
                    if (i == 2) xd = normalize_theta(xd);
                    g += T(2) * P.Qf[i] * (xi[i] + xd);
                }
                if (ball()) {
                    const T ts = SCL(SC_TS), ty = SCL(SC_TY), sig = ty / ts;
                    T adx = T(0);
                    for (int j = 0; j < 3; ++j) if (!fx(j)) adx += SCL(SC_TA + j) * xi[j];
                    g += SCL(SC_TA + i) * (sig * adx + mu / ts + sig * (SCL(SC_TG) + ts)) + T(2) * ty * P.ball_S[i] * xi[i];
                }
                if (costx()) {       // the rows of the terminal block that the variants add: (xi + xd) through the off-diagonal / trapezoid Hessian, dt coupling
                    T xdT[3], z[3], y3[3];
                    xd_final(T(0), xdT);
                    const T xif[3] = {fx(0) ? T(0) : xi[0], fx(1) ? T(0) : xi[1], fx(2) ? T(0) : xi[2]};
                    for (int j = 0; j < 3; ++j) z[j] = xif[j] + xdT[j];
                    if (hasqf()) { offmul(P.Qfo, z, y3); g += T(2) * y3[i]; }
                    if (ball()) { offmul(P.So, xif, y3); g += T(2) * SCL(SC_TY) * y3[i]; }
                    if (P.trapz) {
                        offmul(P.Qo, z, y3);
                        g += SCL(SC_D) * (P.Q[i] * z[i] + y3[i]);
                        offmul(P.Qo, xdT, y3);
                        g += (P.Q[i] * xdT[i] + y3[i]) * SCL(SC_DD);
                    }
                }
                lp[i] = g;
            }
        }
        sync();
        T carry[3] = {T(0), T(0), T(0)};                 // sum of t_m over the chunks already processed (m larger)
        const int last = n - 2;                          // stages m = 1 .. n-2 carry a term t_m
        for (int base = ((last) / kWave) * kWave; base >= 0; base -= kWave) {
            const int m = base + lane;
            const bool act = m >= 1 && m <= last;
            T t0 = T(0), t1 = T(0), t2 = T(0), a0 = T(0), a1 = T(0);
            if (act) {
                const T dx0 = F(L.DX, 0, m), dx1 = F(L.DX, 1, m), dx2 = F(L.DX, 2, m);
                const T duv = F(L.DU, 0, m), duw = F(L.DU, 1, m);
                t0 = delta * dx0 + S_(RA + A00, m) * dx0 + S_(RA + A01, m) * dx1 + S_(RA + A08, m);
                t1 = delta * dx1 + S_(RA + A01, m) * dx0 + S_(RA + A11, m) * dx1 + S_(RA + A18, m);
                t2 = delta * dx2 + S_(RA + A22, m) * dx2 + S_(RA + A26, m) * duv + S_(RA + A27, m) * duw + S_(RA + A25, m) * dd + S_(RA + A28, m);
                if (intf() || dynobs()) { t0 += S_(RA + A05, m) * dd; t1 += S_(RA + A15, m) * dd; }
                if (fpline() || costx()) {        // position-heading coupling of the clearance rows / of a full state weight matrix
                    const T c02 = S_(RA + A02, m), c12 = S_(RA + A12, m);
                    t0 += c02 * dx2; t1 += c12 * dx2; t2 += c02 * dx0 + c12 * dx1;
                }
                a0 = S_(0, m); a1 = S_(1, m);
            }
            const T s0 = wave_suffix_sum(t0) + carry[0];     // sum_{m' >= m} t_m'[0]
            const T s1 = wave_suffix_sum(t1) + carry[1];
            // lam+_m[0..1] = lp + sum_{m' >= m+1} t_m'  = lp + s - t_m
            const T l0 = lp[0] + s0 - t0, l1 = lp[1] + s1 - t1;
            const T t2f = act ? t2 + a0 * l0 + a1 * l1 : T(0);
            const T s2 = wave_suffix_sum(t2f) + carry[2];
            if (act) {       // lam+_{m-1} = lp + sum_{m' >= m} t_m'
                F(L.LAMN, 0, m - 1) = lp[0] + s0; F(L.LAMN, 1, m - 1) = lp[1] + s1; F(L.LAMN, 2, m - 1) = lp[2] + s2;
            }
            carry[0] = lane_bcast(s0, 0); carry[1] = lane_bcast(s1, 0); carry[2] = lane_bcast(s2, 0);
        }
        if (lane == 0) { F(L.LAMN, 0, last) = lp[0]; F(L.LAMN, 1, last) = lp[1]; F(L.LAMN, 2, last) = lp[2]; }
        }

