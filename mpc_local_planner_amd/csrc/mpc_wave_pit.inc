// mpc_wave_pit.inc: the partitioned (parallel-in-time) sweeps: four time segments in the four DPP rows, combine steps, inertia counts -- part of struct IpmWave (mpc_wave.hpp includes this file inside the struct's body; not a translation unit of its own).

    // ================================================================ partitioned ("parallel-in-time") sweeps
    // The serial sweeps above use 12 of 64 lanes and repeat the same arithmetic in all four 16-lane DPP rows.  Here the four rows work on four TIME
    // SEGMENTS of the horizon at once (tests/test_pit_math.py holds the algebra against a dense KKT solve):
    //   backward  row s < 3 sweeps its segment [s Lm, (s+1) Lm) from the identity border (P, p, S, W, om) = (0, 0, I, 0, 0): that yields the segment's
    //             scattering element, lam_a = P xi_a + S lam_b + p, xi_b = S' xi_a + W lam_b + om (the border multiplier is the costate at the segment's
    //             end: five columns, lanes 9..13; the dt column, lane 14, stays e_5); row 3 sweeps the last segment from the terminal value function, after
    //             the N mod 4 leftover stages have been swept by all rows together.  Same stage code as the serial sweep (only the V block differs).
    //   combine   right to left, three times: element + value function at its end -> value function at its start (combine()): every row does the same
    //             arithmetic; the element travels from its row to all rows through one LDS tile (in the step arrays, which are free during a factorisation)
    //   root      as in the serial sweep, from the value function at stage 0
    //   forward   boundary states / costates from the combine's maps (wave-uniform), gains folded per stage with the costate of the stage's own segment,
    //             then every row runs the state recurrence of its segment; the leftover stages follow in row 3
    // What the backward half leaves for the forward half, per mid-segment s: the eliminated tile [X | y | Z] (xi_{b_{s+1}} = X xi_{b_s} + y + Z nu) and the
    // value function [P+ | p+ | S+] at the boundary b_{s+1}, rows 0..4 x 10 columns each, in LDS words that are free during a factorisation: s = 2 in
    // LAMN, s = 1 in the trig cache (read by kkt_pass, rewritten by every line-search trial), s = 0 in DX (over the hand-off tile, dead by then).
    __device__ __forceinline__ int pit_tile(int s) const { return s == 2 ? L.LAMN : (s == 1 ? L.TRIG : L.DX); }
    // Per-lane constants of a combine step, branch-free integer arithmetic (computed once per factorisation for both lane-set variants).
    // Lane sets: A = lanes 0..5, B = lanes 6, 7, 12..15; lp_a: the value function's P+ columns sit in A and the result's in B, else the other way round.
    struct CombLane {
        int bb;        // base tile: S' in the result's lanes, om in lane 8, the identity in the value function's lanes, zeros elsewhere (row i = word i from here)
        int pb;        // the element's own P in the result's lanes, p in lane 8 (row i = 16 i words from here); the other lanes are masked by keep_p
        int sx, sp;    // slot (0..9, -1 = none) of this lane in a saved tile whose block sits in the result's / the value function's lane set
        T sig;         // -1 in the value function's lanes (M = I - W P+), +1 elsewhere
        T keep;        // 1 in the result's lanes and in lanes 8..11
        T keep_p;      // 1 in the result's lanes and in lane 8
    };
    __device__ __forceinline__ CombLane comb_lane(int c, bool lp_a, int TB) const {
        const int in_a = c < 6 ? 1 : 0, in_b = ((c == 6) | (c == 7) | (c >= 12)) ? 1 : 0, is8 = c == 8 ? 1 : 0, is_s = ((c >= 9) & (c < 12)) ? 1 : 0;
        const int qa = c, qb = c < 8 ? c - 6 : c - 10;                     // position inside A / B (meaningful where in_a / in_b)
        const int in_p = lp_a ? in_a : in_b, in_x = lp_a ? in_b : in_a, pp = lp_a ? qa : qb, px = lp_a ? qb : qa;
        CombLane r;
        r.bb = in_x * (TB + 16 * px + 9) + is8 * (TB + 176 + 9) + in_p * (L.ZI + 6 - pp) + (1 - in_x - is8 - in_p) * L.ZI;
        r.pb = TB + in_x * px + is8 * 8 + (1 - in_x - is8) * 15;
        const int tail = (is8 | is_s) * (c - 2) - (1 - (is8 | is_s));     // lanes 8..11 -> slots 6..9, else -1
        r.sx = in_x * px + (1 - in_x) * tail;
        r.sp = in_p * pp + (1 - in_p) * tail;
        r.sig = T(1 - 2 * in_p);
        r.keep = T(in_x | is8 | is_s);
        r.keep_p = T(in_x | is8);
        return r;
    }
    // column c of a partitioned stage: the kind of its coefficient triple (0 1 2 constant triples, 3..6 entries 0 3 6 9 of the stage record, 7 c_k; see backward_pit) and the
    // 5-bit slot of its entry in row r of the stage's cost block (0 = none)
    __device__ __forceinline__ static int pit_kind(int c) {
        constexpr unsigned long long KIND = 1ull | (2ull << 3) | (3ull << 6) | (4ull << 15) | (5ull << 18) | (6ull << 21) | (7ull << 24);
        return c < 12 ? (int)((KIND >> (3 * c)) & 7) : 0;
    }
    __device__ __forceinline__ static int pit_slot(int r, int c) {
        constexpr unsigned long long rows[8] = {stage_add_row(0, EXT), stage_add_row(1, EXT), stage_add_row(2, EXT), stage_add_row(3, EXT),
                                                stage_add_row(4, EXT), stage_add_row(5, EXT), stage_add_row(6, EXT), stage_add_row(7, EXT)};
        return (int)((rows[r] >> (c < 12 ? 5 * c : 60)) & 31);
    }
    // r13, fixed layout (NSC != 0): what a lane's place in the wave decides of the partitioned sweeps -- where its streams start, how far they step, its records of the combine
    // steps -- is the same for every factorisation of a solve.  It is worked out ONCE, in front of the interior-point loop (pit_lane_consts(), called by solve()), packed into
    // 30 words that stay in registers, and unpacked with an AND or a shift where a half uses it; the kernels with a run-time layout have no register to spare for that and
    // work it out per factorisation as before (there PitLaneConsts is empty).  The grid size n stays a run-time value of the solve, so the stages' numbers are in the packed
    // offsets, not in the code.  Every offset is below the record's 40 128 bytes: 16 bits each.
    struct PitLaneFixed {
        unsigned bp[10];       // backward half, streams gp | ap[0..7] | kp: byte offset at the stage the lane's row sweeps first in its segment (low half) and at stage N - 1 (high half)
        unsigned bs[5];        // their steps in bytes, two per word (the even stream in the low half)
        unsigned cl[2][2];     // CombLane for LP_A = true | false: bb | pb << 16;  sx, sp as signed bytes | keep << 16 | keep_p << 17 | (sig < 0) << 31
        unsigned ci;           // pit_combine_inertia: word of the row's saved value function | its first source lane << 16
        unsigned fp[4], fs[4]; // forward half: byte offsets of the eight coefficient streams at the row's first stage and their steps in bytes, two per word
        unsigned fo;           // forward half: byte offset of the lane's output word at the row's first stage | its step in bytes << 16
        unsigned fx;           // forward half: word of the lane's component of its row's boundary state (a zero word where there is none) | segment of stage `lane` << 16 |
                               // min(c, 4) << 29, the lane's row of a saved tile in the boundary products (bits 26..28 are zero: fx >> 26 is that row times 8)
        __device__ __forceinline__ unsigned bptr(int i, bool tail) const { return tail ? bp[i] >> 16 : bp[i] & 0xffffu; }
        __device__ __forceinline__ int bstep(int i) const { return (int)((i & 1) ? bs[i >> 1] >> 16 : bs[i >> 1] & 0xffffu); }
        __device__ __forceinline__ unsigned fptr(int j) const { return (j & 1) ? fp[j >> 1] >> 16 : fp[j >> 1] & 0xffffu; }
        __device__ __forceinline__ int fstep(int j) const { return (int)((j & 1) ? fs[j >> 1] >> 16 : fs[j >> 1] & 0xffffu); }
        __device__ __forceinline__ CombLane comb(int which) const {
            const unsigned a = cl[which][0], b = cl[which][1];
            CombLane r;
            r.bb = (int)(a & 0xffffu); r.pb = (int)(a >> 16);
            r.sx = (int)(signed char)(b & 0xffu); r.sp = (int)(signed char)((b >> 8) & 0xffu);
            r.sig = T(__hiloint2double((int)(0x3ff00000u | (b & 0x80000000u)), 0));      // +-1
            r.keep = T((b >> 16) & 1u); r.keep_p = T((b >> 17) & 1u);
            return r;
        }
    };
    struct PitLaneNone {};
    using PitLaneConsts = std::conditional_t<NSC != 0, PitLaneFixed, PitLaneNone>;
    __device__ __forceinline__ PitLaneConsts pit_lane_consts() const {
        PitLaneConsts C{};
        if constexpr (NSC != 0) {
            static_assert(sizeof(T) == 8 && !GS && (long)LayoutT::total * (long)sizeof(T) < 65536, "PitLaneConsts packs byte offsets of fp64 words in LDS into 16 bits");
            const int N = L.n - 1, Lm = N >> 2;
            const int c = lane & 15, row = lane >> 4;
            const int kf = row * Lm + Lm - 1, kt = N - 1, B8 = (int)sizeof(T);
            auto at = [&](int w0, int s) { return (unsigned)((w0 + kf * s) * B8) | ((unsigned)((w0 + kt * s) * B8) << 16); };
            const int kind = pit_kind(c);
            const int gsw = kind < 3 ? 0 : (kind < 7 ? STG_S : CC_S);
            C.bp[0] = at(kind < 3 ? ZT_W(kind) : (kind < 7 ? STG_W(3 * (kind - 3)) : CC_W(0)), gsw);
            int st[10];
            st[0] = gsw * B8;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int s1 = pit_slot(r, c);
                C.bp[1 + r] = s1 ? at(STG_W(RA - 1 + s1), STG_S) : at(L.ZC, 0);
                st[1 + r] = s1 ? STG_S * B8 : 0;
            }
            const bool wrG = c < 14 && c != 6 && c != 7;
            C.bp[9] = wrG ? at(GAIN_W(c < 6 ? c : (c == 8 ? 6 : 7 + (c - 9))), GAIN_S) : at(GAIN_DUMMY_W(), 0);
            st[9] = wrG ? GAIN_S * B8 : 0;
#pragma unroll
            for (int i = 0; i < 5; ++i) C.bs[i] = (unsigned)st[2 * i] | ((unsigned)st[2 * i + 1] << 16);
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const CombLane r = comb_lane(c, w == 0, L.DX);
                C.cl[w][0] = (unsigned)r.bb | ((unsigned)r.pb << 16);
                C.cl[w][1] = ((unsigned)r.sx & 0xffu) | (((unsigned)r.sp & 0xffu) << 8) | (r.keep != T(0) ? 1u << 16 : 0u) | (r.keep_p != T(0) ? 1u << 17 : 0u) | (r.sig < T(0) ? 1u << 31 : 0u);
            }
            C.ci = (unsigned)(pit_tile(row < 3 ? row : 0) + 50) | ((unsigned)((lane & 48) + 9) << 16);
            // forward half (the LDS form of forward_pit): lanes 0..2 carry dx, lanes 3 4 du, the others run along on constants
            const int k0 = row * Lm;
            int qw[8], qs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { qw[j] = L.ZC; qs[j] = 0; }
            if (c < 3) {
                qw[0] = CH_W(c); qs[0] = 1;
                qw[1 + c] = L.ZC + 4;
                if (c < 2) { qw[3] = STG_W(c); qs[3] = STG_S; }
                qw[6] = STG_W(6 + c); qs[6] = STG_S;
                qw[7] = STG_W(9 + c); qs[7] = STG_S;
            } else if (c < 5) {
                const int a = c - 3;
                qw[0] = GAIN_W(NGH * a + 6); qs[0] = GAIN_S;
#pragma unroll
                for (int j = 0; j < 5; ++j) { qw[1 + j] = GAIN_W(NGH * a + j); qs[1 + j] = GAIN_S; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                C.fp[i] = (unsigned)((qw[2 * i] + qs[2 * i] * k0) * B8) | ((unsigned)((qw[2 * i + 1] + qs[2 * i + 1] * k0) * B8) << 16);
                C.fs[i] = (unsigned)(qs[2 * i] * B8) | ((unsigned)(qs[2 * i + 1] * B8) << 16);
            }
            const int os = c < 5 ? 1 : 0;
            C.fo = (unsigned)(((c < 3 ? L.DX + c * L.NS + 1 : (c < 5 ? L.DU + (c - 3) * L.NS : L.VP + 12)) + os * k0) * B8) | ((unsigned)(os * B8) << 16);
            const int seg = (lane >= Lm ? 1 : 0) + (lane >= 2 * Lm ? 1 : 0) + (lane >= 3 * Lm ? 1 : 0);
            C.fx = (unsigned)((c < 5 && row > 0) ? L.DX + 100 + 5 * (row - 1) + c : L.ZC) | ((unsigned)seg << 16) | ((unsigned)(c < 4 ? c : 4) << 29);
        }
        return C;
    }
    template <bool LP_A>
    __device__ __forceinline__ CombLane comb_of(const PitLaneConsts& PC, int c, int TB) const {
        if constexpr (NSC != 0) return PC.comb(LP_A ? 0 : 1); else return comb_lane(c, LP_A, TB);
    }
    // saved tile: rows 0..4 x 10 slots; every row of the wave holds the same data, so all of them store (same words, same values)
    __device__ __forceinline__ void pit_save(int base, int slot, const T (&M)[6]) const {
        if (slot >= 0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) sm[base + 10 * i + slot] = M[i];
        }
    }
    __device__ __forceinline__ void pit_load(int base, int slot, T (&M)[5]) const {
        const int a = base + (slot >= 0 ? slot : 0);
#pragma unroll
        for (int i = 0; i < 5; ++i) M[i] = sm[a + 10 * i];
    }
    // (EXT = 2, the cost variants: serial sweeps only -- register budget.)  The partitioned sweep parks its tiles in live solver arrays (pit_tile): the hand-off
    // tile (192 words) in DX | DU (5 NS words), the saved tile pairs (100 words each) in LAMN (3 NS words), the trig cache (NTR NS words) and DX.  The capacities
    // are part of the condition, not a consequence of the grid-size threshold (ADVICE r03).  Second invariant: a saved tile overwrites the trig cache, which
    // kkt_pass reads -- every path from a factorisation to the next kkt_pass rewrites TRIG for all k < n - 1 (eval_point / trial_eval of the accepted trial;
    // the solve ends without another kkt_pass when no trial is evaluated).
    // r04, inertia: a factorisation is accepted when the KKT matrix has Ipopt's inertia (riccati_root).  The serial sweep reads it off the signs of its control pivots R_k.  Here
    // every row counts the negative eigenvalues of the pivots of ITS segment (those of the segment's own cost-to-go from the identity border, not the serial ones), and
    // every combine eliminates the pair (costate, state) at a boundary: the block [[W, -I], [-I, P+]] over the five components that have a costate column has the inertia
    // In(W) + In(P+ - W^-1) (Haynsworth), five negative eigenvalues when all is well -- pit_combine_inertia() / pit_block_inertia() return the excess.  The sum of all of it plus the root system's
    // count is the matrix's, whatever the elimination order (Sylvester); tests/test_pit_math.py::test_inertia_of_the_kkt_matrix_from_the_sweeps holds both counts to the
    // eigenvalues of the dense matrix, including the cases where a negative pivot in one place is made up for in another.
    // Where the serial sweeps take over (r04, measured on the MI355X with the inertia test in both, scripts/dev/pit_*_sweep.py): the combines' I - W P+ is eliminated without
    // exchanges and loses the last digits the end game needs.  Headline kernel, three seeds x 1024 cold starts: partitioned sweeps down to mu = tol = 1e-8 converge 990 / 980 / 989
    // instances, down to 1e-6 992 / 985 / 998 -- exactly the serial sweeps' counts and iteration numbers, at the same kernel time.  Kernels with clearance rows (active rows put
    // 1e8-sized entries into the position block of the value functions): car-like footprints x 192 instances 172 / 147 / 163 with the partitioned sweeps down to 1e-8,
    // 179 / 163 / 175 = the serial sweeps' from 1e-6 up; config 3 at 4096 instances 4004 (1e-8), 4015 (1e-6), 4016 = serial (1e-4) at 21.5 ms against 23.8 ms serial.
    // So: partitioned while mu > max(tol, 1e-6) (Problem::pit_mu_min), max(tol, 1e-4) in the kernels with clearance rows (pit_floor()).
    static constexpr bool kPartitionedSweeps = true;
    __device__ __forceinline__ T pit_floor() const { return OBST ? t_max(P.pit_mu_min, T(1e-4)) : P.pit_mu_min; }
    // (the two-wave kernel only runs grids of at most 24 points -- its LDS record has to fit eight times into a CU --: the partitioned sweeps are compiled out of it, a
    //  third of its code; two resident waves per SIMD share the instruction cache: instruction-fetch waits 17 % -> see profiles/r06_wave_kernel_n20_two_waves.md)
    __device__ __forceinline__ bool pit_enabled() const { return kPartitionedSweeps && !W2 && EXT < 2 && P.pit != 0 && L.n >= 40 && 3 * L.NS >= 100 && L.NTR * L.NS >= 100 && 5 * L.NS >= 192; }
    // excess of negative eigenvalues of the pivot blocks of the three combines: n-(W) + n-(P+ - W^-1) - 5 each, by Jacobi's signature rule (negative pivots of the
    // elimination without exchanges).  W (the element's, 5 x 5) is swept in place -- the symmetric sweep operator leaves -W^-1 and shows the same pivots as the
    // elimination --, then G = P+ + (-W^-1) is eliminated (upper triangles; mpc_core.hpp::pit_block_inertia_tri has the arithmetic, compiled for the host by the tests).
    // Nothing of a combine depends on these counts, so they are taken after the last combine, all three at once: row s < 3 evaluates the block that took in ITS
    // segment's element -- W is the row's own wn (lane 9 + b holds W[a][b] as wn[a]; the asymmetry of the accumulated tile is rounding), P+ is the value function at the
    // segment's end, which that combine saved for the forward pass (pit_tile(s) + 50: word 10 a + b = P+[a][b]).  Same values, same arithmetic as one block per
    // combine; one serial chain of ten pivots instead of three.  ok = false when a pivot vanishes in any of them (the caller then repeats the factorisation with the
    // serial sweep).
    // (The kernels with a run-time layout keep one wave-uniform count per combine, pit_block_inertia(): there the code of the lane-parallel pass pushed the
    //  compiler into a stack frame -- 800-864 B of scratch per lane and 3-8 % longer launches of config 3 / config 5 / n = 20.)
    template <bool LP_A>
    __device__ __forceinline__ int pit_block_inertia(const int TB, const T (&Vp)[6], bool& ok) const {
        const int TW = TB + 96;
        T w[15], g[15];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = a; b < 5; ++b) {
                const int u = a * (9 - a) / 2 + b;
                w[u] = T(sm[TW + 16 * a + 9 + b]);                                        // W[a][b] lives in lane 9 + b as wn[a]
                g[u] = rd_lane(Vp[a], LP_A ? b : (b < 2 ? 6 + b : 10 + b));
            }
        return pit_block_inertia_tri(w, g, ok);
    }
    __device__ __forceinline__ int pit_combine_inertia(const PitLaneFixed& PC, const T (&wn)[5], bool& ok) const {
        const int tb = (int)(PC.ci & 0xffffu), src = (int)(PC.ci >> 16);      // pit_tile(row < 3 ? row : 0) + 50, lane 9 of the row
        sync();                                                            // (the combines' saves were made by other lanes)
        T w[15], g[15];
#pragma unroll
        for (int a = 0; a < 5; ++a)
#pragma unroll
            for (int b = a; b < 5; ++b) {
                const int u = a * (9 - a) / 2 + b;
                w[u] = lane_gather(wn[a], src + b);
                g[u] = T(sm[tb + 10 * a + b]);
            }
        bool okr = true;
        const int neg = pit_block_inertia_tri(w, g, okr);
        const int okw = okr ? 1 : 0;
        ok = ok && (__builtin_amdgcn_readlane(okw, 0) & __builtin_amdgcn_readlane(okw, 16) & __builtin_amdgcn_readlane(okw, 32)) != 0;
        return __builtin_amdgcn_readlane(neg, 0) + __builtin_amdgcn_readlane(neg, 16) + __builtin_amdgcn_readlane(neg, 32);
    }
    // one combine step.  LP_A: the value function's P+ columns sit in lane set A (then the result's sit in B), else the other way round.
    // In: Vp / Wp / omp = value function at the segment's end, the element's tile in LDS at TB.  Out: the same registers = value function at the
    // segment's start; the eliminated tile and the old value function go to `save` for the forward pass; wpiv = min |pivot| so far.
    template <bool LP_A>
    __device__ __forceinline__ void combine(const int TB, const int save, const CombLane& cl, const int lm, T (&Vp)[6], T (&Wp)[3], T& omp, T& wpiv, int& inert, bool& iok) const {
        if constexpr (NSC == 0) inert += pit_block_inertia<LP_A>(TB, Vp, iok);        // first: nothing of the combine is live yet
        const int TW = TB + 96;
        T Wt[5], WV[5], A[6], U[6], St[6], Ra[6];
#pragma unroll
        for (int i = 0; i < 5; ++i) Wt[i] = sm[TW + 16 * i + 9 + lm];                      // left factor W: column m in lane m
#pragma unroll
        for (int i = 0; i < 6; ++i) A[i] = sm[cl.bb + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) { St[i] = sm[TB + 16 * i + 9 + lm]; Ra[i] = sm[cl.pb + 16 * i]; }
        MPC_DPP_BLOCK_CWV
#pragma unroll
        for (int i = 0; i < 5; ++i) A[i] += cl.sig * WV[i];
        T gj_pv, gj_r, gj_e, gj_na;
        if constexpr (LP_A) { MPC_DPP_BLOCK_CGJ_A } else { MPC_DPP_BLOCK_CGJ_B }
#pragma unroll
        for (int i = 0; i < 6; ++i) { U[i] = Vp[i]; Ra[i] *= cl.keep_p; }
        if constexpr (LP_A) { MPC_DPP_BLOCK_CU_A } else { MPC_DPP_BLOCK_CU_B }
        MPC_DPP_BLOCK_CRA
        MPC_DPP_BLOCK_CWN
        // for the forward pass: the value function at the segment's END (still in Vp) and the eliminated tile; every read of the hand-off tile is done
        pit_save(save + 50, cl.sp, Vp);
        pit_save(save, cl.sx, A);
#pragma unroll
        for (int i = 0; i < 6; ++i) Vp[i] = Ra[i] * cl.keep;
    }

    __device__ __forceinline__ int backward_pit(const PitLaneConsts& PC, T delta, T dc, T& dd_out, T nu_out[3]) const {
        MPC_LAP_BEGIN(t_lap)
        const int n = L.n, N = n - 1, Lm = N >> 2, rem = N - 4 * Lm;
        const T d = SCL(SC_D);
        const int ZC = W_ZC();
        const int ll = local_lane();
        const int c = ll & 15, row = ll >> 4;
        // columns: 0..5 P, 6 7 the u columns of Hhat, 8 p, 9..13 border (row 3: 9..11 = the fixed goal components), 14 the dt border column, 15 idle
        // (fixed layout: the streams' places and steps come packed in PC, the steps in bytes; kind .. g0 are not computed)
        int kind = 0, gb = 0, gsw = 0, gs, slot1[8] = {}, as_[8];
        if constexpr (NSC != 0) {
            gs = PC.bstep(0);
#pragma unroll
            for (int r = 0; r < 8; ++r) as_[r] = PC.bstep(1 + r);
        } else {
            kind = pit_kind(c);
            gb = kind < 3 ? ZT_W(kind) : (kind < 7 ? STG_W(3 * (kind - 3)) : CC_W(0));
            gsw = kind < 3 ? 0 : (kind < 7 ? STG_S : CC_S);
            gs = sw_step(gsw);
#pragma unroll
            for (int r = 0; r < 8; ++r) { slot1[r] = pit_slot(r, c); as_[r] = sw_step(slot1[r] ? STG_S : 0); }
        }
        const T ec = (c == 5 || (c >= 8 && c < 15)) ? T(1) : T(0);
        const T E3 = c == 6 ? T(1) : T(0), E4 = c == 7 ? T(1) : T(0);
        const T dA0 = c == 0 ? delta : T(0), dA1 = c == 1 ? delta : T(0), dA2 = c == 2 ? delta : T(0);
        const T dA6 = c == 6 ? delta : T(0), dA7 = c == 7 ? delta : T(0);
        const bool wrG = c < 14 && c != 6 && c != 7;                       // every row stores the gains of its own stages
        const int g0 = c < 6 ? c : (c == 8 ? 6 : 7 + (c - 9));
        SwCRef gp;
        SwCRef ap[8];
        SwRef kp;
        int ks;
        if constexpr (NSC != 0) ks = PC.bstep(9); else ks = sw_step(wrG ? GAIN_S : 0);
        // (GS: gp / ap are the byte offsets of the lane's entries inside a stage's tile slot, set once; what moves is kl, the stage this lane's row reads next -- backward_dpp)
        int kl = 0;
        if constexpr (GS) {
            gp = (unsigned)(4 * (kind < 3 ? zt_entry(kind) : (kind < 7 ? 3 * (kind - 3) : TE_CC))) * (unsigned)sizeof(T);
#pragma unroll
            for (int r = 0; r < 8; ++r) ap[r] = (unsigned)(4 * (slot1[r] ? RA - 1 + slot1[r] : TE_Z)) * (unsigned)sizeof(T);
        }
        auto point_at = [&](int k, bool tail) {                           // running pointers at stage k (per lane); tail: k is stage N - 1, else the first stage of the row's segment
            if constexpr (NSC != 0) {
                gp = ldsb(PC.bptr(0, tail));
#pragma unroll
                for (int r = 0; r < 8; ++r) ap[r] = ldsb(PC.bptr(1 + r, tail));
                kp = ldsb(PC.bptr(9, tail));
            } else {
                if constexpr (GS) kl = k;
                else {
                    gp = sw(gb + k * gsw);
#pragma unroll
                    for (int r = 0; r < 8; ++r) ap[r] = sw(slot1[r] ? STG_W(RA - 1 + slot1[r]) + k * STG_S : ZC);
                }
                kp = sw(wrG ? GAIN_W(g0) + k * GAIN_S : GAIN_DUMMY_W());
            }
        };
        T V[6], wn[5] = {T(0), T(0), T(0), T(0), T(0)}, om = T(0);
        if constexpr (NSC != 0) {      // the final rate rows: one step behind stage N - 1 (a lane without the entry has step 0 and reads the zero word its pointer stands on)
            const T a3 = *lds_adv((const LdsT*)ldsb(PC.bptr(4, true)), as_[3]), a4 = *lds_adv((const LdsT*)ldsb(PC.bptr(5, true)), as_[4]), a5 = *lds_adv((const LdsT*)ldsb(PC.bptr(6, true)), as_[5]);
            terminal_value(V, c, delta, d, a3, a4, a5);
        } else {
            const int kf = n - 1;                                          // record of the final rate rows
            const T a3 = slot1[3] ? S_(RA - 1 + slot1[3], kf) : T(0), a4 = slot1[4] ? S_(RA - 1 + slot1[4], kf) : T(0), a5 = slot1[5] ? S_(RA - 1 + slot1[5], kf) : T(0);
            terminal_value(V, c, delta, d, a3, a4, a5);
        }
        T add_dd0 = T(0), add_qd0 = T(0);
        if (mintime()) add_qd0 += T(n - 1);
        if (dtf()) {
            const T dl = d - P.dt_lb, du = P.dt_ub - d;
            const T idl = fast_rcp(dl), idu = fast_rcp(du);
            add_dd0 = SCL(SC_PDL) * idl + SCL(SC_PDU) * idu + delta;
            add_qd0 += mu * idu - mu * idl;
        }
        // stage 0 belongs to row 0: no regularisation on x_0 (it is fixed), the dt-box / objective terms on row 5
        const T s05 = row == 0 ? (c == 5 ? add_dd0 : (c == 8 ? add_qd0 : T(0))) : T(0);
        const T dL0 = row == 0 ? T(0) : dA0, dL1 = row == 0 ? T(0) : dA1, dL2 = row == 0 ? T(0) : dA2;
        T worst = T(1);
        int negc = 0, negc_rem = 0;                                       // negative eigenvalues of the control pivots: this row's segment / the leftover stages all rows sweep together
        auto load_stage = [&](T (&g)[3], T (&a)[8]) {
            if constexpr (GS) {
                const unsigned kb = (unsigned)tile_k(kl) * (unsigned)sizeof(T);      // (per row: the four rows of the wave are at four places of the horizon)
                g[0] = gld(kb, gp); g[1] = gld(kb, gp + 4u * (unsigned)sizeof(T)); g[2] = gld(kb, gp + 8u * (unsigned)sizeof(T));
#pragma unroll
                for (int r = 0; r < 8; ++r) a[r] = gld(kb, ap[r]);
                --kl;
            } else {
                g[0] = sw_ld(gp, 0); g[1] = sw_ld(gp, 1); g[2] = sw_ld(gp, 2);
                if constexpr (NSC != 0) gp = lds_adv(gp, -gs); else gp -= gs;
#pragma unroll
                for (int r = 0; r < 8; ++r) { a[r] = sw_ld(ap[r]); if constexpr (NSC != 0) ap[r] = lds_adv(ap[r], -as_[r]); else ap[r] -= as_[r]; }
            }
        };
        auto stage = [&](T dk0, T dk1, T dk2, T s5, T (&G)[3], T (&A)[8], T (&Gn)[3], T (&An)[8]) {
            load_stage(Gn, An);
            T t[6];
            MPC_DPP_BLOCK_T1
            T h[8];
            h[0] = (A[0] + dk0) + t[0]; h[1] = (A[1] + dk1) + t[1]; h[2] = (A[2] + dk2) + t[2];
            h[3] = A[3]; h[4] = A[4];
            h[5] = (A[5] + s5) + t[5];
            h[6] = (A[6] + dA6) + t[3]; h[7] = (A[7] + dA7) + t[4];
            MPC_DPP_BLOCK_H
            T R00, R01, R11;
            MPC_DPP_BLOCK_R
            const T r2 = R01 * R01;
            const T det = R00 * R11 - r2;
            worst = t_fmin(worst, t_abs(det) - T(1e-14) * (t_abs(R00 * R11) + r2));
            { const int s0 = sign_word(R00), s1 = sign_word(det); negc += (int)((unsigned)s0 >> 31) + (int)((unsigned)(s0 ^ s1) >> 31); }
            const T nid = -fast_rcp(det);
            const T nRi00 = R11 * nid, Ri01 = -(R01 * nid), nRi11 = R00 * nid;
            const T nK0 = nRi00 * h[6] + Ri01 * h[7], nK1 = Ri01 * h[6] + nRi11 * h[7];
            sw_st(kp, 0, nK0); sw_st(kp, NGH, nK1);
            if constexpr (NSC != 0) kp = lds_adv(kp, -ks); else kp -= ks;
            V[0] = h[0]; V[1] = h[1]; V[2] = h[2]; V[3] = h[3]; V[4] = h[4]; V[5] = h[5];
            MPC_DPP_BLOCK_V5
        };
        T Ga[3], Aa[8], Gb[3], Ab[8];
        MPC_LAP(pit_pre, t_lap);
        // ---- the N mod 4 leftover stages at the end of the horizon: all rows together (k = N-1 .. 4 Lm)
        if (rem > 0) {
            point_at(N - 1, true);
            load_stage(Ga, Aa);
            stage(dA0, dA1, dA2, T(0), Ga, Aa, Gb, Ab);
            if (rem > 1) stage(dA0, dA1, dA2, T(0), Gb, Ab, Ga, Aa);
            if (rem > 2) stage(dA0, dA1, dA2, T(0), Ga, Aa, Gb, Ab);
        }
        negc_rem = negc; negc = 0;
        // ---- rows 0..2 start their segments from the identity border
        if (row < 3) {
#pragma unroll
            for (int i = 0; i < 6; ++i) V[i] = c == 9 + i ? T(1) : T(0);
#pragma unroll
            for (int a = 0; a < 5; ++a) wn[a] = T(0);
            om = T(0);
        }
        // ---- the four segments: row s sweeps k = s Lm + Lm - 1 .. s Lm
        point_at(row * Lm + Lm - 1, false);
        load_stage(Ga, Aa);
        int j = Lm;
        for (; j >= 3; j -= 2) {
            MPC_MARK("PIT_LOOP_BEGIN");
            stage(dA0, dA1, dA2, T(0), Ga, Aa, Gb, Ab);
            stage(dA0, dA1, dA2, T(0), Gb, Ab, Ga, Aa);
            MPC_MARK("PIT_LOOP_END");
        }
        if (j == 2) { stage(dA0, dA1, dA2, T(0), Ga, Aa, Gb, Ab); stage(dL0, dL1, dL2, s05, Gb, Ab, Ga, Aa); }
        else stage(dL0, dL1, dL2, s05, Ga, Aa, Gb, Ab);
        {
            const T w4 = t_fmin(t_fmin(rd_lane(worst, 0), rd_lane(worst, 16)), t_fmin(rd_lane(worst, 32), rd_lane(worst, 48)));
            if (!(w4 > T(0))) return 0;
        }
        MPC_LAP(bwd_loop, t_lap);
        // ---- hand-off + combine.  Tile (words from TB): [i][lane] V rows 0..5 | [a][lane] wn rows 0..4 | [lane] om
        const int TB = L.DX;
        // (the sync() on either side is what makes the hand-off visible ACROSS lanes: without it the compiler treats the tile as per-thread memory and
        // lets the other rows' loads overtake this row's stores)
        auto put_tile = [&](int r) {
            sync();
            if (row == r) {
#pragma unroll
                for (int i = 0; i < 6; ++i) sm[TB + 16 * i + c] = V[i];
#pragma unroll
                for (int a = 0; a < 5; ++a) sm[TB + 96 + 16 * a + c] = wn[a];
                sm[TB + 176 + c] = om;
            }
            sync();
        };
        T Vp[6], Wp[3], omp, wpiv = T(1);
        int inert = __builtin_amdgcn_readlane(negc_rem, 0) + __builtin_amdgcn_readlane(negc, 0) + __builtin_amdgcn_readlane(negc, 16) + __builtin_amdgcn_readlane(negc, 32) + __builtin_amdgcn_readlane(negc, 48);
        bool iok = true;
        MPC_MARK("PIT_COMBINE_BEGIN");
        put_tile(3);
        {
            const int cz = (c < 6 || (c >= 8 && c < 12)) ? c : 15;         // everything else reads the idle lane's zeros
#pragma unroll
            for (int i = 0; i < 6; ++i) Vp[i] = sm[TB + 16 * i + cz];
#pragma unroll
            for (int a = 0; a < 3; ++a) Wp[a] = sm[TB + 96 + 16 * a + c];
            omp = sm[TB + 176 + c];
        }
        MPC_DBG_PIT_W("V3")
        const int lm = c < 6 ? c : 0;
        put_tile(2);
        combine<true>(TB, pit_tile(2), comb_of<true>(PC, c, TB), lm, Vp, Wp, omp, wpiv, inert, iok);      // (run-time layout: the per-lane constants are recomputed per step, cheaper than keeping them)
        MPC_DBG_PIT_W("V2")
        put_tile(1);
        combine<false>(TB, pit_tile(1), comb_of<false>(PC, c, TB), lm, Vp, Wp, omp, wpiv, inert, iok);
        MPC_DBG_PIT_W("V1")
        put_tile(0);
        combine<true>(TB, pit_tile(0), comb_of<true>(PC, c, TB), lm, Vp, Wp, omp, wpiv, inert, iok);
        MPC_DBG_PIT_W("V0")
        if constexpr (NSC != 0) inert += pit_combine_inertia(PC, wn, iok);
        MPC_MARK("PIT_COMBINE_END");
        MPC_LAP(bwd_setup, t_lap);
        if (!(rd_lane(wpiv, 0) > T(1e-9)) || !iok) return 0;           // a pivot of I - W P+ (or of the inertia count) broke down: the caller repeats this factorisation with the serial sweep
        // ---- root: the value function at stage 0 has its P columns in lane set B (lane 15 = column 5)
        RicState<T> Vr;
        Vr.neg = inert;                                                    // segments' control pivots + the excess of the three combine blocks (pit_combine_inertia)
        int okr;      // 1 good, -1 wrong inertia (no point in repeating the sweep), 0 breakdown
        if constexpr (SHAPE != 0) {
            // r25: the entries by row broadcast, one v_mov_b64_dpp each, wave-uniform in vector registers -- where the fp64 arithmetic wants them (a v_readlane pair
            // leaves a scalar pair that the next two-operand instruction copies back).  All four DPP rows hold the same Vp / Wp / omp here: they read the same hand-off
            // tiles and run the same combines, whose per-lane constants (comb_lane, lm, cz) depend on the lane's place in its row alone.
            // The profile build counts the roots at which that does not hold (MPC_PROF_ROOT_ROWS; tests/test_gpu_boundary_root.py asserts none in every case).
            T rt_p55, rt_p5, rt_s5[3], rt_om[3], rt_w[3][3];
            MPC_PROF_ROOT_ROWS(Vp[5], omp, Wp[0], Wp[1], Wp[2]);
            MPC_DPP_BLOCK_ROOT
            Vr.P[5][5] = rt_p55;
            Vr.p[5] = rt_p5;
#pragma unroll
            for (int b = 0; b < 3; ++b) { Vr.S[5][b] = rt_s5[b]; Vr.om[b] = rt_om[b]; }
            Vr.W[0][0] = rt_w[0][0] - (fx(0) ? dc : T(0)); Vr.W[1][1] = rt_w[1][1] - (fx(1) ? dc : T(0)); Vr.W[2][2] = rt_w[2][2] - (fx(2) ? dc : T(0));
            Vr.W[0][1] = Vr.W[1][0] = T(0.5) * (rt_w[0][1] + rt_w[1][0]);
            Vr.W[0][2] = Vr.W[2][0] = T(0.5) * (rt_w[0][2] + rt_w[2][0]);
            Vr.W[1][2] = Vr.W[2][1] = T(0.5) * (rt_w[1][2] + rt_w[2][1]);
            okr = riccati_root_uniform<((SHAPE >> 3) & 1) != 0, SHAPE & 7>(Vr, dd_out, nu_out);      // (exchanges as uniform branches, flags read once: mpc_core.hpp)
        } else {
        Vr.P[5][5] = rd_lane(Vp[5], 15);
        Vr.p[5] = rd_lane(Vp[5], 8);
        Vr.S[5][0] = rd_lane(Vp[5], 9); Vr.S[5][1] = rd_lane(Vp[5], 10); Vr.S[5][2] = rd_lane(Vp[5], 11);
        Vr.om[0] = rd_lane(omp, 9); Vr.om[1] = rd_lane(omp, 10); Vr.om[2] = rd_lane(omp, 11);
        {
            const T w00 = rd_lane(Wp[0], 9), w01 = rd_lane(Wp[0], 10), w02 = rd_lane(Wp[0], 11);
            const T w10 = rd_lane(Wp[1], 9), w11 = rd_lane(Wp[1], 10), w12 = rd_lane(Wp[1], 11);
            const T w20 = rd_lane(Wp[2], 9), w21 = rd_lane(Wp[2], 10), w22 = rd_lane(Wp[2], 11);
            Vr.W[0][0] = w00 - (fx(0) ? dc : T(0)); Vr.W[1][1] = w11 - (fx(1) ? dc : T(0)); Vr.W[2][2] = w22 - (fx(2) ? dc : T(0));
            Vr.W[0][1] = Vr.W[1][0] = T(0.5) * (w01 + w10);
            Vr.W[0][2] = Vr.W[2][0] = T(0.5) * (w02 + w20);
            Vr.W[1][2] = Vr.W[2][1] = T(0.5) * (w12 + w21);
        }
        okr = riccati_root(Vr, P, dd_out, nu_out);
        }
        MPC_DBG_ROOT("pit   ", okr, rd_lane(wpiv, 0))
        return okr;
    }

    __device__ __forceinline__ void forward_pit(const PitLaneConsts& PC, T dd, const T nu[3], T delta) const {
        MPC_LAP_BEGIN(t_lap)
        const int n = L.n, N = n - 1, Lm = N >> 2;
        const int ll = local_lane();
        const int c = ll & 15, row = ll >> 4;
        // ---- boundary states (components 0..4; component 5 is dd) and costates, wave-uniform, left to right; they go to a small table behind the s = 0 tiles:
        //      TX + 5 s + i = state at b_{s+1}, TL + 5 s + i = costate at b_{s+1}
        const int TX = L.DX + 100, TL = L.DX + 115;
        if constexpr (NSC != 0) {
            // r25, fixed layout: ONE output component per lane.  A product's five results were five registers that every lane computed alike, a DPP instruction per term
            // and component; here lane i of a row works on row i of the tile (w[j] = column j, word 10 i + j of the tile: one load per column behind one address), the
            // running 5-vector is ONE register with component j in lane j, and a term of the state part is one v_fmac_f64_dpp with that register as the broadcast
            // operand (MPC_DPP_BLOCK_BXT).  Lane i's chain is what acc[i] was, operand for operand and in the same order -- the product's factors change places --, so
            // TX / TL hold the same bits.  The lanes behind the fifth of a row run along as copies of lane 4: same loads, same chain, same store (same word, same value),
            // which spares the exec mask around the stores.  Where a lane's row starts comes packed in PC.fx.
            const unsigned r8 = PC.fx >> 26;                                   // 8 min(c, 4)
            const LdsT* tp = ldsb(r8 * 10u);                                   // row min(c, 4) of a tile that starts at word 0
            LdsT* bp = ldsb(r8);                                               // word min(c, 4) of a 5-vector that starts at word 0
            // (a segment's two tiles are 100 words in a row: behind ONE address of their own the twenty columns are within the reach of the two-word loads' 8-bit offsets;
            //  left to fold the tile's place into the offsets the compiler forms an address per pair of columns.  The empty asm keeps the three addresses apart.)
            //  The words were saved by other lanes (pit_save: every lane its own slot): what orders those stores before these loads is the sync() at the head of
            //  pit_combine_inertia (fixed layout: behind the last combine) and the one behind backward_pit in solve().
            auto cols = [&](int tile, int j0, int j1, T (&wx)[10], T (&wv)[10]) {
                const LdsT* q = tp + tile;
                asm("" : "+v"(q));
#pragma unroll
                for (int j = j0; j < 10; ++j) wx[j] = q[j];
#pragma unroll
                for (int j = j1; j < 10; ++j) wv[j] = q[50 + j];
            };
            auto tail = [&](const T (&w)[10], T cx) {                          // the terms in dd and nu: uniform coefficients, plain fmas in block_bx's order
                cx = __builtin_fma(w[5], dd, cx);
                cx = __builtin_fma(w[7], nu[0], cx); cx = __builtin_fma(w[8], nu[1], cx); cx = __builtin_fma(w[9], nu[2], cx);
                return cx;
            };
            auto prod = [&](const T (&w)[10], T xv) {
                T cx = w[6];
                MPC_DPP_BLOCK_BXT
                return tail(w, cx);
            };
            // all six tiles first (one LDS round trip), then the six products back to back
            T XA0[10], VB0[10], XA1[10], VB1[10], XA2[10], VB2[10];
            cols(pit_tile(0), 5, 0, XA0, VB0);                                 // (the first boundary state starts from xi = 0: no state columns)
            cols(pit_tile(1), 0, 0, XA1, VB1);
            cols(pit_tile(2), 0, 0, XA2, VB2);
            const T x1 = tail(XA0, XA0[6]);
            bp[TX] = x1;
            bp[TL] = prod(VB0, x1);
            const T x2 = prod(XA1, x1);
            bp[TX + 5] = x2;
            bp[TL + 5] = prod(VB1, x2);
            const T x3 = prod(XA2, x2);
            bp[TX + 10] = x3;
            bp[TL + 10] = prod(VB2, x3);
            sync();                                                            // (a word of the table is read by other lanes than the one that wrote it)
        } else {
            const CombLane cla = comb_of<true>(PC, c, L.DX), clb = comb_of<false>(PC, c, L.DX);
            // all six tiles first (one LDS round trip), then the six products back to back
            T XA0[5], VB0[5], XA1[5], VB1[5], XA2[5], VB2[5];
            pit_load(pit_tile(0), cla.sx, XA0); pit_load(pit_tile(0) + 50, cla.sp, VB0);
            pit_load(pit_tile(1), clb.sx, XA1); pit_load(pit_tile(1) + 50, clb.sp, VB1);
            pit_load(pit_tile(2), cla.sx, XA2); pit_load(pit_tile(2) + 50, cla.sp, VB2);
            T acc[5], xi[5];
            { const T (&M)[5] = XA0; MPC_DPP_BLOCK_BX0_B }
#pragma unroll
            for (int i = 0; i < 5; ++i) { xi[i] = acc[i]; sm[TX + i] = acc[i]; }
            { const T (&M)[5] = VB0; MPC_DPP_BLOCK_BX_A }
#pragma unroll
            for (int i = 0; i < 5; ++i) sm[TL + i] = acc[i];
            { const T (&M)[5] = XA1; MPC_DPP_BLOCK_BX_A }
#pragma unroll
            for (int i = 0; i < 5; ++i) { xi[i] = acc[i]; sm[TX + 5 + i] = acc[i]; }
            { const T (&M)[5] = VB1; MPC_DPP_BLOCK_BX_B }
#pragma unroll
            for (int i = 0; i < 5; ++i) sm[TL + 5 + i] = acc[i];
            { const T (&M)[5] = XA2; MPC_DPP_BLOCK_BX_B }
#pragma unroll
            for (int i = 0; i < 5; ++i) { xi[i] = acc[i]; sm[TX + 10 + i] = acc[i]; }
            { const T (&M)[5] = VB2; MPC_DPP_BLOCK_BX_A }
#pragma unroll
            for (int i = 0; i < 5; ++i) sm[TL + 10 + i] = acc[i];
        }
        // component c of the boundary state of this row's segment (row 0 starts at 0): read before the step arrays are written
        T xi_row;
        if constexpr (NSC != 0) xi_row = sm[PC.fx & 0xffffu];      // (a lane without a component reads a zero word)
        else xi_row = (c < 5 && row > 0) ? sm[TX + 5 * (row - 1) + c] : T(0);
        // ---- lane-parallel: fold the border multiplier of the stage's own segment and dd into the affine terms (as forward_states does with nu)
        for (int k = lane; k < n - 1; k += kWave) {
            int seg;
            if constexpr (NSC != 0) seg = (int)((PC.fx >> 16) & 3u);      // (a record of NSC < kWave stages: k is `lane`, the loop has one trip)
            else seg = (k >= Lm ? 1 : 0) + (k >= 2 * Lm ? 1 : 0) + (k >= 3 * Lm ? 1 : 0);
            T m5[5];
#pragma unroll
            for (int b = 0; b < 5; ++b) m5[b] = seg < 3 ? sm[TL + 5 * seg + b] : (b < 3 ? nu[b] : T(0));
            for (int a = 0; a < 2; ++a)
            {      // (GS: kappa^ -> DU, c^ -> LAMN, see forward_states)
                const T kh = G_(NGH * a + 6, k) + (G_(NGH * a + 7, k) * m5[0] + G_(NGH * a + 8, k) * m5[1] + G_(NGH * a + 9, k) * m5[2] + G_(NGH * a + 10, k) * m5[3] + G_(NGH * a + 11, k) * m5[4] +
                                                   G_(NGH * a + 5, k) * dd);
                if constexpr (GS) F(L.DU, a, k) = kh; else G_(NGH * a + 6, k) = kh;
            }
            for (int i = 0; i < 3; ++i) CH_(i, k) = C_(i, k) + S_(3 + i, k) * dd;
        }
        if (lane == 0) { SCL(SC_DD) = dd; F(L.DX, 0, 0) = T(0); F(L.DX, 1, 0) = T(0); F(L.DX, 2, 0) = T(0); }
        sync();
        // ---- the four segments at once: row s carries (dx, du_prev) through its stages, starting from its boundary state
        {
            const int ZC = W_ZC(), k0 = row * Lm;
            int qw[8], qs[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) { qw[j] = ZC; qs[j] = 0; }
            int qk[8];               // the stage a pointer starts at, in strides (a tile pointer is placed at its row's first stage directly)
#pragma unroll
            for (int j = 0; j < 8; ++j) qk[j] = k0;
            if (c < 3) {
                if constexpr (GS) {      // (entries of the stages' tile slots, see forward_states)
                    const int t0 = tile_k(k0);
                    qw[1 + c] = ZC + 4;
                    if (c < 2) { qw[3] = t0 + 4 * c; qs[3] = 1; qk[3] = 0; }
                    qw[6] = t0 + 4 * (6 + c); qs[6] = 1; qk[6] = 0;
                    qw[7] = t0 + 4 * (9 + c); qs[7] = 1; qk[7] = 0;
                } else {
                qw[0] = CH_W(c); qs[0] = 1;
                qw[1 + c] = ZC + 4;
                if (c < 2) { qw[3] = STG_W(c); qs[3] = STG_S; }
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
            for (int j = 0; j < 8; ++j) { qp[j] = sw(qw[j] + qs[j] * qk[j]); qs[j] = sw_step(qs[j]); }
            int os = c < 5 ? 1 : 0;
            LdsT* op = lds((c < 3 ? L.DX + c * L.NS + 1 : (c < 5 ? L.DU + (c - 3) * L.NS : L.VP + 12)) + os * k0);
            if constexpr (NSC != 0) {      // fixed layout: the same places from PC instead (pit_lane_consts() has the table above), the steps in bytes
#pragma unroll
                for (int j = 0; j < 8; ++j) { qp[j] = ldsb(PC.fptr(j)); qs[j] = PC.fstep(j); }
                op = ldsb(PC.fo & 0xffffu); os = (int)(PC.fo >> 16);
            }
            const unsigned tjump = (unsigned)(4 * TNT - 4) * (unsigned)sizeof(T);      // GS: what a tile pointer jumps across a tile boundary, see forward_states; here per row
            const unsigned jl = (GS && c < 3) ? tjump : 0u, jl3 = (GS && c < 2) ? tjump : 0u;
            int kl = k0;
            const LdsT* q0p = lds((c < 3 ? L.LAMN + c * L.NS : (c < 5 ? L.DU + (c - 3) * L.NS : L.ZC)) + (c < 5 ? k0 : 0));      // GS: the constant term from LDS, see forward_states
            const int q0s = c < 5 ? 1 : 0;
            auto load_q = [&](T (&q)[8]) {
                if constexpr (GS) {
                    q[0] = *q0p; q0p += q0s;
#pragma unroll
                    for (int j = 1; j < 8; ++j) { q[j] = sw_ld(qp[j]); qp[j] += qs[j]; }
                    const bool cross = ((kl + GlobalStage::kGuard) & 3) == 3;
                    const unsigned ja = cross ? jl : 0u, jb = cross ? jl3 : 0u;
                    qp[3] += jb; qp[6] += ja; qp[7] += ja;
                    ++kl;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) { q[j] = sw_ld(qp[j]); if constexpr (NSC != 0) qp[j] = lds_adv(qp[j], qs[j]); else qp[j] += qs[j]; }
                }
            };
            T xi = xi_row;
            auto stage = [&](T (&q)[8], T (&qn)[8]) {
                load_q(qn);
                T s = q[0], s2 = T(0), xn;
                MPC_DPP_BLOCK_FWD
                *op = xn; if constexpr (NSC != 0) op = lds_adv(op, os); else op += os;
                xi = xn;
            };
            T qa[8], qb[8];
            MPC_LAP(fwd_pre, t_lap);
            if constexpr (GS) {
                // coefficients from global memory: three stages ahead (see forward_states); every row runs Lm + (N mod 4) stages, the rows below 3 turn to the dummy
                // word after their own Lm (row 3's pointers simply go on into the leftover stages)
                const int cnt = Lm + (N - 4 * Lm);
                int done = 0;
                auto comp = [&](T (&q)[8]) {
                    if (done == Lm && row < 3) { op = lds(L.VP + 12); os = 0; }
                    T s = q[0], s2 = T(0), xn;
                    MPC_DPP_BLOCK_FWD
                    *op = xn; op += os;
                    xi = xn;
                    ++done;
                };
                T q0[8], q1[8], q2[8], q3[8];
                load_q(q0); load_q(q1); load_q(q2);
                int k = 0;
                for (; k + 4 <= cnt; k += 4) { load_q(q3); comp(q0); load_q(q0); comp(q1); load_q(q1); comp(q2); load_q(q2); comp(q3); }
                if (k < cnt) comp(q0);
                if (k + 1 < cnt) comp(q1);
                if (k + 2 < cnt) comp(q2);
            } else {
            load_q(qa);
            int k = 0;
            for (; k + 1 < Lm; k += 2) { stage(qa, qb); stage(qb, qa); }
            if (k < Lm) { stage(qa, qb);
#pragma unroll
                          for (int j = 0; j < 8; ++j) qa[j] = qb[j]; }
            // leftover stages 4 Lm .. N-1: row 3 simply goes on (its pointers are there); the other rows compute along but write to a dummy word
            if (row < 3) { op = lds(L.VP + 12); os = 0; }
            for (k = 4 * Lm; k < N; ++k) { stage(qa, qb);
#pragma unroll
                                           for (int j = 0; j < 8; ++j) qa[j] = qb[j]; }
            }
            MPC_LAP(fwd_loop, t_lap);
        }
        MPC_LAP_BEGIN(t_post)
        multipliers(dd, nu, delta);
        MPC_LAP(fwd_post, t_post);
    }

