// mpc_wave_debug.hpp -- the developer diagnostics of the wave kernel behind ONE set of macros: every macro is empty in the product build, and no
// other kernel source tests a developer switch.  scripts/dev/variants.py names the instrumented builds and compiles each next to the product library, by the product's rule.
//   -DMPC_ASM_MARK            comment markers in the assembly around the phases of an iteration (scripts/dev/asm_phase_count.py counts instructions between them)
//   -DMPC_PROFILE             per-wave cycle counters per phase, read back through mpc_debug_profile (scripts/dev/phase_profile.py); with -DMPC_PROFILE_MULT the multiplier
//                             recurrence is counted in the place of `logs0`
//   -DMPC_PIT_CHECK=<blocks>  both sweeps on every factorisation of the first <blocks> workgroups, differences printed; with -DMPC_PIT_VERBOSE workgroup <blocks> prints
//                             the partitioned sweep's hand-off tiles and both sweeps' roots
//   -DMPC_NANCHECK=<block>    non-finite words per field of that workgroup's record after every sweep, the sweeps' roots, line-search traces
//   -DMPC_POISON_LDS          the kernel fills its LDS record with NaN first: a read of a word the solver did not write shows in the result
// The macros expand INSIDE IpmWave (its members, the solve loop, the sweeps) and use the local names there; MPC_DBG_POISON expands in the kernel body (mpc_solve_kernel.hpp).
#pragma once

#ifdef MPC_ASM_MARK
#define MPC_MARK(name) asm volatile("; " name)
#else
#define MPC_MARK(name) do { } while (0)
#endif

#ifdef MPC_POISON_LDS
#define MPC_DBG_POISON(sm, words, lane) { for (int e_ = lane; e_ < (words); e_ += mpc::kWave) (sm)[e_] = T(NAN); __syncthreads(); }
#else
#define MPC_DBG_POISON(sm, words, lane) do { } while (0)
#endif

#ifdef MPC_PROFILE
// Row of g_mpc_prof, one per workgroup (scripts/dev/variants.py names the same columns in the same order: PROF_COLUMNS).  Every tick of the loop lands in exactly one of the
// phase and glue counters: a phase stamps its own begin and end, a glue section runs from the last stamp to its MPC_GAP_END, so that the counters of an iteration add up to `ticks`.
namespace mpc {
enum ProfCol : int {
    PROF_TICKS, PROF_WALL /* 100 MHz */, PROF_ITERS, PROF_NFAC /* factorisations */, PROF_NTRIAL,
    // phases (MPC_TICK)
    PROF_KKT, PROF_BARRIER_TERMS, PROF_BACKWARD, PROF_FORWARD, PROF_POST, PROF_LOGS0 /* barrier_logs at the current point */, PROF_TRIAL, PROF_ACCEPT, PROF_TRIAL_SETUP,
    // glue (MPC_GAP_END): kkt -> barrier terms (error, stop tests, barrier update) | barrier terms -> a factorisation (pow, delta; between two factorisations) |
    // line-search set-up (post -> trial_setup -> first trial; between two trials) | last trial -> accept | accept -> kkt (loop back edge)
    PROF_GLUE_KKT_TO_BARRIER, PROF_GLUE_BARRIER_TO_FAC, PROF_GLUE_LS_SETUP, PROF_GLUE_TRIAL_TO_ACCEPT, PROF_GLUE_BACK_EDGE,
    // the sweeps' inner counters (MPC_LAP; parts of `backward` / `forward`): backward stage loops | hand-off + combines (serial: the set-up before the loop) | forward stage loop |
    // the partitioned sweeps' fixed work: backward_pit up to its first stage | forward_pit before / behind its segment loop
    PROF_BWD_LOOP, PROF_BWD_SETUP, PROF_FWD_LOOP, PROF_PIT_PRE, PROF_FWD_PRE, PROF_FWD_POST,
    // not ticks (r25, MPC_PROF_ROOT_ROWS): the roots of backward_pit at which the four DPP rows did NOT hold the same bits in the registers the tableau is broadcast from; 0
    PROF_SPARE
};
constexpr int kProfCols = 26;
constexpr int kProfTicks = PROF_GLUE_BACK_EDGE - PROF_KKT + 1;      // the phase + glue counters: tk[] of the solve loop
static_assert(PROF_SPARE + 1 == kProfCols, "one name per column");
}  // namespace mpc
__device__ long long g_mpc_prof[4096][mpc::kProfCols];      // (one per translation unit: solve_profile_add, mpc_solve_kernel.hpp)

#define MPC_PROF_MEMBERS \
    mutable long long prof_mult = 0; \
    mutable long long prof_bwd_loop = 0, prof_bwd_setup = 0, prof_fwd_loop = 0, prof_pit_pre = 0, prof_fwd_pre = 0, prof_fwd_post = 0; \
    mutable long long prof_root_rows = 0;
#define MPC_PROF_BEGIN \
        long long tk[mpc::kProfTicks] = {}; int nfac = 0, ntrial = 0; \
        const long long t_begin = __builtin_readcyclecounter(); \
        long long t_lap = t_begin; \
        const long long w_begin = wall_clock64();
#define MPC_TICK(col, stmt) { long long t0_ = __builtin_readcyclecounter(); stmt; t_lap = __builtin_readcyclecounter(); tk[mpc::PROF_##col - mpc::PROF_KKT] += t_lap - t0_; }
#define MPC_GAP_END(col) { const long long t1_ = __builtin_readcyclecounter(); tk[mpc::PROF_##col - mpc::PROF_KKT] += t1_ - t_lap; t_lap = t1_; }
#define MPC_PROF_COUNT(c) ++c
#define MPC_PROF_END \
        if (lane == 0 && blockIdx.x < 4096) { \
            long long* o = g_mpc_prof[blockIdx.x]; \
            o[mpc::PROF_TICKS] = __builtin_readcyclecounter() - t_begin; o[mpc::PROF_WALL] = wall_clock64() - w_begin; o[mpc::PROF_ITERS] = it; o[mpc::PROF_NFAC] = nfac; o[mpc::PROF_NTRIAL] = ntrial; \
            for (int i = 0; i < mpc::kProfTicks; ++i) o[mpc::PROF_KKT + i] = tk[i]; \
            o[mpc::PROF_BWD_LOOP] = prof_bwd_loop; o[mpc::PROF_BWD_SETUP] = prof_bwd_setup; o[mpc::PROF_FWD_LOOP] = prof_fwd_loop; \
            o[mpc::PROF_PIT_PRE] = prof_pit_pre; o[mpc::PROF_FWD_PRE] = prof_fwd_pre; o[mpc::PROF_FWD_POST] = prof_fwd_post; \
            if (prof_mult) o[mpc::PROF_LOGS0] = prof_mult; \
            o[mpc::PROF_SPARE] = prof_root_rows; \
        }
// the sweeps' inner counters: MPC_LAP_BEGIN(t) stamps a local, MPC_LAP(counter, t) adds the ticks since t's stamp to prof_<counter> and stamps t again
#define MPC_LAP_BEGIN(t) long long t = __builtin_readcyclecounter();
#define MPC_LAP(counter, t) { const long long now_ = __builtin_readcyclecounter(); prof_##counter += now_ - t; t = now_; }
// the shape-known kernels take the root system's entries by ROW broadcasts (MPC_DPP_BLOCK_ROOT), which is right when lanes c, c + 16, c + 32, c + 48 of the five source registers
// hold the same bits: every lane compares its words with those of its column in row 0 (ds_bpermute), and a root at which any lane differs counts once (wave-uniform)
#define MPC_PROF_ROOT_ROWS(v5, om_, w0, w1, w2) { \
            const T src_[5] = {v5, om_, w0, w1, w2}; bool diff_ = false; \
            for (int i_ = 0; i_ < 5; ++i_) { const T r0_ = lane_gather(src_[i_], lane & 15); \
                                             diff_ = diff_ || __double2hiint((double)r0_) != __double2hiint((double)src_[i_]) || __double2loint((double)r0_) != __double2loint((double)src_[i_]); } \
            if (__builtin_amdgcn_ballot_w64(diff_) != 0) ++prof_root_rows; }
#else
#define MPC_PROF_MEMBERS
#define MPC_PROF_BEGIN
#define MPC_TICK(col, stmt) { stmt; }
#define MPC_GAP_END(col) do { } while (0)
#define MPC_PROF_COUNT(c) do { } while (0)
#define MPC_PROF_END
#define MPC_LAP_BEGIN(t)
#define MPC_LAP(counter, t) do { } while (0)
#define MPC_PROF_ROOT_ROWS(v5, om_, w0, w1, w2) do { } while (0)
#endif
#if defined(MPC_PROFILE) && defined(MPC_PROFILE_MULT)      // the ticks of the enclosing scope go to prof_mult, which takes the place of `logs0` in the row
#define MPC_PROF_SCOPE_MULT \
        struct Tick { long long& acc; long long t0; __device__ Tick(long long& a) : acc(a), t0(__builtin_readcyclecounter()) {} __device__ ~Tick() { acc += __builtin_readcyclecounter() - t0; } } tick_(prof_mult);
#else
#define MPC_PROF_SCOPE_MULT
#endif

#ifdef MPC_PIT_CHECK
#define MPC_DBG_PIT_CHECK \
                if (pit && (int)blockIdx.x < MPC_PIT_CHECK) { \
                    T dd1 = T(0), nu1[3] = {T(0), T(0), T(0)}, dd2 = T(0), nu2[3] = {T(0), T(0), T(0)}; \
                    const int g1c = backward_pit(plc, delta, dc, dd1, nu1); sync(); \
                    const bool g1 = g1c > 0; \
                    if (g1) { forward_pit(plc, dd1, nu1, delta); sync(); } \
                    T keepx = T(0), keepu = T(0), keepl = T(0); \
                    const int kk = lane < L.n - 1 ? lane : 0; \
                    keepx = F(L.DX, 2, kk); keepu = F(L.DU, 1, kk); keepl = F(L.LAMN, 2, kk); \
                    sync(); \
                    const bool g2 = backward_dpp(delta, dc, dd2, nu2); sync(); \
                    if (g2) { forward_states(dd2, nu2, delta); sync(); } \
                    const T ex = wave_max(t_abs(keepx - F(L.DX, 2, kk))), eu = wave_max(t_abs(keepu - F(L.DU, 1, kk))), el = wave_max(t_abs(keepl - F(L.LAMN, 2, kk))); \
                    const T sx = wave_max(t_abs(F(L.DX, 2, kk))), su = wave_max(t_abs(F(L.DU, 1, kk))), sl = wave_max(t_abs(F(L.LAMN, 2, kk))); \
                    if (lane == 0 && (g1 != g2 || ex > T(1e-7) * (sx + T(1e-3)) || eu > T(1e-7) * (su + T(1e-3)) || el > T(1e-7) * (sl + T(1e-3)))) \
                        printf("blk %d it %d try %d delta %.2e mu %.1e: pit ok %d (code %d) serial ok %d | dd %.9e vs %.9e | max diff dx %.2e (of %.2e) du %.2e (of %.2e) lam %.2e (of %.2e)\n", (int)blockIdx.x, it, ntry, (double)delta, (double)mu, \
                               (int)g1, g1c, (int)g2, (double)dd1, (double)dd2, (double)ex, (double)sx, (double)eu, (double)su, (double)el, (double)sl); \
                    sync(); \
                }
#else
#define MPC_DBG_PIT_CHECK
#endif

#ifdef MPC_NANCHECK
#define MPC_DBG_NANCHECK_FIELDS \
                if (blockIdx.x == MPC_NANCHECK && lane == 0) { \
                    const int offs[] = {L.X, L.U, L.LAM, L.LAMN, L.SR, L.YR, L.PL, L.PU, L.DX, L.DU, L.CC, L.TRIG, L.GAIN, L.STG, L.SC, L.VP, L.ZC, L.total}; \
                    const char* nm[] = {"X", "U", "LAM", "LAMN", "SR", "YR", "PL", "PU", "DX", "DU", "CC", "TRIG", "GAIN", "STG", "SC", "VP", "ZC"}; \
                    printf("it %d try %d good %d delta %g dd %g nu %g %g %g mu %g |", it, ntry, (int)good, (double)delta, (double)dd, (double)nu[0], (double)nu[1], (double)nu[2], (double)mu); \
                    for (int f = 0; f < 17; ++f) { \
                        int cnt = 0, first = -1; \
                        for (int q = offs[f]; q < offs[f + 1]; ++q) if (!t_finite(sm[q])) { ++cnt; if (first < 0) first = q - offs[f]; } \
                        if (cnt) printf(" %s:%d@%d", nm[f], cnt, first); \
                    } \
                    printf("\n"); \
                }
#define MPC_DBG_NANCHECK_STEP \
                    if (blockIdx.x == MPC_NANCHECK) { \
                        for (int k = lane; k < L.n; k += kWave) { \
                            bool f = t_finite(F(L.DX, 0, k)) && t_finite(F(L.DX, 1, k)) && t_finite(F(L.DX, 2, k)); \
                            if (k < L.n - 1) f = f && t_finite(F(L.DU, 0, k)) && t_finite(F(L.DU, 1, k)) && t_finite(F(L.LAMN, 0, k)) && t_finite(F(L.LAMN, 1, k)) && t_finite(F(L.LAMN, 2, k)); \
                            if (!f) printf("it %d try %d fwd nonfinite at k %d: dx %g %g %g du %g %g lamn %g %g %g\n", it, ntry, k, (double)F(L.DX, 0, k), (double)F(L.DX, 1, k), (double)F(L.DX, 2, k), (double)F(L.DU, 0, k), (double)F(L.DU, 1, k), (double)F(L.LAMN, 0, k), (double)F(L.LAMN, 1, k), (double)F(L.LAMN, 2, k)); \
                        } \
                    }
#define MPC_DBG_NANCHECK_LS_FAILED \
            if (blockIdx.x == MPC_NANCHECK && lane == 0 && !accepted) \
                printf("   ls FAILED: it %d phi0 %.12e Dm %.6e rho %.6e mu %g theta %.6e theta_c %.6e fobj %.9f logs_cur %.9f | last alpha %g f_t %.9f th_t %.6e lg_t %.9f dzmax %g a_p %g\n", \
                       it, (double)phi0, (double)Dm, (double)rho, (double)mu, (double)theta, (double)theta_c, (double)fobj, (double)logs_cur, (double)alpha, (double)f_t, (double)th_t, (double)lg_t, (double)fw.dzmax, (double)fw.a_p);
#define MPC_DBG_NANCHECK_LS \
            if (blockIdx.x == MPC_NANCHECK && lane == 0) \
                printf("   ls: it %d f %.6f -> %.6f theta_c %.3e alpha %.4f a_p %.4f a_d %.4f rho %.3e Dm %.4e hdz %.6e clam %.6e dz2 %.6e dphi %.6e\n", it, (double)fobj, (double)f_t, (double)th_t, (double)alpha, (double)fw.a_p, (double)fw.a_d, (double)rho, (double)Dm, (double)fw.hdz, (double)fw.clam, (double)fw.dz2, (double)fw.dphi);
#else
#define MPC_DBG_NANCHECK_FIELDS
#define MPC_DBG_NANCHECK_STEP
#define MPC_DBG_NANCHECK_LS_FAILED
#define MPC_DBG_NANCHECK_LS
#endif

#ifdef MPC_PIT_VERBOSE
#define MPC_DBG_PIT_W(tag) if (blockIdx.x == MPC_PIT_CHECK) { const double q00 = rd_lane(Wp[0], 9), q01 = rd_lane(Wp[0], 10), q02 = rd_lane(Wp[0], 11), q10 = rd_lane(Wp[1], 9), q11 = rd_lane(Wp[1], 10), q12 = rd_lane(Wp[1], 11), q20 = rd_lane(Wp[2], 9), q22 = rd_lane(Wp[2], 11), o0 = rd_lane(omp, 9); \
            if (lane == 0) printf("   [%s] Wp0 %.9e %.9e %.9e Wp1 %.9e %.9e %.9e Wp2 %.9e .. %.9e om0 %.9e\n", tag, q00, q01, q02, q10, q11, q12, q20, q22, o0); }
#else
#define MPC_DBG_PIT_W(tag)
#endif

// the root system a backward sweep (tag: "serial" / "pit   ") hands to riccati_root and what came of it, behind the root solve: Vr the sweep's RicState, ok the solve's
// result, worst the sweep's smallest pivot measure.  Printed by the workgroup MPC_NANCHECK names, or (MPC_PIT_VERBOSE) the one MPC_PIT_CHECK names
#if defined(MPC_NANCHECK)
#define MPC_DBG_ROOT_BLOCK MPC_NANCHECK
#elif defined(MPC_PIT_VERBOSE)
#define MPC_DBG_ROOT_BLOCK MPC_PIT_CHECK
#endif
#ifdef MPC_DBG_ROOT_BLOCK
#define MPC_DBG_ROOT(tag, ok, worst) \
        if (blockIdx.x == MPC_DBG_ROOT_BLOCK && lane == 0) \
            printf("  %s root: ok %d worst %g P55 %.10e p5 %.10e S5 %.10e %.10e %.10e om %.10e %.10e %.10e W %.10e %.10e %.10e %.10e %.10e %.10e\n", tag, (int)(ok), (double)(worst), (double)Vr.P[5][5], (double)Vr.p[5], \
                   (double)Vr.S[5][0], (double)Vr.S[5][1], (double)Vr.S[5][2], (double)Vr.om[0], (double)Vr.om[1], (double)Vr.om[2], \
                   (double)Vr.W[0][0], (double)Vr.W[0][1], (double)Vr.W[0][2], (double)Vr.W[1][1], (double)Vr.W[1][2], (double)Vr.W[2][2]);
#else
#define MPC_DBG_ROOT(tag, ok, worst)
#endif
