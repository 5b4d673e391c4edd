// mpc_problem.hpp -- host-side translation of the ABI's mpc_config (the reference's ROS
// parameter set, src/controller.cpp:225-805) into the device-side Problem<T> record.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/mpc_hip.h"
#include "mpc_core.hpp"

namespace mpc {

// what mpc_config.line_search = MPC_LS_DEFAULT means: 0 the l1 merit, 1 Ipopt's filter
constexpr int kDefaultLineSearch = 1;

// why mpc_create refuses a configuration (the text mpc_last_error reports), or nullptr.  Checks of the configuration alone; mpc_create adds the device's.
inline const char* config_error(const mpc_config& c) {
    if (c.n < 3 || c.n > 4096) return "mpc_create: n out of range [3,4096]";
    if (c.model < 0 || c.model > 3) return "mpc_create: unknown model";
    if (c.collocation != MPC_COLLOC_FORWARD && c.collocation != MPC_COLLOC_MIDPOINT && c.collocation != MPC_COLLOC_CRANK_NICOLSON)
        return "mpc_create: unknown collocation method";
    if (c.objective != MPC_OBJ_MIN_TIME && c.objective != MPC_OBJ_QUADRATIC && c.objective != MPC_OBJ_MIN_TIME_VIA_POINTS) return "mpc_create: unknown objective";
    if (c.objective == MPC_OBJ_MIN_TIME_VIA_POINTS && (c.max_via_points < 1 || c.max_via_points > 64))
        return "mpc_create: minimum_time_via_points needs 1 <= max_via_points <= 64";
    if (c.objective != MPC_OBJ_QUADRATIC && !c.dt_free) return "mpc_create: minimum_time needs a variable grid (dt_free)";
    if (!(c.dt_ref > 0)) return "mpc_create: dt_ref must be > 0";
    if (c.max_obstacles < 0 || c.max_obstacles > 4096 || (c.max_obstacles > 0 && (c.max_vertices < 1 || c.max_vertices > 64)) || c.max_obstacle_rows > 16)
        return "mpc_create: obstacle capacities out of range (max_obstacles <= 4096, max_vertices <= 64, max_obstacle_rows <= 16)";
    if (c.max_obstacles > 0 && c.footprint_kind != MPC_FOOTPRINT_POINT && c.footprint_kind != MPC_FOOTPRINT_CIRCLE && c.footprint_kind != MPC_FOOTPRINT_LINE &&
        c.footprint_kind != MPC_FOOTPRINT_TWO_CIRCLES && c.footprint_kind != MPC_FOOTPRINT_POLYGON)
        return "mpc_create: unknown footprint model";
    if (c.max_obstacles > 0 && c.footprint_kind == MPC_FOOTPRINT_POLYGON && (c.footprint_n_vertices < 1 || c.footprint_n_vertices > 16))
        return "mpc_create: the polygon footprint needs 1..16 vertices";
    for (int j = 0; j < 2; ++j)
        if (!(c.u_lb[j] < c.u_ub[j])) return "mpc_create: control box must be finite and non-empty";
    if (c.precision != MPC_FP64 && c.precision != MPC_FP32 && c.precision != MPC_MIXED) return "mpc_create: unknown precision";
    if (c.cost_integration != MPC_COST_LEFT_SUM && c.cost_integration != MPC_COST_TRAPEZOIDAL) return "mpc_create: unknown cost_integration";
    if (c.hybrid_cost_minimum_time && c.objective != MPC_OBJ_QUADRATIC) return "mpc_create: hybrid_cost_minimum_time belongs to the quadratic_form objective";
    if (c.n_candidates == 1 && c.candidate_kind[0] != MPC_CAND_REFERENCE)
        return "mpc_create: a single candidate must be MPC_CAND_REFERENCE (other kinds only run as hedges next to it: n_candidates >= 2)";
    if (c.precision == MPC_MIXED && (c.max_obstacles > 0 || c.objective == MPC_OBJ_MIN_TIME_VIA_POINTS))
        return "mpc_create: MPC_MIXED is implemented for problems without clearance rows and via-points (their association would be redone by the refinement phase)";
    if (c.hessian_mode != MPC_HESSIAN_EXACT && c.hessian_mode != MPC_HESSIAN_CONVEXIFIED) return "mpc_create: unknown hessian_mode";
    if (c.mu_strategy != MPC_MU_ADAPTIVE && c.mu_strategy != MPC_MU_MONOTONE) return "mpc_create: unknown mu_strategy";
    if (c.line_search != MPC_LS_DEFAULT && c.line_search != MPC_LS_MERIT && c.line_search != MPC_LS_FILTER) return "mpc_create: unknown line_search";
    if (c.max_time_us < 0) return "mpc_create: max_time_us must be >= 0 (0 = no budget)";
    if (c.n_candidates < 0 || c.n_candidates > MPC_MAX_CANDIDATES) return "mpc_create: n_candidates must be in [0, MPC_MAX_CANDIDATES]";
    for (int k = 0; k < c.n_candidates; ++k)
        if (c.candidate_kind[k] < MPC_CAND_REFERENCE || c.candidate_kind[k] > MPC_CAND_HERMITE_RF || c.candidate_max_iter[k] < 0)
            return "mpc_create: unknown candidate kind or negative candidate_max_iter";
    if (c.dt_free && !(c.dt_lb < c.dt_ub)) return "mpc_create: dt_lb must be below dt_ub on the variable grid";
    if (c.dt_free && !(c.dt_ref >= c.dt_lb && c.dt_ref <= c.dt_ub)) return "mpc_create: dt_ref must lie in [dt_lb, dt_ub] on the variable grid";
    if (c.stage_data != MPC_STAGE_AUTO && c.stage_data != MPC_STAGE_LDS && c.stage_data != MPC_STAGE_GLOBAL) return "mpc_create: unknown stage_data";
    return nullptr;
}

template <typename T>
inline void fill_problem(const mpc_config& c, mpc::Problem<T>& P) {
    P.model = c.model;
    P.n = c.n;
    P.dt_free = c.dt_free ? 1 : 0;
    for (int i = 0; i < 3; ++i) P.xf_fixed[i] = c.xf_fixed[i] ? 1 : 0;
    P.objective = c.objective == MPC_OBJ_MIN_TIME_VIA_POINTS ? MPC_OBJ_MIN_TIME : c.objective;
    P.via = c.objective == MPC_OBJ_MIN_TIME_VIA_POINTS ? 1 : 0;
    P.n_via = P.via ? c.max_via_points : 0;
    P.vp_ordered = c.via_points_ordered ? 1 : 0;
    P.vp_wp = T(c.vp_position_weight);
    P.vp_wo = T(c.vp_orientation_weight);
    P.collocation = c.collocation;
    P.has_Qf = c.has_Qf ? 1 : 0;
    P.max_iter = c.max_iter > 0 ? c.max_iter : 100;
    P.p0 = T(c.model_params[0]);
    P.p1 = T(c.model_params[1]);
    P.dt_ref = T(c.dt_ref);
    P.dt_lb = T(c.dt_lb);
    P.dt_ub = T(c.dt_ub);
    // integral form on the fixed-dt grid (quadratic_cost_se2.cpp:54-83, left sum finite_differences_grid_se2.cpp:61-75): every stage
    // term is multiplied by the constant dt, i.e. the weights are scaled; the terminal cost is not.  (dt free + integral form: see below.)
    const double wsc = (c.integral_form && !c.dt_free) ? c.dt_ref : 1.0;
    // integral form on the variable grid (dt is a decision variable): the weights stay unscaled, the kernel multiplies by the current dt
    // and carries the state-dt / control-dt coupling of the Hessian (wave kernel, A-form slots A05 A15 A25 A56 A57)
    P.integral_form = (c.objective == MPC_OBJ_QUADRATIC && c.integral_form && c.dt_free) ? 1 : 0;
    for (int i = 0; i < 3; ++i) { P.Q[i] = T(c.Q[i] * wsc); P.Qf[i] = T(c.Qf[i]); }
    for (int j = 0; j < 2; ++j) {
        P.R[j] = T(c.R[j] * wsc);
        P.u_lb[j] = T(c.u_lb[j]);
        P.u_ub[j] = T(c.u_ub[j]);
        P.rate_on[j] = c.du_lb[j] > -1e29 ? 1 : 0;
        P.rate_on[2 + j] = c.du_ub[j] < 1e29 ? 1 : 0;
        P.rate_lim[j] = T(P.rate_on[j] ? c.du_lb[j] : 0.0);
        P.rate_lim[2 + j] = T(P.rate_on[2 + j] ? c.du_ub[j] : 0.0);
    }
    const bool f32 = sizeof(T) == 4;
    P.tol = T(c.tol > 0 ? c.tol : (f32 ? 1e-4 : 1e-8));
    P.mu_init = T(c.mu_init > 0 ? c.mu_init : 0.1);
    P.mu_init_warm = T(c.mu_init_warm > 0 ? c.mu_init_warm : (c.mu_init > 0 ? c.mu_init : 0.1));
    P.n_obst = c.max_obstacles > 0 ? c.max_obstacles : 0;
    P.n_vert = c.max_vertices > 0 ? c.max_vertices : 1;
    P.obst_rows = P.n_obst > 0 ? (c.max_obstacle_rows > 0 ? c.max_obstacle_rows : 4) : 0;
    P.footprint_kind = c.footprint_kind;
    P.d_min = T(c.min_obstacle_dist);
    P.force_incl = T(c.force_inclusion_dist);
    P.cutoff = T(c.cutoff_dist);
    P.fp_radius = T(c.footprint_kind == MPC_FOOTPRINT_CIRCLE ? c.footprint_radius : 0.0);
    for (int i = 0; i < 4; ++i) P.fp_line[i] = T(c.footprint_params[i]);
    P.dyn_obst = (c.enable_dynamic_obstacles && c.max_obstacles > 0) ? 1 : 0;
    P.fp_nv = c.footprint_kind == MPC_FOOTPRINT_POLYGON ? (c.footprint_n_vertices < 16 ? c.footprint_n_vertices : 16) : 0;
    for (int i = 0; i < 32; ++i) P.fp_poly[i] = T(i < 2 * P.fp_nv ? c.footprint_vertices[i] : 0.0);
    // TerminalBallSE2 (final_state_conditions_se2.cpp:54-64): the edge exists only with an unfixed final state (finite_differences_grid_se2.cpp:128-143)
    P.ball = (c.terminal_ball && !(c.xf_fixed[0] && c.xf_fixed[1] && c.xf_fixed[2])) ? 1 : 0;
    for (int i = 0; i < 3; ++i) P.ball_S[i] = T(c.terminal_ball_S[i]);
    P.ball_gamma = T(c.terminal_ball_gamma);
    P.n_cand = c.n_candidates > 1 ? (c.n_candidates < MPC_MAX_CANDIDATES ? c.n_candidates : MPC_MAX_CANDIDATES) : 1;
    for (int k = 0; k < 4; ++k) {
        P.cand_kind[k] = (c.n_candidates > 1 && k < P.n_cand) ? c.candidate_kind[k] : MPC_CAND_REFERENCE;
        P.cand_max_iter[k] = (c.n_candidates > 1 && c.candidate_max_iter[k] > 0) ? c.candidate_max_iter[k] : P.max_iter;
        P.cand_param[k] = T((c.n_candidates > 1 && c.candidate_param[k] > 0) ? c.candidate_param[k] : 2.0);
    }
    P.cand_blend = c.candidate_blend > 0 ? c.candidate_blend : 8;
    P.mu_init_dual = T(c.mu_init_dual > 0 ? c.mu_init_dual : 1e-3);
    P.hess_mode = c.hessian_mode == MPC_HESSIAN_CONVEXIFIED ? 1 : 0;
    // ---- cost variants
    const bool quad = c.objective == MPC_OBJ_QUADRATIC;
    P.hybrid = (quad && c.hybrid_cost_minimum_time) ? 1 : 0;
    for (int i = 0; i < 3; ++i) { P.Qo[i] = T(quad ? c.Q_offdiag[i] * wsc : 0.0); P.Qfo[i] = T(c.has_Qf ? c.Qf_offdiag[i] : 0.0); P.So[i] = T(c.terminal_ball_S_offdiag[i]); }
    P.Ro = T(quad ? c.R_offdiag * wsc : 0.0);
    const bool trapezoid = quad && c.integral_form && c.cost_integration == MPC_COST_TRAPEZOIDAL;
    // trapezoidal rule (finite_differences_grid_se2.cpp:63-68): every interval gives half of its state cost to either end, so against the left
    // sum x_0 loses half a term (a constant on the fixed grid: x_0 is not a variable) and the FINAL state gains 0.5 dt xd' Q xd.
    // Fixed grid: that is a terminal cost with weights 0.5 dt_ref Q on top of Qf.  Variable grid: handled in the kernel (P.trapz).
    P.trapz = (trapezoid && c.dt_free) ? 1 : 0;
    if (trapezoid && !c.dt_free) {
        for (int i = 0; i < 3; ++i) {
            P.Qf[i] = T((c.has_Qf ? c.Qf[i] : 0.0) + 0.5 * c.dt_ref * c.Q[i]);
            P.Qfo[i] = T((c.has_Qf ? c.Qf_offdiag[i] : 0.0) + 0.5 * c.dt_ref * c.Q_offdiag[i]);
        }
        P.has_Qf = 1;
    } else if (!c.has_Qf) {
        for (int i = 0; i < 3; ++i) P.Qf[i] = T(0);
    }
    P.pit = 1;
    P.pit_mu_min = P.tol > T(1e-6) ? P.tol : T(1e-6);      // the barrier subproblems below max(tol, 1e-6) are solved with the serial sweeps (measured: mpc_wave.hpp, pit_floor)
    P.acc_tol = T(c.acceptable_tol > 0 ? c.acceptable_tol : (c.acceptable_tol < 0 ? 0.0 : 1e-6));
    P.acc_iter = c.acceptable_iter > 0 ? c.acceptable_iter : (c.acceptable_iter < 0 ? 0 : 15);
    P.max_ticks = c.max_time_us > 0 ? 100ll * c.max_time_us : 0ll;
    P.mu_strategy = c.mu_strategy == MPC_MU_MONOTONE ? 1 : 0;
    P.line_search = c.line_search == MPC_LS_DEFAULT ? kDefaultLineSearch : (c.line_search == MPC_LS_FILTER ? 1 : 0);
    P.costx = (P.trapz || P.Ro != T(0)) ? 1 : 0;
    for (int i = 0; i < 3; ++i) if (P.Qo[i] != T(0) || P.Qfo[i] != T(0) || (P.ball && P.So[i] != T(0))) P.costx = 1;
}

// The two records a handle launches with (the fp64 one for MPC_FP64 and the refinement phase of MPC_MIXED, the fp32 one for MPC_FP32 and the main
// phase of MPC_MIXED), padding zeroed: what mpc_create keeps for the handle's own configuration and mpc_set_parameter_sets builds for every set.
inline void fill_records(const mpc_config& c, Problem<double>& P64, Problem<float>& P32) {
    std::memset(&P64, 0, sizeof(P64));
    std::memset(&P32, 0, sizeof(P32));
    fill_problem<double>(c, P64);
    fill_problem<float>(c, P32);
#ifdef MPC_DEV_SWITCHES      // developer A/B switches read from the environment: compiled out of the shipped library
    if (const char* e = getenv("MPC_NO_PIT")) { if (e[0] == '1') { P64.pit = 0; P32.pit = 0; } }      // serial sweeps only
    if (const char* e = getenv("MPC_PIT_MU")) { char* end = nullptr; const double v = strtod(e, &end); if (end != e && v >= 0) { P64.pit_mu_min = v; P32.pit_mu_min = (float)v; } }      // threshold of the partitioned sweeps
#endif
    if (c.precision == MPC_MIXED) {
        P32.tol = 1e-4f; P32.pit_mu_min = 1e-4f;             // phase 1 stops where fp32 residuals stop making sense
        P64.n_cand = 1;                                      // phase 2 refines the winner
        if (!(c.mu_init_dual > 0)) P64.mu_init_dual = 1e-5;  // phase 1 ended at a barrier of ~1e-5
        P64.mu_init_warm = 1e-3;                             // instances phase 1 did not converge start phase 2 from its last iterate
        P64.mu_strategy = 1;                                 // the refinement follows the central path from mu = 1e-5 down: the monotone rule (fewer refinement iterations than
                                                             // the adaptive one, which re-derives mu from the fp32 iterate's complementarity: CHANGELOG.md)
        if (P64.max_iter > 40) P64.max_iter = 40;            // a refinement that needs more than that is a solve of its own (phase-1 failures would hold the launch for 100)
    }
}

// the integer fields of a record: what selects rows, terms, iteration caps and the kernel (a parameter set must leave every one of them as the handle has it)
template <typename T>
inline bool same_structure(const Problem<T>& a, const Problem<T>& b) {
    auto eq = [](const auto& x, const auto& y) { return std::memcmp(&x, &y, sizeof(x)) == 0; };
    return eq(a.model, b.model) && eq(a.n, b.n) && eq(a.dt_free, b.dt_free) && eq(a.xf_fixed, b.xf_fixed) && eq(a.objective, b.objective) &&
           eq(a.integral_form, b.integral_form) && eq(a.collocation, b.collocation) && eq(a.has_Qf, b.has_Qf) && eq(a.rate_on, b.rate_on) &&
           eq(a.max_iter, b.max_iter) && eq(a.n_obst, b.n_obst) && eq(a.n_vert, b.n_vert) && eq(a.obst_rows, b.obst_rows) &&
           eq(a.footprint_kind, b.footprint_kind) && eq(a.dyn_obst, b.dyn_obst) && eq(a.fp_nv, b.fp_nv) && eq(a.ball, b.ball) && eq(a.via, b.via) &&
           eq(a.n_via, b.n_via) && eq(a.vp_ordered, b.vp_ordered) && eq(a.n_cand, b.n_cand) && eq(a.cand_kind, b.cand_kind) &&
           eq(a.cand_max_iter, b.cand_max_iter) && eq(a.cand_blend, b.cand_blend) && eq(a.hess_mode, b.hess_mode) && eq(a.trapz, b.trapz) &&
           eq(a.hybrid, b.hybrid) && eq(a.costx, b.costx) && eq(a.acc_iter, b.acc_iter) && eq(a.line_search, b.line_search) && eq(a.pit, b.pit) &&
           eq(a.mu_strategy, b.mu_strategy) && eq(a.max_ticks, b.max_ticks);
}

// The int32_t fields of mpc_config, in declaration order: a parameter set (mpc_set_parameter_sets) has to repeat every one of them.
#define MPC_CONFIG_INT_FIELDS(X)                                                                                                                                   \
    X(model) X(n) X(dt_free) X(xf_fixed) X(collocation) X(objective) X(integral_form) X(has_Qf) X(max_iter) X(precision) X(footprint_kind) X(max_obstacles)    \
    X(max_vertices) X(max_obstacle_rows) X(terminal_ball) X(via_points_ordered) X(max_via_points) X(footprint_n_vertices) X(enable_dynamic_obstacles)          \
    X(n_candidates) X(candidate_kind) X(candidate_max_iter) X(candidate_blend) X(dual_warm_start) X(hessian_mode) X(hybrid_cost_minimum_time)                 \
    X(cost_integration) X(mu_strategy) X(stage_data) X(two_wave_min_batch) X(line_search) X(acceptable_iter) X(max_time_us)

// Why a handle created with `handle` cannot solve instances with the parameter set `set` in the same launch (mpc_set_parameter_sets), or "" when it can.
// A set may change the double fields of mpc_config and nothing that selects the kernel: every int32_t field equals the handle's, and so do the two
// switches derived from doubles -- which control-rate bounds are finite (they switch rows on) and whether the off-diagonal cost terms are all zero (they
// select the kernel level).  Then the integer fields of both records and the launch plan come out as the handle's (checked last, as a backstop).
inline std::string parameter_set_error(const mpc_config& handle, const mpc_config& set) {
    auto field = [](const char* name, int count, int i) { return count > 1 ? std::string(name) + "[" + std::to_string(i) + "]" : std::string(name); };
#define MPC_SET_CHECK_INT(f)                                                                                                                                       \
    {                                                                                                                                                              \
        const int32_t* a = reinterpret_cast<const int32_t*>(&handle.f);                                                                                        \
        const int32_t* b = reinterpret_cast<const int32_t*>(&set.f);                                                                                           \
        const int cnt = (int)(sizeof(handle.f) / sizeof(int32_t));                                                                                             \
        for (int i = 0; i < cnt; ++i)                                                                                                                             \
            if (a[i] != b[i])                                                                                                                                     \
                return field(#f, cnt, i) + " is " + std::to_string(b[i]) + " here and " + std::to_string(a[i]) + " in the handle's configuration";            \
    }
    MPC_CONFIG_INT_FIELDS(MPC_SET_CHECK_INT)
#undef MPC_SET_CHECK_INT
    if (const char* why = config_error(set)) return std::strncmp(why, "mpc_create: ", 12) == 0 ? std::string(why + 12) : std::string(why);
    for (int j = 0; j < 2; ++j) {
        const bool hl = handle.du_lb[j] > -1e29, sl = set.du_lb[j] > -1e29, hu = handle.du_ub[j] < 1e29, su = set.du_ub[j] < 1e29;
        auto fin = [](bool f) { return f ? "finite" : "infinite"; };
        if (hl != sl) return field("du_lb", 2, j) + " is " + fin(sl) + " here and " + fin(hl) + " in the handle's configuration";
        if (hu != su) return field("du_ub", 2, j) + " is " + fin(su) + " here and " + fin(hu) + " in the handle's configuration";
    }
    Problem<double> h64, s64;
    Problem<float> h32, s32;
    fill_records(handle, h64, h32);
    fill_records(set, s64, s32);
    if (h64.costx != s64.costx || h32.costx != s32.costx) {
        const double* terms[4] = {set.Q_offdiag, &set.R_offdiag, set.Qf_offdiag, set.terminal_ball_S_offdiag};
        const char* names[4] = {"Q_offdiag", "R_offdiag", "Qf_offdiag", "terminal_ball_S_offdiag"};
        const int cnt[4] = {3, 1, 3, 3};
        if (s64.costx)
            for (int t = 0; t < 4; ++t)
                for (int i = 0; i < cnt[t]; ++i)
                    if (terms[t][i] != 0.0) return field(names[t], cnt[t], i) + " is non-zero here and every off-diagonal cost term is zero in the handle's configuration";
        return "the off-diagonal cost terms are all zero here and not in the handle's configuration (they select the kernel level)";
    }
    if (!same_structure(h64, s64) || !same_structure(h32, s32)) return "the integer fields of its problem record differ from the handle's";
    return std::string();
}

// Consecutive pieces of one block at 256-byte aligned offsets: take(bytes) is where the next piece starts, `off` the bytes taken so far (a multiple of 256).
struct Packer {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t at = off; off = (off + bytes + 255) & ~(size_t)255; return at; }
};

// The pieces of one host-pointer call (mpc_solve_batch / mpc_step_batch) in the handle's two staging blocks: the inputs up to N_IN in the block that goes to the
// device in one copy, the outputs behind them in the block that comes back in one copy.  bytes[i] = 0: the call has no such piece (an optional array the caller
// left out, obstacle arrays of a handle without obstacles, velocities without enable_dynamic_obstacles).  mpc_create sizes the blocks with the same function, at
// max_batch and every optional piece present: a piece only grows with B, so no call packs more (tests/test_step_pieces.py).
struct StepPieces {
    enum { X0, XF, U_PREV, DT_PREV, X_INIT, U_INIT, DT_INIT, N_OBSTACLES, N_VERTICES, VERTICES, RADIUS, VELOCITY, N_IN,
           X_OUT = N_IN, U_OUT, DT_OUT, STATUS, ITERS, N_GRID, N_PIECES };
    size_t bytes[N_PIECES], off[N_PIECES];
    size_t in_bytes, out_bytes;      // what the two copies move
};
inline StepPieces step_pieces(const mpc_config& c, size_t B, bool u_prev, bool dt_prev, bool init, bool radius, bool velocity) {
    const size_t n = (size_t)c.n, O = c.max_obstacles > 0 ? (size_t)c.max_obstacles : 0, V = c.max_vertices > 0 ? (size_t)c.max_vertices : 1;
    const size_t per_instance[StepPieces::N_PIECES] = {
        24, 24, u_prev ? 16u : 0u, dt_prev ? 8u : 0u, init ? n * 24 : 0, init ? n * 16 : 0, init ? 8u : 0u,                                      // x0 xf u_prev dt_prev | x_init u_init dt_init
        O ? 4u : 0u, O * 4, O * V * 16, radius ? O * 8 : 0, velocity && c.enable_dynamic_obstacles ? O * 16 : 0,                             // n_obstacles n_vertices vertices radius velocity
        n * 24, n * 16, 8, 4, 4, 4};                                                                                                           // x_out u_out dt_out status iters n_grid
    StepPieces p{};
    Packer in, out;
    for (int i = 0; i < StepPieces::N_PIECES; ++i) {
        p.bytes[i] = B * per_instance[i];
        p.off[i] = p.bytes[i] ? (i < StepPieces::N_IN ? in : out).take(p.bytes[i]) : 0;
    }
    p.in_bytes = in.off; p.out_bytes = out.off;
    return p;
}

// The pieces of any other host-pointer call (staged_call of mpc_capi.hip) in ONE block that exists once in pinned host memory and once on the device.  A piece is an
// array of the caller's: STAGE_IN goes to the device only (src), STAGE_OUT comes back only (dst), STAGE_INOUT goes and comes back (src and dst, as a rule the same
// array: what a kernel leaves alone returns as it was).  A piece without its pointer(s) or of zero bytes is absent: no room, no device address.  Whatever order the
// caller lists them in, the block holds IN | INOUT | OUT, so that ONE copy [0, h2d_bytes) takes every input over and ONE copy [d2h_begin, d2h_begin + d2h_bytes)
// brings every output back; neither moves the padding behind its last piece.  tests/test_stage_pieces.py walks piece lists through it.
enum StageDir { STAGE_IN, STAGE_INOUT, STAGE_OUT };
struct StagePiece { const void* src; void* dst; size_t bytes; int dir; };
struct StageLayout {
    enum { MAX_PIECES = 24 };
    size_t off[MAX_PIECES];       // 256-byte aligned, 0 for an absent piece
    bool present[MAX_PIECES];
    size_t bytes;                 // the end of the last piece: what either block has to hold
    size_t h2d_bytes, d2h_begin, d2h_bytes;
    void* at(void* base, int i) const { return present[i] ? (char*)base + off[i] : nullptr; }      // piece i in a block at `base`, NULL for an absent one
};
inline StageLayout stage_layout(const StagePiece* pc, int count) {
    StageLayout L{};
    Packer pk;
    size_t in_end = 0;
    for (int dir = STAGE_IN; dir <= STAGE_OUT; ++dir) {
        for (int i = 0; i < count; ++i) {
            const StagePiece& p = pc[i];
            if (p.dir != dir || !p.bytes || (dir != STAGE_OUT && !p.src) || (dir != STAGE_IN && !p.dst)) continue;
            L.present[i] = true;
            L.off[i] = pk.take(p.bytes);
            L.bytes = L.off[i] + p.bytes;
        }
        if (dir == STAGE_IN) { in_end = L.bytes; L.d2h_begin = pk.off; }
        if (dir == STAGE_INOUT) L.h2d_bytes = L.bytes;
    }
    if (L.bytes > in_end) L.d2h_bytes = L.bytes - L.d2h_begin; else L.d2h_begin = 0;      // (nothing comes back: an empty range at 0)
    return L;
}


}  // namespace mpc
