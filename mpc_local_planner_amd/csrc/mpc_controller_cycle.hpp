// mpc_controller_cycle.hpp -- what Controller::step runs AROUND the solve (reference src/controller.cpp:111-179), per planner instance and for a whole
// batch on the device: the state estimate (:131-149), the re-initialisation decision (:152-158), the initial trajectory from the plan
// (generateInitialStateTrajectory, :807-857, sampled as initializeSequences(xinit) does, full_discretization_grid_base_se2.cpp:192-239) and the grid
// update of a slot that is not re-initialised (mpc_grid_update.hpp).  include/mpc_controller.hpp has the same logic on the host for one robot; this file
// restates it as __host__ __device__ functions -- the CPU suite compiles them with g++ (tests/host_harness/controller_cycle_host.cpp) and holds them to the
// facade and to the numpy restatement (oracle/se2_nlp.py) bit for bit -- and as controller_prepare_kernel, which mpc_controller_step_batch_device launches in front of the solve.
//
// All double arithmetic is un-fused and uses +, -, *, /, sqrt and floor only, which round the same way on the host and on gfx950; so host and device agree
// bit for bit.  The one exception is the one transcendental of the cycle, the atan2 that estimates the yaw of an intermediate plan pose (:838-840): the facade and
// the oracle call the host's libm, whose atan2 no device routine can reproduce where it is not correctly rounded (glibc 2.35: 1 ulp off in 0.08 % of random
// arguments, tests/test_controller_cycle_host.py).  The device computes it in double-double arithmetic and rounds once (cc_atan2: the correctly rounded value, held to
// a 200-bit evaluation by the CPU suite); the host build calls libm like the facade unless it is asked for the device's routine (cc_yaw).
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MPC_CC_HD __host__ __device__ __forceinline__
#else
#define MPC_CC_HD inline
#endif

namespace mpc {

// what reinit_out[b] of mpc_controller_step_batch* reports (MPC_REINIT_* of include/mpc_hip.h): 0 = warm start from the slot's previous solution
enum { CC_FIRST = 1, CC_NUM_STEPS = 2, CC_GOAL_DIST = 4, CC_GOAL_ANGULAR = 8, CC_RESET = 16, CC_PLAN_GUESS = 32 };

// ---- double-double arithmetic (Dekker / Knuth, no fused multiply-add), enough for one atan2
struct cc_dd { double h, l; };
MPC_CC_HD cc_dd cc_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b; const double bb = s - a; const double e = (a - (s - bb)) + (b - bb);
    return {s, e};
}
MPC_CC_HD cc_dd cc_quick_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b; const double e = b - (s - a);
    return {s, e};
}
MPC_CC_HD cc_dd cc_two_prod(double a, double b) {
#pragma clang fp contract(off)
    const double p = a * b;
    const double ta = 134217729.0 * a; const double ah = ta - (ta - a); const double al = a - ah;
    const double tb = 134217729.0 * b; const double bh = tb - (tb - b); const double bl = b - bh;
    const double e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;
    return {p, e};
}
MPC_CC_HD cc_dd cc_add(cc_dd a, cc_dd b) {
#pragma clang fp contract(off)
    cc_dd s = cc_two_sum(a.h, b.h); const cc_dd t = cc_two_sum(a.l, b.l);
    s.l = s.l + t.h; s = cc_quick_two_sum(s.h, s.l);
    s.l = s.l + t.l; return cc_quick_two_sum(s.h, s.l);
}
MPC_CC_HD cc_dd cc_neg(cc_dd a) { return {-a.h, -a.l}; }
MPC_CC_HD cc_dd cc_mul(cc_dd a, cc_dd b) {
#pragma clang fp contract(off)
    cc_dd p = cc_two_prod(a.h, b.h);
    const double c1 = a.h * b.l; const double c2 = a.l * b.h;
    p.l = p.l + (c1 + c2);
    return cc_quick_two_sum(p.h, p.l);
}
MPC_CC_HD cc_dd cc_div(cc_dd a, cc_dd b) {
#pragma clang fp contract(off)
    const double q1 = a.h / b.h;
    cc_dd r = cc_add(a, cc_neg(cc_mul(b, {q1, 0.0})));
    const double q2 = r.h / b.h;
    r = cc_add(r, cc_neg(cc_mul(b, {q2, 0.0})));
    const double q3 = r.h / b.h;
    const cc_dd q = cc_quick_two_sum(q1, q2);
    return cc_add(q, {q3, 0.0});
}

// atan2(y, x) for finite arguments of ordinary size (|.| < 1e150, differences of plan coordinates): min / max of the magnitudes, the nearest of atan(k / 8), the
// remainder by its Taylor series (|r| <= 1/16: 14 terms), all in double-double (~100 bits), then one rounding.  Signed zeros as IEEE atan2; NaN in, NaN out.
MPC_CC_HD double cc_atan2(double y, double x) {
#pragma clang fp contract(off)
    const cc_dd kAtan[9] = {{0x0.0p+0, 0x0.0p+0}, {0x1.fd5ba9aac2f6ep-4, -0x1.cd37686760c17p-59}, {0x1.f5b75f92c80ddp-3, 0x1.8ab6e3cf7afbdp-57},
                            {0x1.6f61941e4def1p-2, -0x1.c63aae6f6e918p-56}, {0x1.dac670561bb4fp-2, 0x1.a2b7f222f65e2p-56}, {0x1.1e00babdefeb4p-1, -0x1.928df287a668fp-58},
                            {0x1.4978fa3269ee1p-1, 0x1.2419a87f2a458p-56}, {0x1.700a7c5784634p-1, -0x1.8c34d25aadef6p-56}, {0x1.921fb54442d18p-1, 0x1.1a62633145c07p-55}};
    const cc_dd kPi = {0x1.921fb54442d18p+1, 0x1.1a62633145c07p-53}, kPi2 = {0x1.921fb54442d18p+0, 0x1.1a62633145c07p-54};
    if (x != x || y != y) return x + y;
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const bool xneg = __builtin_signbit(x), yneg = __builtin_signbit(y);
    cc_dd a = {0.0, 0.0};
    if (ax == 0.0 && ay == 0.0) {
        a = xneg ? kPi : a;
    } else {
        const bool swap = ay > ax;
        const cc_dd q = cc_div({swap ? ax : ay, 0.0}, {swap ? ay : ax, 0.0});      // in [0, 1]
        const int k = (int)(q.h * 8.0 + 0.5);
        const double c = (double)k / 8.0;
        const cc_dd r = cc_div(cc_add(q, {-c, 0.0}), cc_add({1.0, 0.0}, cc_mul(q, {c, 0.0})));
        const cc_dd r2 = cc_mul(r, r);
        cc_dd s = cc_div({1.0, 0.0}, {27.0, 0.0});
        for (int j = 12; j >= 0; --j) s = cc_add(cc_div({1.0, 0.0}, {(double)(2 * j + 1), 0.0}), cc_neg(cc_mul(r2, s)));
        a = cc_add(kAtan[k], cc_mul(r, s));
        if (swap) a = cc_add(kPi2, cc_neg(a));
        if (xneg) a = cc_add(kPi, cc_neg(a));
    }
    const double res = a.h + a.l;
    return yneg ? -res : res;
}

// the yaw estimate: on the device cc_atan2; in the host build the host's atan2, as the facade and the oracle, unless device_routine
MPC_CC_HD double cc_yaw(double y, double x, bool device_routine) {
#if !defined(__HIP_DEVICE_COMPILE__)
    if (!device_routine) return ::atan2(y, x);
#endif
    (void)device_routine;
    return cc_atan2(y, x);
}

// include/mpc_local_planner/utils/math_utils.h:81-103
MPC_CC_HD double cc_normalize_theta(double th) {
#pragma clang fp contract(off)
    const double pi = 3.14159265358979323846;
    if (th >= -pi && th < pi) return th;
    double m = __builtin_floor(th / (2.0 * pi));
    th = th - m * 2.0 * pi;
    if (th >= pi) th -= 2.0 * pi;
    if (th < -pi) th += 2.0 * pi;
    return th;
}

// State estimate, src/controller.cpp:131-149: a state measurement younger than two controller periods wins when controller/prefer_x_feedback is set;
// otherwise the odometry pose (the plan's first pose) overwrites the whole state, for every model of the package (BaseRobotSE2::mergeStateFeedbackAndOdomFeedback,
// include/mpc_local_planner/systems/base_robot_se2.h:93-101; include/mpc_controller.hpp, stateFeedbackCallback, has the reasoning).
MPC_CC_HD void cc_state_estimate(const double* plan_first, const double* x_feedback, const double* feedback_age, int b, int prefer_x_feedback, double period, double x0[3]) {
#pragma clang fp contract(off)
    const bool use_fb = prefer_x_feedback && x_feedback && feedback_age && feedback_age[b] < 2.0 * period;
    for (int i = 0; i < 3; ++i) x0[i] = use_fb ? x_feedback[3 * b + i] : plan_first[i];
}

// Re-initialisation decision, src/controller.cpp:152-158: which causes hold (CC_* bits, 0 = none: the slot keeps its previous solution).  `live`: the slot
// has stepped since it was created / since mpc_reset; the goal tests are made on a live slot only (an empty one has no last goal to compare with).
MPC_CC_HD int cc_reinit_causes(int live, int seq, int reset, const double goal[3], const double last_goal[3], int force_reinit_num_steps, double new_goal_dist,
                               double new_goal_angular) {
#pragma clang fp contract(off)
    int c = 0;
    if (!live) c |= CC_FIRST;
    if (reset) c |= CC_RESET;
    if (force_reinit_num_steps > 0 && seq % force_reinit_num_steps == 0) c |= CC_NUM_STEPS;
    if (live) {
        const double dx = goal[0] - last_goal[0], dy = goal[1] - last_goal[1];
        const double qx = dx * dx, qy = dy * dy;
        if (__builtin_sqrt(qx + qy) > new_goal_dist) c |= CC_GOAL_DIST;
        if (__builtin_fabs(cc_normalize_theta(goal[2] - last_goal[2])) > new_goal_angular) c |= CC_GOAL_ANGULAR;
    }
    return c;
}

// The spacing a re-initialised slot's plan is sampled at: the reference samples at the grid's CURRENT dt (full_discretization_grid_base_se2.cpp:61-65), which
// clear() does not put back to dt_ref (:526-536) -- so, on the variable grid, the last optimised dt of a slot that has solved before (include/mpc_controller.hpp,
// setReferenceReinitSampling).
MPC_CC_HD double cc_dt_sample(int reference_reinit_sampling, int has_solution, int dt_free, double dt_solution, double dt_ref) {
    return (reference_reinit_sampling && has_solution && dt_free && dt_solution > 0.0) ? dt_solution : dt_ref;
}

// generateInitialStateTrajectory, src/controller.cpp:807-857: the time stamps of the np poses, equally spaced over (n_ref - 1) dt_ref and ACCUMULATED (t += dt_init, :843)
MPC_CC_HD void cc_plan_times(int np, int n_ref, double dt_ref, double* times) {
#pragma clang fp contract(off)
    const double tf = (double)(n_ref - 1) * dt_ref;
    const double dt_init = tf / (double)(np - 1);
    times[0] = 0.0;
    double t = dt_init;
    for (int i = 1; i < np - 1; ++i) { times[i] = t; t += dt_init; }
    times[np - 1] = tf;
}
// ... and pose i of the time series: the state estimate, the goal, and in between the plan's pose with its yaw from the direction to the next pose when
// controller/initial_plan_estimate_orientation is set (:838-840; the `backward` flip of :841 is discarded by the reference and so here)
MPC_CC_HD void cc_plan_value(const double* plan, int np, int i, const double x0[3], const double xf[3], int estimate_orientation, double out[3], bool device_yaw = false) {
#pragma clang fp contract(off)
    if (i == 0 || i == np - 1) { for (int c = 0; c < 3; ++c) out[c] = i == 0 ? x0[c] : xf[c]; return; }
    out[0] = plan[3 * i]; out[1] = plan[3 * i + 1]; out[2] = plan[3 * i + 2];
    if (estimate_orientation) out[2] = cc_yaw(plan[3 * (i + 1) + 1] - plan[3 * i + 1], plan[3 * (i + 1)] - plan[3 * i], device_yaw);
}
// TimeSeriesSE2::getValuesInterpolate, linear with zero-order hold beyond the end (src/utils/time_series_se2.cpp:34-111)
MPC_CC_HD void cc_interpolate_se2(const double* times, const double* vals, int np, double t, double out[3]) {
#pragma clang fp contract(off)
    int idx = -1;
    for (int i = 0; i < np; ++i) if (times[i] >= t) { idx = i; break; }
    if (idx < 0) { for (int c = 0; c < 3; ++c) out[c] = vals[3 * (np - 1) + c]; return; }
    if (__builtin_fabs(t - times[idx]) < 1e-6 || idx < 1) { for (int c = 0; c < 3; ++c) out[c] = vals[3 * idx + c]; return; }
    const double fr = (t - times[idx - 1]) / (times[idx] - times[idx - 1]);
    for (int c = 0; c < 2; ++c) { const double d = vals[3 * idx + c] - vals[3 * (idx - 1) + c]; const double w = fr * d; out[c] = vals[3 * (idx - 1) + c] + w; }
    const double a1 = vals[3 * (idx - 1) + 2];
    const double w = cc_normalize_theta(vals[3 * idx + 2] - a1); const double fw = fr * w;
    out[2] = cc_normalize_theta(a1 + fw);
}
// row k of the guess of a re-initialised slot, initializeSequences(xinit) (full_discretization_grid_base_se2.cpp:192-239): x_0 and the goal exact, in between
// the time series at k * dt_sample
MPC_CC_HD void cc_guess_row(const double* times, const double* vals, int np, int k, int n_ref, double dt_sample, const double x0[3], const double xf[3], double out[3]) {
#pragma clang fp contract(off)
    if (k == 0 || k == n_ref - 1) { for (int c = 0; c < 3; ++c) out[c] = k == 0 ? x0[c] : xf[c]; return; }
    cc_interpolate_se2(times, vals, np, (double)k * dt_sample, out);
}

#if defined(__HIPCC__)
}  // namespace mpc
#include "mpc_grid_update.hpp"
namespace mpc {

struct CycleArgs {
    // the caller's inputs
    const double* plan;            // [B][plan_stride][3]
    const int32_t* n_plan;         // [B] poses of instance b (clamped to [2, plan_stride])
    int32_t plan_stride;
    const double* x_feedback;      // [B][3] or NULL
    const double* feedback_age;    // [B] or NULL
    const int32_t* reset;          // [B] or NULL
    // mpc_cycle_params
    int32_t n_ref, warm_start, force_reinit_num_steps, estimate_orientation, prefer_x_feedback, reference_reinit_sampling, dt_free, update;
    double new_goal_dist, new_goal_angular, period;
    // the handle's slot state
    int32_t *seq, *live, *has_solution;
    double* last_goal;             // [B][3]
    // what the solve launch reads
    double *x0, *xf;               // [B][3]
    int32_t* init_mode;            // [B] 0: cold start on the device, else: the guess in the slot's arrays
    int32_t* reinit_out;           // [B] CC_* bits or NULL
    GridUpdateArgs g;              // the slot arrays x / u / dt / n_grid, dt_refs / set_of, the kept multipliers; x0 = this struct's x0
};

// One 64-lane workgroup per instance.  Dynamic LDS: 5 n_stride doubles (the trajectory, grid_update_instance) | 4 plan_stride doubles (times, poses of the plan).
__global__ __launch_bounds__(64) void controller_prepare_kernel(CycleArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double csm[];
    __shared__ int s_mode, s_np;
    __shared__ double s_x0[3], s_xf[3], s_dt_sample, s_dt_ref;
    const int b = blockIdx.x, lane = threadIdx.x, ns = a.g.n_stride;
    const double* plan = a.plan + (size_t)b * a.plan_stride * 3;
    if (lane == 0) {
        int np = a.n_plan[b];
        np = np < 2 ? 2 : (np > a.plan_stride ? a.plan_stride : np);
        double x0[3], xf[3], lg[3];
        cc_state_estimate(plan, a.x_feedback, a.feedback_age, b, a.prefer_x_feedback, a.period, x0);      // :131-149
        for (int i = 0; i < 3; ++i) { xf[i] = plan[3 * (np - 1) + i]; lg[i] = a.last_goal[3 * b + i]; }       // the goal is the plan's last pose (:113)
        const int live = a.live[b], seq = a.seq[b], rs = a.reset ? a.reset[b] : 0;
        int causes = cc_reinit_causes(live, seq, rs, xf, lg, a.force_reinit_num_steps, a.new_goal_dist, a.new_goal_angular);      // :152-158
        if (rs && a.g.dual) a.g.dual[(size_t)b * a.g.dual_words] = 0.0;      // Controller::reset(): the slot's kept multipliers go (the facade's reset() is mpc_reset on its own handle)
        int mode = 2;
        if (causes) {
            a.g.n_grid[b] = a.n_ref;
            const double dt_ref = a.g.dt_refs[a.g.set_of ? a.g.set_of[b] : 0];      // the instance's own dt_ref
            const double dt_sample = cc_dt_sample(a.reference_reinit_sampling, a.has_solution[b], a.dt_free, a.g.dt[b], dt_ref);
            mode = (np > 2 || dt_sample != dt_ref) ? 1 : 0;      // a 2-pose plan sampled at dt_ref is the device-side cold start
            if (mode == 1) causes |= CC_PLAN_GUESS;
            s_dt_sample = dt_sample; s_dt_ref = dt_ref;
        }
        for (int i = 0; i < 3; ++i) { s_x0[i] = x0[i]; s_xf[i] = xf[i]; a.x0[3 * b + i] = x0[i]; a.xf[3 * b + i] = xf[i]; a.last_goal[3 * b + i] = xf[i]; }
        a.seq[b] = seq + 1; a.live[b] = 1; a.has_solution[b] = 1;      // :165 ++_ocp_seq, :166 _last_goal; the solve follows on the stream
        a.init_mode[b] = mode;
        if (a.reinit_out) a.reinit_out[b] = causes;
        s_mode = mode; s_np = np;
    }
    __syncthreads();
    const int mode = s_mode;
    if (mode == 2) {
        // not re-initialised: the grid update of the previous solution, in place (fixed grid: warmStartShifting when grid/warm_start is set; variable grid: adaptation +
        // resampling when grid_adaptation is on)
        // (the fixed grid's shift leaves the kept multipliers in place, as the host-side shift of include/mpc_controller.hpp does: their block is hidden from it)
        if (a.update) {
            GridUpdateArgs g = a.g;
            if (g.mode == 0) g.dual = nullptr;
            grid_update_instance(g, b, csm);
        }
        return;
    }
    if (mode == 0) return;
    // the guess from the plan into the slot's arrays
    const int np = s_np, n = a.n_ref;
    double* times = csm + 5 * ns;
    double* vals = times + a.plan_stride;
    if (lane == 0) cc_plan_times(np, n, s_dt_ref, times);
    for (int i = lane; i < np; i += 64) cc_plan_value(plan, np, i, s_x0, s_xf, a.estimate_orientation, &vals[3 * i]);
    __syncthreads();
    double* x = a.g.x + (size_t)b * ns * 3;
    double* u = a.g.u + (size_t)b * ns * 2;
    for (int k = lane; k < n; k += 64) {
        double row[3];
        cc_guess_row(times, vals, np, k, n, s_dt_sample, s_x0, s_xf, row);
        x[3 * k] = row[0]; x[3 * k + 1] = row[1]; x[3 * k + 2] = row[2];
        u[2 * k] = 0.0; u[2 * k + 1] = 0.0;
    }
    if (lane == 0) a.g.dt[b] = s_dt_ref;
}

#endif  // __HIPCC__

}  // namespace mpc
