// mpc_plan_inputs.hpp -- what the reference's plugin does AROUND Controller::step in MpcLocalPlannerROS::computeVelocityCommands (src/mpc_local_planner_ros.cpp:264-461),
// per planner instance and for a whole batch on the device.  Before the step: pruneGlobalPlan (:645-685), transformGlobalPlan (:687-805), updateViaPointsContainer
// (:619-635), the goal-reached test (:312-322), estimateLocalGoalOrientation (:807-852) and the start / goal overwrite of the local plan (:332-354) -- plan_inputs_kernel,
// behind mpc_plan_inputs_batch*.  After the step: what the solve status and the feasibility flag do to the command (:394-452), the controller reset that follows a
// failure and the previous control of the next cycle (:384) -- commands_kernel, behind mpc_commands_batch*.  include/mpc_controller.hpp has the same functions on the host
// for one robot (prune_global_plan, transform_global_plan, via_points_from_plan, estimate_local_goal_orientation).
//
// The global plan of instance b is [gstride][3] poses (x, y, theta) ALREADY IN THE PLANNING FRAME, as transform_global_plan of the facade takes it: the planar transform
// plan -> planning frame is the identity, (yaw, tx, ty) = 0 in estimate_local_goal_orientation, and the robot pose is given in that same frame.
//
// The logic is written as __host__ __device__ functions: un-fused double arithmetic with +, -, *, /, sqrt and floor only, plus the correctly rounded atan2 in double-double of
// mpc_controller_cycle.hpp (cc_atan2, restated as pi_atan2 below so that the kernel needs no scratch), so that a g++ build (tests/host_harness/plan_inputs_host.cpp) and gfx950 agree bit for bit.  pi_instance is the per-instance
// statement in the reference's own loop order; plan_inputs_kernel restates its three scans lane-parallel over chunks of 64 poses and computes the same bits.
//
// Ours, not the reference's:
//   * a selection longer than plan_stride keeps its first plan_stride - 1 poses and its last one, and sets PI_PLAN_TRUNCATED (the reference's vector has no capacity);
//   * more via-points than cfg.max_via_points: the first ones are kept and PI_VIA_DROPPED is set (the greedy walk itself goes on as in the reference);
//   * an empty global plan (n_global - begin < 1; the reference returns INTERNAL_ERROR / INVALID_PATH without a step) yields n_plan = 2 with both poses the robot pose, so
//     that a controller step that follows is harmless, and PI_PLAN_EMPTY;
//   * a direction's cosine and sine are dx / r and dy / r, (1, 0) when r == 0 (libm: atan2(0, 0) = 0), in place of cos(atan2(dy, dx)) and sin(atan2(dy, dx)); near the end of
//     the plan the last pose's heading is wrapped with normalize_theta in place of the quaternion product with the identity;
//   * CMD_NOT_FINITE and u_prev_next: the reference's getTwistFromControl cannot fail for its three models and what _u_seq holds after a failed step is corbo's affair;
//     here a control that is not finite gives a zero command, a reset and a zero previous control.
#pragma once
#include "mpc_controller_cycle.hpp"

namespace mpc {

// enum mpc_plan_flag of include/mpc_hip.h: bits of flags[b]
enum { PI_GOAL_REACHED = 1, PI_PLAN_EMPTY = 2, PI_PLAN_TRUNCATED = 4, PI_VIA_DROPPED = 8, PI_GOAL_INJECTED = 16 };
// enum mpc_cmd_result of include/mpc_hip.h
enum { CMD_SUCCESS = 0, CMD_GOAL_REACHED = 1, CMD_PLAN_EMPTY = 2, CMD_SOLVE_FAILED = 3, CMD_INFEASIBLE = 4, CMD_NOT_FINITE = 5 };

struct PlanParams {      // struct mpc_plan_params of include/mpc_hip.h
    double prune_distance, max_lookahead_dist, viapoint_sep, xy_goal_tolerance, yaw_goal_tolerance;
    int32_t overwrite_orientation, moving_average_length, costmap_size_x, costmap_size_y;
    double resolution;
};

// :665-667, :729-731, :753-755: squared distance of the robot to a plan pose
MPC_CC_HD double pi_sq_dist(double rx, double ry, double px, double py) {
#pragma clang fp contract(off)
    const double dx = rx - px, dy = ry - py;
    const double qx = dx * dx, qy = dy * dy;
    return qx + qy;
}
// teb's distance_points2d(a, b) = (b - a).norm()
MPC_CC_HD double pi_dist(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    const double dx = bx - ax, dy = by - ay;
    const double qx = dx * dx, qy = dy * dy;
    return __builtin_sqrt(qx + qy);
}
// :717-723: the squared radius the selection stays in, 85 % of the larger costmap half size
MPC_CC_HD double pi_sq_threshold(const PlanParams& p) {
#pragma clang fp contract(off)
    const double hx = (double)p.costmap_size_x * p.resolution / 2.0, hy = (double)p.costmap_size_y * p.resolution / 2.0;
    double thr = hx < hy ? hy : hx;      // std::max(hx, hy)
    thr *= 0.85;
    return thr * thr;
}
// the while condition of :746 once pose i - 1 has been pushed: is pose i pushed too?
MPC_CC_HD bool pi_walk_goes_on(int i, int n, double sq_dist, double sq_thr, double max_len, double length) {
    return i < n && sq_dist <= sq_thr && (max_len <= 0 || length <= max_len);
}

// updateViaPointsContainer (:619-635) as a running state: pose k of the selection, in order
struct ViaWalk {
    double px, py;      // the pose inserted last (the selection's first pose counts as inserted, :625)
    int count;          // via-points so far, the dropped ones included
};
MPC_CC_HD void pi_via_step(ViaWalk& w, int k, double x, double y, double th, double sep, int max_via, double* via) {
#pragma clang fp contract(off)
    if (k == 0) { w.px = x; w.py = y; w.count = 0; return; }
    if (sep <= 0) return;
    if (pi_dist(w.px, w.py, x, y) < sep) return;
    if (via && w.count < max_via) { via[3 * w.count] = x; via[3 * w.count + 1] = y; via[3 * w.count + 2] = th; }
    ++w.count;
    w.px = x; w.py = y;
}

// :312-318 against the global plan's last pose
MPC_CC_HD bool pi_goal_reached(const double goal[3], const double robot[3], double xy_tol, double yaw_tol) {
#pragma clang fp contract(off)
    const double dx = goal[0] - robot[0], dy = goal[1] - robot[1];
    const double qx = dx * dx, qy = dy * dy;
    const double delta = cc_normalize_theta(goal[2] - robot[2]);
    return __builtin_fabs(__builtin_sqrt(qx + qy)) < xy_tol && __builtin_fabs(delta) < yaw_tol;
}

// cc_atan2 of mpc_controller_cycle.hpp operation for operation -- the same table, the same double-double steps in the same order, so the same bits on every argument
// (tests/test_plan_inputs_host.py holds the two to each other) -- with its two selections between double-double constants written on the halves.  As cc_atan2 is
// written the compiler keeps those constants in 40 bytes of scratch per lane (controller_prepare_kernel has them); its text is pinned by that kernel, and plan_inputs_kernel
// is to run without scratch.
MPC_CC_HD double pi_atan2(double y, double x) {
#pragma clang fp contract(off)
    const double kAtanH[9] = {0x0.0p+0, 0x1.fd5ba9aac2f6ep-4, 0x1.f5b75f92c80ddp-3, 0x1.6f61941e4def1p-2, 0x1.dac670561bb4fp-2, 0x1.1e00babdefeb4p-1, 0x1.4978fa3269ee1p-1,
                              0x1.700a7c5784634p-1, 0x1.921fb54442d18p-1};
    const double kAtanL[9] = {0x0.0p+0, -0x1.cd37686760c17p-59, 0x1.8ab6e3cf7afbdp-57, -0x1.c63aae6f6e918p-56, 0x1.a2b7f222f65e2p-56, -0x1.928df287a668fp-58, 0x1.2419a87f2a458p-56,
                              -0x1.8c34d25aadef6p-56, 0x1.1a62633145c07p-55};
    const double kPiH = 0x1.921fb54442d18p+1, kPiL = 0x1.1a62633145c07p-53, kPi2H = 0x1.921fb54442d18p+0, kPi2L = 0x1.1a62633145c07p-54;
    if (x != x || y != y) return x + y;
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
    const bool xneg = __builtin_signbit(x), yneg = __builtin_signbit(y);
    double ah = 0.0, al = 0.0;
    if (ax == 0.0 && ay == 0.0) {
        ah = xneg ? kPiH : 0.0; al = xneg ? kPiL : 0.0;
    } else {
        const bool swap = ay > ax;
        const cc_dd q = cc_div({swap ? ax : ay, 0.0}, {swap ? ay : ax, 0.0});      // in [0, 1]
        const int k = (int)(q.h * 8.0 + 0.5);
        const double c = (double)k / 8.0;
        const cc_dd r = cc_div(cc_add(q, {-c, 0.0}), cc_add({1.0, 0.0}, cc_mul(q, {c, 0.0})));
        const cc_dd r2 = cc_mul(r, r);
        cc_dd s = cc_div({1.0, 0.0}, {27.0, 0.0});
        for (int j = 12; j >= 0; --j) s = cc_add(cc_div({1.0, 0.0}, {(double)(2 * j + 1), 0.0}), cc_neg(cc_mul(r2, s)));
        cc_dd a = cc_add({kAtanH[k], kAtanL[k]}, cc_mul(r, s));
        if (swap) a = cc_add({kPi2H, kPi2L}, cc_neg(a));
        if (xneg) a = cc_add({kPiH, kPiL}, cc_neg(a));
        ah = a.h; al = a.l;
    }
    const double res = ah + al;
    return yneg ? -res : res;
}

// estimateLocalGoalOrientation (:807-852) with the identity transform.  plan: the pruned global plan (pose 0 = the front), n its size, local_goal the last selected pose,
// goal_idx its index.
MPC_CC_HD double pi_goal_heading(const double* plan, int n, const double local_goal[3], int goal_idx, int moving_average_length) {
#pragma clang fp contract(off)
    if (goal_idx > n - moving_average_length - 2) {
        if (goal_idx >= n - 1) return local_goal[2];
        return cc_normalize_theta(plan[3 * (n - 1) + 2]);
    }
    if (n - goal_idx - 1 < moving_average_length) moving_average_length = n - goal_idx - 1;
    double px = local_goal[0], py = local_goal[1], sx = 0.0, sy = 0.0;
    const int end = goal_idx + moving_average_length;
    for (int i = goal_idx; i < end; ++i) {
        const double qx = plan[3 * (i + 1)], qy = plan[3 * (i + 1) + 1];
        const double dx = qx - px, dy = qy - py;
        const double ax = dx * dx, ay = dy * dy;
        const double r = __builtin_sqrt(ax + ay);
        sx += r == 0.0 ? 1.0 : dx / r;
        sy += r == 0.0 ? 0.0 : dy / r;
        if (i < end - 1) { px = qx; py = qy; }
    }
    return (sx == 0.0 && sy == 0.0) ? 0.0 : pi_atan2(sy, sx);
}

// what follows the scans (:312-354): goal test, goal heading, start and goal of the local plan, the outputs.  n_sel poses were selected, the last of them at index
// last_idx of the pruned plan gp (size n); poses 1 .. min(n_sel, plan_stride) - 2 of the local plan are written by the caller.
MPC_CC_HD void pi_finish(const PlanParams& p, const double* gp, int n, const double robot[3], int n_sel, int last_idx, int via_count, int max_via, bool have_via,
                         int plan_stride, double* plan_out, int32_t* n_plan, int32_t* n_via, int32_t* goal_idx, int32_t* flags) {
#pragma clang fp contract(off)
    int fl = 0;
    if (n_sel == 0) { n_sel = 1; last_idx = n - 1; fl |= PI_GOAL_INJECTED; }      // :766-774
    if (pi_goal_reached(&gp[3 * (n - 1)], robot, p.xy_goal_tolerance, p.yaw_goal_tolerance)) fl |= PI_GOAL_REACHED;
    double goal[3] = {gp[3 * last_idx], gp[3 * last_idx + 1], gp[3 * last_idx + 2]};
    if (p.overwrite_orientation) goal[2] = pi_goal_heading(gp, n, goal, last_idx, p.moving_average_length);      // :336-343
    int np = n_sel;
    if (np == 1) np = 2;                                           // :350-353 a plan that holds the goal only gets a start in front
    if (np > plan_stride) { np = plan_stride; fl |= PI_PLAN_TRUNCATED; }
    for (int c = 0; c < 3; ++c) { plan_out[c] = robot[c]; plan_out[3 * (np - 1) + c] = goal[c]; }      // :354, :333-347
    *n_plan = np;
    if (have_via) {
        if (via_count > max_via) { via_count = max_via; fl |= PI_VIA_DROPPED; }
        *n_via = via_count;
    }
    if (goal_idx) *goal_idx = last_idx;
    if (flags) *flags = fl;
}
MPC_CC_HD void pi_empty(const double robot[3], bool have_via, double* plan_out, int32_t* n_plan, int32_t* n_via, int32_t* goal_idx, int32_t* flags) {
    for (int c = 0; c < 3; ++c) { plan_out[c] = robot[c]; plan_out[3 + c] = robot[c]; }
    *n_plan = 2;
    if (have_via) *n_via = 0;
    if (goal_idx) *goal_idx = -1;
    if (flags) *flags = PI_PLAN_EMPTY;
}

// One instance in the reference's own order, loop by loop.  global: [n_global][3]; begin (in / out, nullable = 0): the persistent front the reference keeps by erasing;
// plan_out [plan_stride][3]; via [max_via][3] and n_via both or neither; goal_idx (nullable): index of the local goal counted from the front, as after the erase.
MPC_CC_HD void pi_instance(const PlanParams& p, const double* global, int n_global, const double robot[3], int32_t* begin, int plan_stride, int max_via, double* plan_out,
                           int32_t* n_plan, double* via, int32_t* n_via, int32_t* goal_idx, int32_t* flags) {
#pragma clang fp contract(off)
    const bool have_via = via && n_via;
    int front = begin ? *begin : 0;
    if (front < 0) front = 0;
    if (n_global - front < 1) { pi_empty(robot, have_via, plan_out, n_plan, n_via, goal_idx, flags); return; }
    // pruneGlobalPlan (:658-677): the first pose closer than the prune distance becomes the front; none that close: the plan stays
    const double prune_sq = p.prune_distance * p.prune_distance;
    for (int j = front; j < n_global; ++j)
        if (pi_sq_dist(robot[0], robot[1], global[3 * j], global[3 * j + 1]) < prune_sq) { front = j; break; }
    if (begin) *begin = front;
    const double* gp = global + 3 * (size_t)front;
    const int n = n_global - front;
    // transformGlobalPlan (:716-779)
    const double sq_thr = pi_sq_threshold(p);
    int i = 0;
    double sq_dist = 1e10;
    for (int j = 0; j < n; ++j) {
        const double d = pi_sq_dist(robot[0], robot[1], gp[3 * j], gp[3 * j + 1]);
        if (d > sq_thr) break;
        if (d < sq_dist) { sq_dist = d; i = j; }
    }
    double length = 0.0;
    int n_sel = 0;
    ViaWalk w = {0.0, 0.0, 0};
    while (pi_walk_goes_on(i, n, sq_dist, sq_thr, p.max_lookahead_dist, length)) {
        if (n_sel >= 1 && n_sel < plan_stride - 1) for (int c = 0; c < 3; ++c) plan_out[3 * n_sel + c] = gp[3 * i + c];
        if (have_via) pi_via_step(w, n_sel, gp[3 * i], gp[3 * i + 1], gp[3 * i + 2], p.viapoint_sep, max_via, via);      // :310 on the selection as selected
        ++n_sel;
        sq_dist = pi_sq_dist(robot[0], robot[1], gp[3 * i], gp[3 * i + 1]);
        if (i > 0 && p.max_lookahead_dist > 0) length += pi_dist(gp[3 * (i - 1)], gp[3 * (i - 1) + 1], gp[3 * i], gp[3 * i + 1]);
        ++i;
    }
    pi_finish(p, gp, n, robot, n_sel, i - 1, w.count, max_via, have_via, plan_stride, plan_out, n_plan, n_via, goal_idx, flags);
}

// One instance after the step (:394-452).  u0: the first control of the solve; feasible / plan_flags: nullable = feasible / none; infeasible_count (in / out, nullable):
// _no_infeasible_plans.
MPC_CC_HD void cmd_instance(const double u0[2], int status, int feasible, int plan_flags, double cmd[3], int32_t* result, int32_t* reset_next, double* u_prev_next,
                            int32_t* infeasible_count) {
    const bool finite = (u0[0] - u0[0] == 0.0) && (u0[1] - u0[1] == 0.0);
    int res = CMD_SUCCESS, reset = 0;
    if (plan_flags & PI_PLAN_EMPTY) res = CMD_PLAN_EMPTY;               // :325-330 (an empty GLOBAL plan: :301-307)
    else if (plan_flags & PI_GOAL_REACHED) res = CMD_GOAL_REACHED;      // :318-322
    else if (status != 0) { res = CMD_SOLVE_FAILED; reset = 1; }        // :394-404
    else if (!feasible) { res = CMD_INFEASIBLE; reset = 1; }            // :416-428
    else if (!finite) { res = CMD_NOT_FINITE; reset = 1; }              // :432-441
    const bool ok = res == CMD_SUCCESS;
    cmd[0] = ok ? u0[0] : 0.0; cmd[1] = 0.0; cmd[2] = ok ? u0[1] : 0.0;      // getTwistFromControl of every model: linear.x = u_0, angular.z = u_1 (car-like: the steering angle)
    *result = res;
    if (reset_next) *reset_next = reset;
    if (u_prev_next) { u_prev_next[0] = finite ? u0[0] : 0.0; u_prev_next[1] = finite ? u0[1] : 0.0; }
    if (infeasible_count) { if (reset) *infeasible_count = *infeasible_count + 1; else if (ok) *infeasible_count = 0; }      // :399, :423, :436, :448
}

#if defined(__HIPCC__)

struct PlanInputsArgs {
    PlanParams p;
    const double* global;       // [B][gstride][3]
    const int32_t* n_global;    // [B]
    int32_t gstride;
    const double* robot;        // [B][3]
    int32_t* begin;             // [B] in / out, or NULL
    double* plan;               // [B][plan_stride][3]
    int32_t* n_plan;            // [B]
    int32_t plan_stride, max_via;
    int32_t* n_via;             // [B] or NULL
    double* via;                // [B][max_via][3] or NULL
    int32_t* goal_idx;          // [B] or NULL
    int32_t* flags;             // [B] or NULL
};

// poses j0 .. j0 + 63 of a plan of n poses into LDS, 192 consecutive doubles read by consecutive lanes; poses at and beyond n read as 0
__device__ __forceinline__ void pi_load_chunk(const double* gp, int j0, int n, int lane, double* raw) {
    __syncthreads();      // the chunk before has been consumed
    const long long e0 = 3ll * j0, e_end = 3ll * n;
    for (int t = 0; t < 3; ++t) {
        const long long e = e0 + lane + 64 * t;
        raw[lane + 64 * t] = e < e_end ? gp[e] : 0.0;
    }
    __syncthreads();
}

// One wavefront per instance.  The three scans of pi_instance over chunks of 64 poses: every chunk is loaded once with consecutive lanes on consecutive words, the
// squared distances and segment lengths are lane-parallel, and a scan ends with the chunk in which the reference's loop ends -- so the traffic follows the poses inside
// the costmap radius, not the plan's length.  What depends on order (the running length, the greedy via-point walk) is walked left to right over the chunk in LDS, by every
// lane alike: the trip counts are wave-uniform and no lane leaves before the last wave-wide operation.
__global__ __launch_bounds__(64) void plan_inputs_kernel(PlanInputsArgs a) {
#pragma clang fp contract(off)
    __shared__ double raw[192], sd[64], sg[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const PlanParams& p = a.p;
    const double* global = a.global + (size_t)b * a.gstride * 3;
    double* plan_out = a.plan + (size_t)b * a.plan_stride * 3;
    double* via = a.via ? a.via + (size_t)b * a.max_via * 3 : nullptr;
    const bool have_via = a.via && a.n_via;
    const double robot[3] = {a.robot[3 * b], a.robot[3 * b + 1], a.robot[3 * b + 2]};
    int n_global = a.n_global[b];
    if (n_global > a.gstride) n_global = a.gstride;
    int front = a.begin ? a.begin[b] : 0;
    if (front < 0) front = 0;
    if (n_global - front < 1) {      // wave-uniform
        if (lane == 0) pi_empty(robot, have_via, plan_out, &a.n_plan[b], a.n_via ? &a.n_via[b] : nullptr, a.goal_idx ? &a.goal_idx[b] : nullptr, a.flags ? &a.flags[b] : nullptr);
        return;
    }
    // prune: the first pose under the prune distance, from the lowest set bit of the chunk's ballot
    const double prune_sq = p.prune_distance * p.prune_distance;
    for (int j0 = front; j0 < n_global; j0 += 64) {
        pi_load_chunk(global, j0, n_global, lane, raw);
        const bool hit = j0 + lane < n_global && pi_sq_dist(robot[0], robot[1], raw[3 * lane], raw[3 * lane + 1]) < prune_sq;
        const unsigned long long m = __ballot(hit);
        if (m) { front = j0 + __builtin_ctzll(m); break; }
    }
    if (a.begin && lane == 0) a.begin[b] = front;
    const double* gp = global + 3 * (size_t)front;
    const int n = n_global - front;
    // nearest pose: the loop breaks at the first pose outside the radius (ballot); before it the minimum over (distance, index), lowest index on ties
    const double sq_thr = pi_sq_threshold(p);
    const double kInf = __builtin_inf();
    double best_d = kInf;
    int best_j = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        pi_load_chunk(gp, j0, n, lane, raw);
        const double d = pi_sq_dist(robot[0], robot[1], raw[3 * lane], raw[3 * lane + 1]);
        const bool in = j0 + lane < n;
        const unsigned long long m = __ballot(in && d > sq_thr);
        const int brk = m ? __builtin_ctzll(m) : 64;
        double cd = (in && lane < brk && d < 1e10) ? d : kInf;      // (d < sq_dist with sq_dist = 1e10 at the start, :724, :734)
        int cj = j0 + lane;
        for (int s = 32; s >= 1; s >>= 1) {
            const double od = __shfl_xor(cd, s);
            const int oj = __shfl_xor(cj, s);
            if (od < cd || (od == cd && oj < cj)) { cd = od; cj = oj; }
        }
        if (cd < best_d) { best_d = cd; best_j = cj; }      // a later chunk wins only when strictly closer
        if (m) break;
    }
    int i = best_d < kInf ? best_j : 0;
    double sq_dist = best_d < kInf ? best_d : 1e10;
    // the walk: per chunk the distances and segment lengths lane-parallel, then the reference's loop over them in order
    double length = 0.0;
    int n_sel = 0;
    ViaWalk w = {0.0, 0.0, 0};
    bool more = pi_walk_goes_on(i, n, sq_dist, sq_thr, p.max_lookahead_dist, length);
    while (more) {
        const int j0 = i;
        pi_load_chunk(gp, j0, n, lane, raw);
        const double x = raw[3 * lane], y = raw[3 * lane + 1], th = raw[3 * lane + 2];
        double qx = 0.0, qy = 0.0;      // the pose before this lane's
        if (lane > 0) { qx = raw[3 * lane - 3]; qy = raw[3 * lane - 2]; }
        else if (j0 > 0) { qx = gp[3 * (j0 - 1)]; qy = gp[3 * (j0 - 1) + 1]; }
        sd[lane] = pi_sq_dist(robot[0], robot[1], x, y);
        sg[lane] = pi_dist(qx, qy, x, y);
        __syncthreads();
        int cnt = 0;
        for (int l = 0; l < 64 && more; ++l) {
            if (have_via) pi_via_step(w, n_sel + l, raw[3 * l], raw[3 * l + 1], raw[3 * l + 2], p.viapoint_sep, a.max_via, lane == 0 ? via : nullptr);
            sq_dist = sd[l];
            if (i > 0 && p.max_lookahead_dist > 0) length += sg[l];
            ++i; ++cnt;
            more = pi_walk_goes_on(i, n, sq_dist, sq_thr, p.max_lookahead_dist, length);
        }
        const int k = n_sel + lane;      // this lane's pose in the selection; the very last one is written by pi_finish
        if (lane < cnt && !(!more && lane == cnt - 1) && k >= 1 && k < a.plan_stride - 1) { plan_out[3 * k] = x; plan_out[3 * k + 1] = y; plan_out[3 * k + 2] = th; }
        n_sel += cnt;
    }
    if (lane == 0)
        pi_finish(p, gp, n, robot, n_sel, i - 1, w.count, a.max_via, have_via, a.plan_stride, plan_out, &a.n_plan[b], a.n_via ? &a.n_via[b] : nullptr,
                  a.goal_idx ? &a.goal_idx[b] : nullptr, a.flags ? &a.flags[b] : nullptr);
}

struct CommandsArgs {
    const double* u;              // [B][n_stride][2]: u_out of the step
    int32_t n_stride, B;
    const int32_t* status;        // [B]
    const int32_t* feasible;      // [B] or NULL
    const int32_t* plan_flags;    // [B] or NULL
    double* cmd;                  // [B][3]
    int32_t* result;              // [B]
    int32_t* reset_next;          // [B] or NULL
    double* u_prev_next;          // [B][2] or NULL
    int32_t* infeasible_count;    // [B] in / out, or NULL
};

// one lane per instance
__global__ __launch_bounds__(64) void commands_kernel(CommandsArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const double u0[2] = {a.u[(size_t)b * a.n_stride * 2], a.u[(size_t)b * a.n_stride * 2 + 1]};
    double cmd[3];
    int32_t res;
    cmd_instance(u0, a.status[b], a.feasible ? a.feasible[b] : 1, a.plan_flags ? a.plan_flags[b] : 0, cmd, &res, a.reset_next ? &a.reset_next[b] : nullptr,
                 a.u_prev_next ? &a.u_prev_next[2 * b] : nullptr, a.infeasible_count ? &a.infeasible_count[b] : nullptr);
    a.cmd[3 * b] = cmd[0]; a.cmd[3 * b + 1] = cmd[1]; a.cmd[3 * b + 2] = cmd[2];
    a.result[b] = res;
}

#endif  // __HIPCC__

}  // namespace mpc
