// tests only: the host build of mpc_local_planner_amd/csrc/mpc_plan_inputs.hpp (the per-instance logic of mpc_plan_inputs_batch* and mpc_commands_batch*) behind C entry
// points, next to the same steps done with the facade's own functions (include/mpc_controller.hpp: prune_global_plan, transform_global_plan, via_points_from_plan,
// estimate_local_goal_orientation) and a literal restatement of src/mpc_local_planner_ros.cpp:312-354.  No GPU calls.  With -DPIN_MAIN: a stand-alone program that runs
// scripted and random plans through both itself (the sanitizer build of tests/test_plan_inputs_host.py).
#define MPC_FACADE_HOST_LOOP_ONLY
#include "../../include/mpc_controller.hpp"
#include "../../mpc_local_planner_amd/csrc/mpc_plan_inputs.hpp"

#include <cstdio>
#include <cstring>

namespace F = mpc_local_planner_amd;

static mpc::PlanParams to_params(const mpc_plan_params* p) {
    return {p->global_plan_prune_distance, p->max_global_plan_lookahead_dist, p->global_plan_viapoint_sep, p->xy_goal_tolerance, p->yaw_goal_tolerance,
            p->global_plan_overwrite_orientation, p->moving_average_length, p->costmap_size_x, p->costmap_size_y, p->resolution};
}

// B instances through pi_instance, in the layouts of mpc_plan_inputs_batch (every pointer as there; n_global is clamped to gstride as the kernel does)
extern "C" void pin_batch(int B, const mpc_plan_params* p, const double* global, const int32_t* n_global, int gstride, const double* robot, int32_t* begin, double* plan,
                          int32_t* n_plan, int plan_stride, int max_via, int32_t* n_via, double* via, int32_t* goal_idx, int32_t* flags) {
    const mpc::PlanParams q = to_params(p);
    for (int b = 0; b < B; ++b) {
        const int ng = n_global[b] > gstride ? gstride : n_global[b];
        mpc::pi_instance(q, global + (size_t)b * gstride * 3, ng, robot + 3 * b, begin ? begin + b : nullptr, plan_stride, max_via, plan + (size_t)b * plan_stride * 3, n_plan + b,
                         via ? via + (size_t)b * max_via * 3 : nullptr, n_via ? n_via + b : nullptr, goal_idx ? goal_idx + b : nullptr, flags ? flags + b : nullptr);
    }
}

// ONE instance with the facade's functions and :312-354 restated line by line.  Same outputs as pin_batch with B = 1; MPC_PLAN_GOAL_INJECTED is not reported (an injected
// goal and a selection that holds the last pose alone are the same to everything downstream of transform_global_plan).
extern "C" void pin_facade(const mpc_plan_params* p, const double* global, int n_global, const double* robot, int32_t* begin, double* plan, int32_t* n_plan, int plan_stride,
                           int max_via, int32_t* n_via, double* via, int32_t* goal_idx, int32_t* flags) {
    int front = begin ? *begin : 0;
    if (front < 0) front = 0;
    std::vector<F::PoseSE2> g;      // the plugin's _global_plan: what earlier cycles have left of it
    for (int j = front; j < n_global; ++j) { F::PoseSE2 q; q.x = global[3 * j]; q.y = global[3 * j + 1]; q.theta = global[3 * j + 2]; g.push_back(q); }
    F::PoseSE2 rp; rp.x = robot[0]; rp.y = robot[1]; rp.theta = robot[2];
    if (g.empty()) {
        for (int c = 0; c < 3; ++c) { plan[c] = robot[c]; plan[3 + c] = robot[c]; }
        *n_plan = 2; if (n_via) *n_via = 0; if (goal_idx) *goal_idx = -1; if (flags) *flags = MPC_PLAN_EMPTY;
        return;
    }
    const size_t before = g.size();
    F::prune_global_plan(g, rp, p->global_plan_prune_distance);                                         // :295
    front += (int)(before - g.size());
    if (begin) *begin = front;
    std::vector<F::PoseSE2> tp;
    const int gi = F::transform_global_plan(g, rp, p->costmap_size_x, p->costmap_size_y, p->resolution, p->max_global_plan_lookahead_dist, tp);      // :301
    int fl = 0;
    if (n_via && via) {                                                                                   // :310
        const std::vector<F::PoseSE2> vp = F::via_points_from_plan(tp, p->global_plan_viapoint_sep);
        int nv = (int)vp.size();
        if (nv > max_via) { nv = max_via; fl |= MPC_PLAN_VIA_DROPPED; }
        for (int k = 0; k < nv; ++k) { via[3 * k] = vp[(size_t)k].x; via[3 * k + 1] = vp[(size_t)k].y; via[3 * k + 2] = vp[(size_t)k].theta; }
        *n_via = nv;
    }
    {                                                                                                     // :312-322
        const F::PoseSE2& global_goal = g.back();
        const double dx = global_goal.x - rp.x, dy = global_goal.y - rp.y;
        const double delta_orient = F::normalize_theta(global_goal.theta - rp.theta);
        if (std::abs(std::sqrt(dx * dx + dy * dy)) < p->xy_goal_tolerance && std::abs(delta_orient) < p->yaw_goal_tolerance) fl |= MPC_PLAN_GOAL_REACHED;
    }
    F::PoseSE2 robot_goal;                                                                                // :332-347
    robot_goal.x = tp.back().x; robot_goal.y = tp.back().y;
    if (p->global_plan_overwrite_orientation) {
        robot_goal.theta = F::estimate_local_goal_orientation(g, tp.back(), gi, 0.0, 0.0, 0.0, p->moving_average_length);
        tp.back().theta = robot_goal.theta;
    } else
        robot_goal.theta = tp.back().theta;
    if (tp.size() == 1) tp.insert(tp.begin(), F::PoseSE2());                                              // :350-353
    tp.front() = rp;                                                                                      // :354
    int np = (int)tp.size();
    if (np > plan_stride) { np = plan_stride; fl |= MPC_PLAN_TRUNCATED; }
    for (int k = 0; k < np; ++k) {
        const F::PoseSE2& q = k == np - 1 ? tp.back() : tp[(size_t)k];
        plan[3 * k] = q.x; plan[3 * k + 1] = q.y; plan[3 * k + 2] = q.theta;
    }
    *n_plan = np;
    if (goal_idx) *goal_idx = gi;
    if (flags) *flags = fl;
}

// the heading estimate alone: plan = the pruned global plan, the local goal = its pose goal_idx
extern "C" double pin_goal_heading(const double* plan, int n, int goal_idx, int moving_average_length) {
    return mpc::pi_goal_heading(plan, n, plan + 3 * goal_idx, goal_idx, moving_average_length);
}
extern "C" double pin_facade_goal_heading(const double* plan, int n, int goal_idx, int moving_average_length) {
    std::vector<F::PoseSE2> g((size_t)n);
    for (int j = 0; j < n; ++j) { g[(size_t)j].x = plan[3 * j]; g[(size_t)j].y = plan[3 * j + 1]; g[(size_t)j].theta = plan[3 * j + 2]; }
    return F::estimate_local_goal_orientation(g, g[(size_t)goal_idx], goal_idx, 0.0, 0.0, 0.0, moving_average_length);
}

extern "C" double pin_atan2(double y, double x) { return mpc::pi_atan2(y, x); }
extern "C" double pin_cc_atan2(double y, double x) { return mpc::cc_atan2(y, x); }

// B instances through cmd_instance, in the layouts of mpc_commands_batch (u: [B][n_stride][2])
extern "C" void pin_commands(int B, const double* u, int n_stride, const int32_t* status, const int32_t* feasible, const int32_t* plan_flags, double* cmd, int32_t* result,
                             int32_t* reset_next, double* u_prev_next, int32_t* infeasible_count) {
    for (int b = 0; b < B; ++b)
        mpc::cmd_instance(u + (size_t)b * n_stride * 2, status[b], feasible ? feasible[b] : 1, plan_flags ? plan_flags[b] : 0, cmd + 3 * b, result + b,
                          reset_next ? reset_next + b : nullptr, u_prev_next ? u_prev_next + 2 * b : nullptr, infeasible_count ? infeasible_count + b : nullptr);
}

#ifdef PIN_MAIN
static unsigned long long g_rng = 88172645463325252ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (double)(g_rng >> 11) / 9007199254740992.0; }

static int g_cases = 0, g_bad = 0;
// one plan through both codes: every discrete output and every copied pose equal; the local goal's heading within 1.6e-14 rad
static void compare(const char* what, const mpc_plan_params& p, const std::vector<double>& global, const double robot[3], int begin0, int plan_stride, int max_via) {
    const int n = (int)global.size() / 3;
    std::vector<double> pa((size_t)3 * plan_stride, -7.0), pb(pa), va((size_t)3 * (max_via > 0 ? max_via : 1), -7.0), vb(va);
    int32_t ba = begin0, bb = begin0, na = -1, nb = -1, nva = -1, nvb = -1, ga = -9, gb = -9, fa = -1, fb = -1;
    mpc::pi_instance(to_params(&p), global.data(), n, robot, &ba, plan_stride, max_via, pa.data(), &na, max_via > 0 ? va.data() : nullptr, max_via > 0 ? &nva : nullptr, &ga, &fa);
    pin_facade(&p, global.data(), n, robot, &bb, pb.data(), &nb, plan_stride, max_via, max_via > 0 ? &nvb : nullptr, max_via > 0 ? vb.data() : nullptr, &gb, &fb);
    ++g_cases;
    bool same = ba == bb && na == nb && nva == nvb && ga == gb && (fa & ~MPC_PLAN_GOAL_INJECTED) == fb && std::memcmp(va.data(), vb.data(), va.size() * 8) == 0;
    if (same && na >= 2) {
        same = std::memcmp(pa.data(), pb.data(), ((size_t)3 * na - 1) * 8) == 0;
        const double d = std::fabs(F::normalize_theta(pa[(size_t)3 * na - 1] - pb[(size_t)3 * na - 1]));
        if (!(d < 1.6e-14)) same = false;
    }
    if (!same) { ++g_bad; std::printf("%s: differs (front %d / %d, n_plan %d / %d, n_via %d / %d, goal_idx %d / %d, flags %d / %d)\n", what, ba, bb, na, nb, nva, nvb, ga, gb, fa, fb); }
}

int main() {
    const double pi = 3.14159265358979323846;
    mpc_plan_params p;
    p.global_plan_prune_distance = 1.0; p.max_global_plan_lookahead_dist = 1.5; p.global_plan_viapoint_sep = 0.3; p.xy_goal_tolerance = 0.2; p.yaw_goal_tolerance = 0.1;
    p.global_plan_overwrite_orientation = 1; p.moving_average_length = 3; p.costmap_size_x = 120; p.costmap_size_y = 100; p.resolution = 0.05;
    auto line = [](int n, double step) { std::vector<double> g; for (int j = 0; j < n; ++j) { g.push_back(step * j); g.push_back(0.0); g.push_back(0.0); } return g; };
    const double r0[3] = {0.0, 0.0, 0.0};
    // lengths 1, 2, 3; robot at the start, in the middle, far away; begin at 0 and at the last pose
    for (int n = 1; n <= 3; ++n)
        for (int beg = 0; beg < n; ++beg) {
            compare("short plan", p, line(n, 0.5), r0, beg, 8, 4);
            const double far[3] = {40.0, 40.0, 1.0};
            compare("short plan, robot far", p, line(n, 0.5), far, beg, 8, 4);
        }
    { std::vector<double> g = line(40, 0.1); g[3 * 7] = g[3 * 6]; compare("repeated pose", p, g, r0, 0, 64, 8); }
    { std::vector<double> g = line(200, 0.1); for (int j = 60; j < 140; ++j) { g[3 * j] = 0.1 * (j < 100 ? j : 199 - j); g[3 * j + 1] = 0.5; } compare("leaves and returns", p, g, r0, 0, 64, 8); }
    { std::vector<double> g = line(30, 0.1); const double r[3] = {0.25, 0.0, 0.0}; compare("nearest tie", p, g, r, 0, 64, 8); }
    { mpc_plan_params q = p; q.max_global_plan_lookahead_dist = 0.0; compare("no look-ahead limit", q, line(100, 0.05), r0, 0, 256, 8); q.max_global_plan_lookahead_dist = -1.0; compare("no look-ahead limit", q, line(100, 0.05), r0, 0, 16, 8); }
    { mpc_plan_params q = p; q.max_global_plan_lookahead_dist = 1.0; compare("look-ahead hit at a pose", q, line(100, 0.25), r0, 0, 64, 8); }
    { mpc_plan_params q = p; q.global_plan_viapoint_sep = 0.0; compare("no via-points", q, line(100, 0.05), r0, 0, 64, 8); q.global_plan_viapoint_sep = 0.05; compare("via-points dropped", q, line(100, 0.05), r0, 0, 64, 3); }
    compare("truncated", p, line(100, 0.05), r0, 0, 5, 8);
    compare("begin at the last pose", p, line(100, 0.05), r0, 99, 16, 8);
    for (int k = 0; k < 2; ++k) {      // the goal just inside and just outside each tolerance; a heading difference of +-pi
        mpc_plan_params q = p;
        std::vector<double> g = line(4, 0.05);
        q.xy_goal_tolerance = k ? 0.15000000000000002 : std::nextafter(0.15000000000000002, 1.0); compare("xy tolerance", q, g, r0, 0, 8, 4);
        g[3 * 3 + 2] = 0.05; q.xy_goal_tolerance = 0.2;
        q.yaw_goal_tolerance = k ? 0.05 : std::nextafter(0.05, 1.0); compare("yaw tolerance", q, g, r0, 0, 8, 4);
        g[3 * 3 + 2] = k ? pi : -pi; q.yaw_goal_tolerance = 4.0; compare("heading difference pi", q, g, r0, 0, 8, 4);
    }
    // random smooth plans, random robots near them, both orientation modes
    for (int rep = 0; rep < 300; ++rep) {
        const int n = 1 + (int)(rnd() * 150);
        std::vector<double> g;
        double x = 0, y = 0, th = 2 * pi * rnd() - pi;
        for (int j = 0; j < n; ++j) { g.push_back(x); g.push_back(y); g.push_back(th); th += 0.6 * (rnd() - 0.5); const double s = 0.02 + 0.1 * rnd(); x += s * std::cos(th); y += s * std::sin(th); }
        const int at = (int)(rnd() * n);
        const double r[3] = {g[3 * at] + 0.6 * (rnd() - 0.5), g[3 * at + 1] + 0.6 * (rnd() - 0.5), 2 * pi * rnd() - pi};
        mpc_plan_params q = p;
        q.global_plan_overwrite_orientation = rep % 2; q.max_global_plan_lookahead_dist = rep % 5 == 0 ? 0.0 : 0.5 + 2.5 * rnd(); q.global_plan_viapoint_sep = rep % 3 == 0 ? -1.0 : 0.05 + 0.5 * rnd();
        compare("random plan", q, g, r, rep % 4 == 0 ? (int)(rnd() * n) : 0, 4 + (int)(rnd() * 60), 1 + rep % 6);
    }
    // commands: every branch once, the counter over three calls
    {
        const double u[5][2] = {{0.3, -0.2}, {0.3, -0.2}, {0.3, -0.2}, {std::nan(""), 0.1}, {0.1, 0.2}};
        const int32_t st[5] = {0, 1, 0, 0, 0}, fe[5] = {1, 1, 0, 1, 1}, fl[5] = {0, 0, 0, 0, MPC_PLAN_GOAL_REACHED};
        const int32_t expect[5] = {MPC_CMD_SUCCESS, MPC_CMD_SOLVE_FAILED, MPC_CMD_INFEASIBLE, MPC_CMD_NOT_FINITE, MPC_CMD_GOAL_REACHED};
        double cmd[15], up[10]; int32_t res[5], rs[5], cnt[5] = {2, 0, 0, 0, 5};
        for (int call = 0; call < 3; ++call) pin_commands(5, &u[0][0], 1, st, fe, fl, cmd, res, rs, up, cnt);
        const int32_t cnt_expect[5] = {0, 3, 3, 3, 5};
        for (int b = 0; b < 5; ++b, ++g_cases)
            if (res[b] != expect[b] || rs[b] != (b >= 1 && b <= 3) || cnt[b] != cnt_expect[b] || cmd[3 * b] != (b == 0 ? 0.3 : 0.0) || cmd[3 * b + 1] != 0.0) { ++g_bad; std::printf("commands case %d differs\n", b); }
    }
    std::printf("plan_inputs_host: %d cases, %d differ\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
#endif
