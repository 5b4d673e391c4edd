// GPU test program (built and run by tests/test_gpu_controller_batch.py): B facade Controllers (include/mpc_controller.hpp), each with a B = 1 handle of its
// own, against ONE handle with max_batch = B driven by mpc_controller_step_batch, in closed loop (next start = x_out[b][1], u_prev = u_out[b][0], dt_prev = the
// period).  Every cycle and every robot: x, u, dt, converged, iterations, grid size bit for bit, and the re-initialisation flags against what the program works out
// from the facade's public state.  Usage: gpu_controller_batch variable <outer_iterations> | fixed <dual_warm_start>.  Exit code 0 iff every check holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../include/mpc_controller.hpp"

using namespace mpc_local_planner_amd;

static const double kPi = 3.14159265358979323846;
static const int kStride = 9;      // plan_stride of the batched call

struct Robot {
    std::vector<PoseSE2> mid;      // the plan's poses between start and goal
    PoseSE2 pose{0, 0, 0}, goal{2.0, 0.5, 0.3};
    int first_cycle = 0;           // the robot joins the fleet in this cycle
    bool feedback = false;         // gets state measurements: fresh on even cycles, stale on odd ones
    double u_prev[2] = {0, 0};
    // what the program tracks to predict the flags
    int steps = 0;
    PoseSE2 last_goal;
};

static int run(bool variable, int outer, int dual) {
    const int B = variable ? 8 : 4, cycles = variable ? 12 : 8, n_ref = variable ? 8 : 12, stride = 12, every = 7;
    const double period = 0.1, new_goal_dist = 1.0, new_goal_ang = 0.5 * kPi;
    mpc_config c;
    mpc_config_defaults(&c);      // unicycle, variable grid, minimum time, dt_ref .3
    if (!variable) {
        c.dt_free = 0; c.objective = MPC_OBJ_QUADRATIC;
        c.xf_fixed[0] = c.xf_fixed[1] = c.xf_fixed[2] = 0;
        c.Q[0] = c.Q[1] = 2.0; c.Q[2] = 0.25; c.R[0] = 0.1; c.R[1] = 0.05;
        c.has_Qf = 1; c.Qf[0] = c.Qf[1] = 10.0; c.Qf[2] = 0.5;
        c.du_lb[0] = c.du_lb[1] = -0.2; c.du_ub[0] = c.du_ub[1] = 0.2;
        c.dual_warm_start = dual;
    }
    // ---- the scripts
    std::vector<Robot> rb((size_t)B);
    auto curved = [](Robot& r) { r.mid = {{0.5, 0.2, 0.0}, {1.0, 0.6, 0.0}, {1.5, 0.7, 0.0}}; r.goal = {2.0, 1.0, 0.4}; };
    curved(rb[1]);
    rb[2].goal = {2.0, 0.0, 0.0};                                       // jumps by 1.5 m in cycle 4
    if (variable) {
        rb[3].goal = {2.0, 0.3, 0.0};                                   // turns by 100 degrees in cycle 5
        // rb[4]: reset in cycle 3
        rb[5].feedback = true;
        rb[6].pose = {0.0, 0.0, kPi - 0.1}; rb[6].goal = {-2.0, 0.1, -kPi + 0.2};      // 9 poses, the heading passes through +-pi
        for (int i = 1; i <= 7; ++i) rb[6].mid.push_back({-0.25 * i, (i % 2 ? 0.05 : -0.05), 0.0});
        rb[7].goal = {1.5, -0.5, -0.2}; rb[7].first_cycle = 3;          // moves by 0.5 m in cycle 6: no re-initialisation; joins in cycle 3 with a cold start
    }
    const int reset_robot = variable ? 4 : 3;
    // ---- B facades and the batched handle
    std::vector<std::unique_ptr<Controller>> ctl;
    for (int b = 0; b < B; ++b) {
        ctl.emplace_back(new Controller());
        Controller& k = *ctl.back();
        if (variable) k.setGridAdaptation(true, stride, 0.1, 3);
        k.setForceReinit(every, new_goal_dist, new_goal_ang);
        k.setNumOcpIterations(outer);
        k.setPreferStateFeedback(true);
        mpc_config cb = c;
        cb.n = n_ref;
        if (!k.configure(cb)) { std::printf("configure failed: %s\n", k.lastError().c_str()); return 2; }
    }
    mpc_config cs = c;
    cs.n = stride;
    if (!variable) cs.n = n_ref;
    const int n = cs.n;
    mpc_solver* h = nullptr;
    if (mpc_create(&cs, B, 0, &h) != MPC_OK) { std::printf("mpc_create failed: %s\n", mpc_last_error()); return 2; }
    mpc_cycle_params p;
    mpc_cycle_params_defaults(&p);
    p.n_ref = n_ref; p.outer_iterations = outer; p.adapt = variable ? 1 : 0; p.n_min = 3; p.n_max = stride; p.dt_hyst_ratio = 0.1; p.warm_start = 1;
    p.force_reinit_num_steps = every; p.force_reinit_new_goal_dist = new_goal_dist; p.force_reinit_new_goal_angular = new_goal_ang;
    p.prefer_x_feedback = 1; p.period = period;

    std::vector<double> plan((size_t)B * kStride * 3), fb((size_t)B * 3), age((size_t)B), up((size_t)B * 2), dtp((size_t)B), x((size_t)B * n * 3), u((size_t)B * n * 2), dt((size_t)B);
    std::vector<int32_t> npl((size_t)B), rs((size_t)B), st((size_t)B), it((size_t)B), ri((size_t)B), ng((size_t)B);
    int bad = 0, seen = 0, mixed = 0, compared = 0;
    for (int cyc = 0; cyc < cycles; ++cyc) {
        const double t = cyc * period;
        // the script's events
        if (cyc == 4) rb[2].goal.y += 1.5;
        if (variable && cyc == 5) rb[3].goal.theta += 100.0 * kPi / 180.0;
        if (variable && cyc == 6) rb[7].goal.x += 0.5;
        int Bc = 0;
        for (int b = 0; b < B; ++b) if (cyc >= rb[b].first_cycle) Bc = b + 1;
        std::vector<int32_t> expect((size_t)B, 0);
        std::vector<bool> ok((size_t)B, false);
        TimeSeries xs[8], us[8];
        for (int b = 0; b < Bc; ++b) {
            Robot& r = rb[b];
            Controller& k = *ctl[b];
            // the plan of this cycle: the robot's pose, the fixed poses in between, the goal
            std::vector<PoseSE2> pl;
            pl.push_back(r.pose);
            for (const PoseSE2& q : r.mid) pl.push_back(q);
            pl.push_back(r.goal);
            npl[b] = (int32_t)pl.size();
            for (size_t i = 0; i < pl.size(); ++i) { plan[((size_t)b * kStride + i) * 3] = pl[i].x; plan[((size_t)b * kStride + i) * 3 + 1] = pl[i].y; plan[((size_t)b * kStride + i) * 3 + 2] = pl[i].theta; }
            // state measurement: the pose shifted a little, stamped now on even cycles and three periods ago on odd ones; the others have none (an age beyond any period)
            age[b] = 1e9; fb[3 * b] = fb[3 * b + 1] = fb[3 * b + 2] = 0.0;
            if (r.feedback) {
                const double meas[3] = {r.pose.x + 0.01, r.pose.y - 0.01, r.pose.theta + 0.005}, stamp = cyc % 2 == 0 ? t : t - 3.0 * period;
                k.stateFeedbackCallback(meas, stamp);
                age[b] = t - stamp;
                for (int i = 0; i < 3; ++i) fb[3 * b + i] = meas[i];
            }
            rs[b] = (b == reset_robot && cyc == 3) ? 1 : 0;
            if (rs[b]) k.reset();
            up[2 * b] = r.u_prev[0]; up[2 * b + 1] = r.u_prev[1]; dtp[b] = r.steps == 0 ? 0.0 : period;
            // the flags this step must report, from the facade's public state and the rule of src/controller.cpp:152-158
            int e = 0;
            if (r.steps == 0) e |= MPC_REINIT_FIRST;
            if (rs[b]) e |= MPC_REINIT_RESET;
            if (r.steps % every == 0) e |= MPC_REINIT_NUM_STEPS;
            if (r.steps > 0) {
                const double dx = r.goal.x - r.last_goal.x, dy = r.goal.y - r.last_goal.y;
                if (std::sqrt(dx * dx + dy * dy) > new_goal_dist) e |= MPC_REINIT_GOAL_DIST;
                if (std::fabs(normalize_theta(r.goal.theta - r.last_goal.theta)) > new_goal_ang) e |= MPC_REINIT_GOAL_ANGULAR;
            }
            if (e) {
                const double dt_sample = (r.steps > 0 && c.dt_free && k.lastDt() > 0.0) ? k.lastDt() : c.dt_ref;
                if (pl.size() > 2 || dt_sample != c.dt_ref) e |= MPC_REINIT_PLAN_GUESS;
            }
            expect[b] = e;
            k.setPreviousControlInput(r.u_prev, dtp[b]);
            ok[b] = k.step(pl, Twist(), period, t, us[b], xs[b]);
            if (!k.lastError().empty()) { std::printf("facade %d: %s\n", b, k.lastError().c_str()); return 2; }
        }
        if (mpc_controller_step_batch(h, Bc, &p, plan.data(), npl.data(), kStride, fb.data(), age.data(), rs.data(), up.data(), dtp.data(), nullptr, x.data(), u.data(), dt.data(),
                                      st.data(), it.data(), ri.data(), ng.data()) != MPC_OK) { std::printf("mpc_controller_step_batch failed: %s\n", mpc_last_error()); return 2; }
        int kinds = 0;
        for (int b = 0; b < Bc; ++b) {
            Robot& r = rb[b];
            Controller& k = *ctl[b];
            const int nb = k.gridSize();
            const double kdt = k.lastDt();
            bool same = ng[b] == nb && it[b] == k.lastIterations() && (st[b] == MPC_CONVERGED) == ok[b] && std::memcmp(&dt[b], &kdt, 8) == 0 && xs[b].size() == nb;
            if (same) same = std::memcmp(&x[(size_t)b * n * 3], xs[b].values.data(), (size_t)nb * 24) == 0 && std::memcmp(&u[(size_t)b * n * 2], us[b].values.data(), (size_t)nb * 16) == 0;
            if (ri[b] != expect[b]) same = false;
            ++compared;
            if (!same) {
                ++bad;
                std::printf("cycle %d robot %d DIFFERS: n %d/%d iters %d/%d status %d/ok %d dt %.17g/%.17g flags %d/%d x1 %.17g/%.17g\n", cyc, b, ng[b], nb, it[b], k.lastIterations(), st[b],
                            (int)ok[b], dt[b], k.lastDt(), ri[b], expect[b], x[(size_t)b * n * 3 + 3], xs[b].size() > 1 ? xs[b].at(1)[0] : 0.0);
            }
            seen |= ri[b];
            kinds |= ri[b] == 0 ? 4 : ((ri[b] & MPC_REINIT_PLAN_GUESS) ? 2 : 1);
            // closed loop: the next start is the second state of the plan, the previous control its first control
            const double* x1 = &x[(size_t)b * n * 3 + 3];
            r.pose = {x1[0], x1[1], x1[2]};
            r.u_prev[0] = u[(size_t)b * n * 2]; r.u_prev[1] = u[(size_t)b * n * 2 + 1];
            ++r.steps; r.last_goal = r.goal;
        }
        if (kinds == 7) ++mixed;
        std::printf("cycle %2d B %d flags", cyc, Bc);
        for (int b = 0; b < Bc; ++b) std::printf(" %2d", ri[b]);
        std::printf("  n");
        for (int b = 0; b < Bc; ++b) std::printf(" %2d", ng[b]);
        std::printf("  iters");
        for (int b = 0; b < Bc; ++b) std::printf(" %3d", it[b]);
        std::printf("\n");
    }
    // the slot state against the program's own bookkeeping
    std::vector<int32_t> seq((size_t)B), empty((size_t)B);
    std::vector<double> lg((size_t)B * 3);
    if (mpc_controller_state(h, B, seq.data(), empty.data(), lg.data()) != MPC_OK) return 2;
    for (int b = 0; b < B; ++b)
        if (seq[b] != rb[b].steps || empty[b] != 0 || lg[3 * b] != rb[b].goal.x || lg[3 * b + 1] != rb[b].goal.y || lg[3 * b + 2] != rb[b].goal.theta) { ++bad; std::printf("slot state of robot %d differs\n", b); }
    // mpc_reset marks every slot empty and keeps step counts and last goals
    if (mpc_reset(h) != MPC_OK || mpc_controller_state(h, B, seq.data(), empty.data(), lg.data()) != MPC_OK) return 2;
    for (int b = 0; b < B; ++b) if (seq[b] != rb[b].steps || empty[b] != 1 || lg[3 * b] != rb[b].goal.x) { ++bad; std::printf("slot state of robot %d after mpc_reset differs\n", b); }
    mpc_destroy(h);
    const int all_causes = MPC_REINIT_FIRST | MPC_REINIT_NUM_STEPS | MPC_REINIT_GOAL_DIST | MPC_REINIT_RESET | MPC_REINIT_PLAN_GUESS | (variable ? MPC_REINIT_GOAL_ANGULAR : 0);
    std::printf("compared %d robot-cycles, %d differ; causes seen %d (all: %d); launches with cold + plan guess + warm: %d\n", compared, bad, seen & all_causes, all_causes, mixed);
    if ((seen & all_causes) != all_causes) { std::printf("not every cause fired\n"); return 1; }
    if (variable && mixed == 0) { std::printf("no launch mixed the three start kinds\n"); return 1; }
    if (bad) return 1;
    std::printf("BATCH_OK\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("usage: gpu_controller_batch variable <outer_iterations> | fixed <dual_warm_start>\n"); return 2; }
    const bool variable = std::strcmp(argv[1], "variable") == 0;
    return variable ? run(true, std::atoi(argv[2]), 0) : run(false, 1, std::atoi(argv[2]));
}
