// mpc_evaluate.hpp -- what a trajectory is worth under the handle's NLP (mpc_evaluate_batch* of include/mpc_hip.h): the objective the solve minimises, the largest
// violation of the collocation equations and of the inequality rows, and the clearance to EVERY obstacle of the instance.  A kernel of its own, next to the solve
// (the solve kernels are not touched): it reads a trajectory the way a solve would start from it -- x_0 := x0, fixed goal components := xf
// (full_discretization_grid_base_se2.cpp:101-110) -- and evaluates the rows in the REFERENCE's form, in fp64 whatever the handle's precision is:
//   objective     (n-1) dt | via-points (min_time_via_points_cost.cpp:120-145) | quadratic form, sum / left sum / trapezoid, hybrid (quadratic_cost_se2.cpp:31-83,
//                 finite_differences_grid_se2.cpp:61-75) + terminal cost on a goal that is not completely fixed (final_state_conditions_se2.cpp:30-52)
//   equalities    f - (x_{k+1} - x_k) / dt, forward / midpoint / Crank-Nicolson as coded (fd_collocation_se2.h:54-69, 91-108, 130-147: 1.5 f(x_{k+1}) + 0.5 f(x_k))
//   inequalities  control box, dt box, control-rate rows with the first (against u_prev / dt_prev) and the final one (against u_ref = 0)
//                 (stage_inequality_se2.cpp:191-222, finite_differences_grid_se2.cpp:150), terminal ball (final_state_conditions_se2.cpp:54-64)
//   clearance     teb's footprint / obstacle distances, value only (the solve kernel's, mpc_wave_rows.inc, live in LDS and carry derivatives)
// The per-item arithmetic is __host__ __device__: the CPU suite compiles it with g++ (tests/host_harness/evaluate_host.cpp) and holds it to the numpy restatement of the NLP.
// evaluate_instance is written for one lane of `nl`; the reductions go through a policy: the wavefront's butterfly on the device (EvalWaveRed), nothing on the
// host (one lane).  Every reduction has a fixed order, so a result depends neither on the batch nor on the run.
#pragma once
#include <stdint.h>
#include <math.h>

#include "../../include/mpc_hip.h"
#include "mpc_core.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MPC_EV_HD __host__ __device__ __forceinline__
#else
#define MPC_EV_HD inline
#endif

namespace mpc {

// The handle's configuration as the evaluation reads it: fp64, weights unscaled, rows in the reference's form (the solve's Problem<T> is in solver form: weights
// scaled by dt_ref on the fixed grid, the trapezoid's final term folded into Qf).  One record per table entry (entry 0: the handle's own, then the parameter sets).
struct EvalParams {
    int32_t model, n, dt_free, xf_fixed[3], collocation, objective, integral_form, trapz, hybrid, has_Qf, ball;
    int32_t rate_lo[2], rate_hi[2];      // finite control-rate bound?
    int32_t n_via, vp_ordered, fp_kind, fp_nv, dyn, O, V;
    double p0, p1, dt_ref, dt_lb, dt_ub;
    double Q[6], R[3], Qf[6], S[6];      // symmetric weights: diagonal, then the (0,1), (0,2), (1,2) terms (R: (0,1))
    double gamma, u_lb[2], u_ub[2], du_lb[2], du_ub[2], vp_wp, vp_wo, fp_radius, fp_par[4], fp_poly[32];
};

inline void fill_eval_params(const mpc_config& c, EvalParams& E) {
    E = EvalParams();
    const bool quad = c.objective == MPC_OBJ_QUADRATIC, free_goal = !(c.xf_fixed[0] && c.xf_fixed[1] && c.xf_fixed[2]);
    E.model = c.model; E.n = c.n; E.dt_free = c.dt_free ? 1 : 0; E.collocation = c.collocation; E.objective = c.objective;
    for (int i = 0; i < 3; ++i) E.xf_fixed[i] = c.xf_fixed[i] ? 1 : 0;
    E.integral_form = (quad && c.integral_form) ? 1 : 0;
    E.trapz = (E.integral_form && c.cost_integration == MPC_COST_TRAPEZOIDAL) ? 1 : 0;
    E.hybrid = (quad && c.hybrid_cost_minimum_time) ? 1 : 0;
    E.has_Qf = (c.has_Qf && free_goal) ? 1 : 0;       // the edges exist only while the final state is not completely fixed (finite_differences_grid_se2.cpp:128-143)
    E.ball = (c.terminal_ball && free_goal) ? 1 : 0;
    for (int j = 0; j < 2; ++j) { E.rate_lo[j] = c.du_lb[j] > -1e29 ? 1 : 0; E.rate_hi[j] = c.du_ub[j] < 1e29 ? 1 : 0; E.du_lb[j] = c.du_lb[j]; E.du_ub[j] = c.du_ub[j]; E.u_lb[j] = c.u_lb[j]; E.u_ub[j] = c.u_ub[j]; }
    E.n_via = c.objective == MPC_OBJ_MIN_TIME_VIA_POINTS ? c.max_via_points : 0;
    E.vp_ordered = c.via_points_ordered ? 1 : 0; E.vp_wp = c.vp_position_weight; E.vp_wo = c.vp_orientation_weight;
    E.O = c.max_obstacles > 0 ? c.max_obstacles : 0; E.V = c.max_vertices > 0 ? c.max_vertices : 1;
    E.dyn = (c.enable_dynamic_obstacles && E.O > 0) ? 1 : 0;
    E.fp_kind = c.footprint_kind;
    E.fp_nv = c.footprint_kind == MPC_FOOTPRINT_POLYGON ? (c.footprint_n_vertices < 16 ? c.footprint_n_vertices : 16) : 0;
    E.fp_radius = c.footprint_kind == MPC_FOOTPRINT_CIRCLE ? c.footprint_radius : 0.0;
    for (int i = 0; i < 4; ++i) E.fp_par[i] = c.footprint_params[i];
    for (int i = 0; i < 32; ++i) E.fp_poly[i] = i < 2 * E.fp_nv ? c.footprint_vertices[i] : 0.0;
    E.p0 = c.model_params[0]; E.p1 = c.model_params[1]; E.dt_ref = c.dt_ref; E.dt_lb = c.dt_lb; E.dt_ub = c.dt_ub;
    for (int i = 0; i < 3; ++i) {
        E.Q[i] = quad ? c.Q[i] : 0.0; E.Q[3 + i] = quad ? c.Q_offdiag[i] : 0.0;
        E.Qf[i] = c.Qf[i]; E.Qf[3 + i] = c.Qf_offdiag[i];
        E.S[i] = c.terminal_ball_S[i]; E.S[3 + i] = c.terminal_ball_S_offdiag[i];
    }
    E.R[0] = quad ? c.R[0] : 0.0; E.R[1] = quad ? c.R[1] : 0.0; E.R[2] = quad ? c.R_offdiag : 0.0;
    E.gamma = c.terminal_ball_gamma;
}

struct EvalArgs {
    const EvalParams* tab;         // entry 0: the handle's configuration, entries 1 ..: the parameter sets in force
    const int32_t* set_of;         // [B] table entry of instance b, or NULL (entry 0)
    const int32_t* n_grid;         // [B] grid sizes, or NULL (E.n)
    int32_t n_stride;              // cfg.n: the stride of x / u
    const double *x0, *xf, *u_prev, *dt_prev;      // [B][3] [B][3] [B][2] [B], each nullable
    const double *x, *u, *dt;      // [B][n_stride][3], [B][n_stride][2], [B]
    mpc_obstacles ob;              // pointers NULL: no obstacles
    const int32_t* n_via;          // [B] or NULL
    const double* via;             // [B][E.n_via][3]
    mpc_eval_out out;
};

// ---- robot models and the collocation rows in the reference's form
template <int MODEL>
MPC_EV_HD void ev_f(const EvalParams& E, double th, const double u[2], double f[3]) {
    Problem<double> P;      // (only the model parameters are read)
    P.p0 = E.p0; P.p1 = E.p1;
    double tr[4];
    model_trig<double, MODEL>(P, th, u[1], tr);
    model_f<double, MODEL>(P, tr, u[0], u[1], f);
}
MPC_EV_HD void ev_dynamics(const EvalParams& E, double th, const double u[2], double f[3]) {
    switch (E.model) {
        case MODEL_UNICYCLE: ev_f<MODEL_UNICYCLE>(E, th, u, f); break;
        case MODEL_SIMPLE_CAR: ev_f<MODEL_SIMPLE_CAR>(E, th, u, f); break;
        case MODEL_SIMPLE_CAR_FRONT: ev_f<MODEL_SIMPLE_CAR_FRONT>(E, th, u, f); break;
        default: ev_f<MODEL_KINEMATIC_BICYCLE>(E, th, u, f); break;
    }
}
// one FDCollocationEdge (x1, u1, x2, dt) -> 3 rows
MPC_EV_HD void ev_defect(const EvalParams& E, const double x1[3], const double u1[2], const double x2[3], double dt, double r[3]) {
#pragma clang fp contract(off)
    const double dth = normalize_theta(x2[2] - x1[2]);
    const double q[3] = {(x2[0] - x1[0]) / dt, (x2[1] - x1[1]) / dt, dth / dt};
    double f[3];
    if (E.collocation == COLLOC_CN) {
        double f1[3];
        ev_dynamics(E, x1[2], u1, f1);
        ev_dynamics(E, x2[2], u1, f);
        for (int i = 0; i < 3; ++i) { const double h = 0.5 * (f1[i] + f[i]); r[i] = f[i] - (q[i] - h); }      // error = f2; error -= quot - 0.5 (f1 + error)
        return;
    }
    const double th = E.collocation == COLLOC_MID ? normalize_theta(x1[2] + 0.5 * dth) : x1[2];      // interpolate_angle(th1, th2, 0.5)
    ev_dynamics(E, th, u1, f);
    for (int i = 0; i < 3; ++i) r[i] = f[i] - q[i];
}
// xd' W xd for W = (diagonal, (0,1), (0,2), (1,2))
MPC_EV_HD double ev_quad3(const double W[6], const double xd[3]) {
#pragma clang fp contract(off)
    const double d = W[0] * xd[0] * xd[0] + W[1] * xd[1] * xd[1] + W[2] * xd[2] * xd[2];
    const double o = W[3] * xd[0] * xd[1] + W[4] * xd[0] * xd[2] + W[5] * xd[1] * xd[2];
    return d + 2.0 * o;
}
// the start state and the goal of an instance (scalars: an array here ends up in scratch memory)
struct EvEnds { double x0x, x0y, x0t, xfx, xfy, xft; };
MPC_EV_HD double ev_state_error_cost(const double W[6], const double x[3], const EvEnds& e) {
#pragma clang fp contract(off)
    const double xd[3] = {x[0] - e.xfx, x[1] - e.xfy, normalize_theta(x[2] - e.xft)};      // quadratic_cost_se2.cpp:36-37
    return ev_quad3(W, xd);
}

// ---- footprint / obstacle distances (teb semantics, value only): unsigned, closed edge loops without an inside test, 0 where two segments cross
MPC_EV_HD double ev_norm2(double dx, double dy) {
#pragma clang fp contract(off)
    return __builtin_sqrt(dx * dx + dy * dy);
}
MPC_EV_HD double ev_pt_seg(double px, double py, double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    const double abx = bx - ax, aby = by - ay, sq = abx * abx + aby * aby;
    if (sq == 0.0) return ev_norm2(px - ax, py - ay);
    double t = ((px - ax) * abx + (py - ay) * aby) / sq;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    return ev_norm2(px - (ax + t * abx), py - (ay + t * aby));
}
MPC_EV_HD double ev_orient(double px, double py, double qx, double qy, double rx, double ry) {
#pragma clang fp contract(off)
    return (qx - px) * (ry - py) - (qy - py) * (rx - px);
}
MPC_EV_HD double ev_seg_seg(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
#pragma clang fp contract(off)
    const double o1 = ev_orient(ax, ay, bx, by, cx, cy), o2 = ev_orient(ax, ay, bx, by, dx, dy), o3 = ev_orient(cx, cy, dx, dy, ax, ay), o4 = ev_orient(cx, cy, dx, dy, bx, by);
    if (o1 * o2 < 0.0 && o3 * o4 < 0.0) return 0.0;
    const double d0 = ev_pt_seg(ax, ay, cx, cy, dx, dy), d1 = ev_pt_seg(bx, by, cx, cy, dx, dy), d2 = ev_pt_seg(cx, cy, ax, ay, bx, by), d3 = ev_pt_seg(dx, dy, ax, ay, bx, by);
    const double m = d0 < d1 ? d0 : d1, m2 = d2 < d3 ? d2 : d3;
    return m < m2 ? m : m2;
}
// one obstacle: nv vertices (1: point / circle, 2: line, >= 3: closed polygon), moved by (sx, sy); r is subtracted from every distance, as the solve kernel does
struct EvObst { const double* v; int nv; double r, sx, sy; };
MPC_EV_HD double ev_ox(const EvObst& o, int i) { return o.v[2 * i] + o.sx; }
MPC_EV_HD double ev_oy(const EvObst& o, int i) { return o.v[2 * i + 1] + o.sy; }
MPC_EV_HD double ev_pt_obst(double px, double py, const EvObst& o) {
    if (o.nv <= 1) return ev_norm2(px - ev_ox(o, 0), py - ev_oy(o, 0)) - o.r;
    const int ne = o.nv == 2 ? 1 : o.nv;
    double m = INFINITY;
    for (int e = 0; e < ne; ++e) {
        const int e2 = e + 1 < o.nv ? e + 1 : 0;
        const double d = ev_pt_seg(px, py, ev_ox(o, e), ev_oy(o, e), ev_ox(o, e2), ev_oy(o, e2));
        m = d < m ? d : m;
    }
    return m - o.r;
}
MPC_EV_HD double ev_seg_obst(double ax, double ay, double bx, double by, const EvObst& o) {
    if (o.nv <= 1) return ev_pt_seg(ev_ox(o, 0), ev_oy(o, 0), ax, ay, bx, by) - o.r;
    const int ne = o.nv == 2 ? 1 : o.nv;
    double m = INFINITY;
    for (int e = 0; e < ne; ++e) {
        const int e2 = e + 1 < o.nv ? e + 1 : 0;
        const double d = ev_seg_seg(ax, ay, bx, by, ev_ox(o, e), ev_oy(o, e), ev_ox(o, e2), ev_oy(o, e2));
        m = d < m ? d : m;
    }
    return m - o.r;
}
// vertex i of the polygon footprint in the world frame
MPC_EV_HD void ev_fp_vertex(const EvalParams& E, const double pose[3], double s, double c, int i, double& wx, double& wy) {
#pragma clang fp contract(off)
    const double vx = E.fp_poly[2 * i], vy = E.fp_poly[2 * i + 1];
    wx = pose[0] + (c * vx - s * vy); wy = pose[1] + (s * vx + c * vy);
}
// RobotFootprintModel::calculateDistance of the footprint placed at `pose`
MPC_EV_HD double ev_footprint_distance(const EvalParams& E, const double pose[3], const EvObst& o) {
#pragma clang fp contract(off)
    const double px = pose[0], py = pose[1];
    if (E.fp_kind == MPC_FOOTPRINT_POINT) return ev_pt_obst(px, py, o);
    if (E.fp_kind == MPC_FOOTPRINT_CIRCLE) return ev_pt_obst(px, py, o) - E.fp_radius;
    double s, c;
    t_sincos(pose[2], &s, &c);
    if (E.fp_kind == MPC_FOOTPRINT_LINE) {
        const double sx = E.fp_par[0], sy = E.fp_par[1], ex = E.fp_par[2], ey = E.fp_par[3];
        return ev_seg_obst(px + (c * sx - s * sy), py + (s * sx + c * sy), px + (c * ex - s * ey), py + (s * ex + c * ey), o);
    }
    if (E.fp_kind == MPC_FOOTPRINT_TWO_CIRCLES) {
        const double fo = E.fp_par[0], fr = E.fp_par[1], ro = E.fp_par[2], rr = E.fp_par[3];
        const double df = ev_pt_obst(px + fo * c, py + fo * s, o) - fr, dr = ev_pt_obst(px - ro * c, py - ro * s, o) - rr;
        return df < dr ? df : dr;
    }
    // polygon footprint: its closed edge loop (1 vertex: a point, 2: one edge) against the obstacle
    const int nv = E.fp_nv, ne = nv == 2 ? 1 : nv;
    double ax, ay, bx, by;
    ev_fp_vertex(E, pose, s, c, 0, ax, ay);
    if (nv <= 1) return ev_pt_obst(ax, ay, o);
    double m = INFINITY;
    for (int e = 0; e < ne; ++e) {
        ev_fp_vertex(E, pose, s, c, e, ax, ay);
        ev_fp_vertex(E, pose, s, c, e + 1 < nv ? e + 1 : 0, bx, by);
        const double d = o.nv <= 1 ? ev_pt_seg(ev_ox(o, 0), ev_oy(o, 0), ax, ay, bx, by) - o.r : ev_seg_obst(ax, ay, bx, by, o);
        m = d < m ? d : m;
    }
    return m;
}

// ---- one instance, one lane of nl.  Red: sum / max / any over the lanes and the lexicographic arg-min (value, index), the same result in every lane.
struct EvalSerialRed {      // one lane: nothing to reduce
    MPC_EV_HD double sum(double v) const { return v; }
    MPC_EV_HD double max(double v) const { return v; }
    MPC_EV_HD bool any(bool v) const { return v; }
    MPC_EV_HD void argmin(double&, int&) const {}
};

// state k of the trajectory as a solve starts from it: x_0 := x0, fixed goal components := xf
MPC_EV_HD void ev_state(const EvalParams& E, const double* x, int n, int k, const EvEnds& e, double out[3]) {
    const bool first = k == 0, last = k == n - 1;
    out[0] = first ? e.x0x : ((last && E.xf_fixed[0]) ? e.xfx : x[3 * k]);
    out[1] = first ? e.x0y : ((last && E.xf_fixed[1]) ? e.xfy : x[3 * k + 1]);
    out[2] = first ? e.x0t : ((last && E.xf_fixed[2]) ? e.xft : x[3 * k + 2]);
}
MPC_EV_HD bool ev_bad3(const double v[3]) { return !(t_finite(v[0]) && t_finite(v[1]) && t_finite(v[2])); }
MPC_EV_HD double ev_pos(double v) { return v > 0.0 ? v : 0.0; }

template <class Red>
MPC_EV_HD void evaluate_instance(const EvalArgs& a, int b, int lane, int nl, const Red& red) {
#pragma clang fp contract(off)
    const EvalParams& E = a.tab[a.set_of ? a.set_of[b] : 0];
    const int ns = a.n_stride;
    int n = a.n_grid ? a.n_grid[b] : E.n;
    n = n < 3 ? 3 : (n > ns ? ns : n);
    const double* x = a.x + (size_t)b * ns * 3;
    const double* u = a.u + (size_t)b * ns * 2;
    bool bad = false;
    const double* p0 = a.x0 ? a.x0 + 3 * (size_t)b : x;
    const double* pf = a.xf ? a.xf + 3 * (size_t)b : x + 3 * (n - 1);
    const EvEnds ends = {p0[0], p0[1], normalize_theta(p0[2]), pf[0], pf[1], normalize_theta(pf[2])};      // the headings as the solve kernel reads them
    const double up0 = a.u_prev ? a.u_prev[2 * (size_t)b] : 0.0, up1 = a.u_prev ? a.u_prev[2 * (size_t)b + 1] : 0.0;
    const double dtp = a.dt_prev ? a.dt_prev[b] : 0.0;
    const double dt = E.dt_free ? a.dt[b] : E.dt_ref;
    bad = !(t_finite(ends.x0x) && t_finite(ends.x0y) && t_finite(ends.x0t) && t_finite(ends.xfx) && t_finite(ends.xfy) && t_finite(ends.xft) && t_finite(up0) && t_finite(up1) &&
            t_finite(dtp) && t_finite(dt));
    const bool quad = E.objective == MPC_OBJ_QUADRATIC;

    // ---- grid points: item k < n - 1 is interval k (collocation rows, control box, rate row k, stage cost), item n - 1 everything at the end of the horizon
    double obj = 0.0, eq = 0.0, iq = 0.0;
    for (int k = lane; k < n; k += nl) {
        double x1[3];
        ev_state(E, x, n, k, ends, x1);
        bad = bad || ev_bad3(x1);
        if (k < n - 1) {
            double x2[3], r[3];
            const double uk[2] = {u[2 * k], u[2 * k + 1]};
            ev_state(E, x, n, k + 1, ends, x2);
            bad = bad || !t_finite(uk[0]) || !t_finite(uk[1]);
            ev_defect(E, x1, uk, x2, dt, r);
            for (int i = 0; i < 3; ++i) eq = t_max(eq, t_abs(r[i]));
            for (int j = 0; j < 2; ++j) iq = t_max(iq, t_max(E.u_lb[j] - uk[j], uk[j] - E.u_ub[j]));
            if (k > 0 || dtp != 0.0) {      // the first row exists only with a previous control (stage_inequality_se2.cpp:197-201)
                const double d = k > 0 ? dt : dtp;
                for (int j = 0; j < 2; ++j) {
                    const double rate = (uk[j] - (k > 0 ? u[2 * (k - 1) + j] : (j ? up1 : up0))) / d;
                    if (E.rate_lo[j]) iq = t_max(iq, E.du_lb[j] - rate);
                    if (E.rate_hi[j]) iq = t_max(iq, rate - E.du_ub[j]);
                }
            }
            if (quad) {
                const double ctrl = E.R[0] * uk[0] * uk[0] + E.R[1] * uk[1] * uk[1] + 2.0 * (E.R[2] * uk[0] * uk[1]);
                const double l1 = ev_state_error_cost(E.Q, x1, ends) + ctrl;
                if (!E.integral_form) obj += l1;
                else if (E.trapz) obj += 0.5 * dt * (l1 + (ev_state_error_cost(E.Q, x2, ends) + ctrl));      // TrapezoidalIntegralCostEdge(x_k, u_k, x_{k+1}, dt)
                else obj += dt * l1;
            }
        } else {
            for (int j = 0; j < 2; ++j) {      // getFinalControlDeviationEdges(n, u_ref = 0, u_{n-2}, dt)
                const double rate = (0.0 - u[2 * (n - 2) + j]) / dt;
                if (E.rate_lo[j]) iq = t_max(iq, E.du_lb[j] - rate);
                if (E.rate_hi[j]) iq = t_max(iq, rate - E.du_ub[j]);
            }
            if (E.dt_free) iq = t_max(iq, t_max(E.dt_lb - dt, dt - E.dt_ub));
            if (E.ball) { const double xd[3] = {x1[0] - ends.xfx, x1[1] - ends.xfy, normalize_theta(x1[2] - ends.xft)}; iq = t_max(iq, ev_quad3(E.S, xd) - E.gamma); }
            if (!quad || E.hybrid) obj += (double)(n - 1) * dt;
            if (E.has_Qf) obj += ev_state_error_cost(E.Qf, x1, ends);
        }
    }
    obj = red.sum(obj); eq = red.max(eq); iq = red.max(iq);

    // ---- via-points: each attached to its closest grid point of THIS trajectory (MinTimeViaPointsCost::update, min_time_via_points_cost.cpp:39-117), one after
    // the other (the ordered mode starts a search two states behind the previous match); the lanes share a search, the cost term is the same in every lane
    if (E.n_via > 0 && a.n_via && a.via) {
        int nvp = a.n_via[b];
        nvp = nvp < 0 ? 0 : (nvp > E.n_via ? E.n_via : nvp);
        const double* vp = a.via + (size_t)b * E.n_via * 3;
        int start = 0;
        for (int v = 0; v < nvp; ++v) {
            const double vx = vp[3 * v], vy = vp[3 * v + 1], vth = vp[3 * v + 2];
            bad = bad || !t_finite(vx) || !t_finite(vy) || !t_finite(vth);
            double dm = 1.7976931348623157e308, xs[3];
            int im = -1;
            for (int i = start + lane; i < n - 1; i += nl) {      // findClosestPose: the first minimum over start .. n-2 ...
                ev_state(E, x, n, i, ends, xs);
                const double d = ev_norm2(vx - xs[0], vy - xs[1]);
                if (d < dm) { dm = d; im = i; }
            }
            red.argmin(dm, im);
            ev_state(E, x, n, n - 1, ends, xs);
            if (ev_norm2(vx - xs[0], vy - xs[1]) < dm) im = n - 1;      // ... then the final state when it is strictly closer
            if (E.vp_ordered) start = im + 2;
            int idx = im > n - 2 ? n - 2 : im;
            if (idx < 1) { if (!E.vp_ordered) continue; idx = 1; }
            ev_state(E, x, n, idx, ends, xs);
            const double ex = vx - xs[0], ey = vy - xs[1];
            obj += E.vp_wp * (ex * ex + ey * ey);
            if (E.vp_wo > 0.0) obj += E.vp_wo * normalize_theta(vth - xs[2]);      // linear in the heading error, as coded (:139-142)
        }
    }

    // ---- clearance: every (grid point 1 .. n-2, valid obstacle) pair, lexicographic arg-min
    double cl = INFINITY;
    int cp = 0x7fffffff;
    int no = (E.O > 0 && a.ob.n_obstacles && a.ob.n_vertices && a.ob.vertices) ? a.ob.n_obstacles[b] : 0;
    no = no < 0 ? 0 : (no > E.O ? E.O : no);
    const int pairs = (n - 2) * no;
    for (int p = lane; p < pairs; p += nl) {
        const int k = 1 + p / no, o = p % no;
        const size_t bo = (size_t)b * E.O + o;
        double pose[3];
        ev_state(E, x, n, k, ends, pose);
        EvObst ob;
        ob.nv = a.ob.n_vertices[bo]; ob.nv = ob.nv > E.V ? E.V : ob.nv;
        if (ob.nv <= 0) continue;      // an empty slot below n_obstacles[b] is no obstacle (the solve skips it too): its vertices are never read
        ob.v = a.ob.vertices + bo * E.V * 2;
        ob.r = a.ob.radius ? a.ob.radius[bo] : 0.0;
        ob.sx = 0.0; ob.sy = 0.0;
        if (E.dyn && a.ob.velocity) { const double t = (double)k * dt; ob.sx = t * a.ob.velocity[2 * bo]; ob.sy = t * a.ob.velocity[2 * bo + 1]; }      // estimateSpatioTemporalDistance(k dt)
        const double d = ev_footprint_distance(E, pose, ob);
        bad = bad || !t_finite(d);
        if (d < cl) { cl = d; cp = p; }
    }
    red.argmin(cl, cp);
    bad = red.any(bad);

    if (lane == 0) {
        const double nan = __builtin_nan("");
        const bool none = pairs <= 0 || cp == 0x7fffffff;
        if (a.out.objective) a.out.objective[b] = bad ? nan : obj;
        if (a.out.eq_violation) a.out.eq_violation[b] = bad ? nan : eq;
        if (a.out.ineq_violation) a.out.ineq_violation[b] = bad ? nan : ev_pos(iq);
        if (a.out.clearance) a.out.clearance[b] = bad ? nan : cl;
        if (a.out.closest) { a.out.closest[2 * (size_t)b] = (bad || none) ? -1 : 1 + cp / no; a.out.closest[2 * (size_t)b + 1] = (bad || none) ? -1 : cp % no; }
    }
}

#if defined(__HIPCC__)
// the wavefront's reductions: a butterfly over the 64 lanes (xor 32, 16, .., 1); both partners of a step combine the same two values, so every lane ends with the
// same bits and the order of the combination is fixed
struct EvalWaveRed {
    __device__ __forceinline__ double sum(double v) const { for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64); return v; }
    __device__ __forceinline__ double max(double v) const { for (int m = 32; m > 0; m >>= 1) v = t_max(v, __shfl_xor(v, m, 64)); return v; }
    __device__ __forceinline__ bool any(bool v) const { return __ballot(v) != 0ull; }
    __device__ __forceinline__ void argmin(double& d, int& i) const {
        for (int m = 32; m > 0; m >>= 1) {
            const double od = __shfl_xor(d, m, 64);
            const int oi = __shfl_xor(i, m, 64);
            if (od < d || (od == d && oi < i)) { d = od; i = oi; }
        }
    }
};

// one wavefront per instance
__global__ __launch_bounds__(64) void evaluate_kernel(EvalArgs a) {
    evaluate_instance(a, (int)blockIdx.x, (int)threadIdx.x, 64, EvalWaveRed());
}
#endif  // __HIPCC__

}  // namespace mpc
