// Tests-only host build of mpc_local_planner_amd/csrc/mpc_evaluate.hpp: the per-item arithmetic of mpc_evaluate_batch* compiled with g++ and driven one lane at a
// time (tests/test_evaluate_host.py holds it to oracle/se2_nlp.py).  With -DEVALUATE_HOST_MAIN a stand-alone program that runs a few cases (sanitizer builds).
#include <cstdio>
#include <vector>

#include "../../mpc_local_planner_amd/csrc/mpc_evaluate.hpp"

extern "C" {

// instance b is evaluated with sets[set_of[b]] (set_of == NULL: sets[0]); every other argument as mpc_evaluate_batch
int evh_evaluate(const mpc_config* sets, int n_sets, const int32_t* set_of, int B, const int32_t* n_grid, const double* x0, const double* xf, const double* u_prev,
                 const double* dt_prev, const double* x, const double* u, const double* dt, const mpc_obstacles* ob, const int32_t* n_via, const double* via,
                 const mpc_eval_out* out) {
    if (!sets || n_sets < 1 || !x || !u || !out) return -1;
    std::vector<mpc::EvalParams> tab((size_t)n_sets);
    for (int i = 0; i < n_sets; ++i) mpc::fill_eval_params(sets[i], tab[(size_t)i]);
    mpc::EvalArgs a{};
    a.tab = tab.data(); a.set_of = set_of; a.n_grid = n_grid; a.n_stride = sets[0].n;
    a.x0 = x0; a.xf = xf; a.u_prev = u_prev; a.dt_prev = dt_prev; a.x = x; a.u = u; a.dt = dt;
    if (ob) a.ob = *ob;
    a.n_via = n_via; a.via = via; a.out = *out;
    for (int b = 0; b < B; ++b) mpc::evaluate_instance(a, b, 0, 1, mpc::EvalSerialRed());
    return 0;
}

unsigned evh_sizeof_params(void) { return (unsigned)sizeof(mpc::EvalParams); }

}  // extern "C"

#ifdef EVALUATE_HOST_MAIN
int main() {
    mpc_config c{};
    c.model = MPC_MODEL_SIMPLE_CAR; c.model_params[0] = 0.4; c.n = 7; c.dt_ref = 0.3; c.dt_free = 1; c.dt_ub = 10.0;
    c.xf_fixed[0] = c.xf_fixed[1] = c.xf_fixed[2] = 1; c.objective = MPC_OBJ_MIN_TIME;
    c.u_lb[0] = -0.2; c.u_ub[0] = 0.4; c.u_lb[1] = -1.4; c.u_ub[1] = 1.4;
    for (int j = 0; j < 2; ++j) { c.du_lb[j] = -0.5; c.du_ub[j] = 0.5; }
    c.max_obstacles = 2; c.max_vertices = 4; c.footprint_kind = MPC_FOOTPRINT_POLYGON; c.footprint_n_vertices = 3;
    const double fp[6] = {0.3, 0.0, -0.2, 0.15, -0.2, -0.15};
    for (int i = 0; i < 6; ++i) c.footprint_vertices[i] = fp[i];
    const int B = 3, n = c.n;
    std::vector<double> x((size_t)B * n * 3), u((size_t)B * n * 2), dt(B, 0.25), verts((size_t)B * 2 * 4 * 2);
    for (size_t i = 0; i < x.size(); ++i) x[i] = 0.1 * (double)(i % 17) - 0.5;
    for (size_t i = 0; i < u.size(); ++i) u[i] = 0.05 * (double)(i % 7) - 0.1;
    for (size_t i = 0; i < verts.size(); ++i) verts[i] = 0.3 * (double)(i % 5) + 1.0 + (double)(i % 3);
    std::vector<int32_t> no(B, 2), nv((size_t)B * 2, 4), ngrid = {7, 3, 5}, closest((size_t)B * 2);
    no[1] = 0; nv[0] = 1; nv[1] = 2;
    std::vector<double> obj(B), eq(B), iq(B), cl(B);
    const mpc_obstacles ob = {no.data(), nv.data(), verts.data(), nullptr, nullptr};
    const mpc_eval_out out = {obj.data(), eq.data(), iq.data(), cl.data(), closest.data()};
    for (int coll = 0; coll < 3; ++coll) {
        c.collocation = coll;
        if (evh_evaluate(&c, 1, nullptr, B, ngrid.data(), nullptr, nullptr, nullptr, nullptr, x.data(), u.data(), dt.data(), &ob, nullptr, nullptr, &out) != 0) return 1;
        for (int b = 0; b < B; ++b) std::printf("%d %d %.17g %.17g %.17g %.17g %d %d\n", coll, b, obj[b], eq[b], iq[b], cl[b], closest[2 * b], closest[2 * b + 1]);
    }
    return 0;
}
#endif
