// Host build of the parameter-set policy (mpc_problem.hpp::parameter_set_error, fill_records) and of the launch plan (mpc_launch_plan.hpp) for
// tests/test_parameter_sets_host.py: plain g++, no HIP.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../mpc_local_planner_amd/csrc/mpc_launch_plan.hpp"

namespace {

// every field of Problem<T>, in declaration order
#define PROBLEM_FIELDS(X)                                                                                                                                  \
    X(model) X(n) X(dt_free) X(xf_fixed) X(objective) X(integral_form) X(collocation) X(has_Qf) X(rate_on) X(max_iter) X(p0) X(p1) X(dt_ref) X(dt_lb)    \
    X(dt_ub) X(Q) X(R) X(Qf) X(u_lb) X(u_ub) X(rate_lim) X(tol) X(mu_init) X(mu_init_warm) X(n_obst) X(n_vert) X(obst_rows) X(footprint_kind) X(d_min)    \
    X(force_incl) X(cutoff) X(fp_radius) X(fp_line) X(dyn_obst) X(fp_nv) X(fp_poly) X(ball) X(ball_S) X(ball_gamma) X(via) X(n_via) X(vp_ordered) X(vp_wp) \
    X(vp_wo) X(n_cand) X(cand_kind) X(cand_max_iter) X(cand_blend) X(cand_param) X(hess_mode) X(mu_init_dual) X(Qo) X(Ro) X(Qfo) X(So) X(trapz) X(hybrid)   \
    X(costx) X(acc_tol) X(acc_iter) X(line_search) X(pit_mu_min) X(pit) X(mu_strategy) X(max_ticks)

// names of the fields in which two records differ ("" when equal); "?" when the bytes differ outside every named field
template <typename T>
std::string diff(const mpc::Problem<T>& a, const mpc::Problem<T>& b) {
    std::string out;
#define DIFF_FIELD(f) \
    if (std::memcmp(&a.f, &b.f, sizeof(a.f)) != 0) out += std::string(out.empty() ? "" : ",") + #f;
    PROBLEM_FIELDS(DIFF_FIELD)
#undef DIFF_FIELD
    if (out.empty() && std::memcmp(&a, &b, sizeof(a)) != 0) out = "?";
    return out;
}

bool same_layout(const mpc::WaveLayout& a, const mpc::WaveLayout& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

}  // namespace

// sum of the sizes of the named fields of Problem<double> / Problem<float> (the test checks that the list misses none: the rest is padding)
extern "C" int64_t named_bytes(int f32) {
    size_t named = 0;
#define SIZE_FIELD(f) named += f32 ? sizeof(mpc::Problem<float>{}.f) : sizeof(mpc::Problem<double>{}.f);
    PROBLEM_FIELDS(SIZE_FIELD)
#undef SIZE_FIELD
    return (int64_t)named;
}
extern "C" int64_t record_bytes(int f32) { return f32 ? (int64_t)sizeof(mpc::Problem<float>) : (int64_t)sizeof(mpc::Problem<double>); }

// 1 + the reason in err when a handle created with `handle` refuses the set, 0 when it takes it
extern "C" int set_error(const mpc_config* handle, const mpc_config* set, char* err, int errlen) {
    const std::string why = mpc::parameter_set_error(*handle, *set);
    snprintf(err, (size_t)errlen, "%s", why.c_str());
    return why.empty() ? 0 : 1;
}

// the records of `set` against those of `handle` (fill_records: what mpc_create keeps and mpc_set_parameter_sets uploads): "<fp64 fields>;<fp32 fields>"
extern "C" void record_diff(const mpc_config* handle, const mpc_config* set, char* out, int outlen) {
    mpc::Problem<double> h64, s64;
    mpc::Problem<float> h32, s32;
    mpc::fill_records(*handle, h64, h32);
    mpc::fill_records(*set, s64, s32);
    snprintf(out, (size_t)outlen, "%s;%s", diff(h64, s64).c_str(), diff(h32, s32).c_str());
}

// 1 when make_launch_plan gives the same plan for both configurations
extern "C" int same_plan(const mpc_config* handle, const mpc_config* set) {
    const mpc::LaunchPlan a = mpc::make_launch_plan(*handle), b = mpc::make_launch_plan(*set);
    return a.precision == b.precision && a.level == b.level && same_layout(a.WL, b.WL) && same_layout(a.WLg, b.WLg) && a.gs64 == b.gs64 && a.gs32 == b.gs32 &&
           a.w2_ok == b.w2_ok && a.w2_min_batch == b.w2_min_batch && a.lds64 == b.lds64 && a.lds32 == b.lds32 && a.lds_w2 == b.lds_w2 &&
           a.block_bytes == b.block_bytes;
}
