// Host build of the launch decisions (mpc_problem.hpp::config_error, mpc_launch_plan.hpp) for tests/test_launch_plan.py: plain g++, no HIP.
#include <cstdint>
#include <cstdio>

#include "../../mpc_local_planner_amd/csrc/mpc_launch_plan.hpp"

// One row of the test's table (rc 0), or the text mpc_create refuses the configuration with (rc 1).  Columns:
//   level, gs64, gs32, mpc_lds_bytes | fp64 launch of 4095 instances: global form, two waves, LDS | of 4096: the same three | fp32 launch of 4096: global form, LDS |
//   pool blocks per XCD on a device of 256 CUs and 8 XCCs at 4 workgroups per CU, block bytes, kept-multiplier words | the pool's kernel: global form, LDS
// (-1: the handle launches no kernel of that precision)
extern "C" int plan_row(const mpc_config* cfg, int64_t* out, char* err, int errlen) {
    const char* e = mpc::config_error(*cfg);
    const mpc::LaunchPlan p = mpc::make_launch_plan(*cfg);
    if (!e) e = mpc::plan_error(p);
    if (e) { snprintf(err, (size_t)errlen, "%s", e); return 1; }
    const bool f32 = cfg->precision == MPC_FP32, f64 = cfg->precision != MPC_FP32;
    auto put = [&](int at, const mpc::KernelChoice& k, bool w2) { out[at] = k.L.GSF; if (w2) out[at + 1] = k.w2; out[at + (w2 ? 2 : 1)] = (int64_t)k.lds; };
    for (int i = 0; i < 17; ++i) out[i] = -1;
    out[0] = p.level; out[1] = p.gs64; out[2] = p.gs32; out[3] = (int64_t)p.lds();
    if (f64) { put(4, mpc::plan_launch(p, false, 4095), true); put(7, mpc::plan_launch(p, false, 4096), true); }
    if (cfg->precision != MPC_FP64) put(10, mpc::plan_launch(p, true, 4096), false);
    out[12] = mpc::pool_blocks_per_xcd(p, 4, 256, 8); out[13] = (int64_t)p.block_bytes; out[14] = mpc::dual_words(p.WL.NS);
    put(15, mpc::plan_launch(p, f32, 0), false);
    return 0;
}
