// mpc_launch_plan.hpp -- which solve kernel a launch runs, decided once per handle from its mpc_config (host only; plain C++).
//
// A solve launch is served by one kernel instantiation, picked by the kernel level, the form (factorisation data in LDS, or in a block of global memory:
// GlobalStage), one or two waves per SIMD, the fixed n = 50 layout and the dynamic LDS.  mpc_create computes the LaunchPlan; plan_launch() is the one place
// that combines its fields into the answer for one launch (launch, mpc_occupancy and the pool sizing of mpc_capi.hip ask it); select_kernel
// (mpc_solve_kernel.hpp) maps that answer to an instantiation and picks the fixed layout, which is a question of the template parameters.
#pragma once
#include <cstddef>

#include "../../include/mpc_hip.h"
#include "mpc_core.hpp"
#include "mpc_layout.hpp"
#include "mpc_problem.hpp"

namespace mpc {

constexpr size_t kLdsPerCu = 160u * 1024u;      // LDS of a CU
constexpr int kFixedLayoutNS = 50;              // the grid size whose record layout is compiled into a kernel of its own (FixedLayout; select_kernel)

// dynamic LDS of one workgroup: the record of T-sized words, then (16-byte aligned, 16 bytes further) the problem record (mpc_solve_kernel.hpp)
inline size_t lds_bytes(const WaveLayout& L, size_t tsize, size_t psize) { return ((((size_t)L.total * tsize) + 15) & ~(size_t)15) + 16 + ((psize + 15) & ~(size_t)15); }

// what one launch runs
struct KernelChoice {
    int level;          // 0 the headline instantiation, 1 + the rarely used rows / terms / coupling slots, 2 + the cost variants (IpmWave's EXT)
    bool w2;            // the two-waves-per-SIMD kernel (fp64, level 0, no clearance rows, LDS form)
    WaveLayout L;       // the record; L.GSF = 1: the global form
    size_t lds;         // dynamic LDS of one workgroup
    int shape;          // != 0: the fixed-layout kernel that has this shape word compiled in (mpc_core.hpp::kHeadlineShape); 0: the kernel reads the word at run time
};

struct LaunchPlan {
    int precision;              // mpc_config.precision
    int level;
    WaveLayout WL, WLg;         // the LDS form, the global form
    bool gs64, gs32;            // the global form for the fp64 / fp32 launches
    bool w2_ok;                 // fp64 launches of at least w2_min_batch instances run the two-wave kernel
    int w2_min_batch;
    size_t lds64, lds32, lds_w2;      // dynamic LDS of the fp64 / fp32 one-wave kernel and of the two-wave kernel (0 for a kernel the handle never launches)
    size_t block_bytes;         // one block of the per-XCD pools (global form, or the clearance rows' elastic arrays); 0: the handle has no pool
    int flags;                  // the handle's shape word (mpc_core.hpp::shape_flags of its problem record: what solve() computes in the kernel)
    bool shape_ok;              // the one-wave fp64 launches run the fixed-layout kernel compiled for kHeadlineShape
    size_t lds() const { return precision == MPC_FP32 ? lds32 : lds64; }      // the larger of the two phases under MPC_MIXED (mpc_lds_bytes)
};

// what a launch of B instances in fp32 (f32) or fp64 runs; B = 0 asks for the one-wave kernel (the one that claims the pool's blocks)
inline KernelChoice plan_launch(const LaunchPlan& p, bool f32, int B) {
    if (!f32 && p.w2_ok && B >= p.w2_min_batch) return {p.level, true, p.WL, p.lds_w2, 0};
    const bool gs = f32 ? p.gs32 : p.gs64;
    return {p.level, false, gs ? p.WLg : p.WL, f32 ? p.lds32 : p.lds64, (!f32 && p.shape_ok) ? kHeadlineShape : 0};
}

inline LaunchPlan make_launch_plan(const mpc_config& c) {
    Problem<double> P{};
    fill_problem<double>(c, P);
    LaunchPlan p{};
    p.precision = c.precision;
    // the level: the rarely used rows, terms and coupling slots (terminal ball, via-points, integral form on the variable grid, moving obstacles, the convexified
    // Hessian, footprints that turn with the pose) and, on top of them, the cost variants (off-diagonal weights, trapezoidal rule) -- compiled out of the headline kernel
    const bool ext = P.ball || P.via || P.integral_form || P.dyn_obst || P.hess_mode || P.costx ||
                     (P.n_obst > 0 && (P.footprint_kind == MPC_FOOTPRINT_LINE || P.footprint_kind == MPC_FOOTPRINT_TWO_CIRCLES || P.footprint_kind == MPC_FOOTPRINT_POLYGON));
    p.level = !ext ? 0 : (P.costx ? 2 : 1);
    {
        const int O = c.max_obstacles > 0 ? c.max_obstacles : 0;
        const int M = O > 0 ? (c.max_obstacle_rows > 0 ? c.max_obstacle_rows : 4) : 0;
        const bool turning = c.footprint_kind == MPC_FOOTPRINT_LINE || c.footprint_kind == MPC_FOOTPRINT_TWO_CIRCLES || c.footprint_kind == MPC_FOOTPRINT_POLYGON;
        const int ntrig = ((c.model == MPC_MODEL_KINEMATIC_BICYCLE || c.model == MPC_MODEL_SIMPLE_CAR_FRONT) ? 4 : 3) + (c.collocation == MPC_COLLOC_CRANK_NICOLSON ? 2 : 0);
        auto layout = [&](bool gs) {      // (MPC_MIXED has no clearance rows: both of its phases see the same layout)
            return WaveLayout::make(c.n, M, O, c.max_vertices > 0 ? c.max_vertices : 1, ntrig, P.n_via, (O > 0 && (turning || c.enable_dynamic_obstacles)) ? M : 0,
                                    (O > 0 && c.enable_dynamic_obstacles) ? O : 0, ext ? NSTG_EXT : NSTG_BASE, (O > 0 && c.enable_dynamic_obstacles && turning) ? M : 0,
                                    c.precision == MPC_FP32 ? 4 : 8, gs);
        };
        p.WL = layout(false);
        p.WLg = layout(true);
    }
    const size_t p64 = sizeof(Problem<double>), p32 = sizeof(Problem<float>);
    // The form, per precision (MPC_STAGE_AUTO).  The register file holds the one-wave kernels at one wave per SIMD, so a CU has room for four workgroups, and an LDS
    // record that fits fewer than four times leaves SIMDs without a wave; the global form costs some time per iteration at equal residency.  So the global form is taken
    // when the LDS form does not fit at all, or leaves at least half of a CU's SIMDs empty (plain fp32: one of four) and the global form fills more of them
    // (include/mpc_hip.h, mpc_config.stage_data; the measurements are in CHANGELOG.md, 0.5.0 and r06).
    auto per_cu = [](size_t lds) { const size_t k = kLdsPerCu / lds; return k > 4 ? (size_t)4 : k; };
    auto global_form = [&](size_t tsize, size_t psize, size_t most_per_cu) {
        if (c.stage_data == MPC_STAGE_LDS) return false;
        if (c.stage_data == MPC_STAGE_GLOBAL) return true;
        const size_t a = lds_bytes(p.WL, tsize, psize), g = lds_bytes(p.WLg, tsize, psize);
        if (a > kLdsPerCu) return g <= kLdsPerCu;
        return per_cu(a) <= most_per_cu && per_cu(g) > per_cu(a);
    };
    // The fp32 phase of MPC_MIXED follows the fp64 rule (the global form from about n = 140 on, where its LDS record fits only twice).  Its fp64 refinement phase keeps
    // the LDS form unless MPC_STAGE_GLOBAL asks for the other: one candidate and a handful of iterations run faster there.
    p.gs32 = c.precision != MPC_FP64 && global_form(4, p32, c.precision == MPC_FP32 ? 3 : 2);
    p.gs64 = c.precision != MPC_FP32 && (c.precision != MPC_MIXED || c.stage_data == MPC_STAGE_GLOBAL) && global_form(8, p64, 2);
    p.lds32 = c.precision != MPC_FP64 ? lds_bytes(p.gs32 ? p.WLg : p.WL, 4, p32) : 0;
    p.lds64 = c.precision != MPC_FP32 ? lds_bytes(p.gs64 ? p.WLg : p.WL, 8, p64) : 0;
    // Two waves per SIMD (IpmWave's W2): fp64, the headline level without clearance rows, the LDS form fitting eight times into a CU (about n <= 24 grid points, the
    // grid sizes of the reference's shipped parameter files).  A launch of at least w2_min_batch instances has waves waiting for a SIMD, and a second resident wave
    // fills the issue slots the first leaves idle; a smaller launch lasts as long as its slowest wave, which runs fastest alone.  Same arithmetic, same results.
    const size_t w2_lds = lds_bytes(p.WL, 8, p64);
    p.w2_ok = c.precision == MPC_FP64 && c.stage_data == MPC_STAGE_AUTO && p.level == 0 && c.max_obstacles <= 0 && w2_lds <= kLdsPerCu / 8 && c.two_wave_min_batch >= 0;
    p.w2_min_batch = c.two_wave_min_batch > 0 ? c.two_wave_min_batch : 4096;
    p.lds_w2 = p.w2_ok ? w2_lds : 0;
    const size_t blk64 = c.precision != MPC_FP32 ? (size_t)(p.gs64 ? p.WLg.GSW : p.WL.GSW) * 8 : 0;
    const size_t blk32 = c.precision != MPC_FP64 ? (size_t)(p.gs32 ? p.WLg.GSW : p.WL.GSW) * 4 : 0;
    p.block_bytes = blk64 > blk32 ? blk64 : blk32;
    // The shape-known kernel: the handle's word is the headline's, bit for bit, and every condition of the fixed layout holds (fp64, the headline level without clearance
    // rows, the LDS form, the record of the model's FixedLayout).  Any other word on that layout keeps the run-time-flags fixed-layout kernel (select_kernel).  The word is
    // taken from the fp64 record; the fp32 record of a mixed handle is filled from the same mpc_config and has the same int fields.  Kernel and plan evaluate ONE expression
    // (MPC_SHAPE_FLAGS) over int fields that every parameter set shares with its handle, so the kernel's run-time word cannot differ from the one compared here; a shape
    // that select_kernel has no instantiation for fails the launch (hipErrorInvalidConfiguration) instead of running another kernel.
    p.flags = shape_flags(P);
    const bool trig4 = c.model == MPC_MODEL_KINEMATIC_BICYCLE || c.model == MPC_MODEL_SIMPLE_CAR_FRONT;      // (IpmWave::NTRB)
    const bool fixed = trig4 ? FixedLayout<kFixedLayoutNS, 4, NSTG_BASE>::matches(p.WL) : FixedLayout<kFixedLayoutNS, 3, NSTG_BASE>::matches(p.WL);
    p.shape_ok = c.precision != MPC_FP32 && p.flags == kHeadlineShape && p.level == 0 && p.WL.M == 0 && !p.gs64 && fixed;
    return p;
}

// why no kernel can run the plan (the text mpc_last_error reports), or nullptr
inline const char* plan_error(const LaunchPlan& p) {
    if (p.lds() > kLdsPerCu)
        return "mpc_create: the working set of one instance (n, max_obstacles, max_vertices, precision) does not fit in the 160 KB of LDS "
               "of a compute unit (about n <= 215 grid points in fp64 without obstacles; n <= 590 with the factorisation data in global memory)";
    return nullptr;
}

// Blocks per XCD of the pool (mpc_solve_kernel.hpp): twice what ONE XCD holds at once -- the resident workgroups per CU of the kernel that claims them (occupancy <= 0:
// unknown, then 8, two one-wave workgroups per SIMD, the most any build allows) x the CUs of an XCD (the device's CUs over its XCCs) --, at least 64.  A pool then never
// runs dry, and the factor two keeps the claim probe at a step or two when every CU is full.
inline int pool_blocks_per_xcd(const LaunchPlan& p, int occupancy, int n_cu, int n_xcc) {
    if (p.block_bytes == 0) return 0;
    const size_t per_cu = occupancy > 0 ? (size_t)occupancy : 8;
    const size_t cus_per_xcd = ((size_t)n_cu + (size_t)n_xcc - 1) / (size_t)n_xcc;
    const size_t per_xcd = 2 * per_cu * cus_per_xcd;
    return (int)(per_xcd < 64 ? 64 : per_xcd);
}

}  // namespace mpc
