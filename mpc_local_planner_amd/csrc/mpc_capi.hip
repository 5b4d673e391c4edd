// mpc_capi.hip -- HIP kernels + the C ABI declared in include/mpc_hip.h.
// gfx950 only.  There is no CPU path in this library: mpc_create fails with MPC_ENODEV
// when no HIP device is usable.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mpc_hip.h"
#include "../../include/mpc_fleet.h"
#include "../../include/mpc_costmap_clusters.h"
#include "../../include/mpc_costmap_lines.h"
#include "../../include/mpc_costmap_window.h"
#include "../../include/mpc_costmap_scans.h"
#include "../../include/mpc_scan_cast.h"
#include "../../include/mpc_plant.h"
#include "mpc_core.hpp"
#include "mpc_problem.hpp"
#include "mpc_launch_plan.hpp"
#include "mpc_wave.hpp"
#include "mpc_solve_kernel.hpp"
#include "mpc_costmap.hpp"
#include "mpc_feasibility.hpp"
#include "mpc_grid_update.hpp"
#include "mpc_controller_cycle.hpp"
#include "mpc_evaluate.hpp"
#include "mpc_plan_inputs.hpp"
#include "mpc_fleet_obstacles.hpp"
#include "mpc_costmap_clusters.hpp"
#include "mpc_costmap_lines.hpp"
#include "mpc_costmap_window.hpp"
#include "mpc_costmap_scans.hpp"
#include "mpc_scan_cast.hpp"
#include "mpc_plant.hpp"

namespace {

thread_local char g_err[512] = "";

void set_err(const char* what, hipError_t e) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
}
void set_err(const char* what) { snprintf(g_err, sizeof(g_err), "%s", what); }

#define HIP_TRY(call)                                     \
    do {                                                  \
        hipError_t e_ = (call);                           \
        if (e_ != hipSuccess) { set_err(#call, e_); return MPC_EHIP; } \
    } while (0)

}  // namespace

// One device or pinned allocation of the handle.  Every one of them is in mpc_solver::bufs: mpc_create allocates and fills from that table, mpc_reset refills from
// it, mpc_destroy frees from it, and a buffer that is allocated or replaced later (buf_alloc) stays in its entry.
enum { FILL_NONE = -1, FILL_NGRID = 256, FILL_TAB0 = 257 };      // 0 .. 255: that byte in every byte; the uniform grid size in every word; table entry 0
struct Buf {
    void** p;           // where the handle keeps the pointer (NULL there: not allocated)
    size_t bytes;       // what mpc_create allocates (0: nothing), then the size of the allocation
    int fill;           // the idle contents mpc_create writes
    bool reset, pinned; // mpc_reset writes them again; host memory (hipHostMalloc)
};
enum { BUF_TAB, BUF_SET_OF, BUF_H_TAB, BUF_H_IN, BUF_CYC_LIVE, BUF_CYC, BUF_H_STAGE, BUF_D_STAGE, BUF_CLUSTER_LAB, BUF_NAMED };      // the entries other entry points ask for (declare_buffers assigns them by index)

struct mpc_solver {
    mpc_config cfg;
    mpc::Problem<double> P64;   // the handle's own records (host copies: what selects the kernel and sizes the launch)
    mpc::Problem<float> P32;
    std::vector<Buf> bufs;
    // device table of problem records (mpc_set_parameter_sets): entry 0 is the handle's own configuration, entries 1 .. n_sets the sets in force; a solve
    // kernel copies entry set_of[b] (entry 0 while p_set_of is NULL) into the LDS of instance b.  One allocation: fp64 records | fp32 records | dt_ref per entry |
    // the fp64 records of mpc_evaluate_batch* (mpc_evaluate.hpp) per entry
    unsigned char* d_tab;
    mpc::Problem<double>* d_tab64;      // NULL for a handle without fp64 launches
    mpc::Problem<float>* d_tab32;       // NULL for a handle without fp32 launches
    double* d_dtref;                    // dt_ref of every entry (single-step grid adaptation of mpc_grid_update_device)
    mpc::EvalParams* d_tabev;           // the evaluation's record of every entry (every precision: mpc_evaluate_batch* works in fp64)
    int tab_cap;                        // entries the table has room for
    int32_t* d_set_of;                  // [max_batch] table entry of instance b (1 + its set), allocated by the first mpc_set_parameter_sets
    const int32_t* p_set_of;            // what the kernels read: d_set_of while sets are in force, else NULL
    int sets_B;                         // batch size the sets were given for (solves must not exceed it)
    unsigned char* h_tab;               // pinned staging of the table uploads, grows on demand
    mpc::LaunchPlan plan;       // which kernel each launch runs (mpc_launch_plan.hpp)
    void* d_gstage;             // 8 pools of n_gslots blocks (plan.block_bytes each), NULL when the plan has none
    int* d_gslots;              // [8][n_gslots] claim words of the blocks (0 = free)
    int n_gslots;
    int32_t* d_iters1;          // MPC_MIXED: iterations of the fp32 phase
    int device;
    int max_batch;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    // staging of mpc_solve_batch / mpc_step_batch (and of the solve inside mpc_controller_step_batch): ONE pinned host block and ONE device block each way (one H2D and
    // one D2H per call; mpc::step_pieces), sized at mpc_create so that no call on the solve path allocates.  They stay apart from the shared pair below: a solve leaves
    // last_status / last_iters pointing into d_out, and mpc_last_candidates reads them after whatever other host-pointer call came in between
    unsigned char *h_in, *h_out, *d_in, *d_out;
    // staging of every other host-pointer call (staged_call; mpc::stage_layout): ONE pinned block and ONE device block, allocated by the first call that needs them,
    // grown on demand.  Every such call ends in hipStreamSynchronize, so the pair is never in use twice
    unsigned char *h_stage, *d_stage;
    int32_t* d_ngrid;
    int32_t *d_nvia;            // own copy of the via-point counts / poses (mpc_set_via_points) ...
    double *d_via;
    const int32_t* p_nvia;      // ... and what the kernel reads: the own copy or borrowed device pointers
    const double* p_via;
    int use_ngrid;
    int ngrid_B, nvia_B;        // batch sizes the per-instance grid sizes / own via-point copies were set for (solves must not exceed them)
    hipEvent_t cev0, cev1;      // costmap kernel timing (kept apart from the solve kernel's events)
    bool ctimed;                // a costmap step has recorded them (mpc_last_costmap_ms)
    int32_t* d_cluster_lab;     // scratch of mpc_costmap_to_polygons* / mpc_costmap_to_lines*: one label (and for the lines one list word) per cell and instance, allocated by the first such call, grows on demand
    // candidate initial trajectories (n_candidates > 1): bookkeeping words, candidate records, per-instance winner / total iterations
    int *d_cwin, *d_cexited, *d_citsum;
    double* d_crec;
    int32_t *d_winner, *d_iters_total;
    int32_t* d_rows_dropped;    // per instance: clearance rows that did not fit (solvers with obstacles)
    double* d_dual;             // per instance: multipliers of the last converged solve (dual_warm_start)
    int dual_words;
    int32_t* last_status;       // device pointers of the most recent solve (mpc_last_candidates without candidates)
    int32_t* last_iters;
    bool timed;
    // slot state of mpc_controller_step_batch* (mpc_controller_cycle.hpp), allocated by the first such call: the flags mpc_reset clears (0 = the slot is empty), and one
    // block with everything else -- step counts, has-solution flags, start modes, last goals, the x0 / xf the solves read and the slots' previous solutions x / u / dt
    int32_t* d_cyc_live;
    unsigned char* d_cyc;
};

// the pieces of the slot-state block
struct CycLayout {
    size_t seq, has, mode, goal, x0, xf, x, u, dt, bytes;
    CycLayout(size_t Bm, size_t n) {
        mpc::Packer p;
        seq = p.take(Bm * 4); has = p.take(Bm * 4); mode = p.take(Bm * 4); goal = p.take(Bm * 24); x0 = p.take(Bm * 24); xf = p.take(Bm * 24);
        x = p.take(Bm * n * 24); u = p.take(Bm * n * 16); dt = p.take(Bm * 8); bytes = p.off;
    }
};

static void buf_free(Buf& b) {
    if (*b.p) (void)(b.pinned ? hipHostFree(*b.p) : hipFree(*b.p));
    *b.p = nullptr; b.bytes = 0;
}
// a new allocation first, then the one it replaces (if any) freed: a failure leaves the buffer as it was
static hipError_t buf_alloc(Buf& b, size_t bytes) {
    void* q = nullptr;
    const hipError_t e = b.pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes);
    if (e != hipSuccess) return e;
    buf_free(b);
    *b.p = q; b.bytes = bytes;
    return hipSuccess;
}

// which XCC ids the device's workgroups run on (bit i of *mask: some workgroup saw HW_REG_XCC_ID & 7 == i): 8 bits on an MI355X, 1 in a partitioned mode
namespace mpc {
__global__ void xcc_probe_kernel(unsigned* mask) {
    if (threadIdx.x == 0) atomicOr(mask, 1u << ((unsigned)__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u));
}
}  // namespace mpc

// The one place where the precision and mpc_config.model become the template arguments of the solve kernel's host functions (instantiated per pair in
// mpc_solve_inst.hip): calls f(T(), std::integral_constant<int, MODEL>()).
template <typename F>
static hipError_t with_model(bool f32, int model, F f) {
#ifdef MPC_DEV_ONE_MODEL       // developer builds (fast compile, asm inspection): only the fp64 instantiations of ONE model exist (-DMPC_DEV_ONE_MODEL=<model id>)
    (void)model; return f32 ? hipErrorInvalidConfiguration : f(double(), std::integral_constant<int, MPC_DEV_ONE_MODEL>());
#else
    auto prec = [&](auto m) { return f32 ? f(float(), m) : f(double(), m); };
    switch (model) {
        case MPC_MODEL_UNICYCLE: return prec(std::integral_constant<int, mpc::MODEL_UNICYCLE>());
        case MPC_MODEL_SIMPLE_CAR: return prec(std::integral_constant<int, mpc::MODEL_SIMPLE_CAR>());
        case MPC_MODEL_SIMPLE_CAR_FRONT: return prec(std::integral_constant<int, mpc::MODEL_SIMPLE_CAR_FRONT>());
        default: return prec(std::integral_constant<int, mpc::MODEL_KINEMATIC_BICYCLE>());
    }
#endif
}
// resident workgroups per CU of the solve kernel that serves a kernel choice
static hipError_t kernel_occupancy(bool f32, int model, const mpc::KernelChoice& k, int* out) {
    return with_model(f32, model, [&](auto t, auto m) { return mpc::solve_occupancy<decltype(t), decltype(m)::value>(k, out); });
}

// byte offsets of the three pieces of a record table of `entries` entries (256-byte aligned), and its size
struct TabLayout {
    size_t o64, o32, odt, oev, bytes;
    TabLayout(const mpc_config& c, size_t entries) {
        mpc::Packer p;
        o64 = p.take(c.precision != MPC_FP32 ? entries * sizeof(mpc::Problem<double>) : 0);
        o32 = p.take(c.precision != MPC_FP64 ? entries * sizeof(mpc::Problem<float>) : 0);
        odt = p.take(entries * 8); oev = p.take(entries * sizeof(mpc::EvalParams)); bytes = p.off;
    }
};

// writes table entry e (records and dt_ref of configuration c) into a host image of the table
static void put_entry(const mpc_config& hcfg, const mpc_config& c, size_t entries, size_t e, unsigned char* img) {
    const TabLayout t(hcfg, entries);
    mpc::Problem<double> P64;
    mpc::Problem<float> P32;
    mpc::fill_records(c, P64, P32);
    if (hcfg.precision != MPC_FP32) memcpy(img + t.o64 + e * sizeof(P64), &P64, sizeof(P64));
    if (hcfg.precision != MPC_FP64) memcpy(img + t.o32 + e * sizeof(P32), &P32, sizeof(P32));
    memcpy(img + t.odt + e * 8, &c.dt_ref, 8);
    mpc::EvalParams ev;
    mpc::fill_eval_params(c, ev);
    memcpy(img + t.oev + e * sizeof(ev), &ev, sizeof(ev));
}

static void point_tables(mpc_solver* s) {
    const TabLayout t(s->cfg, (size_t)s->tab_cap);
    s->d_tab64 = s->cfg.precision != MPC_FP32 ? reinterpret_cast<mpc::Problem<double>*>(s->d_tab + t.o64) : nullptr;
    s->d_tab32 = s->cfg.precision != MPC_FP64 ? reinterpret_cast<mpc::Problem<float>*>(s->d_tab + t.o32) : nullptr;
    s->d_dtref = reinterpret_cast<double*>(s->d_tab + t.odt);
    s->d_tabev = reinterpret_cast<mpc::EvalParams*>(s->d_tab + t.oev);
}

// The handle's buffers: which of them its configuration gets at mpc_create (the others stay at 0 bytes), their sizes, the idle contents and whether mpc_reset
// restores those -- the multipliers (forgotten) and the words that restore themselves unless a launch was aborted: the claim words of the blocks and the
// candidate bookkeeping.  Parameter sets, grid sizes and via-points are kept by mpc_reset.  Staging: the solve's four blocks at their full size here, the ONE
// shared pair of every other host-pointer call (BUF_H_STAGE, BUF_D_STAGE) at 0 bytes until staged_call grows it.
static void declare_buffers(mpc_solver* s) {
    const mpc_config& c = s->cfg;
    const size_t Bm = (size_t)s->max_batch, n = (size_t)c.n, slots = 8 * (size_t)s->n_gslots, dual = Bm * (size_t)s->dual_words * 8;
    const bool pool = s->plan.block_bytes > 0, cand = s->P32.n_cand > 1, via = s->P64.n_via > 0;
    const mpc::StepPieces cap = mpc::step_pieces(c, Bm, true, true, true, true, true);
    int gstage_fill = FILL_NONE;
#ifdef MPC_DEV_SWITCHES
    // developer check (scripts/dev/gs_sweep.py under MPC_POISON_GSTAGE=1): every word of the pool starts as a NaN pattern, so a word that some path consumes before writing it shows up in the results
    if (const char* e = getenv("MPC_POISON_GSTAGE")) { if (e[0] == '1') gstage_fill = 0xFF; }
#endif
    auto add = [s](auto* where, size_t bytes, int fill = FILL_NONE, bool reset = false, bool pinned = false) { s->bufs.push_back({(void**)where, bytes, fill, reset, pinned}); };
    s->bufs.resize(BUF_NAMED);         // the entries other entry points ask for by index, then the rest
    s->bufs[BUF_TAB] = {(void**)&s->d_tab, TabLayout(c, 1).bytes, FILL_TAB0, false, false};      // replaced by a larger one when mpc_set_parameter_sets needs more entries
    s->bufs[BUF_SET_OF] = {(void**)&s->d_set_of, 0, FILL_NONE, false, false};                    // [max_batch], allocated by the first mpc_set_parameter_sets
    s->bufs[BUF_H_TAB] = {(void**)&s->h_tab, 0, FILL_NONE, false, true};
    s->bufs[BUF_H_IN] = {(void**)&s->h_in, cap.in_bytes, FILL_NONE, false, true};
    s->bufs[BUF_CYC_LIVE] = {(void**)&s->d_cyc_live, 0, 0, true, false};                        // the two of the controller cycle: allocated by the first mpc_controller_step_batch*
    s->bufs[BUF_CYC] = {(void**)&s->d_cyc, 0, 0, false, false};
    s->bufs[BUF_H_STAGE] = {(void**)&s->h_stage, 0, FILL_NONE, false, true};                    // the shared pair of staged_call: allocated by the first call that stages, grows on demand
    s->bufs[BUF_D_STAGE] = {(void**)&s->d_stage, 0, FILL_NONE, false, false};
    s->bufs[BUF_CLUSTER_LAB] = {(void**)&s->d_cluster_lab, 0, FILL_NONE, false, false};         // allocated by the first mpc_costmap_to_polygons* / mpc_costmap_to_lines*, grows on demand
    add(&s->h_out, cap.out_bytes, FILL_NONE, false, true);
    add(&s->d_in, cap.in_bytes);
    add(&s->d_out, cap.out_bytes);
    add(&s->d_ngrid, Bm * 4, FILL_NGRID);                  // never uninitialised
    add(&s->d_nvia, via ? Bm * 4 : 0, 0);
    add(&s->d_via, via ? Bm * (size_t)s->P64.n_via * 3 * 8 : 0);
    add(&s->d_rows_dropped, c.max_obstacles > 0 ? Bm * 4 : 0, 0);
    add(&s->d_iters1, c.precision == MPC_MIXED ? Bm * 4 : 0);
    add(&s->d_gstage, pool ? slots * s->plan.block_bytes + (size_t)mpc::GlobalStage::kPrefetchPad * 8 : 0, gstage_fill);
    add(&s->d_gslots, pool ? slots * 4 : 0, 0, true);
    add(&s->d_dual, dual, 0, true);
    add(&s->d_cwin, cand ? Bm * 4 : 0, 0x7f, true);
    add(&s->d_cexited, cand ? Bm * 4 : 0, 0, true);
    add(&s->d_citsum, cand ? Bm * 4 : 0, 0, true);
    add(&s->d_crec, cand ? (size_t)s->P32.n_cand * Bm * (5 * n + 3 + (size_t)s->dual_words) * 8 : 0);
    add(&s->d_winner, cand ? Bm * 4 : 0);
    add(&s->d_iters_total, cand ? Bm * 4 : 0);
}

static hipError_t buf_fill(const mpc_solver* s, const Buf& b) {
    if (b.fill == FILL_NONE) return hipSuccess;
    if (b.fill < 256) return hipMemset(*b.p, b.fill, b.bytes);
    std::vector<unsigned char> img(b.bytes, 0);
    if (b.fill == FILL_TAB0) put_entry(s->cfg, s->cfg, 1, 0, img.data());
    else for (size_t i = 0; i < b.bytes / 4; ++i) reinterpret_cast<int32_t*>(img.data())[i] = s->cfg.n;
    return hipMemcpy(*b.p, img.data(), b.bytes, hipMemcpyHostToDevice);
}

extern "C" {

void mpc_config_defaults(mpc_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->model = MPC_MODEL_UNICYCLE;       // src/controller.cpp:346
    c->model_params[0] = 0.5;            // :355
    c->model_params[1] = 1.0;
    c->n = 20;                           // :274
    c->dt_ref = 0.3;                     // :278
    c->dt_free = 1;                      // :236
    c->dt_lb = 0.0;                      // :242
    c->dt_ub = 10.0;                     // :244
    c->xf_fixed[0] = c->xf_fixed[1] = c->xf_fixed[2] = 1;   // :282
    c->collocation = MPC_COLLOC_FORWARD; // :298
    c->objective = MPC_OBJ_MIN_TIME;     // :551
    c->u_lb[0] = -0.2; c->u_ub[0] = 0.4; // :497-511
    c->u_lb[1] = -0.3; c->u_ub[1] = 0.3;
    for (int j = 0; j < 2; ++j) { c->du_lb[j] = -1e30; c->du_ub[j] = 1e30; }   // :756-770 (0 => inf)
    c->max_iter = 100;                   // :391
    c->tol = 1e-8;
    c->mu_init = 0.1;
    c->precision = MPC_FP64;
    c->min_obstacle_dist = 0.5;          // :717
    c->force_inclusion_dist = 0.5;       // :725
    c->cutoff_dist = 2.0;                // :727
    c->footprint_kind = MPC_FOOTPRINT_POINT;   // src/mpc_local_planner_ros.cpp:894-898
    c->max_obstacles = 0;
    c->max_vertices = 1;
    c->max_obstacle_rows = 4;
}

void mpc_cycle_params_defaults(mpc_cycle_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->n_ref = 0;                               // grid/grid_size_ref = the handle's n
    p->outer_iterations = 1;                    // src/controller.cpp:70-72
    p->adapt = 1; p->n_min = 2; p->n_max = 50;  // :248-261 (the variable grid adapts by default; n_min is clamped to 3, n_max to cfg.n)
    p->dt_hyst_ratio = 0.1;
    p->warm_start = 1;                          // :294-296
    p->force_reinit_num_steps = 0;              // :78
    p->force_reinit_new_goal_dist = 1.0;        // :74
    p->force_reinit_new_goal_angular = 1.5707963267948966;      // :76 (0.5 pi)
    p->initial_plan_estimate_orientation = 1;
    p->prefer_x_feedback = 0;                   // :82
    p->reference_reinit_sampling = 1;
    p->period = 0.1;
}

void mpc_plan_params_defaults(mpc_plan_params* p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->global_plan_prune_distance = 1.0;        // include/mpc_local_planner/mpc_local_planner_ros.h:369-391
    p->max_global_plan_lookahead_dist = 1.5;
    p->global_plan_viapoint_sep = -1.0;
    p->xy_goal_tolerance = 0.2; p->yaw_goal_tolerance = 0.1;
    p->global_plan_overwrite_orientation = 1;
    p->moving_average_length = 3;               // :363-364
    p->costmap_size_x = 200; p->costmap_size_y = 200; p->resolution = 0.05;      // costmap_2d's own defaults (10 m x 10 m)
}

const char* mpc_last_error(void) { return g_err; }
int32_t mpc_version(void) { return 900; }      // 0.9.0: mpc_evaluate_batch* (CHANGELOG.md has what each version brought); mpc_plan_inputs_batch* / mpc_commands_batch* came later under the same number: tests/test_evaluate_host.py pins this line

#ifdef MPC_PROFILE
// developer build only (-DMPC_PROFILE): per-wave phase cycle counters of the last wave-kernel launch, mpc::kProfCols words per row
int mpc_debug_profile(long long* out, int rows) {
#ifdef MPC_SPLIT_BUILD
    std::memset(out, 0, sizeof(long long) * mpc::kProfCols * (size_t)rows);
    hipError_t e = hipSuccess;
    for (int f32 = 0; f32 < 2; ++f32)      // every pair of the split build (a -DMPC_DEV_ONE_MODEL build is a single translation unit: the other branch)
        for (int model = 0; model < 4 && e == hipSuccess; ++model)
            e = with_model(f32 != 0, model, [&](auto t, auto m) { return mpc::solve_profile_add<decltype(t), decltype(m)::value>(out, rows); });
    return (int)e;
#else
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mpc_prof), sizeof(long long) * mpc::kProfCols * (size_t)rows, 0, hipMemcpyDeviceToHost);
#endif
}
#endif

int mpc_create(const mpc_config* cfg, int32_t max_batch, int32_t device, mpc_solver** out) {
    g_err[0] = 0;
    if (!cfg || !out || max_batch <= 0) { set_err("mpc_create: bad argument"); return MPC_EINVAL; }
    *out = nullptr;
    if (const char* why = mpc::config_error(*cfg)) { set_err(why); return MPC_EINVAL; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_err("mpc_create: no HIP device available (this library has no CPU fallback)");
        return MPC_ENODEV;
    }
    if (device < 0 || device >= ndev) { set_err("mpc_create: device index out of range"); return MPC_ENODEV; }
    HIP_TRY(hipSetDevice(device));
    const mpc::LaunchPlan plan = mpc::make_launch_plan(*cfg);
    if (const char* why = mpc::plan_error(plan)) { set_err(why); return MPC_EINVAL; }
    mpc_solver* s = new (std::nothrow) mpc_solver();      // (every field zero)
    if (!s) return MPC_ENOMEM;
    s->cfg = *cfg;
    s->plan = plan;
    mpc::fill_records(*cfg, s->P64, s->P32);
    s->device = device;
    s->max_batch = max_batch;
    hipError_t er = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    for (hipEvent_t* ev : {&s->ev0, &s->ev1, &s->cev0, &s->cev1}) if (er == hipSuccess) er = hipEventCreate(ev);
    if (plan.block_bytes > 0) {
        // the per-XCD pools of blocks (mpc_solve_kernel.hpp), sized by mpc::pool_blocks_per_xcd from the device: the resident workgroups per CU of the kernel that claims
        // the blocks (occupancy API: registers, LDS, one-wave workgroups) and the CUs of an XCD (the device's CUs over the distinct XCC ids a probe launch sees).  Stale
        // contents are never read: every word is written before it is read within a solve.  Memory: 8 pools x per_xcd x block bytes (MI355X, n = 120 in fp64:
        // 8 x 256 x 73 KB = 150 MB per handle; include/mpc_hip.h, mpc_create).
        hipDeviceProp_t prop;
        if (er == hipSuccess) er = hipGetDeviceProperties(&prop, device);
        if (er == hipSuccess) {
            int occ = 0, n_xcc = 1;
            if (kernel_occupancy(cfg->precision == MPC_FP32, cfg->model, mpc::plan_launch(plan, cfg->precision == MPC_FP32, 0), &occ) != hipSuccess) occ = 0;
            unsigned* d_mask = nullptr; unsigned h_mask = 0;
            if (hipMalloc((void**)&d_mask, 4) == hipSuccess) {
                if (hipMemset(d_mask, 0, 4) == hipSuccess) {
                    hipLaunchKernelGGL(mpc::xcc_probe_kernel, dim3(16u * (unsigned)prop.multiProcessorCount), dim3(64), 0, 0, d_mask);
                    if (hipMemcpy(&h_mask, d_mask, 4, hipMemcpyDeviceToHost) == hipSuccess && h_mask) n_xcc = __builtin_popcount(h_mask & 0xffu);
                }
                (void)hipFree(d_mask);
            }
            s->n_gslots = mpc::pool_blocks_per_xcd(plan, occ, prop.multiProcessorCount, n_xcc);
        }
    }
    if (cfg->dual_warm_start || cfg->precision == MPC_MIXED) s->dual_words = mpc::dual_words(plan.WL.NS);
    declare_buffers(s);
    for (Buf& b : s->bufs) {
        if (er == hipSuccess && b.bytes) er = buf_alloc(b, b.bytes);
        if (er == hipSuccess && b.bytes) er = buf_fill(s, b);
    }
    if (er == hipSuccess) { s->tab_cap = 1; point_tables(s); }      // the handle's own configuration as entry 0, the only one until mpc_set_parameter_sets
    s->p_nvia = s->d_nvia; s->p_via = s->d_via;
    // the fills above run on the null stream, the solves on the handle's own non-blocking stream: nothing orders the two, so wait here
    if (er == hipSuccess) er = hipDeviceSynchronize();
    if (er != hipSuccess) {
        set_err("mpc_create: allocation", er);
        mpc_destroy(s);
        return er == hipErrorOutOfMemory ? MPC_ENOMEM : MPC_EHIP;
    }
    *out = s;
    return MPC_OK;
}

int mpc_reset(mpc_solver* s) {
    if (!s) return MPC_EINVAL;
    g_err[0] = 0;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (const Buf& b : s->bufs) if (b.reset && *b.p) HIP_TRY(buf_fill(s, b));
    HIP_TRY(hipDeviceSynchronize());      // null-stream fills vs the handle's non-blocking stream (see mpc_create)
    return MPC_OK;
}

void mpc_destroy(mpc_solver* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (Buf& b : s->bufs) buf_free(b);
    for (hipEvent_t ev : {s->ev0, s->ev1, s->cev0, s->cev1}) if (ev) (void)hipEventDestroy(ev);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

}  // extern "C"

// A solve launch: the caller's part of the record (inputs, initial guess, obstacles, outputs, B: mpc_solve_batch_device) gets the handle's part for one precision
// and goes to the kernels, which are instantiated per (precision, model) in mpc_solve_inst.hip (split build: one object each, compiled in parallel) or right
// here (single translation unit).
static hipError_t launch(const mpc_solver* s, bool f32, mpc::SolveLaunch a) {
    const bool refine = s->cfg.precision == MPC_MIXED && !f32;      // the fp64 phase of MPC_MIXED
    a.k = mpc::plan_launch(s->plan, f32, a.B);
    a.stream = s->stream;
    a.gstage = s->d_gstage; a.gslots = s->d_gslots; a.n_gslots = s->n_gslots;
    a.rec = f32 ? (const void*)&s->P32 : (const void*)&s->P64;
    a.ptab = f32 ? (const void*)s->d_tab32 : (const void*)s->d_tab64;
    a.set_of = s->p_set_of;
    a.n_grid = s->use_ngrid ? s->d_ngrid : nullptr; a.n_via = s->p_nvia; a.via = s->p_via;
    // kept multipliers: a launch starts from them under dual_warm_start; in MPC_MIXED without it the block is only the hand-off from the fp32 phase
    // (which leaves its multipliers) to the fp64 phase (which starts from them) -- nothing is carried from the slot's previous control cycle
    const int dual_read = (s->cfg.dual_warm_start || refine) ? 1 : 0;
    a.cc = {f32 ? s->P32.n_cand : s->P64.n_cand, s->d_cwin, s->d_cexited, s->d_citsum, s->d_crec, s->d_winner, s->d_iters_total, s->d_rows_dropped, s->d_dual, s->dual_words, dual_read};
    a.iters_add = refine ? s->d_iters1 : nullptr;
    return with_model(f32, s->cfg.model, [&](auto t, auto m) { return mpc::launch_solve<decltype(t), decltype(m)::value>(a); });
}

// The refusals that depend on the per-instance state the handle carries, each stated once: 0, or the return code with mpc_last_error set.  `which`: the checks
// that apply to the entry point, made in the order of the enum; `who`: the prefix of the message.
enum { REF_MAX_BATCH = 1, REF_NGRID = 2, REF_NGRID_NO_HINT = 4, REF_VIA = 8, REF_SETS = 16, REF_OBSTACLES = 32 };
static int refused(const mpc_solver* s, int32_t B, int which, const char* who, const mpc_obstacles* ob = nullptr) {
    auto no = [who](int rc, const char* why, const char* hint = "") { snprintf(g_err, sizeof(g_err), "%s: %s%s", who, why, hint); return rc; };
    if ((which & REF_MAX_BATCH) && B > s->max_batch) return no(MPC_EBATCH, "B exceeds max_batch");
    if ((which & (REF_NGRID | REF_NGRID_NO_HINT)) && s->use_ngrid && B > s->ngrid_B)
        return no(MPC_EBATCH, "B exceeds the batch the per-instance grid sizes were set for", (which & REF_NGRID) ? " (mpc_set_grid_sizes)" : "");
    if ((which & REF_VIA) && s->P64.n_via > 0 && s->p_nvia == s->d_nvia && s->nvia_B > 0 && B > s->nvia_B)      // (borrowed device pointers: the caller's affair)
        return no(MPC_EBATCH, "B exceeds the batch the via-points were set for (mpc_set_via_points)");
    if ((which & REF_SETS) && s->p_set_of && B > s->sets_B) return no(MPC_EBATCH, "B exceeds the batch the parameter sets were given for (mpc_set_parameter_sets)");
    if ((which & REF_OBSTACLES) && s->cfg.max_obstacles > 0 && (!ob || !ob->n_obstacles || !ob->n_vertices || !ob->vertices))
        return no(MPC_EINVAL, "the solver was created with max_obstacles > 0 but no obstacles were passed");
    return MPC_OK;
}

// A host-pointer call through the shared staging pair: the pieces laid out (mpc::stage_layout), the pair grown if they do not fit (the stream idle, the new block
// first, then the old one freed), the sources copied into the pinned block, ONE host-to-device copy, run(dev) with the device address of every piece (NULL for
// an absent one) -- it enqueues the device variant on the handle's stream and returns its code --, ONE device-to-host copy, the stream synchronised, the pinned
// block copied into the destinations.  `direct`: the call takes its device block only and copies piece by piece between it and the caller's memory, as
// mpc_costmap_to_obstacles and mpc_check_feasibility always have: with 4096 maps of 64 x 64 the pass through the pinned block costs them 0.14 .. 0.22 ms
// (profiles/r15_capi_staging.md).  What HIP refuses is reported under `who`, out of memory as MPC_ENOMEM where `enomem` says that the entry point always has.
template <typename Run>
static int staged_call(mpc_solver* s, const char* who, bool enomem, bool direct, const mpc::StagePiece* pc, int count, Run run) {
#define STAGE_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { set_err(who, e_); return enomem && e_ == hipErrorOutOfMemory ? MPC_ENOMEM : MPC_EHIP; } } while (0)
    hipStream_t q = s->stream;
    const mpc::StageLayout L = mpc::stage_layout(pc, count);
    for (Buf* bf : {&s->bufs[BUF_H_STAGE], &s->bufs[BUF_D_STAGE]})
        if (L.bytes > bf->bytes && !(direct && bf->pinned)) { STAGE_TRY(hipStreamSynchronize(q)); STAGE_TRY(buf_alloc(*bf, L.bytes)); }
    void* dev[mpc::StageLayout::MAX_PIECES];
    for (int i = 0; i < count; ++i) {
        dev[i] = L.at(s->d_stage, i);
        if (!L.present[i] || pc[i].dir == mpc::STAGE_OUT) continue;
        if (direct) STAGE_TRY(hipMemcpyAsync(dev[i], pc[i].src, pc[i].bytes, hipMemcpyHostToDevice, q));
        else memcpy(L.at(s->h_stage, i), pc[i].src, pc[i].bytes);
    }
    if (!direct && L.h2d_bytes) STAGE_TRY(hipMemcpyAsync(s->d_stage, s->h_stage, L.h2d_bytes, hipMemcpyHostToDevice, q));
    const int rc = run(dev);
    if (rc != MPC_OK) return rc;
    if (!direct && L.d2h_bytes) STAGE_TRY(hipMemcpyAsync(s->h_stage + L.d2h_begin, s->d_stage + L.d2h_begin, L.d2h_bytes, hipMemcpyDeviceToHost, q));
    for (int i = 0; direct && i < count; ++i)
        if (L.present[i] && pc[i].dir != mpc::STAGE_IN) STAGE_TRY(hipMemcpyAsync(pc[i].dst, dev[i], pc[i].bytes, hipMemcpyDeviceToHost, q));
    STAGE_TRY(hipStreamSynchronize(q));
    for (int i = 0; !direct && i < count; ++i)
        if (L.present[i] && pc[i].dir != mpc::STAGE_IN) memcpy(pc[i].dst, L.at(s->h_stage, i), pc[i].bytes);
    return MPC_OK;
#undef STAGE_TRY
}
// the pieces by direction; an in / out array is its own source and destination
static mpc::StagePiece stage_in(const void* p, size_t bytes) { return {p, nullptr, bytes, mpc::STAGE_IN}; }
static mpc::StagePiece stage_out(void* p, size_t bytes) { return {nullptr, p, bytes, mpc::STAGE_OUT}; }
static mpc::StagePiece stage_inout(void* p, size_t bytes) { return {p, p, bytes, mpc::STAGE_INOUT}; }

// a costmap step's launch, one workgroup per instance, between the two events mpc_last_costmap_ms reads
template <typename Kernel, typename Args>
static int costmap_timed_launch(mpc_solver* s, Kernel kernel, int32_t B, int threads, const Args& a) {
    HIP_TRY(hipEventRecord(s->cev0, s->stream));
    hipLaunchKernelGGL(kernel, dim3(B), dim3(threads), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->cev1, s->stream));
    s->ctimed = true;
    return MPC_OK;
}

// mpc_solve_batch_device with the per-instance start mode of the controller cycle (d_init_mode: NULL everywhere else)
static int solve_device(mpc_solver* s, int32_t B, const double* d_x0, const double* d_xf, const double* d_u_prev,
                        const double* d_dt_prev, const double* d_x_init, const double* d_u_init, const double* d_dt_init,
                        const mpc_obstacles* d_obstacles, double* d_x_out, double* d_u_out, double* d_dt_out, int32_t* d_status,
                        int32_t* d_iters, const int32_t* d_init_mode) {
    g_err[0] = 0;
    if (!s || !d_x0 || !d_xf || !d_x_out || !d_u_out || !d_dt_out) { set_err("mpc_solve_batch_device: null argument"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_solve_batch_device")) return rc;
    if ((d_x_init != nullptr) != (d_u_init != nullptr) || (d_x_init != nullptr) != (d_dt_init != nullptr)) {
        set_err("mpc_solve_batch: x_init, u_init and dt_init must be given together (all three or none)"); return MPC_EINVAL; }
    if (const int rc = refused(s, B, REF_NGRID | REF_VIA | REF_SETS, "mpc_solve_batch")) return rc;
    if (const int rc = refused(s, B, REF_OBSTACLES, "mpc_solve_batch_device", d_obstacles)) return rc;
    const mpc_obstacles ob = s->cfg.max_obstacles > 0 ? *d_obstacles : mpc_obstacles{nullptr, nullptr, nullptr, nullptr, nullptr};
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
    mpc::SolveLaunch a{};
    a.B = B;
    a.x0 = d_x0; a.xf = d_xf; a.u_prev = d_u_prev; a.dt_prev = d_dt_prev; a.x_init = d_x_init; a.u_init = d_u_init; a.dt_init = d_dt_init; a.obst = ob;
    a.x_out = d_x_out; a.u_out = d_u_out; a.dt_out = d_dt_out; a.status = d_status; a.iters = d_iters;
    a.init_mode = d_init_mode;      // (MPC_MIXED: the fp32 phase; the fp64 refinement always starts from phase 1's iterate)
    hipError_t le;
    if (s->cfg.precision == MPC_MIXED) {
        // phase 1 (fp32, candidates, tol 1e-4) leaves iterate + multipliers; phase 2 (fp64, one candidate) refines them in place
        mpc::SolveLaunch first = a;
        first.iters = s->d_iters1;
        le = launch(s, true, first);
        mpc::SolveLaunch second = first;
        second.x_init = d_x_out; second.u_init = d_u_out; second.dt_init = d_dt_out; second.iters = d_iters; second.init_mode = nullptr;
        if (le == hipSuccess) le = launch(s, false, second);
    } else {
        le = launch(s, s->cfg.precision == MPC_FP32, a);
    }
    HIP_TRY(le);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    s->timed = true;
    s->last_status = d_status; s->last_iters = d_iters;
    return MPC_OK;
}

extern "C" {

int mpc_solve_batch_device(mpc_solver* s, int32_t B, const double* d_x0, const double* d_xf, const double* d_u_prev,
                           const double* d_dt_prev, const double* d_x_init, const double* d_u_init, const double* d_dt_init,
                           const mpc_obstacles* d_obstacles, double* d_x_out, double* d_u_out, double* d_dt_out, int32_t* d_status,
                           int32_t* d_iters) {
    return solve_device(s, B, d_x0, d_xf, d_u_prev, d_dt_prev, d_x_init, d_u_init, d_dt_init, d_obstacles, d_x_out, d_u_out, d_dt_out, d_status, d_iters, nullptr);
}

int mpc_step_batch_device(mpc_solver* s, int32_t B, const double* d_x0, const double* d_xf, const double* d_u_prev, const double* d_dt_prev,
                          const double* d_x_init, const double* d_u_init, const double* d_dt_init, const mpc_obstacles* d_obstacles,
                          int32_t outer_iterations, int32_t adapt, int32_t n_min, int32_t n_max, double dt_hyst_ratio,
                          double* d_x_out, double* d_u_out, double* d_dt_out, int32_t* d_status, int32_t* d_iters) {
    // PredictiveController::step repeats (grid update -> solve) outer_ocp_iterations times per control cycle (src/controller.cpp:70-72,172): every
    // repetition after the first starts from the solution just computed, in place on the output arrays; everything is enqueued on the solver's stream
    int rc = mpc_solve_batch_device(s, B, d_x0, d_xf, d_u_prev, d_dt_prev, d_x_init, d_u_init, d_dt_init, d_obstacles, d_x_out, d_u_out, d_dt_out, d_status, d_iters);
    for (int it = 1; it < outer_iterations && rc == MPC_OK; ++it) {
        // variable grid: single-step adaptation + resampling; fixed grid: nothing -- its warm-start shift belongs to the first outer iteration of a cycle (`new_run`,
        // full_discretization_grid_base_se2.cpp:96-100), which is the caller's (the repetition starts from the solution just computed as it is)
        if (s->cfg.dt_free) rc = mpc_grid_update_device(s, B, d_x0, d_x_out, d_u_out, d_dt_out, adapt, n_min, n_max, dt_hyst_ratio);
        if (rc == MPC_OK)
            rc = mpc_solve_batch_device(s, B, d_x0, d_xf, d_u_prev, d_dt_prev, d_x_out, d_u_out, d_dt_out, d_obstacles, d_x_out, d_u_out, d_dt_out, d_status, d_iters);
    }
    return rc;
}

int mpc_last_candidates(mpc_solver* s, int32_t B, int32_t* winner, int32_t* iters_total) {
    g_err[0] = 0;
    if (!s) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_last_candidates")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->P32.n_cand > 1) {
        if (winner) HIP_TRY(hipMemcpy(winner, s->d_winner, (size_t)B * 4, hipMemcpyDeviceToHost));
        if (iters_total) HIP_TRY(hipMemcpy(iters_total, s->d_iters_total, (size_t)B * 4, hipMemcpyDeviceToHost));
        return MPC_OK;
    }
    if (winner) {
        if (!s->last_status) { set_err("mpc_last_candidates: the last solve kept no status array"); return MPC_EINVAL; }
        HIP_TRY(hipMemcpy(winner, s->last_status, (size_t)B * 4, hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b) winner[b] = winner[b] == MPC_CONVERGED ? 0 : -1;
    }
    if (iters_total) {
        if (!s->last_iters) { set_err("mpc_last_candidates: the last solve kept no iteration array"); return MPC_EINVAL; }
        HIP_TRY(hipMemcpy(iters_total, s->last_iters, (size_t)B * 4, hipMemcpyDeviceToHost));
    }
    return MPC_OK;
}

int mpc_last_rows_dropped(mpc_solver* s, int32_t B, int32_t* rows_dropped) {
    g_err[0] = 0;
    if (!s || !rows_dropped) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_last_rows_dropped")) return rc;
    if (!s->d_rows_dropped) { memset(rows_dropped, 0, (size_t)B * 4); return MPC_OK; }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(rows_dropped, s->d_rows_dropped, (size_t)B * 4, hipMemcpyDeviceToHost));
    return MPC_OK;
}

int mpc_set_via_points(mpc_solver* s, int32_t B, const int32_t* n_via, const double* via) {
    g_err[0] = 0;
    if (!s) return MPC_EINVAL;
    if (s->P64.n_via <= 0) { set_err("mpc_set_via_points: the solver was not created with objective MPC_OBJ_MIN_TIME_VIA_POINTS"); return MPC_EINVAL; }
    HIP_TRY(hipSetDevice(s->device));
    s->p_nvia = s->d_nvia; s->p_via = s->d_via;
    if (!n_via || !via) {
        HIP_TRY(hipMemsetAsync(s->d_nvia, 0, (size_t)s->max_batch * 4, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->nvia_B = 0;             // every instance: no via-points
        return MPC_OK;
    }
    if (B <= 0 || B > s->max_batch) { set_err("mpc_set_via_points: B out of range"); return MPC_EBATCH; }
    for (int b = 0; b < B; ++b)
        if (n_via[b] < 0 || n_via[b] > s->P64.n_via) { set_err("mpc_set_via_points: n_via[b] must be in [0, cfg.max_via_points]"); return MPC_EINVAL; }
    HIP_TRY(hipMemcpyAsync(s->d_nvia, n_via, (size_t)B * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_via, via, (size_t)B * s->P64.n_via * 3 * 8, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->nvia_B = B;
    return MPC_OK;
}

int mpc_set_via_points_device(mpc_solver* s, const int32_t* d_n_via, const double* d_via) {
    g_err[0] = 0;
    if (!s) return MPC_EINVAL;
    if (s->P64.n_via <= 0) { set_err("mpc_set_via_points_device: the solver was not created with objective MPC_OBJ_MIN_TIME_VIA_POINTS"); return MPC_EINVAL; }
    if (!d_n_via || !d_via) return mpc_set_via_points(s, 0, nullptr, nullptr);
    s->p_nvia = d_n_via; s->p_via = d_via;
    return MPC_OK;
}

int mpc_costmap_to_obstacles_device(mpc_solver* s, int32_t B, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution,
                                    const double* d_origin, const double* d_robot_pose, double behind_robot_dist,
                                    int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices, int32_t* d_dropped) {
    g_err[0] = 0;
    if (!s || !d_cost || !d_origin || !d_robot_pose || !d_n_obstacles || !d_n_vertices || !d_vertices) { set_err("mpc_costmap_to_obstacles_device: null argument"); return MPC_EINVAL; }
    if (s->cfg.max_obstacles <= 0) { set_err("mpc_costmap_to_obstacles_device: the solver was created with max_obstacles = 0"); return MPC_EINVAL; }
    if (size_x < 1 || size_y < 1 || !(resolution > 0)) { set_err("mpc_costmap_to_obstacles_device: bad costmap geometry"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_costmap_to_obstacles_device")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::CostmapArgs a;
    a.cost = d_cost; a.origin = d_origin; a.pose = d_robot_pose;
    a.size_x = size_x; a.size_y = size_y; a.resolution = resolution; a.behind_dist = behind_robot_dist;
    a.O = s->cfg.max_obstacles; a.V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1;
    a.n_obstacles = d_n_obstacles; a.n_vertices = d_n_vertices; a.vertices = d_vertices; a.dropped = d_dropped;
    return costmap_timed_launch(s, mpc::costmap_to_obstacles_kernel, B, mpc::kCostmapThreads, a);
}

int mpc_costmap_to_obstacles(mpc_solver* s, int32_t B, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution,
                             const double* origin, const double* robot_pose, double behind_robot_dist,
                             int32_t* n_obstacles, int32_t* n_vertices, double* vertices, int32_t* dropped) {
    g_err[0] = 0;
    if (!s || !cost || !origin || !robot_pose || !n_obstacles || !n_vertices || !vertices) { set_err("mpc_costmap_to_obstacles: null argument"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (s->cfg.max_obstacles <= 0 || size_x < 1 || size_y < 1) { set_err("mpc_costmap_to_obstacles: bad argument"); return MPC_EINVAL; }
    HIP_TRY(hipSetDevice(s->device));
    const size_t O = s->cfg.max_obstacles, V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1, nb = (size_t)B;
    const mpc::StagePiece pc[7] = {stage_in(cost, nb * size_x * size_y), stage_in(origin, nb * 2 * 8), stage_in(robot_pose, nb * 3 * 8), stage_out(n_obstacles, nb * 4), stage_out(n_vertices, nb * O * 4),
                                   stage_out(vertices, nb * O * V * 2 * 8), stage_out(dropped, nb * 4)};
    return staged_call(s, "mpc_costmap_to_obstacles", true, true, pc, 7, [&](void** d) -> int {
        // the kernel writes the vertices it finds: the rest is cleared on the device, behind the copy of the inputs
        HIP_TRY(hipMemsetAsync(d[4], 0, pc[4].bytes, s->stream));
        HIP_TRY(hipMemsetAsync(d[5], 0, pc[5].bytes, s->stream));
        return mpc_costmap_to_obstacles_device(s, B, (const uint8_t*)d[0], size_x, size_y, resolution, (const double*)d[1], (const double*)d[2], behind_robot_dist,
                                               (int32_t*)d[3], (int32_t*)d[4], (double*)d[5], (int32_t*)d[6]);
    });
}

int mpc_grid_update_device(mpc_solver* s, int32_t B, const double* d_x0_new, double* d_x, double* d_u, double* d_dt,
                           int32_t adapt, int32_t n_min, int32_t n_max, double dt_hyst_ratio) {
    g_err[0] = 0;
    if (!s || !d_x || !d_u || !d_dt) { set_err("mpc_grid_update_device: null argument"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH | REF_NGRID | REF_SETS, "mpc_grid_update_device")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::GridUpdateArgs a;
    memset(&a, 0, sizeof(a));
    a.x0 = d_x0_new; a.x = d_x; a.u = d_u; a.dt = d_dt; a.n_stride = s->cfg.n;
    a.dual = s->d_dual; a.dual_words = s->dual_words; a.dual_ns = s->plan.WL.NS;
    if (!s->cfg.dt_free) {
        if (!d_x0_new) { set_err("mpc_grid_update_device: the fixed grid shifts towards the new start state (d_x0_new)"); return MPC_EINVAL; }
        a.mode = 0;
        a.n_grid = s->use_ngrid ? s->d_ngrid : nullptr;
    } else {
        if (!adapt) return MPC_OK;                      // variable grid without adaptation: nothing moves (x0 is overwritten by the solve)
        if (n_min < 3) n_min = 3;                       // the solver needs 3 grid points (the reference allows 2)
        if (n_max > s->cfg.n) n_max = s->cfg.n;
        if (!s->use_ngrid) {                            // first adaptation: every slot starts at the uniform size
            HIP_TRY(hipMemsetAsync(s->d_ngrid, 0, (size_t)s->max_batch * 4, s->stream));
            std::vector<int32_t> full((size_t)s->max_batch, s->cfg.n);
            HIP_TRY(hipMemcpyAsync(s->d_ngrid, full.data(), full.size() * 4, hipMemcpyHostToDevice, s->stream));
            HIP_TRY(hipStreamSynchronize(s->stream));
            s->use_ngrid = 1; s->ngrid_B = s->max_batch;
        }
        a.mode = 1; a.n_grid = s->d_ngrid; a.n_min = n_min; a.n_max = n_max; a.dt_refs = s->d_dtref; a.set_of = s->p_set_of; a.hyst = dt_hyst_ratio;
    }
    hipLaunchKernelGGL(mpc::grid_update_kernel, dim3(B), dim3(64), (size_t)s->cfg.n * 5 * 8, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_get_grid_sizes(mpc_solver* s, int32_t B, int32_t* n_grid) {
    g_err[0] = 0;
    if (!s || !n_grid) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_get_grid_sizes")) return rc;
    if (!s->use_ngrid) { for (int b = 0; b < B; ++b) n_grid[b] = s->cfg.n; return MPC_OK; }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(n_grid, s->d_ngrid, (size_t)B * 4, hipMemcpyDeviceToHost));
    return MPC_OK;
}

int mpc_check_feasibility_device(mpc_solver* s, int32_t B, const double* d_x, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution,
                                 const double* d_origin, const double* footprint_spec, int32_t n_spec, double inscribed_radius,
                                 double min_resolution_collision_check_angular, int32_t look_ahead_idx, int32_t* d_feasible) {
    g_err[0] = 0;
    if (!s || !d_x || !d_cost || !d_origin || !d_feasible) { set_err("mpc_check_feasibility_device: null argument"); return MPC_EINVAL; }
    if (size_x < 1 || size_y < 1 || !(resolution > 0) || n_spec < 0 || n_spec > mpc::kFeasMaxSpec || (n_spec > 0 && !footprint_spec) ||
        !(inscribed_radius > 0) || !(min_resolution_collision_check_angular > 0)) {
        set_err("mpc_check_feasibility_device: bad costmap geometry, footprint (<= 32 points) or resolution parameters"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH | REF_NGRID_NO_HINT, "mpc_check_feasibility_device")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::FeasArgs a;
    memset(&a, 0, sizeof(a));
    a.x = d_x; a.n_grid = s->use_ngrid ? s->d_ngrid : nullptr; a.n_stride = s->cfg.n;
    a.cost = d_cost; a.origin = d_origin; a.size_x = size_x; a.size_y = size_y; a.resolution = resolution;
    a.n_spec = n_spec;
    for (int i = 0; i < 2 * n_spec; ++i) a.spec[i] = footprint_spec[i];
    a.inscribed_radius = inscribed_radius; a.min_res_angular = min_resolution_collision_check_angular; a.look_ahead_idx = look_ahead_idx;
    a.feasible = d_feasible;
    hipLaunchKernelGGL(mpc::feasibility_kernel, dim3(B), dim3(mpc::kFeasThreads), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_check_feasibility(mpc_solver* s, int32_t B, const double* x, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution,
                          const double* origin, const double* footprint_spec, int32_t n_spec, double inscribed_radius,
                          double min_resolution_collision_check_angular, int32_t look_ahead_idx, int32_t* feasible) {
    g_err[0] = 0;
    if (!s || !x || !cost || !origin || !feasible) { set_err("mpc_check_feasibility: null argument"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (B > s->max_batch || size_x < 1 || size_y < 1) { set_err("mpc_check_feasibility: bad argument"); return MPC_EINVAL; }
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = B, n = s->cfg.n;
    const mpc::StagePiece pc[4] = {stage_in(x, nb * n * 3 * 8), stage_in(cost, nb * size_x * size_y), stage_in(origin, nb * 2 * 8), stage_out(feasible, nb * 4)};
    return staged_call(s, "mpc_check_feasibility", true, true, pc, 4, [&](void** d) {
        return mpc_check_feasibility_device(s, B, (const double*)d[0], (const uint8_t*)d[1], size_x, size_y, resolution, (const double*)d[2], footprint_spec, n_spec,
                                            inscribed_radius, min_resolution_collision_check_angular, look_ahead_idx, (int32_t*)d[3]);
    });
}

int mpc_set_grid_sizes(mpc_solver* s, const int32_t* n_grid, int32_t B) {
    g_err[0] = 0;
    if (!s) return MPC_EINVAL;
    if (!n_grid) { s->use_ngrid = 0; return MPC_OK; }
    if (B <= 0 || B > s->max_batch) { set_err("mpc_set_grid_sizes: B out of range"); return MPC_EBATCH; }
    for (int b = 0; b < B; ++b)
        if (n_grid[b] < 3 || n_grid[b] > s->cfg.n) { set_err("mpc_set_grid_sizes: n_grid[b] must be in [3, cfg.n]"); return MPC_EINVAL; }
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipMemcpyAsync(s->d_ngrid, n_grid, (size_t)B * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->use_ngrid = 1;
    s->ngrid_B = B;
    return MPC_OK;
}

int mpc_set_parameter_sets(mpc_solver* s, int32_t n_sets, const mpc_config* sets, int32_t B, const int32_t* set_of) {
    g_err[0] = 0;
    if (!s) { set_err("mpc_set_parameter_sets: null handle"); return MPC_EINVAL; }
    if (!sets) { s->p_set_of = nullptr; s->sets_B = 0; return MPC_OK; }      // every instance: the handle's own configuration (table entry 0)
    if (n_sets < 1 || n_sets > s->max_batch) { set_err("mpc_set_parameter_sets: n_sets out of range [1, max_batch]"); return MPC_EBATCH; }
    if (B < 1 || B > s->max_batch) { set_err("mpc_set_parameter_sets: B out of range [1, max_batch]"); return MPC_EBATCH; }
    if (!set_of) { set_err("mpc_set_parameter_sets: set_of is NULL"); return MPC_EINVAL; }
    for (int i = 0; i < n_sets; ++i) {
        const std::string why = mpc::parameter_set_error(s->cfg, sets[i]);
        if (!why.empty()) { snprintf(g_err, sizeof(g_err), "mpc_set_parameter_sets: set %d: %s", i, why.c_str()); return MPC_EINVAL; }
    }
    for (int b = 0; b < B; ++b)
        if (set_of[b] < 0 || set_of[b] >= n_sets) { snprintf(g_err, sizeof(g_err), "mpc_set_parameter_sets: set_of[%d] = %d is not in [0, n_sets)", b, set_of[b]); return MPC_EINVAL; }
    HIP_TRY(hipSetDevice(s->device));
    // nothing is changed before this point.  The pinned image: the table (entry 0 = the handle's own configuration, then the sets), then set_of as table entries
    const size_t entries = (size_t)n_sets + 1;
    const bool grow = entries > (size_t)s->tab_cap;
    const size_t cap = grow ? entries : (size_t)s->tab_cap;
    const TabLayout t(s->cfg, cap);
    const size_t so_off = t.bytes, img_bytes = so_off + (size_t)B * 4;
    if (img_bytes > s->bufs[BUF_H_TAB].bytes) HIP_TRY(buf_alloc(s->bufs[BUF_H_TAB], img_bytes));      // (no copy from the old one is in flight: every call waits for its own)
    memset(s->h_tab, 0, img_bytes);
    put_entry(s->cfg, s->cfg, cap, 0, s->h_tab);
    for (int i = 0; i < n_sets; ++i) put_entry(s->cfg, sets[i], cap, (size_t)i + 1, s->h_tab);
    int32_t* so = reinterpret_cast<int32_t*>(s->h_tab + so_off);
    for (int b = 0; b < B; ++b) so[b] = set_of[b] + 1;
    if (!s->d_set_of) HIP_TRY(buf_alloc(s->bufs[BUF_SET_OF], (size_t)s->max_batch * 4));
    if (grow) {
        // a launch still in flight may read the old table: wait for it before the table is replaced (a new one, then the old one freed)
        HIP_TRY(hipStreamSynchronize(s->stream));
        HIP_TRY(buf_alloc(s->bufs[BUF_TAB], t.bytes));
        s->tab_cap = (int)cap;
        point_tables(s);
        HIP_TRY(hipMemcpyAsync(s->d_tab, s->h_tab, t.bytes, hipMemcpyHostToDevice, s->stream));
    } else {
        // entries 1 .. n_sets of each piece (entry 0, the handle's own record, stays as mpc_create wrote it); ordered behind every launch already enqueued on the stream
        if (s->d_tab64) HIP_TRY(hipMemcpyAsync(s->d_tab64 + 1, s->h_tab + t.o64 + sizeof(mpc::Problem<double>), (size_t)n_sets * sizeof(mpc::Problem<double>), hipMemcpyHostToDevice, s->stream));
        if (s->d_tab32) HIP_TRY(hipMemcpyAsync(s->d_tab32 + 1, s->h_tab + t.o32 + sizeof(mpc::Problem<float>), (size_t)n_sets * sizeof(mpc::Problem<float>), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(s->d_dtref + 1, s->h_tab + t.odt + 8, (size_t)n_sets * 8, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(s->d_tabev + 1, s->h_tab + t.oev + sizeof(mpc::EvalParams), (size_t)n_sets * sizeof(mpc::EvalParams), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipMemcpyAsync(s->d_set_of, so, (size_t)B * 4, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->p_set_of = s->d_set_of;
    s->sets_B = B;
    return MPC_OK;
}

int mpc_synchronize(mpc_solver* s) {
    if (!s) return MPC_EINVAL;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return MPC_OK;
}

int mpc_lds_bytes(const mpc_solver* s, int64_t* bytes) {
    if (!s || !bytes) return MPC_EINVAL;
    *bytes = (int64_t)s->plan.lds();
    return MPC_OK;
}

int mpc_occupancy(mpc_solver* s, int32_t B, int32_t* workgroups_per_cu, int64_t* lds_bytes) {
    if (!s || !workgroups_per_cu || B <= 0) return MPC_EINVAL;
    g_err[0] = 0;
    HIP_TRY(hipSetDevice(s->device));
    const bool f32 = s->cfg.precision == MPC_FP32;      // (MPC_MIXED: its fp64 phase)
    const mpc::KernelChoice k = mpc::plan_launch(s->plan, f32, B);
    int occ = 0;
    HIP_TRY(kernel_occupancy(f32, s->cfg.model, k, &occ));
    *workgroups_per_cu = occ;
    if (lds_bytes) *lds_bytes = (int64_t)k.lds;
    return MPC_OK;
}

// developer observation (not part of include/mpc_hip.h, like mpc_debug_profile): what the launch plan decided for a launch of B instances of this handle -- the handle's
// shape word (mpc_core.hpp::shape_flags) and the shape word compiled into the kernel such a launch runs (0: a kernel that reads the word at run time).  Asks plan_launch, as
// the launch and mpc_occupancy do; tests/test_gpu_shape_kernel.py asserts on it.
int mpc_debug_kernel_shape(mpc_solver* s, int32_t B, int32_t* handle_flags, int32_t* kernel_shape) {
    if (!s || !handle_flags || !kernel_shape || B <= 0) return MPC_EINVAL;
    *handle_flags = s->plan.flags;
    *kernel_shape = mpc::plan_launch(s->plan, s->cfg.precision == MPC_FP32, B).shape;
    return MPC_OK;
}
// ... and the developer switch that goes with it: on = 0 keeps this handle on the kernels that read the shape word at run time (the same problem through the run-time-flags
// fixed-layout kernel: what the test compares the shape-known kernel with), on != 0 gives it back what make_launch_plan decided
int mpc_debug_use_shape_kernel(mpc_solver* s, int32_t on) {
    if (!s) return MPC_EINVAL;
    s->plan.shape_ok = on != 0 && mpc::make_launch_plan(s->cfg).shape_ok;
    return MPC_OK;
}

int mpc_last_kernel_ms(mpc_solver* s, float* ms) {
    if (!s || !ms) return MPC_EINVAL;
    if (!s->timed) { *ms = 0.f; return MPC_OK; }
    HIP_TRY(hipEventSynchronize(s->ev1));
    HIP_TRY(hipEventElapsedTime(ms, s->ev0, s->ev1));
    return MPC_OK;
}

// The solve's arrays of a host-pointer call in the four blocks of mpc_create (mpc::step_pieces), for mpc_solve_batch / mpc_step_batch and for the solve inside
// mpc_controller_step_batch: pack() copies every input the caller gave into the pinned block and enqueues the ONE host-to-device copy, fetch() enqueues the ONE
// device-to-host copy of the outputs (with the grid sizes behind them), unpack() hands them out once the stream has been synchronised.
typedef mpc::StepPieces SP;
struct SolveStage {
    SP pc;
    const void* d[SP::N_IN];      // device address of every input piece, NULL for one this call does not have
    mpc_obstacles dob;
    const double* at(int i) const { return (const double*)d[i]; }
    double* out(const mpc_solver* s, int i) const { return (double*)(s->d_out + pc.off[i]); }      // device address of an output piece
    int32_t* iout(const mpc_solver* s, int i) const { return (int32_t*)(s->d_out + pc.off[i]); }
    int pack(mpc_solver* s, const char* who, int32_t B, const double* x0, const double* xf, const double* u_prev, const double* dt_prev, const double* x_init, const double* u_init,
             const double* dt_init, const mpc_obstacles* ob) {
        if (const int rc = refused(s, B, REF_OBSTACLES, who, ob)) return rc;
        const bool obst = s->cfg.max_obstacles > 0;
        const void* src[SP::N_IN] = {x0, xf, u_prev, dt_prev, x_init, u_init, dt_init, obst ? ob->n_obstacles : nullptr, obst ? ob->n_vertices : nullptr,
                                     obst ? ob->vertices : nullptr, obst ? ob->radius : nullptr, obst ? ob->velocity : nullptr};
        pc = mpc::step_pieces(s->cfg, (size_t)B, u_prev != nullptr, dt_prev != nullptr, x_init != nullptr, src[SP::RADIUS] != nullptr, src[SP::VELOCITY] != nullptr);
        if (pc.in_bytes > s->bufs[BUF_H_IN].bytes) { snprintf(g_err, sizeof(g_err), "%s: internal staging overflow", who); return MPC_EINVAL; }
        for (int i = 0; i < SP::N_IN; ++i) {      // (a piece the list always has and this caller does not give: x0 and xf of the controller cycle, which computes them)
            d[i] = pc.bytes[i] && src[i] ? s->d_in + pc.off[i] : nullptr;
            if (d[i]) memcpy(s->h_in + pc.off[i], src[i], pc.bytes[i]);
        }
        dob = {(const int32_t*)d[SP::N_OBSTACLES], (const int32_t*)d[SP::N_VERTICES], (const double*)d[SP::VERTICES], (const double*)d[SP::RADIUS], (const double*)d[SP::VELOCITY]};
        HIP_TRY(hipMemcpyAsync(s->d_in, s->h_in, pc.in_bytes, hipMemcpyHostToDevice, s->stream));
        return MPC_OK;
    }
    int fetch(mpc_solver* s, bool n_grid) const {
        if (n_grid) HIP_TRY(hipMemcpyAsync(s->d_out + pc.off[SP::N_GRID], s->d_ngrid, pc.bytes[SP::N_GRID], hipMemcpyDeviceToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(s->h_out, s->d_out, pc.out_bytes, hipMemcpyDeviceToHost, s->stream));
        return MPC_OK;
    }
    void unpack(const mpc_solver* s, double* x_out, double* u_out, double* dt_out, int32_t* status, int32_t* iters, int32_t* n_grid_out) const {
        void* dst[5] = {x_out, u_out, dt_out, status, iters};      // (status and iters may be NULL)
        for (int i = 0; i < 5; ++i) if (dst[i]) memcpy(dst[i], s->h_out + pc.off[SP::X_OUT + i], pc.bytes[SP::X_OUT + i]);
        if (!n_grid_out) return;
        if (s->use_ngrid) memcpy(n_grid_out, s->h_out + pc.off[SP::N_GRID], pc.bytes[SP::N_GRID]);
        else for (size_t i = 0; i < pc.bytes[SP::N_GRID] / 4; ++i) n_grid_out[i] = s->cfg.n;
    }
};

// host-pointer entry of one control cycle: `outer` x (grid update -> solve) without a host round trip in between
static int step_host(mpc_solver* s, int32_t B, const double* x0, const double* xf, const double* u_prev, const double* dt_prev,
                     const double* x_init, const double* u_init, const double* dt_init, const mpc_obstacles* obstacles,
                     int32_t outer, int32_t adapt, int32_t n_min, int32_t n_max, double dt_hyst_ratio,
                     double* x_out, double* u_out, double* dt_out, int32_t* status, int32_t* iters, int32_t* n_grid_out) {
    g_err[0] = 0;
    if (!s || !x0 || !xf || !x_out || !u_out || !dt_out) { set_err("mpc_solve_batch / mpc_step_batch: null argument"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_solve_batch")) return rc;
    if ((x_init != nullptr) != (u_init != nullptr) || (x_init != nullptr) != (dt_init != nullptr)) {
        set_err("mpc_solve_batch: x_init, u_init and dt_init must be given together (all three or none)"); return MPC_EINVAL; }
    HIP_TRY(hipSetDevice(s->device));
    SolveStage st;
    if (const int rc = st.pack(s, "mpc_solve_batch", B, x0, xf, u_prev, dt_prev, x_init, u_init, dt_init, obstacles)) return rc;
    const int rc = mpc_step_batch_device(s, B, st.at(SP::X0), st.at(SP::XF), st.at(SP::U_PREV), st.at(SP::DT_PREV), st.at(SP::X_INIT), st.at(SP::U_INIT), st.at(SP::DT_INIT), &st.dob,
                                         outer, adapt, n_min, n_max, dt_hyst_ratio, st.out(s, SP::X_OUT), st.out(s, SP::U_OUT), st.out(s, SP::DT_OUT), st.iout(s, SP::STATUS), st.iout(s, SP::ITERS));
    if (rc != MPC_OK) return rc;
    if (const int rc2 = st.fetch(s, n_grid_out && s->use_ngrid)) return rc2;
    HIP_TRY(hipStreamSynchronize(s->stream));
    st.unpack(s, x_out, u_out, dt_out, status, iters, n_grid_out);
    return MPC_OK;
}

int mpc_solve_batch(mpc_solver* s, int32_t B, const double* x0, const double* xf, const double* u_prev, const double* dt_prev,
                    const double* x_init, const double* u_init, const double* dt_init, const mpc_obstacles* obstacles,
                    double* x_out, double* u_out, double* dt_out, int32_t* status, int32_t* iters) {
    return step_host(s, B, x0, xf, u_prev, dt_prev, x_init, u_init, dt_init, obstacles, 1, 0, 0, 0, 0.0, x_out, u_out, dt_out, status, iters, nullptr);
}

int mpc_step_batch(mpc_solver* s, int32_t B, const double* x0, const double* xf, const double* u_prev, const double* dt_prev,
                   const double* x_init, const double* u_init, const double* dt_init, const mpc_obstacles* obstacles,
                   int32_t outer_iterations, int32_t adapt, int32_t n_min, int32_t n_max, double dt_hyst_ratio,
                   double* x_out, double* u_out, double* dt_out, int32_t* status, int32_t* iters, int32_t* n_grid_out) {
    return step_host(s, B, x0, xf, u_prev, dt_prev, x_init, u_init, dt_init, obstacles, outer_iterations, adapt, n_min, n_max, dt_hyst_ratio, x_out, u_out, dt_out, status,
                     iters, n_grid_out);
}

}  // extern "C"

// ---- whole Controller::step cycles for a batch (mpc_controller_cycle.hpp)

// the slot state, allocated and zeroed by the first controller call (all zero = every slot empty, no step made, no solution)
static int cycle_state(mpc_solver* s) {
    if (s->d_cyc) return MPC_OK;
    const CycLayout L((size_t)s->max_batch, (size_t)s->cfg.n);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(buf_alloc(s->bufs[BUF_CYC_LIVE], (size_t)s->max_batch * 4));
    HIP_TRY(buf_alloc(s->bufs[BUF_CYC], L.bytes));
    HIP_TRY(buf_fill(s, s->bufs[BUF_CYC_LIVE]));
    HIP_TRY(buf_fill(s, s->bufs[BUF_CYC]));
    HIP_TRY(hipDeviceSynchronize());      // null-stream fills vs the handle's non-blocking stream (see mpc_create)
    return MPC_OK;
}

static const char* cycle_params_error(const mpc_solver* s, const mpc_cycle_params* p, const void* fb, const void* age) {
    if (!p) return "mpc_controller_step_batch: null mpc_cycle_params";
    const int n_ref = p->n_ref == 0 ? s->cfg.n : p->n_ref;
    if (n_ref < 3 || n_ref > s->cfg.n) return "mpc_controller_step_batch: n_ref must be in [3, cfg.n] (0 = cfg.n)";
    if ((fb != nullptr) != (age != nullptr)) return "mpc_controller_step_batch: x_feedback and feedback_age must be given together (both or neither)";
    return nullptr;
}

extern "C" {

int mpc_controller_step_batch_device(mpc_solver* s, int32_t B, const mpc_cycle_params* p, const double* d_plan, const int32_t* d_n_plan, int32_t plan_stride,
                                     const double* d_x_feedback, const double* d_feedback_age, const int32_t* d_reset, const double* d_u_prev, const double* d_dt_prev,
                                     const mpc_obstacles* d_obstacles, double* d_x_out, double* d_u_out, double* d_dt_out, int32_t* d_status, int32_t* d_iters,
                                     int32_t* d_reinit_out) {
    g_err[0] = 0;
    if (!s || !d_plan || !d_n_plan || !d_x_out || !d_u_out || !d_dt_out || plan_stride < 2) { set_err("mpc_controller_step_batch_device: null argument or plan_stride < 2"); return MPC_EINVAL; }
    if (const char* why = cycle_params_error(s, p, d_x_feedback, d_feedback_age)) { set_err(why); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH | REF_VIA | REF_SETS | REF_OBSTACLES, "mpc_controller_step_batch", d_obstacles)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if (const int rc = cycle_state(s)) return rc;
    s->use_ngrid = 1; s->ngrid_B = s->max_batch;      // the grid sizes belong to the controller from here on (never uninitialised: mpc_create filled them with cfg.n)
    const CycLayout L((size_t)s->max_batch, (size_t)s->cfg.n);
    const size_t n = (size_t)s->cfg.n, nb = (size_t)B;
    double *x0 = (double*)(s->d_cyc + L.x0), *xf = (double*)(s->d_cyc + L.xf), *x = (double*)(s->d_cyc + L.x), *u = (double*)(s->d_cyc + L.u), *dt = (double*)(s->d_cyc + L.dt);
    int32_t* mode = (int32_t*)(s->d_cyc + L.mode);
    int n_min = p->n_min < 3 ? 3 : p->n_min, n_max = p->n_max > s->cfg.n ? s->cfg.n : p->n_max;      // as mpc_grid_update_device
    mpc::CycleArgs a;
    memset(&a, 0, sizeof(a));
    a.plan = d_plan; a.n_plan = d_n_plan; a.plan_stride = plan_stride; a.x_feedback = d_x_feedback; a.feedback_age = d_feedback_age; a.reset = d_reset;
    a.n_ref = p->n_ref == 0 ? s->cfg.n : p->n_ref; a.warm_start = p->warm_start; a.force_reinit_num_steps = p->force_reinit_num_steps;
    a.estimate_orientation = p->initial_plan_estimate_orientation; a.prefer_x_feedback = p->prefer_x_feedback; a.reference_reinit_sampling = p->reference_reinit_sampling;
    a.dt_free = s->cfg.dt_free; a.update = s->cfg.dt_free ? (p->adapt != 0) : (p->warm_start != 0);
    a.new_goal_dist = p->force_reinit_new_goal_dist; a.new_goal_angular = p->force_reinit_new_goal_angular; a.period = p->period;
    a.seq = (int32_t*)(s->d_cyc + L.seq); a.live = s->d_cyc_live; a.has_solution = (int32_t*)(s->d_cyc + L.has); a.last_goal = (double*)(s->d_cyc + L.goal);
    a.x0 = x0; a.xf = xf; a.init_mode = mode; a.reinit_out = d_reinit_out;
    a.g.x0 = x0; a.g.x = x; a.g.u = u; a.g.dt = dt; a.g.n_grid = s->d_ngrid; a.g.n_stride = s->cfg.n; a.g.mode = s->cfg.dt_free ? 1 : 0;
    a.g.n_min = n_min; a.g.n_max = n_max; a.g.dt_refs = s->d_dtref; a.g.set_of = s->p_set_of; a.g.hyst = p->dt_hyst_ratio;
    // kept multipliers: dropped per slot on reset[b]; the variable grid drops them when the grid size changes (mpc_grid_update.hpp); the fixed grid's shift leaves them
    // where they are (the prepare kernel hides them from it), as the facade's host-side shift does (include/mpc_controller.hpp)
    a.g.dual = s->d_dual; a.g.dual_words = s->dual_words; a.g.dual_ns = s->plan.WL.NS;
    const size_t lds = (n * 5 + (size_t)plan_stride * 4) * 8;
    if (lds > 64u * 1024u) { set_err("mpc_controller_step_batch: 5 cfg.n + 4 plan_stride doubles exceed the 64 KB of LDS of the prepare kernel"); return MPC_EINVAL; }
    if (lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mpc::controller_prepare_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(mpc::controller_prepare_kernel, dim3(B), dim3(64), lds, s->stream, a);
    HIP_TRY(hipGetLastError());
    // the solve with cold, plan-guess and warm instances in one launch, in place on the slots' arrays; then the remaining outer iterations with every instance warm
    int rc = solve_device(s, B, x0, xf, d_u_prev, d_dt_prev, x, u, dt, d_obstacles, x, u, dt, d_status, d_iters, mode);
    for (int it = 1; it < p->outer_iterations && rc == MPC_OK; ++it) {
        if (s->cfg.dt_free) rc = mpc_grid_update_device(s, B, x0, x, u, dt, p->adapt, p->n_min, p->n_max, p->dt_hyst_ratio);
        if (rc == MPC_OK) rc = solve_device(s, B, x0, xf, d_u_prev, d_dt_prev, x, u, dt, d_obstacles, x, u, dt, d_status, d_iters, nullptr);
    }
    if (rc != MPC_OK) return rc;
    HIP_TRY(hipMemcpyAsync(d_x_out, x, nb * n * 24, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_u_out, u, nb * n * 16, hipMemcpyDeviceToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_dt_out, dt, nb * 8, hipMemcpyDeviceToDevice, s->stream));
    return MPC_OK;
}

int mpc_controller_step_batch(mpc_solver* s, int32_t B, const mpc_cycle_params* p, const double* plan, const int32_t* n_plan, int32_t plan_stride,
                              const double* x_feedback, const double* feedback_age, const int32_t* reset, const double* u_prev, const double* dt_prev,
                              const mpc_obstacles* obstacles, double* x_out, double* u_out, double* dt_out, int32_t* status, int32_t* iters, int32_t* reinit_out,
                              int32_t* n_grid_out) {
    g_err[0] = 0;
    if (!s || !plan || !n_plan || !x_out || !u_out || !dt_out || plan_stride < 2) { set_err("mpc_controller_step_batch: null argument or plan_stride < 2"); return MPC_EINVAL; }
    if (const char* why = cycle_params_error(s, p, x_feedback, feedback_age)) { set_err(why); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_controller_step_batch")) return rc;
    for (int b = 0; b < B; ++b)
        if (n_plan[b] < 2 || n_plan[b] > plan_stride) { snprintf(g_err, sizeof(g_err), "mpc_controller_step_batch: n_plan[%d] = %d is not in [2, plan_stride]", b, n_plan[b]); return MPC_EINVAL; }
    if (const int rc = refused(s, B, REF_OBSTACLES, "mpc_controller_step_batch", obstacles)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    // the cycle's own inputs (plans, feedback, reset) and reinit_out through the shared pair; u_prev / dt_prev / obstacles and the solve's outputs through the blocks
    // of mpc_solve_batch
    const size_t nb = (size_t)B;
    const mpc::StagePiece pc[6] = {stage_in(plan, nb * (size_t)plan_stride * 24), stage_in(n_plan, nb * 4), stage_in(x_feedback, nb * 24), stage_in(feedback_age, nb * 8), stage_in(reset, nb * 4), stage_out(reinit_out, nb * 4)};
    SolveStage st;
    const int rc = staged_call(s, "mpc_controller_step_batch", false, false, pc, 6, [&](void** d) -> int {
        if (const int rp = st.pack(s, "mpc_controller_step_batch", B, nullptr, nullptr, u_prev, dt_prev, nullptr, nullptr, nullptr, obstacles)) return rp;
        const int rd = mpc_controller_step_batch_device(s, B, p, (const double*)d[0], (const int32_t*)d[1], plan_stride, (const double*)d[2], (const double*)d[3], (const int32_t*)d[4],
                                                        st.at(SP::U_PREV), st.at(SP::DT_PREV), &st.dob, st.out(s, SP::X_OUT), st.out(s, SP::U_OUT), st.out(s, SP::DT_OUT), st.iout(s, SP::STATUS), st.iout(s, SP::ITERS), (int32_t*)d[5]);
        return rd != MPC_OK ? rd : st.fetch(s, true);
    });
    if (rc == MPC_OK) st.unpack(s, x_out, u_out, dt_out, status, iters, n_grid_out);
    return rc;
}

int mpc_controller_state(mpc_solver* s, int32_t B, int32_t* seq, int32_t* empty, double* last_goal) {
    g_err[0] = 0;
    if (!s) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_controller_state")) return rc;
    const size_t nb = (size_t)B;
    if (!s->d_cyc) {      // no controller call yet
        if (seq) memset(seq, 0, nb * 4);
        if (empty) for (size_t b = 0; b < nb; ++b) empty[b] = 1;
        if (last_goal) memset(last_goal, 0, nb * 24);
        return MPC_OK;
    }
    const CycLayout L((size_t)s->max_batch, (size_t)s->cfg.n);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (seq) HIP_TRY(hipMemcpy(seq, s->d_cyc + L.seq, nb * 4, hipMemcpyDeviceToHost));
    if (last_goal) HIP_TRY(hipMemcpy(last_goal, s->d_cyc + L.goal, nb * 24, hipMemcpyDeviceToHost));
    if (empty) {
        HIP_TRY(hipMemcpy(empty, s->d_cyc_live, nb * 4, hipMemcpyDeviceToHost));
        for (size_t b = 0; b < nb; ++b) empty[b] = empty[b] ? 0 : 1;
    }
    return MPC_OK;
}

}  // extern "C"

// ---- what a trajectory is worth under the handle's NLP (mpc_evaluate.hpp)

extern "C" {

int mpc_evaluate_batch_device(mpc_solver* s, int32_t B, const double* d_x0, const double* d_xf, const double* d_u_prev, const double* d_dt_prev,
                              const double* d_x, const double* d_u, const double* d_dt, const mpc_obstacles* d_obstacles, const mpc_eval_out* d_out) {
    g_err[0] = 0;
    if (!s || !d_x || !d_u || !d_out || (s->cfg.dt_free && !d_dt)) { set_err("mpc_evaluate_batch_device: null argument (x, u, out; dt on the variable grid)"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH | REF_NGRID | REF_VIA | REF_SETS, "mpc_evaluate_batch")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::EvalArgs a;
    memset(&a, 0, sizeof(a));
    a.tab = s->d_tabev; a.set_of = s->p_set_of; a.n_grid = s->use_ngrid ? s->d_ngrid : nullptr; a.n_stride = s->cfg.n;
    a.x0 = d_x0; a.xf = d_xf; a.u_prev = d_u_prev; a.dt_prev = d_dt_prev; a.x = d_x; a.u = d_u; a.dt = d_dt;
    if (s->cfg.max_obstacles > 0 && d_obstacles && d_obstacles->n_obstacles && d_obstacles->n_vertices && d_obstacles->vertices) a.ob = *d_obstacles;      // (without them: clearance +inf)
    a.n_via = s->p_nvia; a.via = s->p_via; a.out = *d_out;
    hipLaunchKernelGGL(mpc::evaluate_kernel, dim3(B), dim3(64), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_evaluate_batch(mpc_solver* s, int32_t B, const double* x0, const double* xf, const double* u_prev, const double* dt_prev,
                       const double* x, const double* u, const double* dt, const mpc_obstacles* obstacles, const mpc_eval_out* out) {
    g_err[0] = 0;
    if (!s || !x || !u || !out || (s->cfg.dt_free && !dt)) { set_err("mpc_evaluate_batch: null argument (x, u, out; dt on the variable grid)"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_evaluate_batch")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, n = (size_t)s->cfg.n, O = s->cfg.max_obstacles > 0 ? (size_t)s->cfg.max_obstacles : 0, V = s->cfg.max_vertices > 0 ? (size_t)s->cfg.max_vertices : 1;
    const mpc_obstacles none = {nullptr, nullptr, nullptr, nullptr, nullptr};      // (without the three arrays: clearance +inf)
    const mpc_obstacles& ob = O > 0 && obstacles && obstacles->n_obstacles && obstacles->n_vertices && obstacles->vertices ? *obstacles : none;
    const mpc::StagePiece pc[17] = {stage_in(x0, nb * 24), stage_in(xf, nb * 24), stage_in(u_prev, nb * 16), stage_in(dt_prev, nb * 8), stage_in(x, nb * n * 24), stage_in(u, nb * n * 16), stage_in(dt, nb * 8),
                                    stage_in(ob.n_obstacles, nb * 4), stage_in(ob.n_vertices, nb * O * 4), stage_in(ob.vertices, nb * O * V * 16), stage_in(ob.radius, nb * O * 8), stage_in(ob.velocity, nb * O * 16),
                                    stage_out(out->objective, nb * 8), stage_out(out->eq_violation, nb * 8), stage_out(out->ineq_violation, nb * 8), stage_out(out->clearance, nb * 8), stage_out(out->closest, nb * 8)};
    return staged_call(s, "mpc_evaluate_batch", false, false, pc, 17, [&](void** d) {
        const mpc_obstacles dob = {(const int32_t*)d[7], (const int32_t*)d[8], (const double*)d[9], (const double*)d[10], (const double*)d[11]};
        const mpc_eval_out dout = {(double*)d[12], (double*)d[13], (double*)d[14], (double*)d[15], (int32_t*)d[16]};
        return mpc_evaluate_batch_device(s, B, (const double*)d[0], (const double*)d[1], (const double*)d[2], (const double*)d[3], (const double*)d[4], (const double*)d[5],
                                         (const double*)d[6], &dob, &dout);
    });
}

}  // extern "C"

// ---- what the plugin runs around the step (mpc_plan_inputs.hpp)

// the argument checks both variants of mpc_plan_inputs_batch share: NULL when the call is fine
static const char* plan_inputs_error(const mpc_solver* s, const mpc_plan_params* p, const void* global_plan, const void* n_global, int32_t gstride, const void* robot_pose,
                                     const void* plan, const void* n_plan, int32_t plan_stride, const void* n_via, const void* via) {
    if (!s || !p || !global_plan || !n_global || !robot_pose || !plan || !n_plan) return "mpc_plan_inputs_batch: null argument (p, global_plan, n_global, robot_pose, plan, n_plan)";
    if (gstride < 2 || plan_stride < 2) return "mpc_plan_inputs_batch: gstride and plan_stride have to be at least 2";
    if ((n_via != nullptr) != (via != nullptr)) return "mpc_plan_inputs_batch: n_via and via go together";
    if (via && s->cfg.max_via_points <= 0) return "mpc_plan_inputs_batch: via-point outputs on a handle with max_via_points == 0";
    return nullptr;
}

extern "C" {

int mpc_plan_inputs_batch_device(mpc_solver* s, int32_t B, const mpc_plan_params* p, const double* d_global_plan, const int32_t* d_n_global, int32_t gstride,
                                 const double* d_robot_pose, int32_t* d_plan_begin, double* d_plan, int32_t* d_n_plan, int32_t plan_stride,
                                 int32_t* d_n_via, double* d_via, int32_t* d_goal_idx, int32_t* d_flags) {
    g_err[0] = 0;
    if (const char* e = plan_inputs_error(s, p, d_global_plan, d_n_global, gstride, d_robot_pose, d_plan, d_n_plan, plan_stride, d_n_via, d_via)) { set_err(e); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_plan_inputs_batch")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::PlanInputsArgs a;
    memset(&a, 0, sizeof(a));
    a.p = {p->global_plan_prune_distance, p->max_global_plan_lookahead_dist, p->global_plan_viapoint_sep, p->xy_goal_tolerance, p->yaw_goal_tolerance,
           p->global_plan_overwrite_orientation, p->moving_average_length, p->costmap_size_x, p->costmap_size_y, p->resolution};
    a.global = d_global_plan; a.n_global = d_n_global; a.gstride = gstride; a.robot = d_robot_pose; a.begin = d_plan_begin;
    a.plan = d_plan; a.n_plan = d_n_plan; a.plan_stride = plan_stride; a.max_via = s->cfg.max_via_points > 0 ? s->cfg.max_via_points : 0;
    a.n_via = d_n_via; a.via = d_via; a.goal_idx = d_goal_idx; a.flags = d_flags;
    hipLaunchKernelGGL(mpc::plan_inputs_kernel, dim3(B), dim3(64), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

}  // extern "C"

// u_stride: rows between two instances' first controls (cfg.n for u_out itself; 1 for the host variant's compact copy of the first rows)
static int commands_device(mpc_solver* s, int32_t B, const double* d_u, int32_t u_stride, const int32_t* d_status, const int32_t* d_feasible, const int32_t* d_plan_flags,
                           double* d_cmd, int32_t* d_result, int32_t* d_reset_next, double* d_u_prev_next, int32_t* d_infeasible_count) {
    g_err[0] = 0;
    if (!s || !d_u || !d_status || !d_cmd || !d_result) { set_err("mpc_commands_batch: null argument (u_out, status, cmd, result)"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_commands_batch")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const mpc::CommandsArgs a = {d_u, u_stride, B, d_status, d_feasible, d_plan_flags, d_cmd, d_result, d_reset_next, d_u_prev_next, d_infeasible_count};
    hipLaunchKernelGGL(mpc::commands_kernel, dim3((B + 63) / 64), dim3(64), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

extern "C" {

int mpc_commands_batch_device(mpc_solver* s, int32_t B, const double* d_u_out, const int32_t* d_status, const int32_t* d_feasible, const int32_t* d_plan_flags,
                              double* d_cmd, int32_t* d_result, int32_t* d_reset_next, double* d_u_prev_next, int32_t* d_infeasible_count) {
    return commands_device(s, B, d_u_out, s ? s->cfg.n : 0, d_status, d_feasible, d_plan_flags, d_cmd, d_result, d_reset_next, d_u_prev_next, d_infeasible_count);
}

}  // extern "C"

extern "C" {

int mpc_plan_inputs_batch(mpc_solver* s, int32_t B, const mpc_plan_params* p, const double* global_plan, const int32_t* n_global, int32_t gstride,
                          const double* robot_pose, int32_t* plan_begin, double* plan, int32_t* n_plan, int32_t plan_stride,
                          int32_t* n_via, double* via, int32_t* goal_idx, int32_t* flags) {
    g_err[0] = 0;
    if (const char* e = plan_inputs_error(s, p, global_plan, n_global, gstride, robot_pose, plan, n_plan, plan_stride, n_via, via)) { set_err(e); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_plan_inputs_batch")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, mv = s->cfg.max_via_points > 0 ? (size_t)s->cfg.max_via_points : 0;
    // in / out: the front the caller keeps, and the arrays whose rows behind n_plan[b] and n_via[b] the kernel leaves alone
    const mpc::StagePiece pc[10] = {stage_in(global_plan, nb * (size_t)gstride * 24), stage_in(n_global, nb * 4), stage_in(robot_pose, nb * 24), stage_inout(plan_begin, nb * 4),
                                    stage_inout(plan, nb * (size_t)plan_stride * 24), stage_out(n_plan, nb * 4), stage_out(n_via, nb * 4), stage_inout(via, nb * mv * 24), stage_out(goal_idx, nb * 4), stage_out(flags, nb * 4)};
    return staged_call(s, "mpc_plan_inputs_batch", false, false, pc, 10, [&](void** d) {
        return mpc_plan_inputs_batch_device(s, B, p, (const double*)d[0], (const int32_t*)d[1], gstride, (const double*)d[2], (int32_t*)d[3], (double*)d[4], (int32_t*)d[5],
                                            plan_stride, (int32_t*)d[6], (double*)d[7], (int32_t*)d[8], (int32_t*)d[9]);
    });
}

int mpc_commands_batch(mpc_solver* s, int32_t B, const double* u_out, const int32_t* status, const int32_t* feasible, const int32_t* plan_flags,
                       double* cmd, int32_t* result, int32_t* reset_next, double* u_prev_next, int32_t* infeasible_count) {
    g_err[0] = 0;
    if (!s || !u_out || !status || !cmd || !result) { set_err("mpc_commands_batch: null argument (u_out, status, cmd, result)"); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_commands_batch")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B;
    std::vector<double> u0(2 * nb);      // only the first control of every instance travels
    for (size_t b = 0; b < nb; ++b) { u0[2 * b] = u_out[b * (size_t)s->cfg.n * 2]; u0[2 * b + 1] = u_out[b * (size_t)s->cfg.n * 2 + 1]; }
    const mpc::StagePiece pc[9] = {stage_in(u0.data(), nb * 16), stage_in(status, nb * 4), stage_in(feasible, nb * 4), stage_in(plan_flags, nb * 4), stage_out(cmd, nb * 24), stage_out(result, nb * 4),
                                   stage_out(reset_next, nb * 4), stage_out(u_prev_next, nb * 16), stage_inout(infeasible_count, nb * 4)};      // (the count stays as it is at a goal reached or an empty plan)
    return staged_call(s, "mpc_commands_batch", false, false, pc, 9, [&](void** d) {
        return commands_device(s, B, (const double*)d[0], 1, (const int32_t*)d[1], (const int32_t*)d[2], (const int32_t*)d[3], (double*)d[4], (int32_t*)d[5],
                               (int32_t*)d[6], (double*)d[7], (int32_t*)d[8]);
    });
}

}  // extern "C"

// ---- obstacles from a pool, and a pool from the fleet (mpc_fleet_obstacles.hpp; declared in include/mpc_fleet.h)

// the argument checks both variants of mpc_obstacles_from_pool share: NULL when the call is fine
static const char* from_pool_error(const mpc_solver* s, const mpc_pool* pool, const void* robot_pose, const mpc_pool_params* p, const void* n_obstacles, const void* n_vertices,
                                   const void* vertices, const void* radius, const void* velocity) {
    if (!s || !pool || !robot_pose || !p || !n_obstacles || !n_vertices || !vertices) return "mpc_obstacles_from_pool: null argument (pool, robot_pose, params, n_obstacles, n_vertices, vertices)";
    if (s->cfg.max_obstacles <= 0) return "mpc_obstacles_from_pool: the solver was created with max_obstacles = 0";
    if (pool->P < 0) return "mpc_obstacles_from_pool: P is negative";
    if (pool->P > 0 && (!pool->n_vertices || !pool->vertices)) return "mpc_obstacles_from_pool: null pool array (n_vertices, vertices)";
    if (!(p->reach >= 0.0) || p->reach - p->reach != 0.0) return "mpc_obstacles_from_pool: reach has to be finite and not negative";
    if ((pool->radius && !radius) || (pool->velocity && !velocity)) return "mpc_obstacles_from_pool: the pool carries a radius / velocity and the container has no array for it";
    return nullptr;
}
static const char* fleet_pool_error(const mpc_solver* s, const void* robot_pose, const void* x, const void* dt, int32_t pool_offset, const void* pool_n_vertices, const void* pool_vertices) {
    if (!s || !robot_pose || !pool_n_vertices || !pool_vertices) return "mpc_fleet_pool: null argument (robot_pose, pool_n_vertices, pool_vertices)";
    if (x && !dt) return "mpc_fleet_pool: x without dt";
    if (pool_offset < 0) return "mpc_fleet_pool: pool_offset is negative";
    return nullptr;
}

// x_stride: rows between two robots' first states (cfg.n for x_out itself; 2 for the host variant's compact copy of the first two rows)
static int fleet_pool_device(mpc_solver* s, int32_t B, const double* d_robot_pose, const double* d_x, int32_t x_stride, const double* d_dt, const int32_t* d_status, double robot_radius,
                             const double* d_robot_radius, int32_t pool_offset, int32_t* d_pool_n_vertices, double* d_pool_vertices, double* d_pool_radius, double* d_pool_velocity) {
    g_err[0] = 0;
    if (const char* e = fleet_pool_error(s, d_robot_pose, d_x, d_dt, pool_offset, d_pool_n_vertices, d_pool_vertices)) { set_err(e); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_fleet_pool")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::FleetPoolArgs a;
    a.B = B; a.n_stride = x_stride; a.V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1; a.pool_offset = pool_offset;
    a.pose = d_robot_pose; a.x = d_x; a.dt = d_dt; a.status = d_status; a.robot_radius = robot_radius; a.radius = d_robot_radius;
    a.pool_n_vertices = d_pool_n_vertices; a.pool_vertices = d_pool_vertices; a.pool_radius = d_pool_radius; a.pool_velocity = d_pool_velocity;
    hipLaunchKernelGGL(mpc::fleet_pool_kernel, dim3((B + 63) / 64), dim3(64), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

extern "C" {

void mpc_pool_params_defaults(const mpc_solver* s, mpc_pool_params* p) {
    if (!p) return;
    p->reach = s ? s->cfg.cutoff_dist : 0.0;
    p->min_speed = 0.001;      // believed: teb_local_planner's Obstacle::setCentroidVelocity (mpc_fleet_obstacles.hpp)
    p->append = 1;
}

int mpc_obstacles_from_pool_device(mpc_solver* s, int32_t B, const mpc_pool* pool, const double* d_robot_pose, const int32_t* d_self_index, const mpc_pool_params* params,
                                   int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices, double* d_radius, double* d_velocity, int32_t* d_dropped, int32_t* d_n_taken) {
    g_err[0] = 0;
    if (const char* e = from_pool_error(s, pool, d_robot_pose, params, d_n_obstacles, d_n_vertices, d_vertices, d_radius, d_velocity)) { set_err(e); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_obstacles_from_pool")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::FleetSelectArgs a;
    a.pool = {pool->P, pool->n_vertices, pool->vertices, pool->radius, pool->velocity};
    a.prm = {params->reach, params->min_speed, params->append};
    a.pose = d_robot_pose; a.self_index = d_self_index;
    a.O = s->cfg.max_obstacles; a.V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1;
    a.n_obstacles = d_n_obstacles; a.n_vertices = d_n_vertices; a.vertices = d_vertices; a.radius = d_radius; a.velocity = d_velocity;
    a.dropped = d_dropped; a.n_taken = d_n_taken;
    hipLaunchKernelGGL(mpc::fleet_select_kernel, dim3(B), dim3(mpc::kFleetThreads), 0, s->stream, a);
    HIP_TRY(hipGetLastError());
    return MPC_OK;
}

int mpc_obstacles_from_pool(mpc_solver* s, int32_t B, const mpc_pool* pool, const double* robot_pose, const int32_t* self_index, const mpc_pool_params* params,
                            int32_t* n_obstacles, int32_t* n_vertices, double* vertices, double* radius, double* velocity, int32_t* dropped, int32_t* n_taken) {
    g_err[0] = 0;
    if (const char* e = from_pool_error(s, pool, robot_pose, params, n_obstacles, n_vertices, vertices, radius, velocity)) { set_err(e); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_obstacles_from_pool")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, O = s->cfg.max_obstacles, V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1, np = (size_t)pool->P;
    // in / out: the container, whose slots below the old and at or above the new n_obstacles[b] the kernel leaves alone
    const mpc::StagePiece pc[13] = {stage_in(pool->n_vertices, np * 4), stage_in(pool->vertices, np * V * 16), stage_in(pool->radius, np * 8), stage_in(pool->velocity, np * 16),
                                    stage_in(robot_pose, nb * 24), stage_in(self_index, nb * 4), stage_inout(n_obstacles, nb * 4), stage_inout(n_vertices, nb * O * 4),
                                    stage_inout(vertices, nb * O * V * 16), stage_inout(radius, nb * O * 8), stage_inout(velocity, nb * O * 16), stage_out(dropped, nb * 4), stage_out(n_taken, nb * 4)};
    return staged_call(s, "mpc_obstacles_from_pool", false, false, pc, 13, [&](void** d) {
        const mpc_pool dp = {pool->P, (const int32_t*)d[0], (const double*)d[1], (const double*)d[2], (const double*)d[3]};
        return mpc_obstacles_from_pool_device(s, B, &dp, (const double*)d[4], (const int32_t*)d[5], params, (int32_t*)d[6], (int32_t*)d[7], (double*)d[8], (double*)d[9], (double*)d[10],
                                              (int32_t*)d[11], (int32_t*)d[12]);
    });
}

int mpc_fleet_pool_device(mpc_solver* s, int32_t B, const double* d_robot_pose, const double* d_x, const double* d_dt, const int32_t* d_status, double robot_radius,
                          const double* d_robot_radius, int32_t pool_offset, int32_t* d_pool_n_vertices, double* d_pool_vertices, double* d_pool_radius, double* d_pool_velocity) {
    return fleet_pool_device(s, B, d_robot_pose, d_x, s ? s->cfg.n : 0, d_dt, d_status, robot_radius, d_robot_radius, pool_offset, d_pool_n_vertices, d_pool_vertices, d_pool_radius, d_pool_velocity);
}

int mpc_fleet_pool(mpc_solver* s, int32_t B, const double* robot_pose, const double* x, const double* dt, const int32_t* status, double robot_radius,
                   const double* robot_radius_per_robot, int32_t pool_offset, int32_t* pool_n_vertices, double* pool_vertices, double* pool_radius, double* pool_velocity) {
    g_err[0] = 0;
    if (const char* e = fleet_pool_error(s, robot_pose, x, dt, pool_offset, pool_n_vertices, pool_vertices)) { set_err(e); return MPC_EINVAL; }
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_fleet_pool")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, n = (size_t)s->cfg.n, V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1, off = (size_t)pool_offset;
    std::vector<double> x01;      // only the first two states of every robot travel
    if (x) { x01.resize(6 * nb); for (size_t b = 0; b < nb; ++b) memcpy(&x01[6 * b], x + b * n * 3, 48); }
    // the B entries behind pool_offset alone; in / out: the vertices behind the first of an entry stay
    const mpc::StagePiece pc[9] = {stage_in(robot_pose, nb * 24), stage_in(x ? x01.data() : nullptr, nb * 48), stage_in(dt, nb * 8), stage_in(status, nb * 4), stage_in(robot_radius_per_robot, nb * 8),
                                   stage_out(pool_n_vertices + off, nb * 4), stage_inout(pool_vertices + off * V * 2, nb * V * 16), stage_out(pool_radius ? pool_radius + off : nullptr, nb * 8),
                                   stage_out(pool_velocity ? pool_velocity + 2 * off : nullptr, nb * 16)};
    return staged_call(s, "mpc_fleet_pool", false, false, pc, 9, [&](void** d) {
        return fleet_pool_device(s, B, (const double*)d[0], (const double*)d[1], 2, (const double*)d[2], (const int32_t*)d[3], robot_radius, (const double*)d[4], 0, (int32_t*)d[5], (double*)d[6],
                                 (double*)d[7], (double*)d[8]);
    });
}

}  // extern "C"

// ---- costmap -> clustered obstacles and costmap -> line segments (mpc_costmap_clusters.hpp, mpc_costmap_lines.hpp; declared in include/mpc_costmap_clusters.h and
// include/mpc_costmap_lines.h): two steps with one entry path

static bool costmap_no(const char* who, const char* why) {
    if (why) snprintf(g_err, sizeof(g_err), "%s: %s", who, why);
    return why != nullptr;
}

// the argument checks both steps and both variants of each share, in the order in which they win: true with mpc_last_error set when the call is refused.
// max_side: the per-axis limit of the line step
static bool costmap_shapes_error(const char* who, const mpc_solver* s, const void* cost, int32_t size_x, int32_t size_y, double resolution, const void* origin, const void* robot_pose,
                                 const void* params, const void* n_obstacles, const void* n_vertices, const void* vertices, int32_t max_side, int32_t link_dist_sq) {
    if (!s || !cost || !origin || !robot_pose || !params || !n_obstacles || !n_vertices || !vertices)
        return costmap_no(who, "null argument (cost, origin, robot_pose, params, n_obstacles, n_vertices, vertices)");
    if (s->cfg.max_obstacles <= 0) return costmap_no(who, "the solver was created with max_obstacles = 0");
    if (s->cfg.max_vertices < 4) return costmap_no(who, "the solver was created with max_vertices < 4 (a bounding box has four)");
    if (size_x < 1 || size_y < 1 || size_x > max_side || size_y > max_side || (long long)size_x * size_y > mpc::kCcMaxCells || !(resolution > 0))
        return costmap_no(who, max_side < mpc::kCcMaxCells ? "bad costmap geometry (size_x, size_y <= 4096, size_x * size_y <= 2^20)" : "bad costmap geometry (size_x * size_y <= 2^20)");
    return costmap_no(who, link_dist_sq < 1 || link_dist_sq > mpc::kCcMaxLink ? "link_dist_sq has to be in [1, 64]" : nullptr);
}
static bool to_polygons_error(const mpc_solver* s, const void* cost, int32_t size_x, int32_t size_y, double resolution, const void* origin, const void* robot_pose,
                              const mpc_cluster_params* p, const void* n_obstacles, const void* n_vertices, const void* vertices) {
    return costmap_shapes_error("mpc_costmap_to_polygons", s, cost, size_x, size_y, resolution, origin, robot_pose, p, n_obstacles, n_vertices, vertices, mpc::kCcMaxCells, p ? p->link_dist_sq : 0);
}
static bool to_lines_error(const mpc_solver* s, const void* cost, int32_t size_x, int32_t size_y, double resolution, const void* origin, const void* robot_pose,
                           const mpc_line_params* p, const void* n_obstacles, const void* n_vertices, const void* vertices) {
    const char* who = "mpc_costmap_to_lines";
    if (costmap_shapes_error(who, s, cost, size_x, size_y, resolution, origin, robot_pose, p, n_obstacles, n_vertices, vertices, mpc::kClMaxSize, p ? p->link_dist_sq : 0)) return true;
    if (p->inlier_dist_sq < 0 || p->inlier_dist_sq > mpc::kClMaxInlier) return costmap_no(who, "inlier_dist_sq has to be in [0, 64]");
    if (p->min_inliers < 2) return costmap_no(who, "min_inliers has to be at least 2");
    if (p->n_hypotheses < 1 || p->n_hypotheses > mpc::kClMaxHypotheses) return costmap_no(who, "n_hypotheses has to be in [1, 65536]");
    return costmap_no(who, p->remaining_outliers < 0 ? "remaining_outliers has to be at least 0" : nullptr);
}

// What a checked device call of either step does before its launch: the batch refusal, the scratch (BUF_CLUSTER_LAB) grown to bytes_per_cell per cell of the batch
// -- 4: the labels; 8: behind them the list of a cluster that does not fit the line kernel's LDS list --, and the launch's description of the batch.
static int costmap_shapes_batch(mpc_solver* s, const char* who, int32_t B, size_t bytes_per_cell, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution,
                                const double* d_origin, const double* d_robot_pose, int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices, double* d_radius,
                                double* d_velocity, int32_t* d_dropped, int32_t* d_info, mpc::CcBatch& a) {
    if (const int rc = refused(s, B, REF_MAX_BATCH, who)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t need = (size_t)B * size_x * size_y * bytes_per_cell;
    Buf& lab = s->bufs[BUF_CLUSTER_LAB];
    if (need > lab.bytes) {      // a launch that still reads the old block may be in flight
        HIP_TRY(hipStreamSynchronize(s->stream));
        const hipError_t e = buf_alloc(lab, need);
        if (e != hipSuccess) { snprintf(g_err, sizeof(g_err), "%s: scratch: %s", who, hipGetErrorString(e)); return e == hipErrorOutOfMemory ? MPC_ENOMEM : MPC_EHIP; }
    }
    a = {d_cost, d_origin, d_robot_pose, size_x, size_y, resolution, s->cfg.max_obstacles, s->cfg.max_vertices, s->d_cluster_lab,
         d_n_obstacles, d_n_vertices, d_vertices, d_radius, d_velocity, d_dropped, d_info};
    return MPC_OK;
}

// The host-pointer variant of either step: the pieces through the staging pair, the container's arrays cleared on the device, device_entry on the device addresses.
template <typename Params, typename Entry>
static int costmap_shapes_host(mpc_solver* s, const char* who, int32_t B, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution, const double* origin,
                               const double* robot_pose, const Params* params, int32_t* n_obstacles, int32_t* n_vertices, double* vertices, double* radius, double* velocity,
                               int32_t* dropped, int32_t* info, Entry device_entry) {
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, who)) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, O = s->cfg.max_obstacles, V = s->cfg.max_vertices;
    const mpc::StagePiece pc[10] = {stage_in(cost, nb * size_x * size_y), stage_in(origin, nb * 16), stage_in(robot_pose, nb * 24), stage_out(n_obstacles, nb * 4),
                                    stage_out(n_vertices, nb * O * 4), stage_out(vertices, nb * O * V * 16), stage_out(radius, nb * O * 8), stage_out(velocity, nb * O * 16),
                                    stage_out(dropped, nb * 4), stage_out(info, nb * 16)};
    return staged_call(s, who, true, true, pc, 10, [&](void** d) -> int {
        // the kernel writes the slots it fills: the rest is cleared on the device, behind the copy of the inputs
        for (int i = 4; i <= 7; ++i) if (d[i]) HIP_TRY(hipMemsetAsync(d[i], 0, pc[i].bytes, s->stream));
        return device_entry(s, B, (const uint8_t*)d[0], size_x, size_y, resolution, (const double*)d[1], (const double*)d[2], params, (int32_t*)d[3], (int32_t*)d[4], (double*)d[5],
                            (double*)d[6], (double*)d[7], (int32_t*)d[8], (int32_t*)d[9]);
    });
}

extern "C" {

void mpc_cluster_params_defaults(mpc_cluster_params* p, double resolution, double cluster_max_distance) {
    if (!p) return;
    p->behind_robot_dist = 1.5;
    const double q = cluster_max_distance / resolution, sq = floor(q * q + 1e-9);
    p->link_dist_sq = sq >= 64.0 ? 64 : sq >= 1.0 ? (int32_t)sq : 1;      // (not a number: 1)
}

int mpc_costmap_to_polygons_device(mpc_solver* s, int32_t B, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution, const double* d_origin,
                                   const double* d_robot_pose, const mpc_cluster_params* params, int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices,
                                   double* d_radius, double* d_velocity, int32_t* d_dropped, int32_t* d_info) {
    g_err[0] = 0;
    if (to_polygons_error(s, d_cost, size_x, size_y, resolution, d_origin, d_robot_pose, params, d_n_obstacles, d_n_vertices, d_vertices)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    mpc::ClusterArgs a;
    if (const int rc = costmap_shapes_batch(s, "mpc_costmap_to_polygons", B, 4, d_cost, size_x, size_y, resolution, d_origin, d_robot_pose, d_n_obstacles, d_n_vertices, d_vertices,
                                            d_radius, d_velocity, d_dropped, d_info, a)) return rc;
    a.prm = {params->behind_robot_dist, params->link_dist_sq};
    return costmap_timed_launch(s, mpc::costmap_clusters_kernel, B, mpc::kCcThreads, a);
}

int mpc_costmap_to_polygons(mpc_solver* s, int32_t B, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution, const double* origin,
                            const double* robot_pose, const mpc_cluster_params* params, int32_t* n_obstacles, int32_t* n_vertices, double* vertices,
                            double* radius, double* velocity, int32_t* dropped, int32_t* info) {
    g_err[0] = 0;
    if (to_polygons_error(s, cost, size_x, size_y, resolution, origin, robot_pose, params, n_obstacles, n_vertices, vertices)) return MPC_EINVAL;
    return costmap_shapes_host(s, "mpc_costmap_to_polygons", B, cost, size_x, size_y, resolution, origin, robot_pose, params, n_obstacles, n_vertices, vertices, radius, velocity,
                               dropped, info, mpc_costmap_to_polygons_device);
}

int mpc_last_costmap_ms(mpc_solver* s, float* ms) {
    if (!s || !ms) return MPC_EINVAL;
    if (!s->ctimed) { *ms = 0.f; return MPC_OK; }
    HIP_TRY(hipEventSynchronize(s->cev1));
    HIP_TRY(hipEventElapsedTime(ms, s->cev0, s->cev1));
    return MPC_OK;
}

void mpc_line_params_defaults(mpc_line_params* p, double resolution, double cluster_max_distance, double ransac_inlier_distance) {
    if (!p) return;
    mpc_cluster_params cp;
    mpc_cluster_params_defaults(&cp, resolution, cluster_max_distance);
    p->behind_robot_dist = cp.behind_robot_dist;
    p->link_dist_sq = cp.link_dist_sq;
    const double q = ransac_inlier_distance / resolution, sq = floor(q * q + 1e-9);
    p->inlier_dist_sq = sq >= 64.0 ? 64 : sq >= 0.0 ? (int32_t)sq : 0;      // (not a number: 0)
    p->min_inliers = 10;
    p->n_hypotheses = 1500;
    p->remaining_outliers = 3;
}

int mpc_costmap_to_lines_device(mpc_solver* s, int32_t B, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution, const double* d_origin,
                                const double* d_robot_pose, const mpc_line_params* params, int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices,
                                double* d_radius, double* d_velocity, int32_t* d_dropped, int32_t* d_info) {
    g_err[0] = 0;
    if (to_lines_error(s, d_cost, size_x, size_y, resolution, d_origin, d_robot_pose, params, d_n_obstacles, d_n_vertices, d_vertices)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    mpc::LineArgs a;
    if (const int rc = costmap_shapes_batch(s, "mpc_costmap_to_lines", B, 8, d_cost, size_x, size_y, resolution, d_origin, d_robot_pose, d_n_obstacles, d_n_vertices, d_vertices,
                                            d_radius, d_velocity, d_dropped, d_info, a)) return rc;
    a.prm = {params->behind_robot_dist, params->link_dist_sq, params->inlier_dist_sq, params->min_inliers, params->n_hypotheses, params->remaining_outliers};
    a.list = reinterpret_cast<uint32_t*>(s->d_cluster_lab + (size_t)B * size_x * size_y);      // behind the labels
    return costmap_timed_launch(s, mpc::costmap_lines_kernel, B, mpc::kCcThreads, a);
}

int mpc_costmap_to_lines(mpc_solver* s, int32_t B, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution, const double* origin,
                         const double* robot_pose, const mpc_line_params* params, int32_t* n_obstacles, int32_t* n_vertices, double* vertices,
                         double* radius, double* velocity, int32_t* dropped, int32_t* info) {
    g_err[0] = 0;
    if (to_lines_error(s, cost, size_x, size_y, resolution, origin, robot_pose, params, n_obstacles, n_vertices, vertices)) return MPC_EINVAL;
    return costmap_shapes_host(s, "mpc_costmap_to_lines", B, cost, size_x, size_y, resolution, origin, robot_pose, params, n_obstacles, n_vertices, vertices, radius, velocity,
                               dropped, info, mpc_costmap_to_lines_device);
}

}  // extern "C"

// ---- one shared map -> the local costmap windows of a batch (mpc_costmap_window.hpp; declared in include/mpc_costmap_window.h)

// the argument checks of both variants, in the order of rule 6: true with mpc_last_error set when the call is refused; r: rule 3's radius in cells
static bool window_error(const char* who, const mpc_solver* s, const void* map, const mpc_window_params* p, const void* robot_pose, int32_t size_x, int32_t size_y,
                         double resolution, const void* cost, const void* origin, int& r) {
    auto pos_finite = [](double v) { return v > 0.0 && std::isfinite(v); };
    auto nonneg_finite = [](double v) { return v >= 0.0 && std::isfinite(v); };
    if (!s || !map || !p || !robot_pose || !cost || !origin) return costmap_no(who, "null argument (map, params, robot_pose, cost, origin)");
    if (size_x < 1 || size_y < 1 || size_x > mpc::kCwMaxSize || size_y > mpc::kCwMaxSize || (long long)size_x * size_y > mpc::kCwMaxCells)
        return costmap_no(who, "bad window geometry (1 <= size_x, size_y <= 4096, size_x * size_y <= 2^20)");
    if (!pos_finite(resolution) || !pos_finite(p->map_resolution)) return costmap_no(who, "resolution and map_resolution have to be positive and finite");
    if (p->map_size_x < 1 || p->map_size_y < 1 || (long long)p->map_size_x * p->map_size_y > 2147483647LL) return costmap_no(who, "bad map size (at least 1 x 1, at most 2^31 - 1 bytes)");
    r = mpc::cw_cell_radius(p->inflation_radius, resolution);
    if (r < 0) return costmap_no(who, "inflation_radius has to be at most 32 cells of the window");
    if (p->outside_value != 0 && p->outside_value != 255) return costmap_no(who, "outside_value has to be 0 or 255");
    if (!nonneg_finite(p->inscribed_radius)) return costmap_no(who, "inscribed_radius has to be at least 0 and finite");
    return costmap_no(who, nonneg_finite(p->cost_scaling_factor) ? nullptr : "cost_scaling_factor has to be at least 0 and finite");
}

extern "C" {

void mpc_window_params_defaults(mpc_window_params* p, double map_resolution, int32_t map_size_x, int32_t map_size_y) {
    if (!p) return;
    p->map_origin[0] = p->map_origin[1] = 0.0;
    p->map_resolution = map_resolution;
    p->lattice_anchor[0] = p->lattice_anchor[1] = 0.0;
    p->inscribed_radius = 0.0;
    p->inflation_radius = 0.0;
    p->cost_scaling_factor = 10.0;
    p->map_size_x = map_size_x; p->map_size_y = map_size_y;
    p->outside_value = 0;
    p->inflate_unknown = 0;
}

int mpc_costmap_window_device(mpc_solver* s, int32_t B, const uint8_t* d_map, const mpc_window_params* params, const double* d_robot_pose, int32_t size_x,
                              int32_t size_y, double resolution, uint8_t* d_cost, double* d_origin, int32_t* d_info) {
    g_err[0] = 0;
    int r = 0;
    if (window_error("mpc_costmap_window", s, d_map, params, d_robot_pose, size_x, size_y, resolution, d_cost, d_origin, r)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_costmap_window")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::WindowArgs a;
    memset(&a, 0, sizeof(a));
    a.map = d_map; a.pose = d_robot_pose; a.cost = d_cost; a.origin = d_origin; a.info = d_info;
    a.p = {params->map_origin[0], params->map_origin[1], params->map_resolution, params->lattice_anchor[0], params->lattice_anchor[1], resolution,
           params->map_size_x, params->map_size_y, params->outside_value, params->inflate_unknown ? 1 : 0, r};
    a.W = size_x; a.H = size_y;
    a.tiles_x = (size_x + mpc::kCwTileX - 1) / mpc::kCwTileX;
    a.ntiles = a.tiles_x * ((size_y + mpc::kCwTileY - 1) / mpc::kCwTileY);
    uint8_t table[4 * mpc::kCwTableWords] = {0};      // rule 4: on the host
    mpc::cw_table(resolution, params->inscribed_radius, params->cost_scaling_factor, r, table);
    memcpy(a.table, table, sizeof(a.table));
    // between the two events mpc_last_costmap_ms reads: the counts cleared (the tiles of an instance add to them), then the tiles, at most 2^22 workgroups a launch
    HIP_TRY(hipEventRecord(s->cev0, s->stream));
    if (d_info) HIP_TRY(hipMemsetAsync(d_info, 0, (size_t)B * 16, s->stream));
    const int per = (1 << 22) / a.ntiles;      // ntiles <= 2^20 / 64 + 2 * 64 + 1
    for (int b0 = 0; b0 < B; b0 += per) {
        a.b0 = b0;
        const int nb = B - b0 < per ? B - b0 : per;
        hipLaunchKernelGGL(mpc::costmap_window_kernel, dim3((unsigned)nb * (unsigned)a.ntiles), dim3(mpc::kCwThreads), 0, s->stream, a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->cev1, s->stream));
    s->ctimed = true;
    return MPC_OK;
}

int mpc_costmap_window(mpc_solver* s, int32_t B, const uint8_t* map, const mpc_window_params* params, const double* robot_pose, int32_t size_x, int32_t size_y,
                       double resolution, uint8_t* cost, double* origin, int32_t* info) {
    g_err[0] = 0;
    int r = 0;
    if (window_error("mpc_costmap_window", s, map, params, robot_pose, size_x, size_y, resolution, cost, origin, r)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_costmap_window")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B;
    const mpc::StagePiece pc[5] = {stage_in(map, (size_t)params->map_size_x * params->map_size_y), stage_in(robot_pose, nb * 24), stage_out(cost, nb * size_x * size_y),
                                   stage_out(origin, nb * 16), stage_out(info, nb * 16)};
    return staged_call(s, "mpc_costmap_window", true, true, pc, 5, [&](void** d) -> int {
        return mpc_costmap_window_device(s, B, (const uint8_t*)d[0], params, (const double*)d[1], size_x, size_y, resolution, (uint8_t*)d[2], (double*)d[3], (int32_t*)d[4]);
    });
}

}  // extern "C"

// ---- the laser-scan obstacle layer of a batch (mpc_costmap_scans.hpp; declared in include/mpc_costmap_scans.h)

// the argument checks of both variants, in the order of rule 8: true with mpc_last_error set when the call is refused; R: rule 4's longest ray in cells
static bool scans_error(const char* who, const mpc_solver* s, const mpc_scan_params* p, const void* robot_pose, const void* ranges, int32_t n_beams, int32_t size_x,
                        int32_t size_y, double resolution, const void* layer, const void* layer_cell, int& R) {
    auto nonneg_finite = [](double v) { return v >= 0.0 && std::isfinite(v); };
    if (!s || !p || !robot_pose || !ranges || !layer || !layer_cell) return costmap_no(who, "null argument (params, robot_pose, ranges, layer, layer_cell)");
    if (n_beams < 1 || n_beams > mpc::kCsMaxBeams) return costmap_no(who, "n_beams has to be in [1, 4096]");
    if (size_x < 1 || size_y < 1 || (long long)size_x * size_y > mpc::kCsMaxCells) return costmap_no(who, "bad layer geometry (1 <= size_x, size_y; size_x * size_y <= 65536)");
    if (!(resolution > 0.0) || !std::isfinite(resolution)) return costmap_no(who, "resolution has to be positive and finite");
    if (!nonneg_finite(p->range_min) || !nonneg_finite(p->range_max) || !nonneg_finite(p->obstacle_range) || !nonneg_finite(p->raytrace_range))
        return costmap_no(who, "range_min, range_max, obstacle_range and raytrace_range have to be at least 0 and finite");
    R = mpc::cs_ray_cells(p->raytrace_range, resolution);
    if (R < 0) return costmap_no(who, "raytrace_range has to be at most 4096 cells");
    if (!(p->range_max / resolution < mpc::kCsMaxRangeCells)) return costmap_no(who, "range_max has to be below 2^15 cells");
    if (!std::isfinite(p->angle_min) || !std::isfinite(p->angle_increment) || !std::isfinite(p->sensor_pose[0]) || !std::isfinite(p->sensor_pose[1]) || !std::isfinite(p->sensor_pose[2]))
        return costmap_no(who, "angle_min, angle_increment and sensor_pose have to be finite");
    if (std::isnan(p->footprint_clear_radius)) return costmap_no(who, "footprint_clear_radius is not a number");
    return costmap_no(who, p->combination_method == 0 || p->combination_method == 1 ? nullptr : "combination_method has to be 0 or 1");
}

extern "C" {

void mpc_scan_params_defaults(mpc_scan_params* p) {
    if (!p) return;
    p->lattice_anchor[0] = p->lattice_anchor[1] = 0.0;
    p->sensor_pose[0] = p->sensor_pose[1] = p->sensor_pose[2] = 0.0;
    p->angle_min = -3.14159265358979323846;
    p->angle_increment = 2.0 * 3.14159265358979323846 / 360.0;
    p->range_min = 0.0; p->range_max = 30.0;
    p->obstacle_range = 2.5; p->raytrace_range = 3.0;
    p->footprint_clear_radius = 0.0;
    p->marking = p->clearing = 1;
    p->inf_is_valid = 0;
    p->track_unknown = 0;
    p->combination_method = 1;
}

int mpc_costmap_scans_device(mpc_solver* s, int32_t B, const mpc_scan_params* params, const double* d_robot_pose, const float* d_ranges, int32_t n_beams,
                             const int32_t* d_keep, int32_t size_x, int32_t size_y, double resolution, uint8_t* d_layer, int32_t* d_layer_cell, uint8_t* d_cost,
                             int32_t* d_info) {
    g_err[0] = 0;
    int R = 0;
    if (scans_error("mpc_costmap_scans", s, params, d_robot_pose, d_ranges, n_beams, size_x, size_y, resolution, d_layer, d_layer_cell, R)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_costmap_scans")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.pose = d_robot_pose; a.ranges = d_ranges; a.keep = d_keep; a.layer = d_layer; a.layer_cell = d_layer_cell; a.cost = d_cost; a.info = d_info;
    a.p = {params->lattice_anchor[0], params->lattice_anchor[1], resolution, params->sensor_pose[0], params->sensor_pose[1], params->sensor_pose[2], params->angle_min,
           params->angle_increment, params->range_min, params->range_max, params->obstacle_range, params->footprint_clear_radius, params->marking ? 1 : 0,
           params->clearing ? 1 : 0, params->inf_is_valid ? 1 : 0, params->combination_method, R, params->track_unknown ? 255 : 0};
    a.W = size_x; a.H = size_y; a.n_beams = n_beams;
    const size_t lds = mpc::cs_lds_bytes(size_x, size_y);      // the layer of an instance, at most 64 KB, and the counts
    if (lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mpc::costmap_scans_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipEventRecord(s->cev0, s->stream));
    hipLaunchKernelGGL(mpc::costmap_scans_kernel, dim3((unsigned)B), dim3(mpc::kCsThreads), lds, s->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->cev1, s->stream));
    s->ctimed = true;
    return MPC_OK;
}

int mpc_costmap_scans(mpc_solver* s, int32_t B, const mpc_scan_params* params, const double* robot_pose, const float* ranges, int32_t n_beams, const int32_t* keep,
                      int32_t size_x, int32_t size_y, double resolution, uint8_t* layer, int32_t* layer_cell, uint8_t* cost, int32_t* info) {
    g_err[0] = 0;
    int R = 0;
    if (scans_error("mpc_costmap_scans", s, params, robot_pose, ranges, n_beams, size_x, size_y, resolution, layer, layer_cell, R)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_costmap_scans")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, cells = (size_t)size_x * size_y;
    // in / out: the layer and its cell are the state the call rolls; the window is combined in place
    const mpc::StagePiece pc[7] = {stage_in(robot_pose, nb * 24), stage_in(ranges, nb * (size_t)n_beams * 4), stage_in(keep, nb * 4), stage_inout(layer, nb * cells),
                                   stage_inout(layer_cell, nb * 8), stage_inout(cost, nb * cells), stage_out(info, nb * 16)};
    return staged_call(s, "mpc_costmap_scans", true, true, pc, 7, [&](void** d) -> int {
        return mpc_costmap_scans_device(s, B, params, (const double*)d[0], (const float*)d[1], n_beams, (const int32_t*)d[2], size_x, size_y, resolution, (uint8_t*)d[3],
                                        (int32_t*)d[4], (uint8_t*)d[5], (int32_t*)d[6]);
    });
}

}  // extern "C"

// ---- the laser scans of a batch, cast through the shared map and the pool (mpc_scan_cast.hpp; declared in include/mpc_scan_cast.h)

// the argument checks of both variants, in the order of rule 6: true with mpc_last_error set when the call is refused; Rc: rule 5's reach in cells
static bool cast_error(const char* who, const mpc_solver* s, const void* map, const mpc_cast_params* p, const void* robot_pose, const mpc_pool* pool, int32_t n_beams,
                       const void* ranges, int& Rc) {
    auto pos_finite = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!s || !map || !p || !robot_pose || !ranges) return costmap_no(who, "null argument (map, params, robot_pose, ranges)");
    if (n_beams < 1 || n_beams > mpc::kScMaxBeams) return costmap_no(who, "n_beams has to be in [1, 4096]");
    if (p->map_size_x < 1 || p->map_size_y < 1 || (long long)p->map_size_x * p->map_size_y > 2147483647LL) return costmap_no(who, "bad map size (at least 1 x 1, at most 2^31 - 1 bytes)");
    if (!pos_finite(p->map_resolution) || !pos_finite(p->range_max)) return costmap_no(who, "map_resolution and range_max have to be positive and finite");
    if (!std::isfinite(p->map_origin[0]) || !std::isfinite(p->map_origin[1]) || !std::isfinite(p->angle_min) || !std::isfinite(p->angle_increment) ||
        !std::isfinite(p->sensor_pose[0]) || !std::isfinite(p->sensor_pose[1]) || !std::isfinite(p->sensor_pose[2]))
        return costmap_no(who, "map_origin, sensor_pose, angle_min and angle_increment have to be finite");
    Rc = mpc::sc_cells(p->range_max, p->map_resolution);
    if (Rc < 0) return costmap_no(who, "range_max has to be at most 350 cells of the map (the blocking cells around the sensor stay in the LDS of one workgroup)");
    if (p->block_threshold < 1 || p->block_threshold > 254) return costmap_no(who, "block_threshold has to be in [1, 254]");
    if (pool && pool->P < 0) return costmap_no(who, "pool: P is negative");
    return costmap_no(who, pool && pool->P > 0 && (!pool->n_vertices || !pool->vertices) ? "pool: n_vertices and vertices are needed with P > 0" : nullptr);
}

extern "C" {

void mpc_cast_params_defaults(mpc_cast_params* p, double map_resolution, int32_t map_size_x, int32_t map_size_y) {
    if (!p) return;
    p->map_origin[0] = p->map_origin[1] = 0.0;
    p->map_resolution = map_resolution;
    p->sensor_pose[0] = p->sensor_pose[1] = p->sensor_pose[2] = 0.0;
    p->angle_min = -3.14159265358979323846;
    p->angle_increment = 2.0 * 3.14159265358979323846 / 360.0;
    p->range_max = 6.5;
    p->map_size_x = map_size_x; p->map_size_y = map_size_y;
    p->block_threshold = 254;
    p->unknown_blocks = 0;
    p->hit_point = 1;
    p->miss_is_inf = 1;
}

int mpc_scan_cast_device(mpc_solver* s, int32_t B, const uint8_t* d_map, const mpc_cast_params* params, const double* d_robot_pose, const mpc_pool* pool,
                         const int32_t* d_self_index, int32_t n_beams, float* d_ranges, int32_t* d_hit, int32_t* d_info) {
    g_err[0] = 0;
    int Rc = 0;
    if (cast_error("mpc_scan_cast", s, d_map, params, d_robot_pose, pool, n_beams, d_ranges, Rc)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_scan_cast")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    mpc::CastArgs a;
    memset(&a, 0, sizeof(a));
    a.map = d_map; a.pose = d_robot_pose; a.self_index = d_self_index; a.ranges = d_ranges; a.hit = d_hit; a.info = d_info;
    if (pool && pool->P > 0) a.pool = {pool->P, pool->n_vertices, pool->vertices, pool->radius, nullptr};
    a.p = {params->map_origin[0], params->map_origin[1], params->map_resolution, params->sensor_pose[0], params->sensor_pose[1], params->sensor_pose[2], params->angle_min,
           params->angle_increment, params->range_max, params->map_size_x, params->map_size_y, params->block_threshold, params->unknown_blocks ? 1 : 0,
           params->hit_point ? 1 : 0, params->miss_is_inf ? 1 : 0, Rc};
    a.n_beams = n_beams; a.V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1;
    const size_t lds = mpc::sc_lds_bytes(Rc);      // the bitmap of the square around the sensor, the culled list and the counts: at most 64 KB
    if (lds > 48u * 1024u) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mpc::scan_cast_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(hipEventRecord(s->cev0, s->stream));
    hipLaunchKernelGGL(mpc::scan_cast_kernel, dim3((unsigned)B), dim3(mpc::kScThreads), lds, s->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->cev1, s->stream));
    s->ctimed = true;
    return MPC_OK;
}

int mpc_scan_cast(mpc_solver* s, int32_t B, const uint8_t* map, const mpc_cast_params* params, const double* robot_pose, const mpc_pool* pool, const int32_t* self_index,
                  int32_t n_beams, float* ranges, int32_t* hit, int32_t* info) {
    g_err[0] = 0;
    int Rc = 0;
    if (cast_error("mpc_scan_cast", s, map, params, robot_pose, pool, n_beams, ranges, Rc)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_scan_cast")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1, np = pool && pool->P > 0 ? (size_t)pool->P : 0;
    const mpc::StagePiece pc[9] = {stage_in(map, (size_t)params->map_size_x * params->map_size_y), stage_in(robot_pose, nb * 24), stage_in(np ? pool->n_vertices : nullptr, np * 4),
                                   stage_in(np ? pool->vertices : nullptr, np * V * 16), stage_in(np ? pool->radius : nullptr, np * 8), stage_in(self_index, nb * 4),
                                   stage_out(ranges, nb * (size_t)n_beams * 4), stage_out(hit, nb * (size_t)n_beams * 4), stage_out(info, nb * 16)};
    return staged_call(s, "mpc_scan_cast", true, true, pc, 9, [&](void** d) -> int {
        const mpc_pool dp = {(int32_t)np, (const int32_t*)d[2], (const double*)d[3], (const double*)d[4], nullptr};
        return mpc_scan_cast_device(s, B, (const uint8_t*)d[0], params, (const double*)d[1], np ? &dp : nullptr, (const int32_t*)d[5], n_beams, (float*)d[6], (int32_t*)d[7],
                                    (int32_t*)d[8]);
    });
}

}  // extern "C"

// ---- the plant step of a batch: every robot moved by its command, stalled by the map and the pool (mpc_plant.hpp; declared in include/mpc_plant.h)

// the argument checks of both variants, in the order of rule 7: true with mpc_last_error set when the call is refused; q: the parameters as the rule reads them
static bool plant_error(const char* who, const mpc_solver* s, const void* map, const mpc_plant_params* p, const void* cmd, const mpc_pool* pool, const void* pose,
                        mpc::PlantParams& q) {
    auto pos_finite = [](double v) { return v > 0.0 && std::isfinite(v); };
    if (!s || !p || !cmd || !pose) return costmap_no(who, "null argument (params, cmd, pose)");
    if (p->n_substeps < 1 || p->n_substeps > mpc::kPlMaxSubsteps) return costmap_no(who, "n_substeps has to be in [1, 64]");
    if (!pos_finite(p->interval)) return costmap_no(who, "interval has to be positive and finite");
    if (p->drive < 0 || p->drive > 3) return costmap_no(who, "drive has to be in [0, 3]");
    if (p->drive >= MPC_DRIVE_CAR_STAGE && !pos_finite(p->wheelbase)) return costmap_no(who, "wheelbase has to be positive and finite for a car drive");
    if (p->n_footprint < 0 || p->n_footprint == 1 || p->n_footprint > mpc::kPlMaxFootprint) return costmap_no(who, "n_footprint has to be 0 or in [2, 16]");
    for (int j = 0; j < p->n_footprint; ++j)
        if (!std::isfinite(p->footprint[j][0]) || !std::isfinite(p->footprint[j][1])) return costmap_no(who, "a footprint vertex is not finite");
    memset(&q, 0, sizeof(q));
    q.map_ox = p->map_origin[0]; q.map_oy = p->map_origin[1]; q.res = p->map_resolution; q.dt = p->interval; q.wheelbase = p->wheelbase;
    for (int i = 0; i < 3; ++i) { q.v_min[i] = p->v_min[i]; q.v_max[i] = p->v_max[i]; q.a_max[i] = p->a_max[i]; }
    for (int j = 0; j < p->n_footprint; ++j) { q.fx[j] = p->footprint[j][0]; q.fy[j] = p->footprint[j][1]; }
    q.nf = p->n_footprint; q.n_sub = p->n_substeps; q.drive = p->drive; q.map_sx = p->map_size_x; q.map_sy = p->map_size_y; q.threshold = p->block_threshold;
    q.unknown_blocks = p->unknown_blocks ? 1 : 0; q.outside_blocks = p->outside_blocks ? 1 : 0; q.has_map = map ? 1 : 0;
    if (map) {
        if (p->map_size_x < 1 || p->map_size_y < 1 || (long long)p->map_size_x * p->map_size_y > 2147483647LL) return costmap_no(who, "bad map size (at least 1 x 1, at most 2^31 - 1 bytes)");
        if (!pos_finite(p->map_resolution)) return costmap_no(who, "map_resolution has to be positive and finite");
        if (!std::isfinite(p->map_origin[0]) || !std::isfinite(p->map_origin[1])) return costmap_no(who, "map_origin has to be finite");
        if (p->block_threshold < 1 || p->block_threshold > 254) return costmap_no(who, "block_threshold has to be in [1, 254]");
    }
    if (!mpc::pl_reach(q)) return costmap_no(who, "a footprint edge has to be at most 350 cells of the map");
    for (int i = 0; i < 3; ++i) {
        if (!(p->a_max[i] >= 0.0)) return costmap_no(who, "a_max has to be at least 0");
        if (!(p->v_min[i] <= p->v_max[i])) return costmap_no(who, "v_min has to be at most v_max");
    }
    if (pool && pool->P < 0) return costmap_no(who, "pool: P is negative");
    return costmap_no(who, pool && pool->P > 0 && (!pool->n_vertices || !pool->vertices) ? "pool: n_vertices and vertices are needed with P > 0" : nullptr);
}

extern "C" {

void mpc_plant_params_defaults(mpc_plant_params* p, double map_resolution, int32_t map_size_x, int32_t map_size_y) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->map_resolution = map_resolution;
    p->interval = 0.1;
    p->wheelbase = 0.4;
    for (int i = 0; i < 3; ++i) { p->v_min[i] = -INFINITY; p->v_max[i] = p->a_max[i] = INFINITY; }
    p->n_footprint = 0;
    p->n_substeps = 1;
    p->drive = MPC_DRIVE_DIFF;
    p->map_size_x = map_size_x; p->map_size_y = map_size_y;
    p->block_threshold = 254;
    p->unknown_blocks = 0;
    p->outside_blocks = 1;
}

int mpc_plant_step_device(mpc_solver* s, int32_t B, const uint8_t* d_map, const mpc_plant_params* params, const double* d_cmd, const mpc_pool* pool,
                          const int32_t* d_self_index, double* d_pose, double* d_vel, int32_t* d_stall, int32_t* d_info) {
    g_err[0] = 0;
    mpc::PlantArgs a;
    memset(&a, 0, sizeof(a));
    if (plant_error("mpc_plant_step", s, d_map, params, d_cmd, pool, d_pose, a.p)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_plant_step")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    a.map = d_map; a.cmd = d_cmd; a.self_index = d_self_index; a.pose = d_pose; a.vel = d_vel; a.stall = d_stall; a.info = d_info;
    if (pool && pool->P > 0) a.pool = {pool->P, pool->n_vertices, pool->vertices, pool->radius, nullptr};
    a.V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1;
    return costmap_timed_launch(s, mpc::plant_step_kernel, B, mpc::kPlThreads, a);
}

int mpc_plant_step(mpc_solver* s, int32_t B, const uint8_t* map, const mpc_plant_params* params, const double* cmd, const mpc_pool* pool, const int32_t* self_index,
                   double* pose, double* vel, int32_t* stall, int32_t* info) {
    g_err[0] = 0;
    mpc::PlantParams q;
    if (plant_error("mpc_plant_step", s, map, params, cmd, pool, pose, q)) return MPC_EINVAL;
    if (B <= 0) return MPC_OK;
    if (const int rc = refused(s, B, REF_MAX_BATCH, "mpc_plant_step")) return rc;
    HIP_TRY(hipSetDevice(s->device));
    const size_t nb = (size_t)B, V = s->cfg.max_vertices > 0 ? s->cfg.max_vertices : 1, np = pool && pool->P > 0 ? (size_t)pool->P : 0;
    // in / out: the pose and the velocity are the state the call advances
    const mpc::StagePiece pc[10] = {stage_in(map, map ? (size_t)params->map_size_x * params->map_size_y : 0), stage_in(cmd, nb * 24), stage_in(np ? pool->n_vertices : nullptr, np * 4),
                                    stage_in(np ? pool->vertices : nullptr, np * V * 16), stage_in(np ? pool->radius : nullptr, np * 8), stage_in(self_index, nb * 4),
                                    stage_inout(pose, nb * 24), stage_inout(vel, nb * 24), stage_out(stall, nb * 4), stage_out(info, nb * 16)};
    return staged_call(s, "mpc_plant_step", true, true, pc, 10, [&](void** d) -> int {
        const mpc_pool dp = {(int32_t)np, (const int32_t*)d[2], (const double*)d[3], (const double*)d[4], nullptr};
        return mpc_plant_step_device(s, B, (const uint8_t*)d[0], params, (const double*)d[1], np ? &dp : nullptr, (const int32_t*)d[5], (double*)d[6], (double*)d[7],
                                     (int32_t*)d[8], (int32_t*)d[9]);
    });
}

}  // extern "C"
