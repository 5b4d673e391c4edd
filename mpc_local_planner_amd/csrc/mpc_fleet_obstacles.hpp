// mpc_fleet_obstacles.hpp -- obstacles that are not in the costmap, per planner instance and for a whole batch on the device: what
// MpcLocalPlannerROS::updateObstacleContainerWithCustomObstacles (src/mpc_local_planner_ros.cpp:543-617, called at :366 behind the costmap update) does with a shared
// obstacle message -- every obstacle of the message is appended to the robot's container, with its centroid velocity (:612-614), which under enable_dynamic_obstacles
// moves the clearance rows along k * dt * v (src/optimal_control/stage_inequality_se2.cpp:99-106,177-189) -- behind mpc_obstacles_from_pool*; and a pool made of the
// fleet itself (robot b = a circle at its pose with the velocity of the first interval of its own plan, the constant-velocity model of :177-189) behind mpc_fleet_pool*.
//
// The POOL is P obstacles in the planning frame, laid out like one instance of mpc_obstacles: n_vertices [P], vertices [P][V][2] (V = cfg.max_vertices), radius [P] or
// NULL, velocity [P][2] or NULL.  Instance b looks at it from (rx, ry) = robot_pose[b][0..1]:
//   key(p)     = min over the valid vertices j < min(n_vertices[p], V) of dx * dx + dy * dy, dx = rx - vx, dy = ry - vy (products and sum un-fused, as pi_sq_dist);
//   candidate  : n_vertices[p] >= 1, p != self_index[b], every valid vertex's squared distance finite, key(p) <= reach * reach (false for NaN: an entry with a vertex
//                that is not finite is never taken, a robot pose that is not finite takes nothing);
//   selection  : free = O - base entries fit (base = clamp(n_obstacles[b], 0, O) when appending, else 0).  At most `free` candidates: all are taken.  More: the `free`
//                smallest in the lexicographic order (key, p) -- nearest first, ties to the lower pool index;
//   emission   : the taken entries in increasing p at slots base, base + 1, ...: n_vertices, the valid vertices, radius (0 when the pool has none), velocity -- the pool's
//                when sqrt(vx * vx + vy * vy) >= min_speed, else (0, 0): teb's Obstacle::setCentroidVelocity(TwistWithCovariance, Quaternion), which :612-614 call, is
//                BELIEVED to treat a speed below 0.001 as static (teb_local_planner is not part of the reference's tree; the default 0.001 is cited as believed);
//   counts     : n_obstacles[b] = base + taken, dropped[b] = candidates - taken, n_taken[b] = taken.
// Slots below base and slots at or above the new n_obstacles[b] stay byte for byte as they were, and so do the vertices j >= n_vertices of a written slot.
//
// Ours, not the reference's:
//   * the reference culls nothing here (its containers have no capacity; the association of the solve culls by cutoff_dist).  `reach` and the nearest-first rule are forced
//     by the fixed capacity O: the rule max_obstacle_rows documents ("the M CLOSEST of them when they do not all fit"), one level up.  reach is a culling radius on vertex
//     distances, not a clearance: radii are not subtracted;
//   * self_index: the reference's message comes from elsewhere and does not hold the robot itself; a pool made of the fleet does;
//   * the pool-fill rule as a whole: the reference receives velocities, it does not derive them.
//
// The logic is written as __host__ __device__ functions in un-fused double arithmetic with +, -, *, /, comparisons and sqrt only, so that a g++ build
// (tests/host_harness/fleet_obstacles_host.cpp) and gfx950 agree bit for bit.  fo_instance is the per-instance statement; fleet_select_kernel restates it for a
// 256-thread workgroup (counts by ballot, the cut of the selection by a radix select on the keys' bit patterns) and computes the same bytes.
#pragma once
#include "mpc_controller_cycle.hpp"

namespace mpc {

struct FleetPool {       // struct mpc_pool of include/mpc_fleet.h
    int32_t P;
    const int32_t* n_vertices;    // [P]
    const double* vertices;       // [P][V][2]
    const double* radius;         // [P] or NULL
    const double* velocity;       // [P][2] or NULL
};
struct FleetParams { double reach, min_speed; int32_t append; };      // struct mpc_pool_params of include/mpc_fleet.h

// one instance's container: slot o at n_vertices[o], vertices[o][V][2], radius[o] (nullable), velocity[o][2] (nullable)
struct FleetContainer { int32_t* n_vertices; double* vertices; double* radius; double* velocity; };

constexpr uint64_t kFoNoKey = ~0ull;      // not a candidate; a finite non-negative double's bit pattern is below 0x7ff0000000000000

MPC_CC_HD bool fo_finite(double v) { return v - v == 0.0; }

MPC_CC_HD uint64_t fo_bits(double v) { uint64_t u; __builtin_memcpy(&u, &v, 8); return u; }

MPC_CC_HD double fo_reach_sq(double reach) {
#pragma clang fp contract(off)
    return reach * reach;
}

// The key of pool entry p seen from (rx, ry) as its bit pattern -- keys are finite and >= +0, so the patterns order as the values do -- or kFoNoKey when p is no candidate.
MPC_CC_HD uint64_t fo_key(const FleetPool& pool, int V, int p, int self, double rx, double ry, double reach_sq) {
#pragma clang fp contract(off)
    int nv = pool.n_vertices[p];
    if (nv < 1 || p == self) return kFoNoKey;
    if (nv > V) nv = V;
    const double* v = pool.vertices + (size_t)p * V * 2;
    double key = 0.0;
    bool finite = true;
    for (int j = 0; j < nv; ++j) {
        const double dx = rx - v[2 * j], dy = ry - v[2 * j + 1];
        const double qx = dx * dx, qy = dy * dy;
        const double d = qx + qy;
        finite = finite && fo_finite(d);
        if (j == 0 || d < key) key = d;
    }
    return finite && key <= reach_sq ? fo_bits(key) : kFoNoKey;
}

// pool entry p into slot `slot` of the container
MPC_CC_HD void fo_emit(const FleetPool& pool, int V, int p, double min_speed, const FleetContainer& c, int slot) {
#pragma clang fp contract(off)
    int nv = pool.n_vertices[p];
    if (nv > V) nv = V;
    c.n_vertices[slot] = nv;
    const double* v = pool.vertices + (size_t)p * V * 2;
    double* w = c.vertices + (size_t)slot * V * 2;
    for (int j = 0; j < 2 * nv; ++j) w[j] = v[j];
    if (c.radius) c.radius[slot] = pool.radius ? pool.radius[p] : 0.0;
    if (c.velocity) {
        double vx = 0.0, vy = 0.0;
        if (pool.velocity) {
            const double px = pool.velocity[2 * p], py = pool.velocity[2 * p + 1];
            const double qx = px * px, qy = py * py;
            if (__builtin_sqrt(qx + qy) >= min_speed) { vx = px; vy = py; }
        }
        c.velocity[2 * slot] = vx; c.velocity[2 * slot + 1] = vy;
    }
}

MPC_CC_HD int fo_base(int n_obstacles, int O, int append) {
    if (!append || n_obstacles < 0) return 0;
    return n_obstacles > O ? O : n_obstacles;
}

// One instance, as stated above: a candidate is taken iff fewer than `free` candidates come before it in the order (key, p).
MPC_CC_HD void fo_instance(const FleetPool& pool, int V, int O, double rx, double ry, int self, const FleetParams& prm, int32_t* n_obstacles, const FleetContainer& c,
                           int32_t* dropped, int32_t* n_taken) {
    const int base = fo_base(*n_obstacles, O, prm.append), free = O - base;
    const double reach_sq = fo_reach_sq(prm.reach);
    int candidates = 0;
    for (int p = 0; p < pool.P; ++p) candidates += fo_key(pool, V, p, self, rx, ry, reach_sq) != kFoNoKey;
    int taken = 0;
    for (int p = 0; p < pool.P; ++p) {
        const uint64_t k = fo_key(pool, V, p, self, rx, ry, reach_sq);
        if (k == kFoNoKey) continue;
        bool take = candidates <= free;
        if (!take) {
            int before = 0;
            for (int q = 0; q < pool.P && before < free; ++q) {
                const uint64_t kq = fo_key(pool, V, q, self, rx, ry, reach_sq);
                before += kq != kFoNoKey && (kq < k || (kq == k && q < p));
            }
            take = before < free;
        }
        if (take) { fo_emit(pool, V, p, prm.min_speed, c, base + taken); ++taken; }
    }
    *n_obstacles = base + taken;
    if (dropped) *dropped = candidates - taken;
    if (n_taken) *n_taken = taken;
}

// Pool fill: robot b as pool entry `entry` -- one vertex at its pose, its radius, and the velocity of the first interval of its own plan ((0, 0) without a plan, after a
// solve that did not converge (converged: MPC_CONVERGED = 0), with dt <= 0, or when one of the five numbers is not finite).  x: the robot's [n][3] states or NULL.
MPC_CC_HD void fp_instance(const double pose[3], const double* x, double dt, bool converged, double radius, int V, int entry, int32_t* pool_n_vertices,
                           double* pool_vertices, double* pool_radius, double* pool_velocity) {
#pragma clang fp contract(off)
    pool_n_vertices[entry] = 1;
    pool_vertices[(size_t)entry * V * 2] = pose[0];
    pool_vertices[(size_t)entry * V * 2 + 1] = pose[1];
    if (pool_radius) pool_radius[entry] = radius;
    if (pool_velocity) {
        double vx = 0.0, vy = 0.0;
        if (x && converged && dt > 0.0 && fo_finite(dt) && fo_finite(x[0]) && fo_finite(x[1]) && fo_finite(x[3]) && fo_finite(x[4])) {
            const double ex = x[3] - x[0], ey = x[4] - x[1];
            vx = ex / dt; vy = ey / dt;
        }
        pool_velocity[2 * entry] = vx; pool_velocity[2 * entry + 1] = vy;
    }
}

#if defined(__HIPCC__)

constexpr int kFleetThreads = 256;
constexpr int kFleetLdsKeys = 2048;      // pools up to this size keep their keys in LDS (16 KB); larger ones recompute them in every pass

struct FleetSelectArgs {
    FleetPool pool;
    FleetParams prm;
    const double* pose;           // [B][3]
    const int32_t* self_index;    // [B] or NULL
    int32_t O, V;
    int32_t* n_obstacles;         // [B] in / out
    int32_t* n_vertices;          // [B][O]
    double* vertices;             // [B][O][V][2]
    double* radius;               // [B][O] or NULL
    double* velocity;             // [B][O][2] or NULL
    int32_t* dropped;             // [B] or NULL
    int32_t* n_taken;             // [B] or NULL
};

// Exclusive prefix over the workgroup's 256 threads, in thread order, of two flags at once, and both totals: ballot + popcount inside a wave, the four waves' counts
// through LDS (ws: 8 words).  Every thread of the workgroup calls it.
__device__ __forceinline__ void fo_scan_flags(bool f0, bool f1, int* ws, int& pre0, int& pre1, int& tot0, int& tot1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m0 = __ballot(f0), m1 = __ballot(f1);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) { ws[wave] = __popcll(m0); ws[4 + wave] = __popcll(m1); }
    __syncthreads();
    pre0 = __popcll(m0 & below); pre1 = __popcll(m1 & below);
    tot0 = 0; tot1 = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c0 = ws[w], c1 = ws[4 + w];
        if (w < wave) { pre0 += c0; pre1 += c1; }
        tot0 += c0; tot1 += c1;
    }
    __syncthreads();      // ws is free again
}

// One workgroup (256 threads) per instance; the pool in chunks of 256 consecutive entries, thread t on entry c0 + t (coalesced; the pool is shared by every workgroup
// and lives in L2).  Three steps, each a sweep over the pool:
//   count  : the candidates, by ballot / popcount;
//   cut    : only when they do not all fit -- the free-th smallest key, exactly, by a radix select over the eight 8-bit digits of the keys' bit patterns from the top,
//            with a 256-bin histogram of integer LDS atomics (order-independent, hence deterministic; no floating-point atomics anywhere), then the number of entries
//            AT the cut key that still fit, taken in pool order;
//   emit   : a taken entry's slot is base + (entries below the cut before it) + min(entries at the cut before it, those that fit): a running prefix in pool order,
//            without sorting, as costmap_to_obstacles_kernel positions its cells.
// Every count is an integer and every key is computed by fo_key alone: the result depends neither on B, nor on the position in the batch, nor on the run.
__global__ __launch_bounds__(kFleetThreads) void fleet_select_kernel(FleetSelectArgs a) {
    __shared__ uint64_t keys[kFleetLdsKeys];
    __shared__ unsigned int hist[256];
    __shared__ int ws[8];
    __shared__ int sel[2];      // the digit the cut falls into, and its rank inside that bin
    const int b = blockIdx.x, t = threadIdx.x;
    const FleetPool& pool = a.pool;
    const int P = pool.P, V = a.V, O = a.O;
    const double rx = a.pose[3 * b], ry = a.pose[3 * b + 1];
    const int self = a.self_index ? a.self_index[b] : -1;
    const int base = fo_base(a.n_obstacles[b], O, a.prm.append), free = O - base;
    const double reach_sq = fo_reach_sq(a.prm.reach);
    const bool in_lds = P <= kFleetLdsKeys;
    // ---- count (and the keys into LDS)
    int mine = 0;
    for (int c0 = 0; c0 < P; c0 += kFleetThreads) {
        const int p = c0 + t;
        if (p < P) {
            const uint64_t k = fo_key(pool, V, p, self, rx, ry, reach_sq);
            if (in_lds) keys[p] = k;
            mine += k != kFoNoKey;
        }
    }
    for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s);
    if ((t & 63) == 0) ws[t >> 6] = mine;
    __syncthreads();      // (also: the keys are in LDS)
    const int candidates = ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    // ---- cut: entries with a key below `cut` are taken, and the first `at_cut` of those with key == cut
    uint64_t cut = kFoNoKey;      // everything fits: every candidate is below
    int at_cut = 0;
    if (free == 0) cut = 0;       // nothing fits: no key is below 0
    else if (candidates > free) {      // workgroup-uniform
        uint64_t prefix = 0;
        int k = free;             // the cut is the k-th smallest (1-based) of the keys that share the digits found so far
        for (int d = 7; d >= 0; --d) {
            hist[t] = 0u;
            __syncthreads();
            for (int c0 = 0; c0 < P; c0 += kFleetThreads) {
                const int p = c0 + t;
                if (p >= P) continue;
                const uint64_t key = in_lds ? keys[p] : fo_key(pool, V, p, self, rx, ry, reach_sq);
                if (key != kFoNoKey && (d == 7 || (key >> (8 * d + 8)) == (prefix >> (8 * d + 8)))) atomicAdd(&hist[(unsigned)(key >> (8 * d)) & 255u], 1u);
            }
            __syncthreads();
            // inclusive scan of the bins in thread order: the bin whose running count first reaches k
            const int h = (int)hist[t];
            int inc = h;
            for (int s = 1; s < 64; s <<= 1) { const int v = __shfl_up(inc, s); if ((t & 63) >= s) inc += v; }
            if ((t & 63) == 63) ws[t >> 6] = inc;
            __syncthreads();
            for (int w = 0; w < (t >> 6); ++w) inc += ws[w];
            if (inc >= k && inc - h < k) { sel[0] = t; sel[1] = k - (inc - h); }      // exactly one thread: the counts are non-decreasing and end at >= k
            __syncthreads();
            prefix |= (uint64_t)sel[0] << (8 * d);
            k = sel[1];
            __syncthreads();
        }
        cut = prefix; at_cut = k;
    }
    // ---- emit
    FleetContainer c;
    c.n_vertices = a.n_vertices + (size_t)b * O;
    c.vertices = a.vertices + (size_t)b * O * V * 2;
    c.radius = a.radius ? a.radius + (size_t)b * O : nullptr;
    c.velocity = a.velocity ? a.velocity + (size_t)b * O * 2 : nullptr;
    int run_below = 0, run_at = 0;
    for (int c0 = 0; c0 < P; c0 += kFleetThreads) {
        const int p = c0 + t;
        uint64_t key = kFoNoKey;
        if (p < P) key = in_lds ? keys[p] : fo_key(pool, V, p, self, rx, ry, reach_sq);
        const bool below = key != kFoNoKey && key < cut, at = key != kFoNoKey && key == cut;
        int pre_below, pre_at, tot_below, tot_at;
        fo_scan_flags(below, at, ws, pre_below, pre_at, tot_below, tot_at);
        const int before_at = run_at + pre_at;      // entries at the cut before this one, in pool order
        if (below || (at && before_at < at_cut)) {
            const int slot = base + run_below + pre_below + (before_at < at_cut ? before_at : at_cut);
            if (slot < O) fo_emit(pool, V, p, a.prm.min_speed, c, slot);      // (always: taken entries number at most `free`)
        }
        run_below += tot_below; run_at += tot_at;
    }
    if (t == 0) {
        const int taken = run_below + (run_at < at_cut ? run_at : at_cut);
        a.n_obstacles[b] = base + taken;
        if (a.dropped) a.dropped[b] = candidates - taken;
        if (a.n_taken) a.n_taken[b] = taken;
    }
}

struct FleetPoolArgs {
    int32_t B, n_stride, V, pool_offset;
    const double* pose;           // [B][3]
    const double* x;              // [B][n_stride][3] or NULL
    const double* dt;             // [B] (with x)
    const int32_t* status;        // [B] or NULL
    double robot_radius;
    const double* radius;         // [B] or NULL: the scalar
    int32_t* pool_n_vertices;
    double* pool_vertices;
    double* pool_radius;          // or NULL
    double* pool_velocity;        // or NULL
};

// one thread per robot
__global__ __launch_bounds__(64) void fleet_pool_kernel(FleetPoolArgs a) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    const double pose[3] = {a.pose[3 * b], a.pose[3 * b + 1], a.pose[3 * b + 2]};
    fp_instance(pose, a.x ? a.x + (size_t)b * a.n_stride * 3 : nullptr, a.x ? a.dt[b] : 0.0, a.status ? a.status[b] == 0 : true, a.radius ? a.radius[b] : a.robot_radius, a.V,
                a.pool_offset + b, a.pool_n_vertices, a.pool_vertices, a.pool_radius, a.pool_velocity);
}

#endif  // __HIPCC__

}  // namespace mpc
