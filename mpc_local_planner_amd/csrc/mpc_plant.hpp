// mpc_plant.hpp -- the plant step: every robot of a batch moved by its command on the device, the last arrow of the fleet's control cycle.  mpc_commands_batch_device
// writes cmd [B][3]; this step turns it into the next pose, and into a stall when the robot's outline meets the map or another body.  In every demo of the reference
// the plant is the `position` model of the Stage simulator: ex/stage/robots/*.inc declare drive "diff", "car" with wheelbase 0.4, or "omni", and a size and origin
// that give the footprint printed in carlike_robot.inc:16; the ex/stage/*.world files set interval_sim 100, the floorplan has boundary 1 and the robots obstruct each
// other.  Stage is not part of the reference's tree and is not available where this was written: lines marked (!) restate Stage's published `position` model FROM
// MEMORY OF ITS SOURCE and cannot be verified here.  Lines marked OURS are a rule of ours, declared as such.
//
// The rule, per instance (pose = pose[b][0..2], cmd = (c0, c1, c2) = cmd[b][0..2], vel = vel[b][0..2] when given; dt = interval; res = map_resolution; a map byte
// blocks as in mpc_scan_cast.hpp):
//   1. validity : OURS: the instance is INVALID when a component of the pose, of the command or of the given velocity is not finite, when th = cs_wrap(pose theta)
//                 does not wrap, for a car drive when phi = cs_wrap(c2) does not wrap, or when a component of the target velocity of rule 2 is not finite (the
//                 rear-axle car at a quarter turn of steering).  An invalid instance does not move: pose and vel are not written, stall = 0, info = {-1, -1, -1, -1}.
//   2. target   : the body velocity (vx, vy, w) the command asks for, once per call:
//                   diff      (c0, 0, c2)                                                       (!)
//                   omni      (c0, c1, c2)                                                      (!)
//                   car, Stage: (s, c) = cs_sincos(phi); (c0 * c, 0, (c0 * s) / wheelbase)       (!)
//                   car, rear : (c0, 0, (c0 * (s / c)) / wheelbase): the reference's simple_car model, include/mpc_local_planner/systems/simple_car.h:74-76
//                               (f[2] = u[0] * tan(u[1]) / wheelbase), the tangent as the quotient of cs_sincos' two values.  OURS as a plant.
//                 mpc_commands_batch* writes the steering angle into cmd[2] for the car-like models.
//   3. bounds   : OURS.  v_prev is vel when given, else the target.  Per sub-step and component: d = target - v_prev; d = min(d, a_max * dt); d = max(d, -(a_max * dt));
//                 v = v_prev + d; v = max(v, v_min); v = min(v, v_max); v_prev of the next sub-step is v, whether or not the sub-step moves.  vel, when given, receives
//                 the v of the last sub-step; without it nothing is kept between calls.
//   4. move     : (!) Stage's pose sum, one Euler step in the frame at the start of the sub-step: (dx, dy, da) = (vx * dt, vy * dt, w * dt); (s, c) = cs_sincos(th);
//                 x' = x + (dx * c - dy * s), y' = y + (dx * s + dy * c), every product rounded on its own; th' = cs_wrap(th + da).  A th' that does not wrap blocks the
//                 sub-step with reason -4; OURS: so does an x' or y' that is not finite.
//   5. collision: OURS: an exact test of the OUTLINE at the candidate pose (x', y', th'), for n_footprint >= 2.  World vertex j: cs_place_sensor(x', y', th', fx_j, fy_j).
//                 Edge j runs from w_j to w_(j+1): the closed loop for n_footprint >= 3, the one segment for 2.  e = w_(j+1) - w_j, len = sqrt(ex * ex + ey * ey), the
//                 direction (ex / len, ey / len), and (1, 0) for len == 0.
//                   map : (a map given) u = (wx - map_origin_x) / res, v likewise; the vertex's cell (floor(u), floor(v)).  A vertex whose cell is off the map: reason -3
//                         with outside_blocks, ignored without.  Otherwise the edge is followed from its first vertex by sc_walk (mpc_scan_cast.hpp rule 2) with len in
//                         the place of range_max and hit_point 0: any finite return means the map blocks, reason -2.  (sc_walk's Rc is one number per call: sc_cells of
//                         the longest edge of the footprint as given, plus one cell for the rounding of the placed vertices.  The clause it feeds never fires -- the
//                         range test ends the walk first --, so the result is that of any Rc of at least sc_cells(len, res).)
//                   pool: sc_pool_entry(pool, V, p, self, w_j, direction, t) (mpc_scan_cast.hpp rule 3, what it skips included): entry p blocks when t <= len.  The pool
//                         stands where it was when the call began.
//                 If nothing blocks the pose becomes the candidate.  Otherwise the pose stays, the sub-step counts as a stall and the next sub-step is tried from the
//                 unchanged pose ((!) Stage restores the pose on a collision and sets `stall`).
//   6. outputs  : pose is written once, at the end: (x, y, th) when a sub-step moved, untouched when none did.  stall = the number of blocked sub-steps.  info = {sub-steps
//                 moved, the first blocked sub-step or -1, its reason or -1, the lowest edge j that shows that reason (the lowest vertex j for -3; -1 for -4 and without
//                 a blocked sub-step)}.  The reason is the first that applies of -4, -3, -2, then the lowest pool p.  All of these are minima (pl_key), so the result
//                 depends neither on the order of edges or entries, on B, on the place in the batch or on the run.
//   7. refusals : a null required pointer (s, params, cmd, pose); n_substeps outside 1 .. 64; interval not positive and finite; drive outside 0 .. 3; wheelbase not
//                 positive and finite for a car drive; n_footprint below 0, of 1 or above 16, or a footprint vertex that is not finite; with a map: map_size_x or
//                 map_size_y below 1 or their product above 2^31 - 1, map_resolution not positive and finite, map_origin not finite, block_threshold outside 1 .. 254,
//                 an edge of the footprint whose sc_cells exceeds kScMaxRc; a_max negative or not a number, or v_min <= v_max not holding; P < 0, or P > 0 without
//                 n_vertices and vertices.
// Declared limits, and so visible deviations from Stage: the OUTLINE only -- a body wholly inside the footprint is not seen; every robot is tested against the others
// where they stood when the call began, where Stage moves its models one after the other; no odom_error, the pose is the true one (Stage's localization "gps"); pool
// entries are not moved; z is ignored.
// Every double is produced by + - * /, floor, sqrt and cs_sincos (its fmas explicit) under `#pragma clang fp contract(off)`, so a g++ build and the device round alike.
//
// pl_instance is the per-instance statement (host code, serial).  plant_step_kernel restates it for one 64-thread workgroup per instance.  Both take a sub-step from
// the same host / device functions (pl_start, pl_bound, pl_candidate, pl_vertex, pl_edge, pl_vertex_off, pl_edge_map, sc_pool_entry, pl_key).
#pragma once
#include "mpc_scan_cast.hpp"

namespace mpc {

constexpr int kPlThreads = 64;
constexpr int kPlListCap = 512;       // pool entries the workgroup's culled list holds; what comes behind is tested from global memory
constexpr int kPlMaxFootprint = 16;
constexpr int kPlMaxSubsteps = 64;
enum { PL_DIFF = 0, PL_OMNI = 1, PL_CAR_STAGE = 2, PL_CAR_REAR = 3 };

// the fields of mpc_plant_params the rule reads; has_map: a map was given; Rc: rule 5's; reach: the footprint's circumradius (the kernel's culling)
struct PlantParams {
    double map_ox, map_oy, res, dt, wheelbase, reach;
    double v_min[3], v_max[3], a_max[3];
    double fx[kPlMaxFootprint], fy[kPlMaxFootprint];
    int32_t nf, n_sub, drive, map_sx, map_sy, threshold, unknown_blocks, outside_blocks, has_map, Rc;
};

// rule 5's Rc and the circumradius from the footprint as given: false when an edge's sc_cells exceeds the cap (only asked with a map)
inline bool pl_reach(PlantParams& p) {
    double longest = 0.0, far2 = 0.0;
    const int edges = p.nf == 2 ? 1 : p.nf;
    for (int j = 0; j < p.nf; ++j) {
        const double r2 = p.fx[j] * p.fx[j] + p.fy[j] * p.fy[j];
        if (r2 > far2) far2 = r2;
        if (j >= edges) continue;
        const int j1 = j + 1 < p.nf ? j + 1 : 0;
        const double ex = p.fx[j1] - p.fx[j], ey = p.fy[j1] - p.fy[j];
        const double len = __builtin_sqrt(ex * ex + ey * ey);
        if (len > longest) longest = len;
    }
    p.reach = __builtin_sqrt(far2);
    p.Rc = 1;
    if (!p.has_map || p.nf < 2) return true;
    const int cells = sc_cells(longest, p.res);
    if (cells < 0) return false;
    p.Rc = cells + 1;
    return true;
}

// the state of an instance between sub-steps
struct PlantState { double x, y, th, v[3]; };

// rules 1 and 2: false for an invalid instance; else the state at the start of the call and the target velocity (vel: three doubles, read when has_vel)
MPC_CM_HD bool pl_start(const PlantParams& p, const double* pose, const double* cmd, const double* vel, bool has_vel, PlantState& st, double* target) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) ok = ok && fo_finite(pose[i]) && fo_finite(cmd[i]) && (!has_vel || fo_finite(vel[i]));
    target[0] = target[1] = target[2] = 0.0;
    st.x = st.y = st.th = st.v[0] = st.v[1] = st.v[2] = 0.0;
    if (!ok) return false;
    const double th = cs_wrap(pose[2]);
    if (!cs_wrapped(th)) return false;
    if (p.drive == PL_DIFF) { target[0] = cmd[0]; target[2] = cmd[2]; }
    else if (p.drive == PL_OMNI) { target[0] = cmd[0]; target[1] = cmd[1]; target[2] = cmd[2]; }
    else {
        const double phi = cs_wrap(cmd[2]);
        if (!cs_wrapped(phi)) return false;
        double s, c;
        cs_sincos(phi, s, c);
        if (p.drive == PL_CAR_STAGE) {
            const double along = cmd[0] * s;
            target[0] = cmd[0] * c;
            target[2] = along / p.wheelbase;
        } else {
            const double tangent = s / c;
            const double along = cmd[0] * tangent;
            target[0] = cmd[0];
            target[2] = along / p.wheelbase;
        }
    }
    if (!fo_finite(target[0]) || !fo_finite(target[1]) || !fo_finite(target[2])) return false;
    st.x = pose[0]; st.y = pose[1]; st.th = th;
#pragma unroll
    for (int i = 0; i < 3; ++i) st.v[i] = has_vel ? vel[i] : target[i];
    return true;
}

// rule 3: the bounded velocity of a sub-step, in place of the previous one
MPC_CM_HD void pl_bound(const PlantParams& p, const double* target, double* v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double lim = p.a_max[i] * p.dt;
        double d = target[i] - v[i];
        if (d > lim) d = lim;
        if (d < -lim) d = -lim;
        double w = v[i] + d;
        if (w < p.v_min[i]) w = p.v_min[i];
        if (w > p.v_max[i]) w = p.v_max[i];
        v[i] = w;
    }
}

// rule 4: the candidate pose of a sub-step; false when it blocks with reason -4
MPC_CM_HD bool pl_candidate(const PlantParams& p, const PlantState& st, double& xc, double& yc, double& thc) {
#pragma clang fp contract(off)
    const double dx = st.v[0] * p.dt, dy = st.v[1] * p.dt, da = st.v[2] * p.dt;
    double s, c;
    cs_sincos(st.th, s, c);
    const double xa = dx * c, xb = dy * s, ya = dx * s, yb = dy * c;
    const double rx = xa - xb, ry = ya + yb;
    xc = st.x + rx;
    yc = st.y + ry;
    thc = cs_wrap(st.th + da);
    return cs_wrapped(thc) && fo_finite(xc) && fo_finite(yc);
}

// rule 5: world vertex j of the footprint at the candidate pose (fx, fy: the vertex in the robot frame)
MPC_CM_HD void pl_vertex(double xc, double yc, double thc, double fx, double fy, double& wx, double& wy) { cs_place_sensor(xc, yc, thc, fx, fy, wx, wy); }

// rule 5: the edge from (ax, ay) to (bx, by): its direction and its length
MPC_CM_HD void pl_edge(double ax, double ay, double bx, double by, double& ux, double& uy, double& len) {
#pragma clang fp contract(off)
    const double ex = bx - ax, ey = by - ay;
    const double xx = ex * ex, yy = ey * ey;
    len = __builtin_sqrt(xx + yy);
    if (len == 0.0) { ux = 1.0; uy = 0.0; return; }
    ux = ex / len;
    uy = ey / len;
}

// rule 5: the frame sc_walk takes for a walk that begins at (wx, wy): sc_frame's lines behind the placement of the sensor
MPC_CM_HD CastFrame pl_frame(const PlantParams& p, double wx, double wy) {
#pragma clang fp contract(off)
    CastFrame f;
    f.sx = wx; f.sy = wy;
    const double dx = wx - p.map_ox, dy = wy - p.map_oy;
    f.u = dx / p.res;
    f.v = dy / p.res;
    f.i0 = f.j0 = 0;
    f.valid = true;
    const double fi = __builtin_floor(f.u), fj = __builtin_floor(f.v);
    f.on_map = fi >= 0.0 && fi < (double)p.map_sx && fj >= 0.0 && fj < (double)p.map_sy;      // false for a NaN
    if (f.on_map) { f.i0 = (int32_t)fi; f.j0 = (int32_t)fj; }
    return f;
}

// rule 5: whether the cell of vertex (wx, wy) is off the map
MPC_CM_HD bool pl_vertex_off(const PlantParams& p, double wx, double wy) { return !pl_frame(p, wx, wy).on_map; }

// rule 5: whether the map blocks the edge that leaves (wx, wy) along (ux, uy) for len; the map bytes are read where they lie
MPC_CM_HD bool pl_edge_map(const PlantParams& p, const uint8_t* map, double wx, double wy, double ux, double uy, double len) {
    const CastFrame f = pl_frame(p, wx, wy);
    if (!f.on_map) return false;
    CastParams c;
    c.map_ox = p.map_ox; c.map_oy = p.map_oy; c.res = p.res;
    c.sensor_x = c.sensor_y = c.sensor_yaw = c.angle_min = c.angle_inc = 0.0;
    c.range_max = len;
    c.map_sx = p.map_sx; c.map_sy = p.map_sy; c.threshold = p.threshold; c.unknown_blocks = p.unknown_blocks;
    c.hit_point = 0; c.miss_is_inf = 1; c.Rc = p.Rc;
    const int sx = p.map_sx, threshold = p.threshold, unknown = p.unknown_blocks;
    const double r = sc_walk(c, f, ux, uy, [=](int i, int j) { return sc_blocks(map[(size_t)j * sx + i], threshold, unknown); });
    return r < __builtin_inf();
}

// rule 6: what blocks a sub-step as one number whose minimum is the reported reason and edge: -4, -3, -2, then the pool entries in their order, and within one
// reason the lowest edge
constexpr unsigned long long kPlFree = ~0ull;
MPC_CM_HD unsigned long long pl_key(int reason, int j) { return ((unsigned long long)(reason + 4) << 5) | (unsigned long long)(j < 0 ? 0 : j); }
MPC_CM_HD int pl_key_reason(unsigned long long k) { return (int)(long long)(k >> 5) - 4; }
MPC_CM_HD int pl_key_edge(unsigned long long k) { return pl_key_reason(k) == -4 ? -1 : (int)(k & 31ull); }

// the kernel's culling radius, which only has to err on the side of keeping: every candidate pose of the call lies within n_substeps * dt * |v| of the start, and a
// bounded |v_i| never exceeds the largest of |v_prev_i|, |target_i| and the finite ones of |v_min_i|, |v_max_i|; the outline lies within the circumradius of the
// pose.  sc_may_reach adds the entry's own extent and the slack for the rounding.  A sum that overflows keeps everything.
MPC_CM_HD double pl_cull_radius(const PlantParams& p, const PlantState& st, const double* target) {
#pragma clang fp contract(off)
    double m2 = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        double m = st.v[i] < 0.0 ? -st.v[i] : st.v[i];
        const double t = target[i] < 0.0 ? -target[i] : target[i];
        const double lo = p.v_min[i] < 0.0 ? -p.v_min[i] : p.v_min[i], hi = p.v_max[i] < 0.0 ? -p.v_max[i] : p.v_max[i];
        if (t > m) m = t;
        if (fo_finite(lo) && lo > m) m = lo;
        if (fo_finite(hi) && hi > m) m = hi;
        m2 = m2 + m * m;
    }
    const double travel = ((double)p.n_sub * p.dt) * __builtin_sqrt(m2);
    return (p.reach + travel) * 1.000001 + 1e-9;
}

// ---- the statement (host).  pose: 3 doubles in / out; vel: 3 doubles in / out or NULL; stall: a word or NULL; info: 4 words or NULL.  map NULL: no map test;
// pool.P == 0: no pool.
inline void pl_instance(const PlantParams& p, const uint8_t* map, const FleetPool& pool, int V, int self, const double* cmd, double* pose, double* vel, int32_t* stall,
                        int32_t* info) {
    PlantState st;
    double target[3];
    const double none[3] = {0.0, 0.0, 0.0};
    if (!pl_start(p, pose, cmd, vel ? vel : none, vel != nullptr, st, target)) {
        if (stall) *stall = 0;
        if (info) info[0] = info[1] = info[2] = info[3] = -1;
        return;
    }
    int moved = 0, stalled = 0, first = -1, reason = -1, edge = -1;
    const int edges = p.nf == 2 ? 1 : p.nf;
    for (int m = 0; m < p.n_sub; ++m) {
        pl_bound(p, target, st.v);
        double xc, yc, thc;
        unsigned long long key = kPlFree;
        if (!pl_candidate(p, st, xc, yc, thc)) key = pl_key(-4, -1);
        else if (p.nf >= 2) {
            double wx[kPlMaxFootprint], wy[kPlMaxFootprint];
            for (int j = 0; j < p.nf; ++j) pl_vertex(xc, yc, thc, p.fx[j], p.fy[j], wx[j], wy[j]);
            for (int j = 0; j < p.nf && map; ++j)
                if (p.outside_blocks && pl_vertex_off(p, wx[j], wy[j]) && pl_key(-3, j) < key) key = pl_key(-3, j);
            for (int j = 0; j < edges; ++j) {
                const int j1 = j + 1 < p.nf ? j + 1 : 0;
                double ux, uy, len;
                pl_edge(wx[j], wy[j], wx[j1], wy[j1], ux, uy, len);
                if (map && pl_edge_map(p, map, wx[j], wy[j], ux, uy, len) && pl_key(-2, j) < key) key = pl_key(-2, j);
                for (int e = 0; e < pool.P; ++e) {
                    double t;
                    if (sc_pool_entry(pool, V, e, self, wx[j], wy[j], ux, uy, t) && t <= len && pl_key(e, j) < key) key = pl_key(e, j);
                }
            }
        }
        if (key == kPlFree) { st.x = xc; st.y = yc; st.th = thc; ++moved; }
        else {
            if (first < 0) { first = m; reason = pl_key_reason(key); edge = pl_key_edge(key); }
            ++stalled;
        }
    }
    if (moved) { pose[0] = st.x; pose[1] = st.y; pose[2] = st.th; }
    if (vel) { vel[0] = st.v[0]; vel[1] = st.v[1]; vel[2] = st.v[2]; }
    if (stall) *stall = stalled;
    if (info) { info[0] = moved; info[1] = first; info[2] = reason; info[3] = edge; }
}

#if defined(__HIPCC__)

struct PlantArgs {
    const uint8_t* map;           // [map_sy][map_sx], shared by every instance, or NULL
    const double* cmd;            // [B][3]
    FleetPool pool;               // P == 0: none
    const int32_t* self_index;    // [B] or NULL
    double* pose;                 // [B][3] in / out
    double* vel;                  // [B][3] in / out or NULL
    int32_t* stall;               // [B] or NULL
    int32_t* info;                // [B][4] or NULL
    PlantParams p;
    int32_t V;
};
static_assert(std::is_trivially_copyable<PlantArgs>::value, "a kernel argument");

// One workgroup of ONE WAVE (64 threads) per instance.  Why 64 and not 256: the sub-steps are a serial chain, each one a handful of small parallel pieces -- at most
// 16 vertices, 16 map walks of a few cells, 16 edges times a culled list that holds the few bodies within a footprint and a call's travel of the robot -- with a
// decision between them.  One wave covers 16 edges x 4 listed entries a pass, its hand-offs through LDS are ordered inside the wave and cost no workgroup barrier
// across waves, and a fleet of 1024 robots is still 1024 waves, one for each SIMD of the device.  Only the culling would gain from 256 threads (4 chunks of the pool
// instead of 16), once per call.
//   start  : every lane holds the instance's state in registers (wave-uniform values); lane j holds footprint vertex j, picked from the kernel argument by an unrolled
//            compare so that no array is indexed by the lane.
//   cull   : the pool in chunks of 64 consecutive entries, lane t on entry c0 + t; the entries sc_may_reach keeps within pl_cull_radius of the start pose go to the LDS
//            list in pool order (ballot and popcount prefix).  The first chunk that would not fit ends the culling: `tail` is its first entry, and every sub-step
//            tests the entries from there on from global memory, in increasing p.
//   substep: wave-uniform loop.  Lane j places vertex j into LDS; lane j makes edge j from the vertices j and j + 1 and keeps it in registers and in LDS; the map
//            phase is one vertex test and one walk per lane, the map bytes read straight from global memory through L2, where neighbouring robots share them (a
//            footprint spans a few cells: there is nothing to stage); the pool phase hands (listed entry, edge) pairs to the lanes, 64 a pass, then (tail entry, edge)
//            pairs.  Every finding is a pl_key; the wave's minimum is taken with an LDS atomic minimum, and the pool phase is skipped when the map has blocked (a
//            map key is below every pool key).
// No private arrays, plain vector stores and LDS only.
__global__ __launch_bounds__(kPlThreads) void plant_step_kernel(PlantArgs a) {
    __shared__ int s_list[kPlListCap];
    __shared__ double s_w[kPlMaxFootprint][2];      // the placed vertices
    __shared__ double s_e[kPlMaxFootprint][3];      // the edges: direction and length
    __shared__ unsigned long long s_key;
    const int lane = threadIdx.x, b = blockIdx.x;
    const int nf = a.p.nf, edges = nf == 2 ? 1 : nf;
    const double* pose_in = a.pose + 3 * (size_t)b;
    const double* cmd_in = a.cmd + 3 * (size_t)b;
    const double pose3[3] = {pose_in[0], pose_in[1], pose_in[2]};
    const double cmd3[3] = {cmd_in[0], cmd_in[1], cmd_in[2]};
    double vel3[3] = {0.0, 0.0, 0.0};
    if (a.vel) { vel3[0] = a.vel[3 * (size_t)b]; vel3[1] = a.vel[3 * (size_t)b + 1]; vel3[2] = a.vel[3 * (size_t)b + 2]; }
    const int self = a.self_index ? a.self_index[b] : -1;
    PlantState st;
    double target[3];
    if (!pl_start(a.p, pose3, cmd3, vel3, a.vel != nullptr, st, target)) {      // wave-uniform
        if (lane == 0 && a.stall) a.stall[b] = 0;
        if (lane < 4 && a.info) a.info[4 * (size_t)b + lane] = -1;
        return;
    }
    double fx = 0.0, fy = 0.0;      // lane j: vertex j in the robot frame
#pragma unroll
    for (int j = 0; j < kPlMaxFootprint; ++j)
        if (lane == j) { fx = a.p.fx[j]; fy = a.p.fy[j]; }
    // ---- cull
    int listed = 0, tail = 0;      // wave-uniform
    const int P = nf >= 2 ? a.pool.P : 0;
    {
        const double radius = pl_cull_radius(a.p, st, target);
        tail = P;
        for (int c0 = 0; c0 < P; c0 += kPlThreads) {
            const int p = c0 + lane;
            const bool keep = p < P && sc_may_reach(a.pool, a.V, p, self, st.x, st.y, radius);
            const unsigned long long m = __ballot(keep);
            const int total = __popcll(m);
            if (listed + total > kPlListCap) { tail = c0; break; }
            if (keep) s_list[listed + __popcll(m & ((1ull << lane) - 1ull))] = p;
            listed += total;
        }
    }
    __syncthreads();
    // ---- sub-steps
    int moved = 0, stalled = 0, first = -1, reason = -1, edge = -1;      // wave-uniform
    const int pairs = listed * edges;
    for (int m = 0; m < a.p.n_sub; ++m) {
        pl_bound(a.p, target, st.v);
        double xc, yc, thc;
        unsigned long long key = kPlFree;
        if (!pl_candidate(a.p, st, xc, yc, thc)) key = pl_key(-4, -1);
        else if (nf >= 2) {
            if (lane == 0) s_key = kPlFree;
            if (lane < nf) {
                double wx, wy;
                pl_vertex(xc, yc, thc, fx, fy, wx, wy);
                s_w[lane][0] = wx; s_w[lane][1] = wy;
            }
            __syncthreads();
            double wx = 0.0, wy = 0.0, ux = 1.0, uy = 0.0, len = 0.0;
            if (lane < nf) { wx = s_w[lane][0]; wy = s_w[lane][1]; }
            if (lane < edges) {
                const int j1 = lane + 1 < nf ? lane + 1 : 0;
                pl_edge(wx, wy, s_w[j1][0], s_w[j1][1], ux, uy, len);
                s_e[lane][0] = ux; s_e[lane][1] = uy; s_e[lane][2] = len;
            }
            if (a.map) {
                unsigned long long mine = kPlFree;
                if (lane < nf && a.p.outside_blocks && pl_vertex_off(a.p, wx, wy)) mine = pl_key(-3, lane);
                if (mine == kPlFree && lane < edges && pl_edge_map(a.p, a.map, wx, wy, ux, uy, len)) mine = pl_key(-2, lane);
                if (mine != kPlFree) atomicMin(&s_key, mine);
            }
            __syncthreads();
            key = s_key;
            if (key == kPlFree && P > 0) {      // wave-uniform
                for (int q0 = 0; q0 < pairs; q0 += kPlThreads) {
                    const int q = q0 + lane;
                    if (q < pairs) {
                        const int e = q / edges, j = q - e * edges, p = s_list[e];
                        double t;
                        if (sc_pool_entry(a.pool, a.V, p, self, s_w[j][0], s_w[j][1], s_e[j][0], s_e[j][1], t) && t <= s_e[j][2]) atomicMin(&s_key, pl_key(p, j));
                    }
                }
                if (lane < edges)
                    for (int p = tail; p < P; ++p) {
                        double t;
                        if (sc_pool_entry(a.pool, a.V, p, self, wx, wy, ux, uy, t) && t <= len) { atomicMin(&s_key, pl_key(p, lane)); break; }      // a later p is no minimum
                    }
                __syncthreads();
                key = s_key;
            }
            __syncthreads();      // s_key, s_w and s_e are free again
        }
        if (key == kPlFree) { st.x = xc; st.y = yc; st.th = thc; ++moved; }
        else {
            if (first < 0) { first = m; reason = pl_key_reason(key); edge = pl_key_edge(key); }
            ++stalled;
        }
    }
    if (lane == 0) {
        if (moved) {
            double* pose = a.pose + 3 * (size_t)b;
            pose[0] = st.x; pose[1] = st.y; pose[2] = st.th;
        }
        if (a.vel) {
            double* vel = a.vel + 3 * (size_t)b;
            vel[0] = st.v[0]; vel[1] = st.v[1]; vel[2] = st.v[2];
        }
        if (a.stall) a.stall[b] = stalled;
        if (a.info) {
            int32_t* info = a.info + 4 * (size_t)b;
            info[0] = moved; info[1] = first; info[2] = reason; info[3] = edge;
        }
    }
}

#endif  // __HIPCC__

}  // namespace mpc
