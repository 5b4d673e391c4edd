// mpc_scan_cast.hpp -- the laser scan of every robot of a batch, cast on the device through one shared map and through a pool of other bodies: the step in front of
// mpc_costmap_scans.hpp, whose ranges [B][n_beams] nothing in this library could produce so far.  Every demo of the reference takes that array from the Stage
// simulator: ex/stage/robots/carlike_robot.inc and diff_drive_robot.inc define a `ranger` (range_max 6.5, fov 58.0, samples 640, pose [-0.1 0.0 ...]) and the
// ex/stage/*.world files set laser_return 1 on the map and on the other robots.  Stage is not part of the reference's tree.  Lines marked (!) restate published source
// (Stage's ranger reports range_max for a beam without a return; laser_geometry / mpc_costmap_scans.hpp rule 3 for what the consumer does with a range) and cannot be
// verified here; lines marked OURS are a rule of ours, declared as such.
//
// The rule, per instance (pose = robot_pose[b][0..2]; res = map_resolution; a map byte v BLOCKS when block_threshold <= v <= 254, or v == 255 with unknown_blocks):
//   1. geometry: rule 3 of mpc_costmap_scans.hpp, called and not restated: heading = cs_wrap(yaw); the sensor at pose_xy + R(heading) * sensor_xy
//                (cs_place_sensor); beam k along th_k = cs_wrap(((yaw + sensor_yaw) + angle_min) + k * angle_increment); (cos, sin) = (c, s) by cs_sincos.  OURS: a pose
//                whose x, y or yaw is not finite, or a heading cs_wrap cannot bring into [-pi, pi): every beam of the instance misses, info = {-1, 0, 0, 0}.  A beam
//                angle that does not wrap: that beam misses.
//   2. map     : OURS: an exact cell traversal, no marching step.  u = (sensor_x - map_origin_x) / res, v likewise, i = floor(u), j = floor(v): the sensor's cell.  A
//                sensor whose cell is off the map (0 <= i < map_size_x and 0 <= j < map_size_y does not hold) hits nothing on the map.  When the sensor's own cell
//                blocks, t = 0.  Otherwise inv_x = 1 / c once, for c != 0 (inv_y = 1 / s), and per step the crossing parameter of the next boundary on each axis is
//                ((c > 0 ? i + 1 : i) - u) * inv_x -- recomputed from the integer index at every step, never accumulated -- and +inf for c == 0.  The walk steps
//                along the axis with the smaller parameter, x on a tie; t_in is that parameter.  The beam misses the map when t_in * res < range_max does not hold,
//                and when the cell it steps into is off the map.  (A cell more than Rc = ceil(range_max / res) + 1 cells from the sensor's on either axis also
//                ends the walk as a miss: the range test keeps the walk inside that square, the clause is there so that it provably does.)  When the cell blocks,
//                t_out is the smaller crossing parameter from the new indices, t = hit_point ? (t_in + t_out) * 0.5 : t_in, and r_map = t * res.
//                Why the chord's middle is the default: a range reported exactly on the cell's edge is put back by the consumer as sensor + (double)(float)r * dir
//                (cs_beam), on either side of the edge, and would mark the free cell in front of the wall.
//   3. pool    : the layout of mpc_pool (include/mpc_fleet.h) with V = cfg.max_vertices; nv = min(n_vertices[p], V).  Skipped: n_vertices[p] < 1, p == self_index[b],
//                a valid vertex that is not finite, a disc whose radius is not finite.  With d = centre - sensor, every product and sum rounded on its own:
//                  disc (nv == 1, radius > 0; a point without a radius returns nothing): bq = d . dir, cq = d . d - radius^2.  cq <= 0: t = 0.  Else bq <= 0 or
//                  bq^2 - cq < 0: none.  Else t = bq - sqrt(bq^2 - cq).
//                  segments (nv == 2: one segment; nv >= 3: the closed loop; the radius is ignored, OURS), e = q1 - q0, w = q0 - sensor: den = dir x e, zero: none;
//                  t = (w x e) / den, s = (w x dir) / den; a hit when t >= 0 and 0 <= s <= 1; the entry's t is the smallest over its segments.
//                r_pool is the smallest t (metres already), ties to the lower p.
//   4. result  : r = min(r_map, r_pool), the map wins a tie.  The beam misses unless r < range_max.  ranges = (float)r, or the miss value: +inf with miss_is_inf,
//                else (float)range_max (!) (Stage).  Values below the consumer's range_min are reported as they are.  hit = -2 for the map, p for a pool entry, -1
//                for a miss.
//   5. info    : {beams returned by the map, beams returned by a pool entry, beams without a return, blocking map cells within Rc cells of the sensor's cell on
//                either axis -- 0 when the sensor's cell is off the map}.
//   6. refusals: a null required pointer; n_beams outside 1 .. kScMaxBeams = 4096; map_size_x or map_size_y below 1 or their product above 2^31 - 1; map_resolution or
//                range_max not positive and finite; map_origin, sensor_pose, angle_min or angle_increment not finite; Rc above kScMaxRc; block_threshold outside
//                1 .. 254; P < 0, or P > 0 without n_vertices and vertices.
// Out of scope, and so visible deviations from Stage: no sensor noise, not Stage's own 0.02 m ray resolution, one sensor, the plant is not moved here (mpc_plant.hpp), marks are not
// inflated.
// Every double is produced by + - * /, floor and sqrt in un-fused arithmetic (and cs_sincos' explicit fmas), so a g++ build and the device round alike; a beam's
// result is a function of its own inputs, so the output depends neither on B, the place in the batch, the order of beams or the run.
//
// sc_instance is the per-instance statement (host code, serial).  scan_cast_kernel restates it for one 256-thread workgroup per instance.  Both take a beam from
// the same host / device functions (sc_frame, sc_beam_dir, sc_walk, sc_pool_entry, sc_result); they differ in where sc_walk's cell test looks: the map, or the bits
// the kernel made of it.
#pragma once
#include "mpc_costmap_scans.hpp"
#include "mpc_fleet_obstacles.hpp"

namespace mpc {

constexpr int kScThreads = 256;
constexpr int kScMaxBeams = 4096;
constexpr int kScListCap = 512;                  // pool entries the workgroup's culled list holds; what comes behind is tested from global memory
// The kernel keeps the blocking cells of the (2 Rc + 1)^2 square around the sensor's cell as bits in LDS, a row in whole 64-bit words, next to the culled list and 16
// words of counts: (2 Rc + 1) * ceil((2 Rc + 1) / 64) * 8 + 4 * kScListCap + 64 bytes (sc_lds_bytes) within the 65536 of one workgroup.  2 Rc + 1 = 703 takes 11 words a
// row, 61864 + 2112 bytes; 705 would take 12 words a row, 67680 bytes.  (6.5 m at 0.05 m is Rc = 131: 17 KB.  16 m at 0.05 m is Rc = 321: 57 KB.)
constexpr int kScMaxRc = 351;
constexpr int kScMaxLds = 65536;

// the fields of mpc_cast_params the rule reads, and Rc
struct CastParams {
    double map_ox, map_oy, res, sensor_x, sensor_y, sensor_yaw, angle_min, angle_inc, range_max;
    int32_t map_sx, map_sy, threshold, unknown_blocks, hit_point, miss_is_inf, Rc;
};

inline int sc_row_words(int Rc) { return (2 * Rc + 1 + 63) / 64; }
inline size_t sc_lds_bytes(int Rc) { return (size_t)(2 * Rc + 1) * sc_row_words(Rc) * 8 + 4 * (size_t)kScListCap + 64; }
static_assert((2 * kScMaxRc + 1) * ((2 * kScMaxRc + 1 + 63) / 64) * 8 + 4 * kScListCap + 64 <= kScMaxLds, "the cap fits one workgroup's LDS");
static_assert((2 * kScMaxRc + 3) * ((2 * kScMaxRc + 3 + 63) / 64) * 8 + 4 * kScListCap + 64 > kScMaxLds, "and is the largest that does");

// rule 6's Rc from the parameters: -1 when it is above kScMaxRc or not a number
inline int sc_cells(double range_max, double res) {
    const double rd = __builtin_ceil(range_max / res) + 1.0;
    if (!(rd <= (double)kScMaxRc)) return -1;
    return rd > 1.0 ? (int)rd : 1;
}

MPC_CM_HD bool sc_blocks(uint8_t v, int threshold, int unknown_blocks) { return ((int)v >= threshold && v <= kLethal) || (unknown_blocks && v == 255); }

// what the instance's beams share (rules 1 and 2)
struct CastFrame {
    double sx, sy, u, v;      // the sensor in the world and in cells of the map
    int32_t i0, j0;           // the sensor's cell, when on_map
    bool valid, on_map;       // rule 1; the sensor's cell lies on the map
};

MPC_CM_HD CastFrame sc_frame(const CastParams& p, const double* pose) {
#pragma clang fp contract(off)
    CastFrame f;
    f.sx = f.sy = f.u = f.v = 0.0;
    f.i0 = f.j0 = 0;
    f.on_map = false;
    f.valid = fo_finite(pose[0]) && fo_finite(pose[1]) && fo_finite(pose[2]);
    if (!f.valid) return f;
    const double th = cs_wrap(pose[2]);
    f.valid = cs_wrapped(th);
    if (!f.valid) return f;
    cs_place_sensor(pose[0], pose[1], th, p.sensor_x, p.sensor_y, f.sx, f.sy);
    const double dx = f.sx - p.map_ox, dy = f.sy - p.map_oy;
    f.u = dx / p.res;
    f.v = dy / p.res;
    const double fi = __builtin_floor(f.u), fj = __builtin_floor(f.v);
    f.on_map = fi >= 0.0 && fi < (double)p.map_sx && fj >= 0.0 && fj < (double)p.map_sy;      // false for a NaN
    if (f.on_map) { f.i0 = (int32_t)fi; f.j0 = (int32_t)fj; }
    return f;
}

// rule 1: the direction of beam k; false when its angle does not wrap
MPC_CM_HD bool sc_beam_dir(const CastParams& p, double yaw, int k, double& c, double& s) {
#pragma clang fp contract(off)
    const double a0 = yaw + p.sensor_yaw, a1 = a0 + p.angle_min;
    const double turn = (double)k * p.angle_inc;
    const double th = cs_wrap(a1 + turn);
    c = 1.0; s = 0.0;
    if (!cs_wrapped(th)) return false;
    cs_sincos(th, s, c);
    return true;
}

// rule 2: the crossing parameter of the next boundary on one axis, from the integer index
MPC_CM_HD double sc_cross(double c, int i, double u, double inv) {
#pragma clang fp contract(off)
    if (c == 0.0) return __builtin_inf();
    const double edge = (double)(c > 0.0 ? i + 1 : i);
    const double d = edge - u;
    return d * inv;
}

// rule 2: r_map of the beam along (c, s), +inf when the map returns nothing.  blocks(i, j): whether cell (i, j) -- on the map, within Rc of the sensor's -- blocks.
template <typename Blocks>
MPC_CM_HD double sc_walk(const CastParams& p, const CastFrame& f, double c, double s, Blocks blocks) {
#pragma clang fp contract(off)
    const double none = __builtin_inf();
    if (!f.on_map) return none;
    int i = f.i0, j = f.j0;
    if (blocks(i, j)) return 0.0 * p.res;
    const double inv_x = c != 0.0 ? 1.0 / c : 0.0, inv_y = s != 0.0 ? 1.0 / s : 0.0;
    const int di = c > 0.0 ? 1 : -1, dj = s > 0.0 ? 1 : -1;
    for (;;) {
        const double tx = sc_cross(c, i, f.u, inv_x), ty = sc_cross(s, j, f.v, inv_y);
        const bool along_x = tx <= ty;
        const double t_in = along_x ? tx : ty;
        if (!(t_in * p.res < p.range_max)) return none;      // (also a NaN, and c == s == 0)
        if (along_x) i += di; else j += dj;
        if (i < 0 || i >= p.map_sx || j < 0 || j >= p.map_sy) return none;
        if (i - f.i0 > p.Rc || f.i0 - i > p.Rc || j - f.j0 > p.Rc || f.j0 - j > p.Rc) return none;
        if (blocks(i, j)) {
            const double ox = sc_cross(c, i, f.u, inv_x), oy = sc_cross(s, j, f.v, inv_y);
            const double t_out = ox <= oy ? ox : oy;
            const double mid = (t_in + t_out) * 0.5;
            const double t = p.hit_point ? mid : t_in;
            return t * p.res;
        }
    }
}

// rule 3: pool entry p against the beam from (sx, sy) along (c, s): true with its t when it returns the beam
MPC_CM_HD bool sc_pool_entry(const FleetPool& pool, int V, int p, int self, double sx, double sy, double c, double s, double& t_hit) {
#pragma clang fp contract(off)
    int nv = pool.n_vertices[p];
    if (nv < 1 || p == self) return false;
    if (nv > V) nv = V;
    const double* q = pool.vertices + (size_t)p * V * 2;
    for (int j = 0; j < nv; ++j) if (!fo_finite(q[2 * j]) || !fo_finite(q[2 * j + 1])) return false;
    if (nv == 1) {
        const double rad = pool.radius ? pool.radius[p] : 0.0;
        if (!fo_finite(rad) || !(rad > 0.0)) return false;
        const double dx = q[0] - sx, dy = q[1] - sy;
        const double bx = dx * c, by = dy * s;
        const double bq = bx + by;
        const double xx = dx * dx, yy = dy * dy;
        const double dd = xx + yy, rr = rad * rad;
        const double cq = dd - rr;
        if (cq <= 0.0) { t_hit = 0.0; return true; }
        if (bq <= 0.0) return false;
        const double b2 = bq * bq;
        const double disc = b2 - cq;
        if (disc < 0.0) return false;
        const double t = bq - __builtin_sqrt(disc);
        if (!(t >= 0.0)) return false;      // (a NaN of inf - inf; a rounded sqrt is never above bq)
        t_hit = t;
        return true;
    }
    bool any = false;
    double best = 0.0;
    const int segments = nv == 2 ? 1 : nv;
    for (int j = 0; j < segments; ++j) {
        const int j1 = j + 1 < nv ? j + 1 : 0;
        const double ax = q[2 * j], ay = q[2 * j + 1];
        const double ex = q[2 * j1] - ax, ey = q[2 * j1 + 1] - ay;
        const double wx = ax - sx, wy = ay - sy;
        const double d0 = c * ey, d1 = s * ex;
        const double den = d0 - d1;
        if (den == 0.0) continue;
        const double n0 = wx * ey, n1 = wy * ex;
        const double t = (n0 - n1) / den;
        const double m0 = wx * s, m1 = wy * c;
        const double sp = (m0 - m1) / den;
        if (t >= 0.0 && sp >= 0.0 && sp <= 1.0 && (!any || t < best)) { any = true; best = t; }
    }
    t_hit = best;
    return any;
}

// rule 4: the beam's range word and its hit word from r_map and the nearest pool entry (r_pool = +inf, pool_p = -1 for none)
MPC_CM_HD float sc_result(const CastParams& p, double r_map, double r_pool, int pool_p, int32_t& hit) {
    const bool map_wins = r_map <= r_pool;
    const double r = map_wins ? r_map : r_pool;
    if (!(r < p.range_max)) { hit = -1; return p.miss_is_inf ? __builtin_inff() : (float)p.range_max; }
    hit = map_wins ? -2 : pool_p;
    return (float)r;
}

// Whether pool entry p can return a beam of a sensor at (sx, sy): the kernel's culling test, which only has to err on the side of keeping.  A point of a segment lies within half
// the segment's length of one of its ends, a point of a disc within its radius of the centre; 1e-6 of slack covers the rounding of the squares.  What rule 3 skips is
// dropped here too; a sum that overflows compares as it may.
MPC_CM_HD bool sc_may_reach(const FleetPool& pool, int V, int p, int self, double sx, double sy, double range_max) {
#pragma clang fp contract(off)
    int nv = pool.n_vertices[p];
    if (nv < 1 || p == self) return false;
    if (nv > V) nv = V;
    const double* q = pool.vertices + (size_t)p * V * 2;
    double near2 = __builtin_inf(), edge2 = 0.0;
    for (int j = 0; j < nv; ++j) {
        const double dx = q[2 * j] - sx, dy = q[2 * j + 1] - sy;
        const double d2 = dx * dx + dy * dy;
        if (!(d2 >= near2)) near2 = d2;      // a NaN is kept: rule 3 decides
        const int j1 = j + 1 < nv ? j + 1 : 0;
        const double ex = q[2 * j1] - q[2 * j], ey = q[2 * j1 + 1] - q[2 * j + 1];
        const double e2 = ex * ex + ey * ey;
        if (!(e2 <= edge2)) edge2 = e2;
    }
    const double rad = nv == 1 ? (pool.radius ? pool.radius[p] : 0.0) : 0.5 * __builtin_sqrt(edge2);
    const double reach = (range_max + rad) * 1.000001 + 1e-9;
    return !(near2 > reach * reach);
}

// ---- the statement (host).  ranges: n_beams floats; hit: n_beams words or NULL; info: 4 words or NULL.  pool.P == 0: no pool.
inline void sc_instance(const CastParams& p, const uint8_t* map, const FleetPool& pool, int V, int self, const double* pose, int n_beams, float* ranges, int32_t* hit,
                        int32_t* info) {
    const CastFrame f = sc_frame(p, pose);
    int n_map = 0, n_pool = 0, n_miss = 0, n_cells = 0;
    auto blocks = [&](int i, int j) { return sc_blocks(map[(size_t)j * p.map_sx + i], p.threshold, p.unknown_blocks); };
    for (int k = 0; k < n_beams; ++k) {
        int32_t h = -1;
        float r = p.miss_is_inf ? __builtin_inff() : (float)p.range_max;
        double c, s;
        if (f.valid && sc_beam_dir(p, pose[2], k, c, s)) {
            const double r_map = sc_walk(p, f, c, s, blocks);
            double r_pool = __builtin_inf();
            int pool_p = -1;
            for (int e = 0; e < pool.P; ++e) {
                double t;
                if (sc_pool_entry(pool, V, e, self, f.sx, f.sy, c, s, t) && t < r_pool) { r_pool = t; pool_p = e; }
            }
            r = sc_result(p, r_map, r_pool, pool_p, h);
        }
        ranges[k] = r;
        if (hit) hit[k] = h;
        n_map += h == -2; n_pool += h >= 0; n_miss += h == -1;
    }
    if (f.valid && f.on_map)
        for (int j = f.j0 - p.Rc; j <= f.j0 + p.Rc; ++j)
            for (int i = f.i0 - p.Rc; i <= f.i0 + p.Rc; ++i)
                if (i >= 0 && i < p.map_sx && j >= 0 && j < p.map_sy) n_cells += blocks(i, j) ? 1 : 0;
    if (info) { info[0] = f.valid ? n_map : -1; info[1] = f.valid ? n_pool : 0; info[2] = f.valid ? n_miss : 0; info[3] = n_cells; }
}

#if defined(__HIPCC__)

struct CastArgs {
    const uint8_t* map;           // [map_sy][map_sx], shared by every instance
    const double* pose;           // [B][3]
    FleetPool pool;               // P == 0: none
    const int32_t* self_index;    // [B] or NULL
    float* ranges;                // [B][n_beams]
    int32_t* hit;                 // [B][n_beams] or NULL
    int32_t* info;                // [B][4] or NULL
    CastParams p;
    int32_t n_beams, V;
};
static_assert(std::is_trivially_copyable<CastArgs>::value, "a kernel argument");

// One workgroup (256 threads) per instance.  Dynamic LDS (sc_lds_bytes): the bitmap, the culled list, 16 words of counts.
//   bitmap : (sensor on the map) the square of 2 Rc + 1 map cells around the sensor's cell, a wave per row and a lane per byte: neighbouring lanes read neighbouring
//            map bytes, neighbouring instances read the same map out of L2.  A 64-bit ballot of the blocking bytes is one word of the row; rule 5's count is the sum of
//            their popcounts.  The words of a row are loaded back to back before the first ballot, so that a wave has a row's loads in flight.
//   cull   : the pool in chunks of 256 consecutive entries, thread t on entry c0 + t; the entries sc_may_reach keeps go to the list in pool order (ballot and popcount
//            prefix).  The first chunk that would not fit ends the culling: `tail` is its first entry, and the beams test every entry from there on from global memory.
//   beams  : a lane per beam, a wave's 64 beams in step: sc_walk on the LDS bits, sc_pool_entry on the listed entries and on the tail -- in increasing p either
//            way, so the nearest entry and its tie rule are the statement's --, one 4-byte store to ranges and one to hit, neighbouring lanes on neighbouring words.  The
//            counts of rule 5 by ballot and popcount per wave, by LDS atomics across waves.
// The only private arrays are the four bytes and flags of the bitmap's loads, indexed by unrolled constants; plain vector stores and LDS only.
__global__ __launch_bounds__(kScThreads) void scan_cast_kernel(CastArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t sc_smem[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.x, Rc = a.p.Rc, side = 2 * Rc + 1, wpr = (side + 63) >> 6;
    unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(sc_smem);
    int* s_list = reinterpret_cast<int*>(sc_smem + (size_t)side * wpr * 8);
    int* s_cnt = s_list + kScListCap;      // map, pool, miss, cells; [4 .. 7]: the culling's wave counts
    const double* pose = a.pose + 3 * (size_t)b;
    const double pose3[3] = {pose[0], pose[1], pose[2]};
    const CastFrame f = sc_frame(a.p, pose3);      // workgroup-uniform
    const int self = a.self_index ? a.self_index[b] : -1;
    if (t < 16) s_cnt[t] = 0;
    __syncthreads();
    // ---- bitmap
    if (f.valid && f.on_map) {
        int n_cells = 0;      // wave-uniform
        const int i_first = f.i0 - Rc, j_first = f.j0 - Rc;
        for (int row = wave; row < side; row += kScThreads / 64) {
            const int j = j_first + row;
            const bool row_in = j >= 0 && j < a.p.map_sy;
            const uint8_t* src = a.map + (size_t)(row_in ? j : 0) * (size_t)a.p.map_sx;
            for (int w0 = 0; w0 < wpr; w0 += 4) {
                uint8_t v[4];
                bool in[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = 64 * (w0 + q) + lane, i = i_first + col;
                    in[q] = row_in && w0 + q < wpr && col < side && i >= 0 && i < a.p.map_sx;
                    v[q] = 0;
                    if (in[q]) v[q] = src[i];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (w0 + q >= wpr) break;      // wave-uniform
                    const unsigned long long bits = __ballot(in[q] && sc_blocks(v[q], a.p.threshold, a.p.unknown_blocks));
                    if (lane == 0) s_bits[row * wpr + w0 + q] = bits;
                    n_cells += __popcll(bits);
                }
            }
        }
        if (lane == 0 && n_cells) atomicAdd(&s_cnt[3], n_cells);
    }
    // ---- cull
    int listed = 0, tail = 0;      // workgroup-uniform
    if (f.valid) {
        const int P = a.pool.P;
        tail = P;
        for (int c0 = 0; c0 < P; c0 += kScThreads) {
            const int p = c0 + t;
            const bool keep = p < P && sc_may_reach(a.pool, a.V, p, self, f.sx, f.sy, a.p.range_max);
            const unsigned long long m = __ballot(keep);
            if (lane == 0) s_cnt[4 + wave] = __popcll(m);
            __syncthreads();
            int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int w = 0; w < kScThreads / 64; ++w) { const int n = s_cnt[4 + w]; before += w < wave ? n : 0; total += n; }
            __syncthreads();      // the wave counts are free again
            if (listed + total > kScListCap) { tail = c0; break; }
            if (keep) s_list[listed + before] = p;
            listed += total;
        }
    }
    __syncthreads();
    // ---- beams
    {
        float* ranges = a.ranges + (size_t)b * a.n_beams;
        int32_t* hits = a.hit ? a.hit + (size_t)b * a.n_beams : nullptr;
        const float miss = a.p.miss_is_inf ? __builtin_inff() : (float)a.p.range_max;
        const int i_first = f.i0 - Rc, j_first = f.j0 - Rc;
        auto blocks = [&](int i, int j) {
            const int col = i - i_first, row = j - j_first;      // 0 <= col, row < side: sc_walk stays within Rc of the sensor's cell
            return ((s_bits[row * wpr + (col >> 6)] >> (col & 63)) & 1ull) != 0ull;
        };
        int n_map = 0, n_pool = 0, n_miss = 0;      // wave-uniform
        for (int k = t; k - lane < a.n_beams; k += kScThreads) {
            const bool act = k < a.n_beams;
            int32_t h = -1;
            float r = miss;
            double c, s;
            if (act && f.valid && sc_beam_dir(a.p, pose3[2], k, c, s)) {
                const double r_map = sc_walk(a.p, f, c, s, blocks);
                double r_pool = __builtin_inf();
                int pool_p = -1;
                for (int e = 0; e < listed; ++e) {
                    const int p = s_list[e];
                    double tp;
                    if (sc_pool_entry(a.pool, a.V, p, self, f.sx, f.sy, c, s, tp) && tp < r_pool) { r_pool = tp; pool_p = p; }
                }
                for (int p = tail; p < a.pool.P; ++p) {
                    double tp;
                    if (sc_pool_entry(a.pool, a.V, p, self, f.sx, f.sy, c, s, tp) && tp < r_pool) { r_pool = tp; pool_p = p; }
                }
                r = sc_result(a.p, r_map, r_pool, pool_p, h);
            }
            if (act) {
                ranges[k] = r;
                if (hits) hits[k] = h;
            }
            n_map += __popcll(__ballot(act && h == -2));
            n_pool += __popcll(__ballot(act && h >= 0));
            n_miss += __popcll(__ballot(act && h == -1));
        }
        if (lane == 0) {
            if (n_map) atomicAdd(&s_cnt[0], n_map);
            if (n_pool) atomicAdd(&s_cnt[1], n_pool);
            if (n_miss) atomicAdd(&s_cnt[2], n_miss);
        }
    }
    __syncthreads();
    if (t == 0 && a.info) {
        int32_t* info = a.info + 4 * (size_t)b;
        info[0] = f.valid ? s_cnt[0] : -1;
        info[1] = f.valid ? s_cnt[1] : 0;
        info[2] = f.valid ? s_cnt[2] : 0;
        info[3] = s_cnt[3];
    }
}

#endif  // __HIPCC__

}  // namespace mpc
