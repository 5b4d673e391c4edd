// mpc_costmap_scans.hpp -- the laser-scan obstacle layer of every robot of a batch, kept on the device between cycles: the step between mpc_costmap_window.hpp, which
// cuts the local costmap from the static map alone, and the costmap converters.  Both shipped local costmaps (cfg/*/local_costmap_params.yaml) list a
// costmap_2d::StaticLayer AND a costmap_2d::ObstacleLayer (cfg/*/costmap_common_params.yaml: obstacle_range 3.0, raytrace_range 4.0 / 3.5, track_unknown_space true,
// combination_method 1, one LaserScan source, marking and clearing): the reference's planner avoids what the laser sees.  costmap_2d is not part of the reference's
// tree.  Lines marked (!) restate its published source (ROS navigation 1.17: obstacle_layer.cpp, costmap_2d.cpp / .h, costmap_layer.cpp) or
// laser_geometry's range test and cannot be verified here; lines marked OURS are a rule of ours, declared as such.
//
// The state of the layer is the caller's: layer [B][H][W] bytes and layer_cell [B][2], the lattice index of the window origin the layer was last written for.
// The rule, per instance (pose = robot_pose[b][0..2]; W = size_x, H = size_y; res = resolution; def = track_unknown ? 255 : 0, the value of an untouched cell (!)):
//   1. origin  : rule 1 of mpc_costmap_window.hpp, the same arithmetic per axis (cs_origin_axis restates cw_origin_axis and also keeps the integer index c; the host
//                test holds the two origins equal).  An instance whose pose_x, pose_y or yaw is not finite, or for which |cx| < 2^30 or |cy| < 2^30 does not hold, is
//                INVALID: its layer is def throughout, layer_cell = {0, 0}, its cost is left as it was, info = {-1, 0, 0, 0}.
//   2. roll    : with keep, new(x, y) = old(x + (cx - layer_cell_x), y + (cy - layer_cell_y)), def where that lies outside the old layer; a shift of a window or more
//                on either axis empties the layer.  costmap_2d::updateOrigin (!) derives the shift from doubles; OURS is exact in integers (64-bit: layer_cell is the
//                caller's word), because the origins lie on the lattice.  Without keep the layer is def throughout and layer_cell is not read.  Then layer_cell = (cx, cy).
//   3. beams   : heading = cs_wrap(yaw); the sensor sits at pose_xy + R(heading) * sensor_xy, every product and sum rounded on its own.  Beam k has the angle
//                cs_wrap(((yaw + sensor_yaw) + angle_min) + k * angle_increment).  cs_wrap is normalize_theta (include/mpc_local_planner/utils/math_utils.h:81-91) in
//                the form the device compiles (a multiplication by 1 / (2 pi)), stated once for both sides.  OURS: an angle it cannot bring into [-pi, pi) -- a
//                heading so large that one unit in its last place exceeds a turn -- drops the beam; when the heading itself is such, no beam is kept.
//                The range is ranges[b][k] converted to double; +inf becomes range_max - 1e-4 when inf_is_valid (!).  A NaN, a range below range_min or one at or
//                above range_max drops the beam (!) (laser_geometry).  The endpoint is sensor + range * (cos, sin), products and sums rounded on their own.
//                cs_sincos is sincos_reduced of mpc_core.hpp with its contraction written out: that function is compiled under the device's default contraction,
//                which fuses z * z * pc into the sum in front of it, and a g++ build does not.  Here every fused operation is an explicit __builtin_fma and
//                contraction is off for the rest, so that a g++ host build and the device round alike.  No libm sin, cos or hypot.
//   4. clear   : (clearing != 0, every kept beam) from the sensor's lattice cell to the endpoint's, cells floor((w - origin) / res) on the window's lattice, which may
//                leave the window.  The walk is costmap_2d's bresenham2D (!): the major axis a is the one with the larger |d|, x on a tie; error = da / 2; visit, then
//                step along a, add db to the error and step along b when it reaches da; visit once more after the last step.  Every visited cell inside the window
//                becomes 0.  The number of steps is da when dx^2 + dy^2 <= R^2, R = max(0, ceil(raytrace_range / res)) (!) (cellDistance); otherwise the largest
//                integer m with m^2 (dx^2 + dy^2) <= R^2 da^2, in 64-bit integers.  OURS: costmap_2d takes (unsigned)(min(1, R / hypot(dx, dy)) * da) in doubles, which
//                can land one below the exact value where R da / hypot is an integer.  OURS: costmap_2d clips the endpoint to the window first and walks the
//                clipped line; here the line is walked in full and writes outside the window are dropped.  When the sensor's own cell lies outside the window,
//                nothing is cleared (!).
//   5. mark    : (marking != 0, after all clearing) the endpoint p is kept when (p - sensor)^2 < obstacle_range^2 (!) and its cell lies in the window
//                (Costmap2D::worldToMap (!)); that cell becomes 254.  Then, when footprint_clear_radius > 0, layer cells whose centre (cm_world) lies within that
//                distance of (pose_x, pose_y), squared and compared with <=, become 0.  OURS: a disc where costmap_2d clears the footprint polygon.
//   6. combine : (cost given) per cell with layer value l and window value s: l == 255: s stays.  Method 1 (updateWithMax (!)): s = l when s == 255 or s < l.
//                Method 0 (updateWithOverwrite (!)): s = l.
//   7. info    : {beams kept, layer cells equal to 254 after the call, layer cells equal to 0 after the call, window cells the combination changed}.
//   8. refusals: a null required pointer; n_beams below 1 or above kCsMaxBeams = 4096; W or H below 1, W * H above kCsMaxCells = 65536; res not positive and finite;
//                range_min, range_max, obstacle_range or raytrace_range negative or not finite; R above kCsMaxR = 4096; range_max / res at or above 2^15; an angle or
//                a sensor pose that is not finite; a footprint_clear_radius that is not a number; a combination_method other than 0 or 1.
// Phases 4, 5 and the disc each write a single value, so the result depends neither on the order of beams or threads, nor on B, the position in the batch or the run.
// Marks are not inflated: the shipped local costmaps have no inflation layer; a window cut with inflation_radius > 0 keeps the inflation of its static cells only.
//
// cs_instance is the per-instance statement (host code, serial).  costmap_scans_kernel restates it for one 256-thread workgroup per instance with the layer in LDS.
// Both take rules 1, 3, 4's walk, 5's tests and 6 from the same host / device functions (cs_origin_axis, cs_beam, cs_steps, cs_walk, cs_in_disc, cs_combine).
#pragma once
#include "mpc_costmap.hpp"

#include <stddef.h>
#include <type_traits>
#include <vector>

namespace mpc {

constexpr int kCsThreads = 256;
constexpr int kCsMaxBeams = 4096;
constexpr int kCsMaxCells = 65536;               // the layer of an instance stays in the LDS of one workgroup
constexpr int kCsMaxR = 4096;                    // the longest cleared ray, cells
constexpr double kCsMaxRangeCells = 32768.0;     // range_max / res at or above this is refused: the differences of a walk fit 17 bits, its products 64

// the fields of mpc_scan_params the rule reads, the resolution, R and def
struct ScanParams {
    double anchor_x, anchor_y, res;
    double sensor_x, sensor_y, sensor_yaw, angle_min, angle_inc, range_min, range_max, obstacle_range, clear_radius;
    int32_t marking, clearing, inf_is_valid, method, R, def;
};

// rule 1 on one axis: cw_origin_axis's statement, which also keeps the integer index; false for an invalid instance
MPC_CM_HD bool cs_origin_axis(double pose, int size, double res, double anchor, double& origin, int32_t& cell) {
#pragma clang fp contract(off)
    const double s = ((double)(size - 1) + 0.5) * res;
    const double half = s / 2;
    const double a = pose - half;
    const double q = (a - anchor) / res;
    const double c = __builtin_floor(q);
    if (!(__builtin_fabs(pose) < __builtin_inf()) || !(__builtin_fabs(c) < 1073741824.0)) return false;
    const double off = c * res;
    origin = anchor + off;
    cell = (int32_t)c;
    return true;
}

// rule 3: normalize_theta in the device's form; the caller tests the result against [-pi, pi)
MPC_CM_HD double cs_wrap(double th) {
#pragma clang fp contract(off)
    const double pi = 3.14159265358979323846, two_pi = 6.28318530717958647692;
    if (th >= -pi && th < pi) return th;
    const double m = __builtin_floor(th * 0.15915494309189533577);
    const double turns = m * two_pi;
    th = th - turns;
    if (th >= pi) th = th - two_pi;
    if (th < -pi) th = th + two_pi;
    return th;
}
MPC_CM_HD bool cs_wrapped(double th) { return th >= -3.14159265358979323846 && th < 3.14159265358979323846; }

// rule 3: sine and cosine of an angle in [-pi, pi): the operations of sincos_reduced (mpc_core.hpp), every fused one an explicit fma, nothing else contracted
MPC_CM_HD void cs_sincos(double x, double& sn, double& cs) {
#pragma clang fp contract(off)
    const double k = __builtin_rint(x * 6.36619772367581382433e-01);
    double r = __builtin_fma(-k, 1.57079632673412561417e+00, x);
    r = __builtin_fma(-k, 6.07710050650619224932e-11, r);
    const double z = r * r;
    double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
    ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
    ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
    ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
    ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
    const double zr = z * r;
    const double s = __builtin_fma(zr, ps, r);
    double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
    pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
    pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
    pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
    pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
    const double hz = 0.5 * z;
    const double wv = 1.0 - hz;
    const double zz = z * z;
    const double tail = zz * pc;
    const double lost = (1.0 - wv) - hz;
    const double corr = lost + tail;
    const double c = wv + corr;
    const int q = (int)k & 3;      // |k| <= 2
    const double s1 = (q & 1) ? c : s, c1 = (q & 1) ? s : c;
    sn = (q & 2) ? -s1 : s1;
    cs = ((q + 1) & 2) ? -c1 : c1;
}

// the lattice cell of the world coordinate w on one axis, as a double: floor((w - origin) / res); inside the window when 0 <= cell < size
MPC_CM_HD double cs_cell(double w, double origin, double res) {
#pragma clang fp contract(off)
    const double d = w - origin;
    return __builtin_floor(d / res);
}
MPC_CM_HD bool cs_inside(double cell, int size) { return cell >= 0.0 && cell < (double)size; }

// rule 3: the sensor of a robot at (px, py) with the wrapped heading th: pose_xy + R(th) * sensor_xy, every product and sum rounded on its own (mpc_scan_cast.hpp
// places its sensor by the same lines)
MPC_CM_HD void cs_place_sensor(double px, double py, double th, double sensor_x, double sensor_y, double& sx, double& sy) {
#pragma clang fp contract(off)
    double sn, cs;
    cs_sincos(th, sn, cs);
    const double xa = cs * sensor_x, xb = sn * sensor_y, ya = sn * sensor_x, yb = cs * sensor_y;
    const double rx = xa - xb, ry = ya + yb;
    sx = px + rx;
    sy = py + ry;
}

// what the instance's beams share: the origin and the sensor (rule 3), the sensor's cell when it lies in the window (rule 4)
struct ScanFrame {
    double ox, oy, sx, sy;
    int32_t cx, cy, scx, scy;      // the lattice index of the origin; the sensor's cell
    bool valid, heading, sensor_in;      // rule 1; the heading wraps; the sensor's cell lies in the window
};

MPC_CM_HD ScanFrame cs_frame(const ScanParams& p, const double* pose, int W, int H) {
#pragma clang fp contract(off)
    ScanFrame f;
    f.ox = f.oy = f.sx = f.sy = 0.0;
    f.cx = f.cy = f.scx = f.scy = 0;
    f.heading = f.sensor_in = false;
    const bool okx = cs_origin_axis(pose[0], W, p.res, p.anchor_x, f.ox, f.cx), oky = cs_origin_axis(pose[1], H, p.res, p.anchor_y, f.oy, f.cy);
    f.valid = okx && oky && __builtin_fabs(pose[2]) < __builtin_inf();
    if (!f.valid) return f;
    const double th = cs_wrap(pose[2]);
    f.heading = cs_wrapped(th);
    if (!f.heading) return f;
    cs_place_sensor(pose[0], pose[1], th, p.sensor_x, p.sensor_y, f.sx, f.sy);
    const double fx = cs_cell(f.sx, f.ox, p.res), fy = cs_cell(f.sy, f.oy, p.res);
    f.sensor_in = cs_inside(fx, W) && cs_inside(fy, H);
    if (f.sensor_in) { f.scx = (int32_t)fx; f.scy = (int32_t)fy; }
    return f;
}

// one beam (rule 3) and what rules 4 and 5 take from it
struct ScanBeam {
    bool kept;          // counted in info[0]
    bool mark;          // rule 5: closer than obstacle_range and its cell in the window
    int32_t ex, ey;     // the endpoint's lattice cell: meaningful when the sensor's cell lies in the window (then it is within 2^15 + 1 cells of it), or when mark
};

MPC_CM_HD ScanBeam cs_beam(const ScanParams& p, const ScanFrame& f, double yaw, float range, int k, int W, int H) {
#pragma clang fp contract(off)
    ScanBeam b;
    b.kept = b.mark = false;
    b.ex = b.ey = 0;
    if (!f.heading) return b;
    double r = (double)range;
    if (p.inf_is_valid && r == __builtin_inf()) r = p.range_max - 1e-4;
    if (!(r >= p.range_min) || !(r < p.range_max)) return b;      // a NaN fails the first test
    const double a0 = yaw + p.sensor_yaw, a1 = a0 + p.angle_min;
    const double turn = (double)k * p.angle_inc;
    const double th = cs_wrap(a1 + turn);
    if (!cs_wrapped(th)) return b;
    b.kept = true;
    double sn, cs;
    cs_sincos(th, sn, cs);
    const double lx = r * cs, ly = r * sn;
    const double px = f.sx + lx, py = f.sy + ly;
    const double fx = cs_cell(px, f.ox, p.res), fy = cs_cell(py, f.oy, p.res);
    const bool in = cs_inside(fx, W) && cs_inside(fy, H);
    if (in || f.sensor_in) { b.ex = (int32_t)fx; b.ey = (int32_t)fy; }      // |fx - scx| <= range_max / res + 2 < 2^15 + 2 when the sensor is in the window
    const double dx = px - f.sx, dy = py - f.sy;
    const double xx = dx * dx, yy = dy * dy;
    const double lim = p.obstacle_range * p.obstacle_range;
    b.mark = in && (xx + yy) < lim;
    return b;
}

// rule 4: the steps of the walk over (dx, dy) cells under R
MPC_CM_HD int cs_steps(int dx, int dy, int R) {
    const long long adx = dx < 0 ? -(long long)dx : dx, ady = dy < 0 ? -(long long)dy : dy, da = adx >= ady ? adx : ady;
    const long long d2 = adx * adx + ady * ady, lim = (long long)R * R;
    if (d2 <= lim) return (int)da;
    const long long rhs = lim * da * da;      // < 2^24 * 2^31
    long long lo = 0, hi = da;                // lo^2 d2 <= rhs < (hi)^2 d2: d2 > R^2 puts da itself beyond
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (mid * mid * d2 <= rhs) lo = mid; else hi = mid;
    }
    return (int)lo;
}

// rule 4: costmap_2d's bresenham2D from (x0, y0) over (dx, dy), n steps; visit(x, y) on every cell, the last one included
template <typename Visit>
MPC_CM_HD void cs_walk(int x0, int y0, int dx, int dy, int n, Visit visit) {
    const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
    const int sx = dx > 0 ? 1 : dx < 0 ? -1 : 0, sy = dy > 0 ? 1 : dy < 0 ? -1 : 0;
    const bool xmajor = adx >= ady;
    const int da = xmajor ? adx : ady, db = xmajor ? ady : adx;
    int err = da / 2, x = x0, y = y0;
    for (int i = 0; i < n; ++i) {
        visit(x, y);
        if (xmajor) x += sx; else y += sy;
        err += db;
        if (err >= da) { if (xmajor) y += sy; else x += sx; err -= da; }
    }
    visit(x, y);
}

// rule 5: the centre of cell (i, j) within rad of the robot's position
MPC_CM_HD bool cs_in_disc(const ScanFrame& f, int i, int j, double res, double px, double py, double rad) {
#pragma clang fp contract(off)
    const double dx = cm_world(f.ox, i, res) - px, dy = cm_world(f.oy, j, res) - py;
    const double xx = dx * dx, yy = dy * dy;
    return (xx + yy) <= rad * rad;
}

// rule 6: the window byte s under the layer byte l
MPC_CM_HD uint8_t cs_combine(uint8_t s, uint8_t l, int method) {
    if (l == 255) return s;
    if (method == 0) return l;
    return (s == 255 || s < l) ? l : s;
}

// rule 8's R from the parameters: -1 when it is above kCsMaxR or not a number
inline int cs_ray_cells(double raytrace_range, double res) {
    const double rd = __builtin_ceil(raytrace_range / res);
    if (!(rd <= (double)kCsMaxR)) return -1;
    return rd > 0.0 ? (int)rd : 0;
}

// ---- the statement (host).  layer: W * H bytes, in and out; layer_cell: 2 words, in and out; cost: W * H bytes in and out, or NULL; info: 4 words or NULL.
inline void cs_instance(const ScanParams& p, const double* pose, const float* ranges, int n_beams, bool keep, int W, int H, uint8_t* layer, int32_t* layer_cell,
                        uint8_t* cost, int32_t* info) {
    const size_t cells = (size_t)W * H;
    const uint8_t def = (uint8_t)p.def;
    const ScanFrame f = cs_frame(p, pose, W, H);
    if (!f.valid) {
        for (size_t e = 0; e < cells; ++e) layer[e] = def;
        layer_cell[0] = layer_cell[1] = 0;
        if (info) { info[0] = -1; info[1] = info[2] = info[3] = 0; }
        return;
    }
    // roll
    std::vector<uint8_t> L(cells, def);
    if (keep) {
        const long long sx = (long long)f.cx - layer_cell[0], sy = (long long)f.cy - layer_cell[1];
        if (sx > -W && sx < W && sy > -H && sy < H)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const long long xs = x + sx, ys = y + sy;
                    if (xs >= 0 && xs < W && ys >= 0 && ys < H) L[(size_t)y * W + x] = layer[(size_t)ys * W + (size_t)xs];
                }
    }
    layer_cell[0] = f.cx; layer_cell[1] = f.cy;
    // clear, then mark
    int kept = 0;
    for (int k = 0; k < n_beams; ++k) {
        const ScanBeam b = cs_beam(p, f, pose[2], ranges[k], k, W, H);
        kept += b.kept ? 1 : 0;
        if (!b.kept || !p.clearing || !f.sensor_in) continue;
        const int dx = b.ex - f.scx, dy = b.ey - f.scy;
        cs_walk(f.scx, f.scy, dx, dy, cs_steps(dx, dy, p.R), [&](int x, int y) { if (x >= 0 && x < W && y >= 0 && y < H) L[(size_t)y * W + x] = 0; });
    }
    for (int k = 0; k < n_beams && p.marking; ++k) {
        const ScanBeam b = cs_beam(p, f, pose[2], ranges[k], k, W, H);
        if (b.mark) L[(size_t)b.ey * W + b.ex] = kLethal;
    }
    if (p.clear_radius > 0.0)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (cs_in_disc(f, x, y, p.res, pose[0], pose[1], p.clear_radius)) L[(size_t)y * W + x] = 0;
    // out, combined
    int n_lethal = 0, n_free = 0, changed = 0;
    for (size_t e = 0; e < cells; ++e) {
        const uint8_t l = L[e];
        layer[e] = l;
        n_lethal += l == kLethal ? 1 : 0;
        n_free += l == 0 ? 1 : 0;
        if (cost) { const uint8_t s = cost[e], o = cs_combine(s, l, p.method); cost[e] = o; changed += o != s ? 1 : 0; }
    }
    if (info) { info[0] = kept; info[1] = n_lethal; info[2] = n_free; info[3] = changed; }
}

#if defined(__HIPCC__)

struct ScanArgs {
    const double* pose;       // [B][3]
    const float* ranges;      // [B][n_beams]
    const int32_t* keep;      // [B] or NULL
    uint8_t* layer;           // [B][H][W], in and out
    int32_t* layer_cell;      // [B][2], in and out
    uint8_t* cost;            // [B][H][W], in and out, or NULL
    int32_t* info;            // [B][4] or NULL
    ScanParams p;
    int32_t W, H, n_beams;
};
static_assert(std::is_trivially_copyable<ScanArgs>::value, "a kernel argument");

// dynamic LDS of a launch: the layer in whole 16-byte pieces, then the four counts of rule 7
inline size_t cs_lds_bytes(int W, int H) { return (((size_t)W * H + 15) & ~(size_t)15) + 16; }

// 16 bytes of a piece as four words, indexed by unrolled constants only
struct CsPiece { uint32_t w[4]; };
__device__ __forceinline__ uint32_t cs_byte(const CsPiece& q, int e) { return (q.w[e >> 2] >> (8 * (e & 3))) & 0xFFu; }

// the sum over the wave of a per-lane count below 2^13, from one ballot per bit (wave-uniform)
__device__ __forceinline__ int cs_wave_sum(int v) {
    int sum = 0;
#pragma unroll
    for (int bit = 0; bit < 13; ++bit) sum += __popcll(__ballot((v >> bit) & 1)) << bit;
    return sum;
}

// One workgroup (256 threads) per instance; the layer stays in LDS for the whole call (dynamic, cs_lds_bytes: 3 KB for the demo's 55 x 55, 64 KB at the limit).
//   load   : the roll IS the load: a thread per (row, 16 cells) reads the old layer at the shifted address -- one 16-byte load where the piece lies inside the old row
//            and its address allows it, byte loads where not -- and writes the LDS row; without keep, or for an invalid instance, def.
//   clear  : a lane per beam, a wave's 64 beams together: cs_beam, the kept beams counted by a ballot, cs_walk writing LDS bytes.
//   mark   : after a barrier, a lane per beam again (cs_beam recomputed: no per-beam state is kept across the barrier): one LDS byte.
//   disc   : after a barrier, a thread per cell of the rows the disc can reach.
//   out    : after a barrier, the layer as a flat run of 16-byte pieces, neighbouring lanes on neighbouring pieces: LDS -> the layer, and in the same sweep the
//            window's piece read, combined and written; the counts of rule 7 per lane, summed over the wave by ballots and over the waves in LDS.
// Every private array is indexed by unrolled constants; nothing is spilled.  Plain vector stores and LDS only.
__global__ __launch_bounds__(kCsThreads) void costmap_scans_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t cs_smem[];
    const int t = threadIdx.x, lane = t & 63;
    const int b = blockIdx.x, W = a.W, H = a.H, cells = W * H;
    const int padded = (cells + 15) & ~15;
    uint8_t* s_layer = cs_smem;
    int* s_cnt = reinterpret_cast<int*>(cs_smem + padded);      // kept, lethal, free, changed
    const double* pose = a.pose + 3 * (size_t)b;
    const double pose_x = pose[0], pose_y = pose[1], yaw = pose[2];
    const double pose3[3] = {pose_x, pose_y, yaw};
    const ScanFrame f = cs_frame(a.p, pose3, W, H);      // workgroup-uniform
    const uint32_t def4 = (uint32_t)a.p.def * 0x01010101u;
    uint8_t* g_layer = a.layer + (size_t)b * cells;
    // ---- load
    long long shx = 0, shy = 0;
    bool roll = f.valid && a.keep && a.keep[b] != 0;
    if (roll) {
        shx = (long long)f.cx - a.layer_cell[2 * (size_t)b];
        shy = (long long)f.cy - a.layer_cell[2 * (size_t)b + 1];
        roll = shx > -W && shx < W && shy > -H && shy < H;
    }
    if (t < 4) s_cnt[t] = 0;
    if (!roll) {
        for (int e = t; e < padded / 16; e += kCsThreads) *reinterpret_cast<uint4*>(s_layer + 16 * e) = make_uint4(def4, def4, def4, def4);
    } else {
        const int sx = (int)shx, sy = (int)shy, ppr = (W + 15) >> 4;      // pieces per row
        for (int it = t; it < H * ppr; it += kCsThreads) {
            const int y = it / ppr, x0 = (it - y * ppr) * 16;
            const int nvalid = W - x0 < 16 ? W - x0 : 16;
            const int ys = y + sy, xs0 = x0 + sx;
            CsPiece q;
            q.w[0] = q.w[1] = q.w[2] = q.w[3] = def4;
            if (ys >= 0 && ys < H) {
                const uint8_t* src = g_layer + (size_t)ys * W + xs0;      // formed only; read where 0 <= xs0 + e < W
                if (xs0 >= 0 && xs0 + 16 <= W && (reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
                    const uint4 v = *reinterpret_cast<const uint4*>(src);
                    q.w[0] = v.x; q.w[1] = v.y; q.w[2] = v.z; q.w[3] = v.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int xs = xs0 + e;
                        if (e < nvalid && xs >= 0 && xs < W) q.w[e >> 2] = (q.w[e >> 2] & ~(0xFFu << (8 * (e & 3)))) | ((uint32_t)g_layer[(size_t)ys * W + xs] << (8 * (e & 3)));
                    }
                }
            }
            uint8_t* dst = s_layer + y * W + x0;
            if (nvalid == 16 && ((y * W + x0) & 15) == 0) *reinterpret_cast<uint4*>(dst) = make_uint4(q.w[0], q.w[1], q.w[2], q.w[3]);
            else {
#pragma unroll
                for (int e = 0; e < 16; ++e) if (e < nvalid) dst[e] = (uint8_t)cs_byte(q, e);
            }
        }
    }
    __syncthreads();
    if (f.valid) {
        // ---- clear: the whole wave runs the same number of rounds
        const float* ranges = a.ranges + (size_t)b * a.n_beams;
        int kept = 0;      // wave-uniform
        for (int k = t; k - lane < a.n_beams; k += kCsThreads) {
            const bool act = k < a.n_beams;
            const ScanBeam bm = cs_beam(a.p, f, yaw, act ? ranges[k] : -1.0f, k, W, H);
            const bool is_kept = act && bm.kept;
            kept += __popcll(__ballot(is_kept));
            if (is_kept && a.p.clearing && f.sensor_in) {
                const int dx = bm.ex - f.scx, dy = bm.ey - f.scy;
                cs_walk(f.scx, f.scy, dx, dy, cs_steps(dx, dy, a.p.R), [&](int x, int y) { if (x >= 0 && x < W && y >= 0 && y < H) s_layer[y * W + x] = 0; });
            }
        }
        if (lane == 0 && kept) atomicAdd(&s_cnt[0], kept);
        __syncthreads();
        // ---- mark
        if (a.p.marking)
            for (int k = t; k < a.n_beams; k += kCsThreads) {
                const ScanBeam bm = cs_beam(a.p, f, yaw, ranges[k], k, W, H);
                if (bm.mark) s_layer[bm.ey * W + bm.ex] = kLethal;
            }
        __syncthreads();
        // ---- disc
        if (a.p.clear_radius > 0.0) {
            for (int e = t; e < cells; e += kCsThreads) {
                const int y = e / W, x = e - y * W;
                if (cs_in_disc(f, x, y, a.p.res, pose_x, pose_y, a.p.clear_radius)) s_layer[e] = 0;
            }
            __syncthreads();
        }
    }
    // ---- out
    {
        uint8_t* g_cost = a.cost && f.valid ? a.cost + (size_t)b * cells : nullptr;
        int n_lethal = 0, n_free = 0, n_changed = 0;
        for (int piece = t; 16 * piece < cells; piece += kCsThreads) {
            const int e0 = 16 * piece, nvalid = cells - e0 < 16 ? cells - e0 : 16;
            const uint4 v = *reinterpret_cast<const uint4*>(s_layer + e0);
            CsPiece l;
            l.w[0] = v.x; l.w[1] = v.y; l.w[2] = v.z; l.w[3] = v.w;
            uint8_t* dl = g_layer + e0;
            const bool wide = nvalid == 16 && (reinterpret_cast<uintptr_t>(dl) & 15u) == 0u;
            if (wide) *reinterpret_cast<uint4*>(dl) = v;
            else {
#pragma unroll
                for (int e = 0; e < 16; ++e) if (e < nvalid) dl[e] = (uint8_t)cs_byte(l, e);
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                n_lethal += e < nvalid && cs_byte(l, e) == kLethal ? 1 : 0;
                n_free += e < nvalid && cs_byte(l, e) == 0u ? 1 : 0;
            }
            if (g_cost) {
                uint8_t* dc = g_cost + e0;
                const bool cwide = nvalid == 16 && (reinterpret_cast<uintptr_t>(dc) & 15u) == 0u;
                CsPiece s, o;
                s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0u;
                if (cwide) { const uint4 c = *reinterpret_cast<const uint4*>(dc); s.w[0] = c.x; s.w[1] = c.y; s.w[2] = c.z; s.w[3] = c.w; }
                else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) if (e < nvalid) s.w[e >> 2] |= (uint32_t)dc[e] << (8 * (e & 3));
                }
                o.w[0] = o.w[1] = o.w[2] = o.w[3] = 0u;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint8_t sv = (uint8_t)cs_byte(s, e), ov = e < nvalid ? cs_combine(sv, (uint8_t)cs_byte(l, e), a.p.method) : sv;
                    n_changed += ov != sv ? 1 : 0;
                    o.w[e >> 2] |= (uint32_t)ov << (8 * (e & 3));
                }
                if (cwide) *reinterpret_cast<uint4*>(dc) = make_uint4(o.w[0], o.w[1], o.w[2], o.w[3]);
                else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) if (e < nvalid) dc[e] = (uint8_t)cs_byte(o, e);
                }
            }
        }
        // a lane holds at most 16 cells of each of its 16 pieces: below 2^13
        const int w_lethal = cs_wave_sum(n_lethal), w_free = cs_wave_sum(n_free), w_changed = cs_wave_sum(n_changed);
        if (lane == 0) {
            if (w_lethal) atomicAdd(&s_cnt[1], w_lethal);
            if (w_free) atomicAdd(&s_cnt[2], w_free);
            if (w_changed) atomicAdd(&s_cnt[3], w_changed);
        }
    }
    __syncthreads();
    if (t == 0) {
        a.layer_cell[2 * (size_t)b] = f.valid ? f.cx : 0;
        a.layer_cell[2 * (size_t)b + 1] = f.valid ? f.cy : 0;
        if (a.info) {
            int32_t* info = a.info + 4 * (size_t)b;
            info[0] = f.valid ? s_cnt[0] : -1;
            info[1] = f.valid ? s_cnt[1] : 0;
            info[2] = f.valid ? s_cnt[2] : 0;
            info[3] = f.valid ? s_cnt[3] : 0;
        }
    }
}

#endif  // __HIPCC__

}  // namespace mpc
