// mpc_costmap_window.hpp -- one shared map -> the local costmap window of every robot of a batch, on the device: the step in front of the costmap converters
// (mpc_costmap.hpp, mpc_costmap_clusters.hpp, mpc_costmap_lines.hpp), the controller cycle and the feasibility check, which all start from cost [B][size_y][size_x]
// and origin [B][2].  The shipped demos run a rolling-window local costmap (cfg/*/local_costmap_params.yaml: rolling_window true, width / height 5.5, resolution 0.1,
// a StaticLayer) over one static map (maps/*.yaml, 0.05 m per cell): a fleet shares that map, so it lies on the device once and a window is a gather plus,
// optionally, an inflation.  costmap_2d is not part of the reference's tree.  Lines marked (!) restate its published source (ROS navigation
// 1.17: costmap_2d.cpp, static_layer.cpp, inflation_layer.{h,cpp}) and cannot be verified here; lines marked OURS are a rule of ours, declared as such.
//
// The rule, per instance (pose = robot_pose[b][0..1]; W = size_x, H = size_y; res = resolution of the window; r = the inflation radius in cells, rule 3):
//   1. origin  : sx = ((W - 1) + 0.5) * res (!) (Costmap2D::getSizeInMetersX), cx = floor((pose_x - sx / 2 - anchor_x) / res), origin_x = anchor_x + cx * res; y the
//                same with H.  Every operation is rounded on its own (no fused multiply-add).  OURS: costmap_2d truncates relative to the previous origin and so
//                carries state; this origin is a function of the pose alone, on the lattice anchor + k * res.
//                An instance whose pose_x or pose_y is not finite, or for which |cx| < 2^30 or |cy| < 2^30 does not hold, is INVALID: every cell of its window is
//                outside_value, origin = anchor, info = {-1, 0, 0, 0}.
//   2. sample  : lattice cell (i, j) -- any integers, the window is 0 <= i < W, 0 <= j < H -- has its centre at (cm_world(origin_x, i, res), cm_world(origin_y, j, res)).
//                Its map cell follows Costmap2D::worldToMap (!), per axis and in the arithmetic of feas_world_to_map (mpc_feasibility.hpp): a coordinate w below
//                map_origin is outside; otherwise f = (w - map_origin) / map_resolution, outside unless f < 2147483000, the index is (int)f, outside when
//                >= map_size.  s(i, j) is the map byte map[my * map_size_x + mx], or outside_value for a cell that is outside on either axis.  Nearest-cell sampling, as
//                the StaticLayer does in a rolling window (!).  OURS: one frame, no transform.
//   3. inflate : r = ceil(inflation_radius / res) (!) (cellDistance), 0 for inflation_radius <= 0.  r = 0: cost = s.  Otherwise, for a window cell (i, j), d2 is the
//                smallest di * di + dj * dj <= r * r over the lattice cells (i + di, j + dj) with s == 254 -- the lattice reaches r cells beyond the window on every
//                side and is sampled by rule 2.  OURS: costmap_2d inflates from the cells inside the window only, and its wavefront does not always find the nearest
//                source; here the nearest is exact, in integers.  No such cell: cost = s.  Otherwise c = table[d2] and (InflationLayer::updateCosts (!))
//                    s == 255 : cost = c when (inflate_unknown ? c > 0 : c >= 253), else 255;
//                    else     : cost = max(s, c).
//   4. table   : table[d2], d2 = 0 .. r * r, is InflationLayer::computeCost (!): table[0] = 254; with d = sqrt(d2): 253 when d * res <= inscribed_radius, else
//                (unsigned char)(252 * exp(-cost_scaling_factor * (d * res - inscribed_radius))).  It is built ON THE HOST (cw_table, plain C++ with the C library's sqrt
//                and exp) inside the entry point and handed to the kernel.
//   5. info    : {window cells sampled inside the map, window cells with s == 254, window cells with cost != s, lattice cells with s == 254 in the halo only (within
//                r cells of the window on both axes, not in it)}.
//   6. refusals: a null required pointer; W or H below 1 or above kCwMaxSize = 4096, W * H > 2^20; res or map_resolution not positive and finite; map_size_x or
//                map_size_y below 1, map_size_x * map_size_y > 2^31 - 1; r > kCwMaxR = 32 (an inflation_radius that is not a number included); outside_value other
//                than 0 or 255; inscribed_radius or cost_scaling_factor negative or not finite.
// Beyond rules 1 and 2 the device does integer work only, so it equals a host build of this header bit for bit, and the output depends on neither B, the position in
// the batch nor the run.
//
// cw_instance is the per-instance statement (host code, serial).  costmap_window_kernel restates it for a 256-thread workgroup per (instance, tile of 64 x 64 window
// cells).  Both take rules 1 and 2 and the combination of rule 3 from the same host / device functions (cw_origin_axis, cw_map_index, cw_combine).
#pragma once
#include "mpc_costmap.hpp"

#include <cmath>
#include <type_traits>
#include <vector>

namespace mpc {

constexpr int kCwThreads = 256;
constexpr int kCwTileX = 64, kCwTileY = 64;      // window cells of a workgroup's tile
constexpr int kCwMaxR = 32;                      // the largest inflation radius, cells
constexpr int kCwMaxSize = 4096;                 // size_x, size_y above this are refused
constexpr int kCwMaxCells = 1 << 20;             // size_x * size_y above this is refused
constexpr int kCwSpanX = kCwTileX + 2 * kCwMaxR, kCwSpanY = kCwTileY + 2 * kCwMaxR;      // a tile with its halo
constexpr int kCwGatherRows = 4;                 // lattice rows a wave loads back to back in the gather
constexpr int kCwTableWords = (kCwMaxR * kCwMaxR + 1 + 3) / 4;                            // the table, four entries to a word
static_assert(kCwTileX == 64 && kCwSpanX <= 128, "a lattice row of a tile is one 64-bit ballot of window cells inside two 64-bit words of lethal bits");

// the fields of mpc_window_params the rule reads per cell, and r
struct WindowParams {
    double map_ox, map_oy, map_res, anchor_x, anchor_y, res;
    int32_t map_sx, map_sy, outside, inflate_unknown, r;
};

// rule 1 on one axis: false for an invalid instance
MPC_CM_HD bool cw_origin_axis(double pose, int size, double res, double anchor, double& origin) {
#pragma clang fp contract(off)
    const double s = ((double)(size - 1) + 0.5) * res;
    const double half = s / 2;
    const double a = pose - half;
    const double q = (a - anchor) / res;
    const double c = __builtin_floor(q);
    if (!(__builtin_fabs(pose) < __builtin_inf()) || !(__builtin_fabs(c) < 1073741824.0)) return false;
    const double off = c * res;
    origin = anchor + off;
    return true;
}

// rule 2 on one axis: the map index of the world coordinate w, -1 when it is outside
MPC_CM_HD int cw_map_index(double w, double map_origin, double map_res, int map_size) {
#pragma clang fp contract(off)
    if (w < map_origin) return -1;
    const double f = (w - map_origin) / map_res;
    if (!(f < 2147483000.0)) return -1;
    const int m = (int)f;
    return m < map_size ? m : -1;
}

// rule 3: the sampled byte s under the table's value c of its nearest lethal cell
MPC_CM_HD uint8_t cw_combine(uint8_t s, uint8_t c, int inflate_unknown) {
    if (s == 255) return (inflate_unknown ? c > 0 : c >= 253) ? c : (uint8_t)255;
    return s > c ? s : c;
}

// rule 3's r from the parameters: -1 when it is above kCwMaxR or not a number
inline int cw_cell_radius(double inflation_radius, double res) {
    if (inflation_radius <= 0.0) return 0;
    const double rd = std::ceil(inflation_radius / res);
    return rd <= (double)kCwMaxR ? (int)rd : -1;
}

// rule 4: table[0 .. r * r]
inline void cw_table(double res, double inscribed_radius, double cost_scaling_factor, int r, uint8_t* table) {
#pragma clang fp contract(off)
    table[0] = kLethal;
    for (int d2 = 1; d2 <= r * r; ++d2) {
        const double d = std::sqrt((double)d2);
        const double dist = d * res;
        if (dist <= inscribed_radius) { table[d2] = 253; continue; }
        const double over = dist - inscribed_radius;
        const double factor = std::exp(-cost_scaling_factor * over);
        table[d2] = (unsigned char)(252 * factor);
    }
}

// ---- the statement (host).  cost: W * H bytes; origin: 2; info: 4 words or NULL; d2_out: W * H words or NULL, rule 3's d2 per window cell, -1 where there is none.
inline void cw_instance(const WindowParams& p, const uint8_t* table, const uint8_t* map, const double* pose, int W, int H, uint8_t* cost, double* origin, int32_t* info,
                        int32_t* d2_out) {
    double ox = 0.0, oy = 0.0;
    const bool okx = cw_origin_axis(pose[0], W, p.res, p.anchor_x, ox), oky = cw_origin_axis(pose[1], H, p.res, p.anchor_y, oy);
    if (!okx || !oky) {
        for (size_t e = 0; e < (size_t)W * H; ++e) { cost[e] = (uint8_t)p.outside; if (d2_out) d2_out[e] = -1; }
        origin[0] = p.anchor_x; origin[1] = p.anchor_y;
        if (info) { info[0] = -1; info[1] = info[2] = info[3] = 0; }
        return;
    }
    origin[0] = ox; origin[1] = oy;
    const int r = p.r, EW = W + 2 * r, EH = H + 2 * r;      // the lattice with its halo: cell (i, j) at [j + r][i + r]
    std::vector<int> mx(EW), my(EH);
    for (int e = 0; e < EW; ++e) mx[e] = cw_map_index(cm_world(ox, e - r, p.res), p.map_ox, p.map_res, p.map_sx);
    for (int e = 0; e < EH; ++e) my[e] = cw_map_index(cm_world(oy, e - r, p.res), p.map_oy, p.map_res, p.map_sy);
    std::vector<uint8_t> s((size_t)EW * EH), g((size_t)EW * EH);
    int inside = 0, lethal = 0, changed = 0, halo = 0;
    for (int ej = 0; ej < EH; ++ej)
        for (int ei = 0; ei < EW; ++ei) {
            const bool in = mx[ei] >= 0 && my[ej] >= 0;
            const uint8_t v = in ? map[(size_t)my[ej] * p.map_sx + mx[ei]] : (uint8_t)p.outside;
            s[(size_t)ej * EW + ei] = v;
            const bool window = ei >= r && ei < r + W && ej >= r && ej < r + H;
            inside += window && in ? 1 : 0;
            lethal += window && v == kLethal ? 1 : 0;
            halo += !window && v == kLethal ? 1 : 0;
        }
    // pass 1, per lattice row: the distance to the nearest lethal cell of the row, r + 1 for anything farther
    for (int ej = 0; ej < EH && r > 0; ++ej) {
        uint8_t* row = g.data() + (size_t)ej * EW;
        const uint8_t* srow = s.data() + (size_t)ej * EW;
        int run = r + 1;
        for (int ei = 0; ei < EW; ++ei) { run = srow[ei] == kLethal ? 0 : run < r + 1 ? run + 1 : r + 1; row[ei] = (uint8_t)run; }
        run = r + 1;
        for (int ei = EW - 1; ei >= 0; --ei) { run = srow[ei] == kLethal ? 0 : run < r + 1 ? run + 1 : r + 1; if (run < row[ei]) row[ei] = (uint8_t)run; }
    }
    // pass 2, per window cell: the smallest dj^2 + g(i, j + dj)^2, then the table and the combination
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) {
            const uint8_t v = s[(size_t)(j + r) * EW + i + r];
            int best = -1;
            for (int dj = -r; dj <= r && r > 0; ++dj) {
                const int gv = g[(size_t)(j + r + dj) * EW + i + r], d = dj * dj + gv * gv;
                if (d <= r * r && (best < 0 || d < best)) best = d;
            }
            const uint8_t out = best < 0 ? v : cw_combine(v, table[best], p.inflate_unknown);
            cost[(size_t)j * W + i] = out;
            changed += out != v ? 1 : 0;
            if (d2_out) d2_out[(size_t)j * W + i] = best;
        }
    if (info) { info[0] = inside; info[1] = lethal; info[2] = changed; info[3] = halo; }
}

#if defined(__HIPCC__)

struct WindowArgs {
    const uint8_t* map;       // [map_sy][map_sx], shared by every instance
    const double* pose;       // [B][3]
    uint8_t* cost;            // [B][H][W]
    double* origin;           // [B][2]
    int32_t* info;            // [B][4] or NULL; zero before the launch
    WindowParams p;
    int32_t W, H, tiles_x, ntiles, b0;      // b0: the first instance of this launch
    uint32_t table[kCwTableWords];
};
static_assert(std::is_trivially_copyable<WindowArgs>::value, "a kernel argument");

// bits n .. n + 63 of the 128-bit word (hi, lo), 0 <= n < 128
__device__ __forceinline__ unsigned long long cw_bits_from(unsigned long long lo, unsigned long long hi, int n) {
    const unsigned long long a = n < 64 ? lo >> (n & 63) : hi >> (n & 63);
    const unsigned long long b = (n & 63) && n < 64 ? hi << (64 - (n & 63)) : 0ull;
    return a | b;
}

// One workgroup (256 threads) per (instance, tile of 64 x 64 window cells); the tile's lattice region is the tile plus r cells on every side, at most 128 x 128.
//   index  : the map column of every lattice column of the region and the map row of every lattice row (rule 2 is separable) into LDS; the table into LDS.
//   gather : a wave per lattice row, four rows in flight, a lane per column: the map byte (neighbouring lanes read neighbouring map bytes; neighbouring instances read the same map,
//            from L2) into the region's bytes, the row's lethal cells as two 64-bit ballots, the counts of rule 5 from ballots.  A lethal cell of the halo is
//            counted by the tile that holds the window cell nearest to it, so that every halo cell of the instance is counted once.
//   pass 1 : (r > 0 and a lethal cell in the region) per lattice row and tile column, the distance to the row's nearest lethal cell, r + 1 for anything farther, from
//            the row's bits by count-leading / count-trailing zeros, as bytes, 16 to a thread.
//   pass 2 : a thread per 16 window cells of one row: the smallest dj^2 + g^2 over the 2 r + 1 rows around it (one 16-byte LDS read per row; neighbouring lanes read
//            neighbouring pieces), the table, the combination, and the 16 bytes to the window row: one 16-byte store where the address allows it.
// LDS: 16 KB region + 8 KB distances + 2 KB bits + 1 KB indices + 1 KB table.  Every private array is indexed by unrolled constants.
__global__ __launch_bounds__(kCwThreads) __attribute__((amdgpu_waves_per_eu(4))) void costmap_window_kernel(WindowArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_s[kCwSpanY * kCwSpanX];
    __shared__ __attribute__((aligned(16))) uint8_t s_g[kCwSpanY * kCwTileX];
    __shared__ unsigned long long s_bits[kCwSpanY * 2];
    __shared__ int s_mx[kCwSpanX], s_my[kCwSpanY];
    __shared__ uint32_t s_tab[kCwTableWords];
    __shared__ int s_cnt[5];      // rule 5's four, then the lethal cells of the whole region
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = a.b0 + (int)(blockIdx.x / (unsigned)a.ntiles), tile = (int)(blockIdx.x % (unsigned)a.ntiles);
    const int W = a.W, H = a.H, r = a.p.r;
    const int tx0 = (tile % a.tiles_x) * kCwTileX, ty0 = (tile / a.tiles_x) * kCwTileY;
    const int tw = W - tx0 < kCwTileX ? W - tx0 : kCwTileX, th = H - ty0 < kCwTileY ? H - ty0 : kCwTileY;      // the tile's window cells
    const int LW = tw + 2 * r, LH = th + 2 * r;                                                               // its lattice region
    double ox = 0.0, oy = 0.0;
    const bool okx = cw_origin_axis(a.pose[3 * (size_t)b], W, a.p.res, a.p.anchor_x, ox), oky = cw_origin_axis(a.pose[3 * (size_t)b + 1], H, a.p.res, a.p.anchor_y, oy);
    const bool valid = okx && oky;      // workgroup-uniform
    // ---- index
    for (int e = t; e < LW; e += kCwThreads) s_mx[e] = valid ? cw_map_index(cm_world(ox, tx0 - r + e, a.p.res), a.p.map_ox, a.p.map_res, a.p.map_sx) : -1;
    for (int e = t; e < LH; e += kCwThreads) s_my[e] = valid ? cw_map_index(cm_world(oy, ty0 - r + e, a.p.res), a.p.map_oy, a.p.map_res, a.p.map_sy) : -1;
    for (int e = t; e < kCwTableWords; e += kCwThreads) s_tab[e] = a.table[e];
    if (t < 5) s_cnt[t] = 0;
    __syncthreads();
    // ---- gather: kCwGatherRows rows of a wave are loaded back to back (loads in flight) before they are examined
    {
        int n_in = 0, n_lethal = 0, n_halo = 0, n_all = 0;      // wave-uniform
        int mx[2];
        bool wcol[2], ocol[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int col = lane + 64 * half, i = tx0 - r + col;
            const int ci = i < 0 ? 0 : i > W - 1 ? W - 1 : i;
            mx[half] = col < LW ? s_mx[col] : -2;      // -2: no column of the region
            wcol[half] = col >= r && col < r + tw;
            ocol[half] = ci >= tx0 && ci < tx0 + tw;
        }
        constexpr int kWaves = kCwThreads / 64;
        for (int row0 = wave; row0 < LH; row0 += kWaves * kCwGatherRows) {
            uint8_t v[kCwGatherRows][2];
            bool in[kCwGatherRows][2];
#pragma unroll
            for (int u = 0; u < kCwGatherRows; ++u) {
                const int row = row0 + kWaves * u;
                const int my = row < LH ? s_my[row] : -1;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    in[u][half] = mx[half] >= 0 && my >= 0;
                    v[u][half] = (uint8_t)a.p.outside;
                    if (in[u][half]) v[u][half] = a.map[(size_t)my * (size_t)a.p.map_sx + (size_t)mx[half]];
                }
            }
#pragma unroll
            for (int u = 0; u < kCwGatherRows; ++u) {
                const int row = row0 + kWaves * u;
                if (row >= LH) break;      // wave-uniform
                const int j = ty0 - r + row;
                const int cj = j < 0 ? 0 : j > H - 1 ? H - 1 : j;
                const bool wrow = row >= r && row < r + th, orow = cj >= ty0 && cj < ty0 + th;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const bool act = mx[half] != -2;
                    if (act) s_s[row * kCwSpanX + lane + 64 * half] = v[u][half];
                    const bool lethal = act && v[u][half] == kLethal, window = wrow && wcol[half];
                    const unsigned long long bits = __ballot(lethal);
                    if (lane == 0) s_bits[2 * row + half] = bits;
                    n_all += __popcll(bits);
                    n_in += __popcll(__ballot(in[u][half] && window));
                    n_lethal += __popcll(__ballot(lethal && window));
                    n_halo += __popcll(__ballot(lethal && !window && orow && ocol[half]));
                }
            }
        }
        if (lane == 0 && valid) {
            if (n_in) atomicAdd(&s_cnt[0], n_in);
            if (n_lethal) atomicAdd(&s_cnt[1], n_lethal);
            if (n_halo) atomicAdd(&s_cnt[3], n_halo);
            if (n_all) atomicAdd(&s_cnt[4], n_all);
        }
    }
    __syncthreads();
    const bool inflate = valid && r > 0 && s_cnt[4] > 0;      // workgroup-uniform
    // ---- pass 1
    if (inflate) {
        const unsigned long long low_r = (1ull << r) - 1ull;      // r <= 32
        for (int it = t; it < LH * (kCwTileX / 16); it += kCwThreads) {
            const int row = it >> 2, piece = it & 3;
            const unsigned long long lo = s_bits[2 * row], hi = s_bits[2 * row + 1];
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int x = piece * 16 + e;      // the tile column; its lattice column in the region is x + r
                const unsigned long long right = cw_bits_from(lo, hi, x + r), left = cw_bits_from(lo, hi, x) & low_r;      // columns x + r .. ; columns x .. x + r - 1
                const int dr = right ? __builtin_ctzll(right) : 64, dl = left ? r - (63 - __builtin_clzll(left)) : 64;
                int g = dr < dl ? dr : dl;
                g = g < r + 1 ? g : r + 1;
                w[e >> 2] |= (uint32_t)g << (8 * (e & 3));
            }
            *reinterpret_cast<uint4*>(s_g + row * kCwTileX + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
    __syncthreads();
    // ---- pass 2 and the output
    {
        const int row = t >> 2, piece = t & 3;
        const int nvalid = tw - piece * 16 < 0 ? 0 : tw - piece * 16 < 16 ? tw - piece * 16 : 16;
        if (row < th && nvalid > 0) {
            const uint8_t* sp = s_s + (row + r) * kCwSpanX + r + piece * 16;
            uint32_t out[4] = {0u, 0u, 0u, 0u};
            int changed = 0;
            if (inflate) {
                int best[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) best[e] = 0x7fffffff;
                for (int dj = -r; dj <= r; ++dj) {
                    const uint4 q = *reinterpret_cast<const uint4*>(s_g + (row + r + dj) * kCwTileX + piece * 16);
                    const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
                    const int dj2 = dj * dj;
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int gv = (int)((qw[e >> 2] >> (8 * (e & 3))) & 0xFFu), d = dj2 + gv * gv;
                        best[e] = d < best[e] ? d : best[e];
                    }
                }
                const int r2 = r * r;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint8_t v = e < nvalid ? sp[e] : (uint8_t)0;
                    uint8_t o = v;
                    if (e < nvalid && best[e] <= r2) o = cw_combine(v, (uint8_t)((s_tab[best[e] >> 2] >> (8 * (best[e] & 3))) & 0xFFu), a.p.inflate_unknown);
                    changed += o != v ? 1 : 0;
                    out[e >> 2] |= (uint32_t)o << (8 * (e & 3));
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) out[e >> 2] |= (uint32_t)(e < nvalid ? sp[e] : (uint8_t)0) << (8 * (e & 3));
            }
            if (changed) atomicAdd(&s_cnt[2], changed);
            uint8_t* dst = a.cost + ((size_t)b * H + (size_t)(ty0 + row)) * W + tx0 + piece * 16;
            if (nvalid == 16 && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) *reinterpret_cast<uint4*>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
            else {
#pragma unroll
                for (int e = 0; e < 16; ++e) if (e < nvalid) dst[e] = (uint8_t)((out[e >> 2] >> (8 * (e & 3))) & 0xFFu);
            }
        }
    }
    __syncthreads();
    if (t == 0) {
        if (tile == 0) { a.origin[2 * (size_t)b] = valid ? ox : a.p.anchor_x; a.origin[2 * (size_t)b + 1] = valid ? oy : a.p.anchor_y; }
        if (a.info) {
            int32_t* info = a.info + 4 * (size_t)b;
            if (!valid) { if (tile == 0) info[0] = -1; }
            else for (int k = 0; k < 4; ++k) if (s_cnt[k]) atomicAdd(&info[k], s_cnt[k]);
        }
    }
}

#endif  // __HIPCC__

}  // namespace mpc
