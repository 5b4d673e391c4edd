// mpc_costmap_clusters.hpp -- costmap -> clustered obstacles (points, lines, convex polygons) for a batch on the device: the step that stands where
// mpc_costmap_to_obstacles_device stands when the costmap is to reach the solve as a few shapes instead of one point per lethal cell.  The reference gets such shapes
// from a costmap_converter plugin (updateObstacleContainerWithCostmapConverter, src/mpc_local_planner_ros.cpp:501-541; its shipped demo configures
// CostmapToPolygonsDBSMCCH with cluster_max_distance 0.4 and cluster_min_pts 2).  costmap_converter is not part of the reference's tree and its plugins stay out of scope
// (DESIGN.md section 8): what follows is a deterministic rule OF OURS, declared as `reach` and the nearest-first rule of mpc_fleet_obstacles.hpp are.
//
// The rule, per instance:
//   1. kept cells : exactly the cells costmap_to_obstacles_kernel keeps -- value 254, i < size_x - 1, j < size_y - 1, not (behind the robot and farther than
//                   behind_robot_dist): cm_keep on cm_world, un-fused.  The scan order is the reference's, i outer, j inner: the scan position of a cell is i * size_y + j.
//   2. clusters   : two kept cells are linked when di * di + dj * dj <= link_dist_sq (integers; 1: 4-neighbours, 2: 8-neighbours, 64: 0.4 m at 0.05 m per cell);
//                   clusters are the connected components.  The key of a cluster is the scan position of its first cell; clusters are emitted in increasing key.
//                   With cluster_min_pts <= 2 this IS DBSCAN: every cell with a neighbour is a core point, and lone cells are noise, which the converter emits as points.
//   3. shape      : the convex hull of the cluster's cell indices by Andrew's monotone chain in exact integer cross products, collinear points dropped (cross <= 0 pops);
//                   counter-clockwise in (i, j), starting at the first cell.  One cell: a point (1 vertex).  A collinear cluster: a line (2 vertices, first and last cell).
//                   Otherwise a polygon.  A hull with more than V = cfg.max_vertices vertices is replaced by its index bounding box (imin,jmin), (imax,jmin), (imax,jmax),
//                   (imin,jmax): conservative, the box contains the hull.  So is a cluster of more than one row that spans more than kCcMaxSpan = 4096 columns (one of a
//                   single row is the line from its first to its last cell): the kernel keeps the column extremes of a cluster in LDS.
//   4. robot      : u = (px - origin_x) / resolution - 0.5, v likewise (un-fused).  A polygon contains the robot when (ax-ox)*(v-oy) - (ay-oy)*(u-ox) >= 0 on every edge
//                   o -> a, a box when imin <= u <= imax && jmin <= v <= jmax (closed sets; a pose that is not a number contains nothing).  A containing shape would put
//                   the robot at distance 0 from a blob it is not in (a U-shaped wall, a room): such a cluster is emitted as its cells, one point each, in scan order.
//                   Points and lines are never tested.
//   5. output     : vertices are cm_world of the indices; obstacles go to slots 0, 1, ... of the mpc_obstacles layout (n_vertices, vertices, radius 0 and velocity (0, 0)
//                   where the container has the arrays).  n_obstacles = min(total, O), dropped = total - n_obstacles,
//                   info = {kept cells, clusters, hulls replaced by their box, clusters emitted as cells}.  Slots at or above n_obstacles and the vertices behind the valid
//                   ones of a written slot keep their bytes.
// The result depends neither on B, nor on the position in the batch, nor on the run.
//
// CONVEX HULLS OVERREACH CONCAVE CLUSTERS: an L-shaped wall becomes a triangle, and the free corner inside it is closed to the robot.  That is the converter's
// behaviour too (its CCH variant); where it hurts, use the point path (mpc_costmap_to_obstacles*).
//
// cc_instance is the per-instance statement (host code: serial union-find, the monotone chain on all cells of a cluster).  costmap_clusters_kernel restates it for a
// 256-thread workgroup and computes the same bytes: both take every number that reaches the output from the same host / device functions (cm_world, cm_keep, cc_cross,
// cc_left_of, cc_in_box), and everything else is integers whose result does not depend on the order of evaluation.
//
// SCRATCH: 4 bytes per cell and instance (one int32 label), owned by the handle: B * size_x * size_y * 4 bytes, 64 MB at 1024 instances of 128 x 128.
#pragma once
#include "mpc_costmap.hpp"
#include "mpc_fleet_obstacles.hpp"      // fo_scan_flags (the kernel's ordered counts)

#include <cmath>
#include <type_traits>
#include <vector>

namespace mpc {

constexpr int kCcMaxCells = 1 << 20;      // size_x * size_y above this is refused
constexpr int kCcMaxLink = 64;            // link_dist_sq in [1, kCcMaxLink]
constexpr int kCcMaxSpan = 4096;          // columns a cluster may span and still get its hull (rule 3)

struct ClusterParams { double behind_dist; int32_t link_dist_sq; };      // struct mpc_cluster_params of include/mpc_costmap_clusters.h

// one instance's map and robot; hx, hy = cos / sin of the heading (PoseSE2::orientationUnitVec)
struct CcMap {
    const uint8_t* cost;      // [size_y][size_x]
    int32_t W, H;
    double res, ox0, oy0, px, py, hx, hy;
};
// one instance's container: slot o at n_vertices[o], vertices[o][V][2], radius[o] (nullable), velocity[o][2] (nullable)
struct CcContainer { int32_t* n_vertices; double* vertices; double* radius; double* velocity; };

// What a launch of costmap_clusters_kernel and of costmap_lines_kernel (mpc_costmap_lines.hpp) is told about its batch, and what the host builds of the tests are: the
// arrays of include/mpc_costmap_clusters.h, instance b at b times the size of one.
struct CcBatch {
    const uint8_t* cost;      // [B][size_y][size_x]
    const double* origin;     // [B][2]
    const double* pose;       // [B][3]
    int32_t size_x, size_y;
    double resolution;
    int32_t O, V;
    int32_t* lab;             // [B][size_x * size_y]   the scratch: labels (the kernels; the host statement brings its own)
    int32_t* n_obstacles;     // [B]
    int32_t* n_vertices;      // [B][O]
    double* vertices;         // [B][O][V][2]
    double* radius;           // [B][O] or NULL
    double* velocity;         // [B][O][2] or NULL
    int32_t* dropped;         // [B] or NULL
    int32_t* info;            // [B][4] or NULL
};

// map, robot and container of instance b
MPC_CM_HD void cc_view(const CcBatch& a, int b, CcMap& m, CcContainer& c) {
    const int W = a.size_x, H = a.size_y, O = a.O, V = a.V;
    const int ncell = W * H;
    m.cost = a.cost + (size_t)b * ncell; m.W = W; m.H = H; m.res = a.resolution;
    m.ox0 = a.origin[2 * b]; m.oy0 = a.origin[2 * b + 1];
    m.px = a.pose[3 * b]; m.py = a.pose[3 * b + 1];
    const double th = a.pose[3 * b + 2];
#if defined(__HIP_DEVICE_COMPILE__)
    m.hx = cos(th); m.hy = sin(th);
#else
    m.hx = std::cos(th); m.hy = std::sin(th);
#endif
    c.n_vertices = a.n_vertices + (size_t)b * O;
    c.vertices = a.vertices + (size_t)b * O * V * 2;
    c.radius = a.radius ? a.radius + (size_t)b * O : nullptr;
    c.velocity = a.velocity ? a.velocity + (size_t)b * O * 2 : nullptr;
}

// rule 5's counts of one instance (dropped, info: nullable)
MPC_CM_HD void cc_finish(long long total, int O, int32_t* n_obstacles, int32_t* dropped, int32_t* info, int i0, int i1, int i2, int i3) {
    *n_obstacles = total < O ? (int)total : O;
    if (dropped) *dropped = total > O ? (int)(total - O) : 0;
    if (info) { info[0] = i0; info[1] = i1; info[2] = i2; info[3] = i3; }
}

MPC_CM_HD bool cc_kept(const CcMap& m, int i, int j, double behind) {
    return m.cost[(size_t)j * m.W + i] == kLethal && cm_keep(cm_world(m.ox0, i, m.res), cm_world(m.oy0, j, m.res), m.px, m.py, m.hx, m.hy, behind);
}

MPC_CM_HD int cc_isqrt(int v) { int r = 0; while ((r + 1) * (r + 1) <= v) ++r; return r; }

// (a - o) x (b - o): > 0 when o -> a -> b turns counter-clockwise in (i, j)
MPC_CM_HD long long cc_cross(int oi, int oj, int ai, int aj, int bi, int bj) {
    return (long long)(ai - oi) * (long long)(bj - oj) - (long long)(aj - oj) * (long long)(bi - oi);
}

// the robot in index coordinates
MPC_CM_HD double cc_index_of(double p, double origin, double res) {
#pragma clang fp contract(off)
    const double d = p - origin;
    const double q = d / res;
    return q - 0.5;
}
// (u, v) on or to the left of the edge o -> a (false when u or v is not a number)
MPC_CM_HD bool cc_left_of(int oi, int oj, int ai, int aj, double u, double v) {
#pragma clang fp contract(off)
    const double ex = (double)(ai - oi), ey = (double)(aj - oj);
    const double du = u - (double)oi, dv = v - (double)oj;
    const double s = ex * dv, t = ey * du;
    return s - t >= 0.0;
}
MPC_CM_HD bool cc_in_box(int imin, int imax, int jmin, int jmax, double u, double v) {
    return (double)imin <= u && u <= (double)imax && (double)jmin <= v && v <= (double)jmax;
}

MPC_CM_HD void cc_put_vertex(const CcMap& m, const CcContainer& c, int V, int slot, int k, int i, int j) {
    double* w = c.vertices + ((size_t)slot * V + k) * 2;
    w[0] = cm_world(m.ox0, i, m.res);
    w[1] = cm_world(m.oy0, j, m.res);
}
MPC_CM_HD void cc_close_slot(const CcContainer& c, int slot, int nv) {
    c.n_vertices[slot] = nv;
    if (c.radius) c.radius[slot] = 0.0;
    if (c.velocity) { c.velocity[2 * slot] = 0.0; c.velocity[2 * slot + 1] = 0.0; }
}
MPC_CM_HD void cc_put_point(const CcMap& m, const CcContainer& c, int V, int O, int slot, int i, int j) {
    if (slot >= O) return;
    cc_put_vertex(m, c, V, slot, 0, i, j);
    cc_close_slot(c, slot, 1);
}
MPC_CM_HD void cc_put_box(const CcMap& m, const CcContainer& c, int V, int O, int slot, int imin, int imax, int jmin, int jmax) {
    if (slot >= O) return;
    cc_put_vertex(m, c, V, slot, 0, imin, jmin);
    cc_put_vertex(m, c, V, slot, 1, imax, jmin);
    cc_put_vertex(m, c, V, slot, 2, imax, jmax);
    cc_put_vertex(m, c, V, slot, 3, imin, jmax);
    cc_close_slot(c, slot, 4);
}

// ---- the statement (host).  lab: size_x * size_y words of scratch; info: 4 words or NULL; dropped: nullable.
inline int cc_root(int32_t* lab, int x) { while (lab[x] != x) x = lab[x]; return x; }

// rules 1 and 2: lab[p] becomes the key of the cluster of the kept cell at scan position p, -1 everywhere else; returns the number of kept cells
inline int cc_label(const CcMap& m, const ClusterParams& prm, int32_t* lab) {
    const int H = m.H, ncol = m.W - 1, nrow = m.H - 1, L = prm.link_dist_sq, r = cc_isqrt(L);
    const size_t N = (size_t)m.W * m.H;
    for (size_t p = 0; p < N; ++p) lab[p] = -1;
    int kept = 0;
    for (int i = 0; i < ncol; ++i)
        for (int j = 0; j < nrow; ++j)
            if (cc_kept(m, i, j, prm.behind_dist)) { lab[i * H + j] = i * H + j; ++kept; }
    // rule 2: the root of a component is its smallest scan position (the larger root always hangs under the smaller one)
    for (int i = 0; i < ncol; ++i)
        for (int j = 0; j < nrow; ++j) {
            if (lab[i * H + j] < 0) continue;
            for (int di = 0; di <= r && di <= i; ++di)
                for (int dj = -r; dj <= r; ++dj) {
                    const int jj = j + dj;
                    if ((di == 0 && dj >= 0) || jj < 0 || jj >= nrow || di * di + dj * dj > L || lab[(i - di) * H + jj] < 0) continue;
                    const int a = cc_root(lab, i * H + j), b = cc_root(lab, (i - di) * H + jj);
                    if (a < b) lab[b] = a; else if (b < a) lab[a] = b;
                }
        }
    for (int p = 0; p < ncol * H; ++p) if (lab[p] >= 0) lab[p] = cc_root(lab, p);
    return kept;
}

// the cells of the cluster `key` in scan order
inline void cc_cells_of(const CcMap& m, const int32_t* lab, int key, std::vector<int>& cells) {
    cells.clear();
    for (int p = key; p < (m.W - 1) * m.H; ++p) if (lab[p] == key) cells.push_back(p);
}

// rules 3 to 5 for one cluster: its cells (scan positions, in scan order) as one shape or, when that contains the robot (u, v), one point per cell, from slot `total`
// on; total, boxes and as_cells are counted up
inline void cc_emit_cluster(const CcMap& m, int V, int O, const std::vector<int>& cells, double u, double v, const CcContainer& c, long long& total, int& boxes, int& as_cells) {
    const int H = m.H;
    int imax = 0, jmin = m.H, jmax = 0;
    for (size_t k = 0; k < cells.size(); ++k) {
        const int i = cells[k] / H, j = cells[k] % H;
        imax = i > imax ? i : imax; jmin = j < jmin ? j : jmin; jmax = j > jmax ? j : jmax;
    }
    const int first = cells.front(), last = cells.back(), imin = first / H;
    bool box = false, inside = false;
    std::vector<int> lower, upper, hull;      // scan positions
    if (cells.size() == 1) hull.push_back(first);
    else if (imax - imin + 1 > kCcMaxSpan) {
        if (jmin == jmax) { hull.push_back(first); hull.push_back(last); }
        else box = true;
    } else {
        // rule 3: Andrew's monotone chain; the cells are sorted as they come
        auto chain = [&](std::vector<int>& st, int p) {
            while (st.size() >= 2 && cc_cross(st[st.size() - 2] / H, st[st.size() - 2] % H, st.back() / H, st.back() % H, p / H, p % H) <= 0) st.pop_back();
            st.push_back(p);
        };
        for (size_t k = 0; k < cells.size(); ++k) chain(lower, cells[k]);
        for (size_t k = cells.size(); k-- > 0;) chain(upper, cells[k]);
        hull.assign(lower.begin(), lower.end() - 1);
        hull.insert(hull.end(), upper.begin(), upper.end() - 1);
        if ((int)hull.size() > V) box = true;
    }
    if (box) { ++boxes; inside = cc_in_box(imin, imax, jmin, jmax, u, v); }
    else if (hull.size() >= 3) {
        inside = true;
        for (size_t k = 0; k < hull.size(); ++k) {
            const int o = hull[k], a = hull[(k + 1) % hull.size()];
            inside = inside && cc_left_of(o / H, o % H, a / H, a % H, u, v);
        }
    }
    if (inside) {      // rule 4
        ++as_cells;
        for (size_t k = 0; k < cells.size(); ++k, ++total)
            if (total < O) cc_put_point(m, c, V, O, (int)total, cells[k] / H, cells[k] % H);
        return;
    }
    if (total < O) {
        const int slot = (int)total;
        if (box) cc_put_box(m, c, V, O, slot, imin, imax, jmin, jmax);
        else {
            for (size_t k = 0; k < hull.size(); ++k) cc_put_vertex(m, c, V, slot, (int)k, hull[k] / H, hull[k] % H);
            cc_close_slot(c, slot, (int)hull.size());
        }
    }
    ++total;
}

inline void cc_instance(const CcMap& m, const ClusterParams& prm, int V, int O, int32_t* lab, int32_t* n_obstacles, const CcContainer& c, int32_t* dropped, int32_t* info) {
    const int kept = cc_label(m, prm, lab);
    const double u = cc_index_of(m.px, m.ox0, m.res), v = cc_index_of(m.py, m.oy0, m.res);
    long long total = 0;
    int clusters = 0, boxes = 0, as_cells = 0;
    std::vector<int> cells;
    for (int key = 0; key < (m.W - 1) * m.H; ++key) {
        if (lab[key] != key) continue;
        ++clusters;
        cc_cells_of(m, lab, key, cells);
        cc_emit_cluster(m, V, O, cells, u, v, c, total, boxes, as_cells);
    }
    cc_finish(total, O, n_obstacles, dropped, info, kept, clusters, boxes, as_cells);
}

#if defined(__HIPCC__)

constexpr int kCcThreads = 256;

struct ClusterArgs : CcBatch { ClusterParams prm; };
static_assert(std::is_trivially_copyable<ClusterArgs>::value, "a kernel argument");

// The labels are read and written with relaxed device-scope atomics throughout: the unions below go through atomicMin, which works in L2, and a plain load
// could be served from a line the CU's L1 still holds from before.
__device__ __forceinline__ int cc_ld(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_st(int32_t* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// a parent is never above its child, so the walk ends; a value that another lane has replaced meanwhile was an ancestor and still is
__device__ __forceinline__ int cc_find(const int32_t* lab, int x) {
    for (;;) { const int p = cc_ld(lab + x); if (p == x) return x; x = p; }
}
// Lock-free union towards the smaller scan position: the larger root is hung under the smaller one with atomicMin, and when the larger one was no root any more
// (old != a) the union goes on with what it pointed to.  Every step lowers a or b, so it ends; when all unions are done the root of a component is its minimum
// whatever order the lanes ran in.
__device__ __forceinline__ void cc_union(int32_t* lab, int a, int b) {
    for (;;) {
        a = cc_find(lab, a); b = cc_find(lab, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

// inclusive prefix of v over the workgroup in thread order, and the total (part: 256 words; every thread calls it)
__device__ __forceinline__ int cc_block_scan(int v, int* part, int& total) {
    const int t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (int off = 1; off < kCcThreads; off <<= 1) {
        const int x = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    const int inc = part[t];
    total = part[kCcThreads - 1];
    __syncthreads();
    return inc;
}

// The hull of one cluster from its column extremes (only a column's lowest and highest cell can be a vertex): lo[c], hi[c] for the columns imin + c, c < w (lo > hi:
// the cluster has no cell there).  Gift wrapping from the first cell (imin, lo[0]), counter-clockwise: the next vertex is the candidate that has no other to the
// right of the edge towards it, the farthest of those in line with it -- the vertices and the order of the monotone chain with its collinear points dropped, without
// a stack.  Returns the number of vertices, or V + 1 as soon as there are more than V.  inside: every edge has (u, v) on it or to its left.  With c: the vertices go
// to slot `slot`.
__device__ __forceinline__ int cc_wrap(const int* lo, const int* hi, int w, int imin, int V, double u, double v, bool& inside, const CcMap* m, const CcContainer* c, int slot) {
    const int si = imin, sj = lo[0];
    int ci = si, cj = sj, count = 0;
    inside = true;
    for (;;) {
        if (count == V) return V + 1;
        if (c) cc_put_vertex(*m, *c, V, slot, count, ci, cj);
        ++count;
        int bi = ci, bj = cj;      // best so far; (ci, cj) itself: none yet
        for (int k = 0; k < w; ++k) {
            const int l = lo[k], h = hi[k];
            if (l > h) continue;
            for (int e = 0; e < 2; ++e) {
                const int qi = imin + k, qj = e ? h : l;
                if (qi == ci && qj == cj) continue;
                if (bi == ci && bj == cj) { bi = qi; bj = qj; continue; }
                const long long cr = cc_cross(ci, cj, bi, bj, qi, qj);
                if (cr > 0) continue;
                const long long db = (long long)(bi - ci) * (bi - ci) + (long long)(bj - cj) * (bj - cj), dq = (long long)(qi - ci) * (qi - ci) + (long long)(qj - cj) * (qj - cj);
                if (cr < 0 || dq > db) { bi = qi; bj = qj; }
            }
        }
        inside = inside && cc_left_of(ci, cj, bi, bj, u, v);
        if (bi == si && bj == sj) return count;
        ci = bi; cj = bj;
    }
}

// maps of up to this many cells keep a bitmap of their kept cells in LDS while the cells are linked -- in the words of the column extremes, which are not in use yet --
// so that the up to 112 probes around a cell at link_dist_sq 64 are nine 17-bit windows read from LDS, and behind it, while they fit, a list of the kept cells, so that the
// passes over the kept cells alone keep all lanes busy; larger maps probe the labels in global memory
constexpr int kCcBitmapCells = 2 * kCcMaxSpan * 32;

constexpr int kCcKindPoint = 0, kCcKindHull = 1, kCcKindBox = 2, kCcKindCells = 3, kCcKindLine = 4;

// The first three steps of a workgroup (256 threads) on its instance, shared by costmap_clusters_kernel and costmap_lines_kernel (mpc_costmap_lines.hpp).  The labels
// live at their scan position, lab[i * size_y + j], so that a sweep in thread order is a sweep in scan order.
//   keep   : 16-byte pieces of the costmap rows (cm_load, cm_lethal_mask, cm_keep), the lanes along j: a kept cell gets its own scan position, every other word is -1
//            (and, on maps of up to kCcBitmapCells cells, its bit in an LDS bitmap and an entry in an LDS list, which the next step reads);
//   link   : every kept cell is united with the kept cells before it in scan order within link_dist_sq (in its own column the nearest one is enough) by cc_union,
//            then every label is replaced by its root: the fixed point -- the component's smallest scan position -- is unique, and nothing counts passes;
//   rank   : an ordered count of the roots gives every cluster its rank in key order; the labels become -2 - rank.
// s_ext: 2 * kCcMaxSpan words of LDS, free again on return; s_ws: 8 words; s_nlist: one word.  Every thread calls it; it ends behind a barrier.
__device__ __forceinline__ void cc_label_device(const CcMap& m, double behind_dist, int L, int32_t* lab, int* s_ext, int* s_ws, int* s_nlist_p, int& kept, int& nclusters) {
    unsigned* const s_bits = reinterpret_cast<unsigned*>(s_ext);
    int& s_nlist = *s_nlist_p;
    const int t = threadIdx.x;
    const int W = m.W, H = m.H, ncol = W - 1, nrow = H - 1;
    const int ncell = W * H, nscan = ncol > 0 && nrow > 0 ? ncol * H : 0;      // the sweeps' range: the scan positions of the visited columns
    const int r = cc_isqrt(L);

    // ---- keep
    const bool bitmap = ncell <= kCcBitmapCells;
    const int nwords = bitmap ? (ncell + 31) / 32 : 0;
    int* const s_list = s_ext + nwords;                            // the kept cells in any order, behind the bitmap
    const int cap = bitmap ? 2 * kCcMaxSpan - nwords : 0;
    for (int p = t; p < ncell; p += kCcThreads) cc_st(lab + p, -1);
    for (int e = t; e < nwords; e += kCcThreads) s_bits[e] = 0u;
    if (t == 0) s_nlist = 0;
    __syncthreads();
    if (nscan > 0) {
        const int G = (ncol + kCmPiece - 1) / kCmPiece;
        for (int q = t; q < G * nrow; q += kCcThreads) {
            const int grp = q / nrow, j = q - grp * nrow;
            const int i0 = grp * kCmPiece;
            const int valid = ncol - i0 < kCmPiece ? ncol - i0 : kCmPiece;
            const CmPiece pc = cm_load(m.cost + (size_t)j * W + i0, valid);
            if (!cm_any_lethal(pc)) continue;
            const double wy = cm_world(m.oy0, j, m.res);
            for (uint32_t msk = cm_lethal_mask(pc); msk; msk &= msk - 1) {
                const int i = i0 + __builtin_ctz(msk);
                if (!cm_keep(cm_world(m.ox0, i, m.res), wy, m.px, m.py, m.hx, m.hy, behind_dist)) continue;
                const int p = i * H + j;
                cc_st(lab + p, p);
                if (bitmap) {
                    atomicOr(&s_bits[p >> 5], 1u << (p & 31));
                    const int e = atomicAdd(&s_nlist, 1);
                    if (e < cap) s_list[e] = p;
                }
            }
        }
    }
    __syncthreads();
    const int nlist = s_nlist;
    const bool listed = bitmap && nlist <= cap;      // every kept cell is in the list: the passes over the kept cells alone go through it, all lanes busy
    // ---- link
    // the kept cells among the scan positions q0 + lo .. q0 + hi (at most 17, all on the map), bit k for q0 + lo + k
    auto window = [&](int q0, int lo, int hi) -> unsigned {
        const int at = q0 + lo, w0 = at >> 5, w1 = w0 + 1 < nwords ? w0 + 1 : w0;
        const unsigned long long two = (unsigned long long)s_bits[w0] | ((unsigned long long)s_bits[w1] << 32);
        return (unsigned)(two >> (at & 31)) & ((1u << (hi - lo + 1)) - 1u);
    };
    auto link_cell = [&](int p) {
        const int i = p / H, j = p - i * H;
        if (bitmap) {
            if (j > 0) {      // its own column: the nearest one before it
                const int lo = -(r < j ? r : j);
                const unsigned wb = window(p, lo, -1);
                if (wb) cc_union(lab, p, p + lo + 31 - __builtin_clz(wb));
            }
            for (int di = 1; di <= r && di <= i; ++di) {
                const int sp = cc_isqrt(L - di * di);
                const int lo = -(sp < j ? sp : j), hi = sp < nrow - 1 - j ? sp : nrow - 1 - j;
                const int q0 = p - di * H;
                for (unsigned wb = window(q0, lo, hi); wb; wb &= wb - 1) cc_union(lab, p, q0 + lo + __builtin_ctz(wb));
            }
            return;
        }
        for (int dj = 1; dj <= r && dj <= j; ++dj)
            if (cc_ld(lab + p - dj) >= 0) { cc_union(lab, p, p - dj); break; }
        for (int di = 1; di <= r && di <= i; ++di)
            for (int dj = -r; dj <= r; ++dj) {
                const int jj = j + dj;
                if (jj < 0 || jj >= nrow || di * di + dj * dj > L) continue;
                const int q = p - di * H + dj;
                if (cc_ld(lab + q) >= 0) cc_union(lab, p, q);
            }
    };
    if (listed) for (int e = t; e < nlist; e += kCcThreads) link_cell(s_list[e]);
    else for (int p = t; p < nscan; p += kCcThreads) if (cc_ld(lab + p) >= 0) link_cell(p);
    __syncthreads();
    if (listed) for (int e = t; e < nlist; e += kCcThreads) cc_st(lab + s_list[e], cc_find(lab, s_list[e]));
    else for (int p = t; p < nscan; p += kCcThreads) if (cc_ld(lab + p) >= 0) cc_st(lab + p, cc_find(lab, p));
    __syncthreads();
    // ---- rank
    kept = 0; nclusters = 0;
    for (int p0 = 0; p0 < nscan; p0 += kCcThreads) {
        const int p = p0 + t;
        const int l = p < nscan ? cc_ld(lab + p) : -1;
        int pre_k, pre_r, tot_k, tot_r;
        fo_scan_flags(l >= 0, l == p, s_ws, pre_k, pre_r, tot_k, tot_r);
        if (l == p) cc_st(lab + p, -2 - (nclusters + pre_r));
        kept += tot_k; nclusters += tot_r;
    }
    __syncthreads();
    // a root's word is final and below -1; only the words of the other cells are written here
    if (listed) for (int e = t; e < nlist; e += kCcThreads) { const int p = s_list[e], l = cc_ld(lab + p); if (l >= 0) cc_st(lab + p, cc_ld(lab + l)); }
    else for (int p = t; p < nscan; p += kCcThreads) { const int l = cc_ld(lab + p); if (l >= 0) cc_st(lab + p, cc_ld(lab + l)); }
    __syncthreads();
}

// The workgroup's steps on the ranked labels that costmap_clusters_kernel and costmap_lines_kernel share.  Every thread calls them.

// Count, first cell and bounding box of the clusters of rank r0 .. r0 + nc - 1 (nc <= 256), cluster r0 + k at word k of the five arrays, by integer LDS atomics
// (order-independent).  It ends behind a barrier.
__device__ __forceinline__ void cc_chunk_stats(const int32_t* lab, int nscan, int H, int r0, int nc, int* s_cnt, int* s_first, int* s_imax, int* s_jmin, int* s_jmax) {
    const int t = threadIdx.x;
    s_cnt[t] = 0; s_first[t] = 0x7fffffff; s_imax[t] = -1; s_jmin[t] = 0x7fffffff; s_jmax[t] = -1;
    __syncthreads();
    for (int p = t; p < nscan; p += kCcThreads) {
        const int k = -2 - cc_ld(lab + p) - r0;
        if (k < 0 || k >= nc) continue;
        const int i = p / H, j = p - i * H;
        atomicAdd(&s_cnt[k], 1); atomicMin(&s_first[k], p); atomicMax(&s_imax[k], i); atomicMin(&s_jmin[k], j); atomicMax(&s_jmax[k], j);
    }
    __syncthreads();
}

constexpr int kCcNoStop = 0x7fffffff;

// The cells of the cluster whose label is `want` among the scan positions [pbeg, pend), in scan order, numbered by ballot: f(p, place) for each, the places counted
// on from `at`; returns the place behind the last one.  The sweep ends early once that place has reached `stop` (kCcNoStop: never).  s_ws: 8 words.
template <typename F>
__device__ __forceinline__ int cc_sweep_cluster(const int32_t* lab, int want, int pbeg, int pend, int at, int stop, int* s_ws, F f) {
    const int t = threadIdx.x;
    for (int p0 = pbeg; p0 < pend && at < stop; p0 += kCcThreads) {
        const int p = p0 + t;
        const bool is = p < pend && cc_ld(lab + p) == want;
        int pre, pre1, tot, tot1;
        fo_scan_flags(is, false, s_ws, pre, pre1, tot, tot1);
        if (is) f(p, at + pre);
        at += tot;
    }
    return at;
}

// One thread writes the shape chosen for a cluster (kind: kCcKind*) into slot `slot`: nothing for kCcKindCells, and nothing at or above O.  nv: the vertices of a
// hull, which cc_wrap finds again in the w words of column extremes at lo, hi; j0: the row of the first cell.
__device__ __forceinline__ void cc_put_shape(const CcMap& m, const CcContainer& c, int V, int O, int slot, int kind, int nv, int w, const int* lo, const int* hi, int imin, int imax,
                                             int j0, int jmin, int jmax, double u, double v) {
    if (slot < O) {
        if (kind == kCcKindPoint) cc_put_point(m, c, V, O, slot, imin, j0);
        else if (kind == kCcKindBox) cc_put_box(m, c, V, O, slot, imin, imax, jmin, jmax);
        else if (kind == kCcKindLine) {      // one row, first and last cell
            cc_put_vertex(m, c, V, slot, 0, imin, jmin);
            cc_put_vertex(m, c, V, slot, 1, imax, jmin);
            cc_close_slot(c, slot, 2);
        } else if (kind == kCcKindHull) {
            bool inside;
            cc_wrap(lo, hi, w, imin, V, u, v, inside, &m, &c, slot);
            cc_close_slot(c, slot, nv);
        }
    }
}

// One workgroup (256 threads) per instance: keep, link and rank by cc_label_device, then
//   shape  : the clusters in chunks of 256 in rank order, thread k on cluster r0 + k.  Count, first cell and bounding box by cc_chunk_stats;
//            then runs of clusters whose column spans fit kCcMaxSpan words together: column extremes by LDS atomicMin / atomicMax, cc_wrap per thread once for the
//            vertex count and the robot test, an ordered prefix of the obstacles every cluster emits gives the slots, cc_wrap again writes the vertices;
//   cells  : a cluster that contains the robot is swept in scan order by the whole workgroup, its cells numbered by ballot.
__global__ __launch_bounds__(kCcThreads) void costmap_clusters_kernel(ClusterArgs a) {
    __shared__ int s_cnt[kCcThreads], s_first[kCcThreads], s_imax[kCcThreads], s_jmin[kCcThreads], s_jmax[kCcThreads];
    __shared__ int s_inc[kCcThreads], s_kind[kCcThreads];
    int* const s_slot = s_cnt;       // a chunk's counts are in registers once its runs begin (40 KB of LDS: four workgroups per compute unit)
    int* const s_part = s_kind;      // the scans' workspace: a scan is over before the kinds of its run are written, and those are read before the next scan
    __shared__ int s_ext[2 * kCcMaxSpan];
    int* const s_lo = s_ext;
    int* const s_hi = s_ext + kCcMaxSpan;
    __shared__ int s_ws[8];
    __shared__ int s_tot[2];
    __shared__ int s_nlist;
    const int b = blockIdx.x, t = threadIdx.x;
    const int W = a.size_x, H = a.size_y, ncol = W - 1, nrow = H - 1, O = a.O, V = a.V;
    const int ncell = W * H, nscan = ncol > 0 && nrow > 0 ? ncol * H : 0;      // the sweeps' range: the scan positions of the visited columns
    int32_t* lab = a.lab + (size_t)b * ncell;
    CcMap m;
    CcContainer c;
    cc_view(a, b, m, c);
    const double u = cc_index_of(m.px, m.ox0, m.res), v = cc_index_of(m.py, m.oy0, m.res);
    if (t < 2) s_tot[t] = 0;
    int kept, nclusters;
    cc_label_device(m, a.prm.behind_dist, a.prm.link_dist_sq, lab, s_ext, s_ws, &s_nlist, kept, nclusters);
    // ---- shape
    int total = 0;      // obstacles emitted so far (workgroup-uniform)
    for (int r0 = 0; r0 < nclusters; r0 += kCcThreads) {
        const int nc = nclusters - r0 < kCcThreads ? nclusters - r0 : kCcThreads;
        cc_chunk_stats(lab, nscan, H, r0, nc, s_cnt, s_first, s_imax, s_jmin, s_jmax);
        const bool mine = t < nc;
        const int cnt = mine ? s_cnt[t] : 0, first = mine ? s_first[t] : 0, imax = mine ? s_imax[t] : 0, jmin = mine ? s_jmin[t] : 0, jmax = mine ? s_jmax[t] : 0;
        const int imin = first / H, span = imax - imin + 1;
        const int w = mine && cnt > 1 && span <= kCcMaxSpan ? span : 0;      // words of column extremes this cluster needs
        int wtot;
        const int winc = cc_block_scan(w, s_part, wtot);
        s_inc[t] = winc;
        __syncthreads();
        for (int k0 = 0; k0 < nc;) {
            // the run [k0, k1): as many clusters as fit
            const int wbase = k0 > 0 ? s_inc[k0 - 1] : 0;
            int pre0, pre1, fit, unused;
            fo_scan_flags(t >= k0 && t < nc && s_inc[t] - wbase <= kCcMaxSpan, false, s_ws, pre0, pre1, fit, unused);
            const int k1 = k0 + (fit > 0 ? fit : 1);      // fit >= 1: a single cluster needs at most kCcMaxSpan words
            const int words = s_inc[k1 - 1] - wbase;
            for (int e = t; e < words; e += kCcThreads) { s_lo[e] = 0x7fffffff; s_hi[e] = -1; }
            __syncthreads();
            if (words > 0)
                for (int p = t; p < nscan; p += kCcThreads) {
                    const int k = -2 - cc_ld(lab + p) - r0;
                    if (k < k0 || k >= k1) continue;
                    const int wk = s_inc[k] - (k > 0 ? s_inc[k - 1] : 0);      // 0: a single cell, or wider than the span
                    if (wk == 0) continue;
                    const int i = p / H, j = p - i * H;
                    const int e = s_inc[k] - wk - wbase + (i - s_first[k] / H);
                    atomicMin(&s_lo[e], j); atomicMax(&s_hi[e], j);
                }
            __syncthreads();
            const bool run = t >= k0 && t < k1;
            const int mine_at = run && w > 0 ? winc - w - wbase : 0;      // where this cluster's column extremes begin
            const int* lo = s_lo + mine_at;
            const int* hi = s_hi + mine_at;
            int kind = kCcKindPoint, nout = 0, nv = 1;
            if (run) {
                bool inside = false;
                if (cnt == 1) kind = kCcKindPoint;
                else if (w == 0) kind = jmin == jmax ? kCcKindLine : kCcKindBox;
                else {
                    nv = cc_wrap(lo, hi, w, imin, V, u, v, inside, nullptr, nullptr, 0);
                    kind = nv > V ? kCcKindBox : kCcKindHull;
                    if (nv < 3) inside = false;
                }
                if (kind == kCcKindBox) { atomicAdd(&s_tot[0], 1); inside = cc_in_box(imin, imax, jmin, jmax, u, v); }
                if (inside) { atomicAdd(&s_tot[1], 1); kind = kCcKindCells; }
                nout = kind == kCcKindCells ? cnt : 1;
            }
            int ntot;
            const int ninc = cc_block_scan(nout, s_part, ntot);
            const int slot = total + ninc - nout;
            s_kind[t] = run ? kind : kCcKindPoint; s_slot[t] = slot;
            if (run) cc_put_shape(m, c, V, O, slot, kind, nv, w, lo, hi, imin, imax, first - imin * H, jmin, jmax, u, v);
            __syncthreads();
            // ---- cells: the clusters of the run that contain the robot, one after the other
            for (int k = k0; k < k1; ++k) {
                if (s_kind[k] != kCcKindCells) continue;      // workgroup-uniform
                const int want = -2 - (r0 + k), pbeg = (s_first[k] / H) * H, pend = (s_imax[k] + 1) * H;
                cc_sweep_cluster(lab, want, pbeg, pend, s_slot[k], O, s_ws, [&](int p, int place) { cc_put_point(m, c, V, O, place, p / H, p % H); });
            }
            __syncthreads();
            total += ntot;
            k0 = k1;
        }
    }
    if (t == 0) cc_finish(total, O, a.n_obstacles + b, a.dropped ? a.dropped + b : nullptr, a.info ? a.info + 4 * b : nullptr, kept, nclusters, s_tot[0], s_tot[1]);
}

#endif  // __HIPCC__

}  // namespace mpc
