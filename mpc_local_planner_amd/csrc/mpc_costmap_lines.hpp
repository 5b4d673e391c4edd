// mpc_costmap_lines.hpp -- costmap -> line segments that follow the walls, for a batch on the device: the third step for the one slot of the fleet cycle where
// mpc_costmap_to_obstacles_device (one point per cell) and mpc_costmap_to_polygons_device (one convex shape per cluster, mpc_costmap_clusters.hpp) stand.  The
// reference's shipped demo configures costmap_converter::CostmapToLinesDBSRANSAC (cfg/diff_drive/costmap_converter_params.yaml: ransac_inlier_distance 0.15,
// ransac_min_inliers 10, ransac_no_iterations 1500, ransac_remainig_outliers 3).  costmap_converter is not part of the reference's tree and its plugins stay out of
// scope: what follows is a deterministic rule OF OURS in integer arithmetic, declared as `reach` and the hull rule of mpc_costmap_clusters.hpp are.
// Where the converter draws random samples, this rule's hypotheses are a fixed function of (h, rho, r): the result is exactly reproducible.
//
// The rule, per instance:
//   1. kept cells and clusters : exactly those of mpc_costmap_to_polygons (cc_kept / cm_keep / cm_world; scan position i * size_y + j; connected components under
//                   di * di + dj * dj <= link_dist_sq, keyed and emitted in the order of their first cell).  The cells of a cluster are taken in scan order.
//   2. small clusters : a cluster of fewer than min_inliers cells is emitted exactly as mpc_costmap_to_polygons emits it (point, line, hull, box, robot inside: its cells).
//   3. line extraction for a cluster of m >= min_inliers cells.  R: the remaining cells in scan order, r = |R|; rho: the lines already taken from this cluster.
//      Repeat while r > remaining_outliers:
//        hypotheses : hypothesis h is an ordered pair (p, q) = (R[a], R[b]), a != b.  If r (r - 1) / 2 <= n_hypotheses: all pairs a < b in lexicographic order.
//                   Otherwise, for h = 0 .. n_hypotheses - 1:  a  = (mix(2h ^ (rho * 0x9E3779B9)) * r) >> 32,  b' = (mix((2h + 1) ^ (rho * 0x9E3779B9)) * (r - 1)) >> 32,
//                   b = b' + (b' >= a);  mix is the 32-bit "lowbias32" finaliser  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16;  unsigned
//                   32-bit arithmetic with 64-bit products.  The hypotheses depend on (h, rho, r) alone: not on the instance, the cluster or the run.
//        score      : in index coordinates, len2 = |q - p|^2, cr = cc_cross(p, q, c), t = (c - p) . (q - p).  A cell c of R is an inlier when
//                   cr * cr <= inlier_dist_sq * len2 and 0 <= t <= len2.  The score is the number of inliers (p and q count).  The winner is the highest score, ties
//                   to the lowest h.  If the winner's score is < min_inliers: stop.
//        gap rule   : (keeps a line from closing a doorway between two collinear wall pieces that are joined elsewhere in the cluster.)  Order the winner's inliers
//                   by (t, scan position) and break the sequence wherever (t[k+1] - t[k])^2 > link_dist_sq * len2.  Keep the run with the most cells, on a tie the
//                   first along t.  If that run has < min_inliers cells: stop.
//        emit       : a line of 2 vertices, the cell centres (cm_world) of the run's first and last cell, in that order.  Remove the run's cells from R, rho += 1.  The
//                   other inliers stay in R for later rounds.
//      When the loop ends, every cell left in R is emitted as a point, in scan order: nothing that was kept is left unrepresented.
//   4. output     : as mpc_costmap_to_polygons: slots 0, 1, ... of the mpc_obstacles layout, radius 0, velocity (0, 0); clusters in key order, within a cluster its
//                   lines in extraction order, then its leftover points.  n_obstacles = min(total, O), dropped = total - n_obstacles,
//                   info = {kept cells, clusters, lines emitted, cells emitted as points by rule 3}.  Unwritten slots and the vertices behind the valid ones keep their bytes.
//   5. parameters : LineParams below; link_dist_sq in [1, 64], inlier_dist_sq in [0, 64] (cells^2), min_inliers >= 2, n_hypotheses in [1, 65536], remaining_outliers >= 0.
//   6. refusals   : size_x or size_y above kClMaxSize = 4096 (cr * cr < 2^50 and every product of the rule stay inside int64), everything mpc_costmap_to_polygons refuses.
// No floating-point arithmetic reaches an output beyond cm_world, and no endpoint is refined: the result depends neither on B, nor on the position in the batch, nor on
// the run, and the kernel equals the host statement bit for bit because both implement the same integer rule.
//
// cl_instance is the per-instance statement (host code: serial, the inliers sorted).  costmap_lines_kernel restates it for a 256-thread workgroup.  Both take the
// hypotheses and the inlier test from the same host / device functions (cl_hypothesis, cl_inlier), the small clusters from mpc_costmap_clusters.hpp.
//
// SCRATCH: 8 bytes per cell and instance, owned by the handle: the int32 label of mpc_costmap_clusters.hpp and one packed word for the cell list of a cluster of more
// than kClListCap cells, which does not fit the kernel's LDS list.
#pragma once
#include "mpc_costmap_clusters.hpp"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace mpc {

constexpr int kClMaxSize = 4096;          // size_x, size_y above this are refused
constexpr int kClMaxInlier = 64;          // inlier_dist_sq in [0, kClMaxInlier]
constexpr int kClMaxHypotheses = 65536;   // n_hypotheses in [1, kClMaxHypotheses]
constexpr int kClListCap = 3584;          // cells of a cluster the kernel's LDS list holds; a larger cluster keeps its list in the handle's scratch

// struct mpc_line_params of include/mpc_costmap_lines.h
struct LineParams { double behind_dist; int32_t link_dist_sq, inlier_dist_sq, min_inliers, n_hypotheses, remaining_outliers; };

MPC_CM_HD uint32_t cl_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// pairs (a', b') with a' < a among r cells, a' < b' < r
MPC_CM_HD int cl_pairs_before(int a, int r) { return a * (2 * r - a - 1) / 2; }

// hypothesis h of round rho on r remaining cells (rule 3): the indices into R.  all_pairs: r (r - 1) / 2 <= n_hypotheses, so r < 364.
MPC_CM_HD void cl_hypothesis(bool all_pairs, uint32_t h, uint32_t rho, uint32_t r, int& a, int& b) {
    if (all_pairs) {
        // the row of the triangle h falls in: an estimate by the quadratic's root, set right in integers
        const double s = (double)(2 * r - 1);
        int g = (int)((s - sqrt(s * s - 8.0 * (double)h)) * 0.5);
        g = g < 0 ? 0 : g > (int)r - 2 ? (int)r - 2 : g;
        while (cl_pairs_before(g, (int)r) > (int)h) --g;
        while (cl_pairs_before(g + 1, (int)r) <= (int)h) ++g;
        a = g; b = g + 1 + ((int)h - cl_pairs_before(g, (int)r));
        return;
    }
    const uint32_t salt = rho * 0x9E3779B9u;
    const uint32_t ua = (uint32_t)(((uint64_t)cl_mix((2u * h) ^ salt) * r) >> 32);
    const uint32_t ub = (uint32_t)(((uint64_t)cl_mix((2u * h + 1u) ^ salt) * (r - 1u)) >> 32);
    a = (int)ua; b = (int)(ub + (ub >= ua ? 1u : 0u));
}

// is the cell c an inlier of the hypothesis p -> q (len2 = |q - p|^2)?  t: its place along the line, (c - p) . (q - p)
MPC_CM_HD bool cl_inlier(int pi, int pj, int qi, int qj, long long len2, int inlier_dist_sq, int ci, int cj, long long& t) {
    const long long cr = cc_cross(pi, pj, qi, qj, ci, cj);
    t = (long long)(ci - pi) * (long long)(qi - pi) + (long long)(cj - pj) * (long long)(qj - pj);
    return cr * cr <= (long long)inlier_dist_sq * len2 && t >= 0 && t <= len2;
}

MPC_CM_HD long long cl_len2(int pi, int pj, int qi, int qj) { return (long long)(qi - pi) * (qi - pi) + (long long)(qj - pj) * (qj - pj); }

// floor(sqrt(v)), 0 <= v < 2^52
MPC_CM_HD long long cl_isqrt(long long v) {
    long long s = (long long)sqrt((double)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

MPC_CM_HD void cl_put_line(const CcMap& m, const CcContainer& c, int V, int O, int slot, int i0, int j0, int i1, int j1) {
    if (slot >= O) return;
    cc_put_vertex(m, c, V, slot, 0, i0, j0);
    cc_put_vertex(m, c, V, slot, 1, i1, j1);
    cc_close_slot(c, slot, 2);
}

// ---- the statement (host).  lab: size_x * size_y words of scratch; info: 4 words or NULL; dropped: nullable.

// rule 3 for one cluster: its cells (scan positions, in scan order) as lines and leftover points from slot `total` on
inline void cl_extract(const CcMap& m, const LineParams& prm, int V, int O, const std::vector<int>& cells, const CcContainer& c, long long& total, int& lines, int& points) {
    const int H = m.H;
    std::vector<int> R = cells;
    std::vector<std::pair<long long, int>> in;      // (t, index into R) of the winner's inliers
    std::vector<char> gone;
    uint32_t rho = 0;
    while ((long long)R.size() > prm.remaining_outliers) {
        const int r = (int)R.size();
        const long long npairs = (long long)r * (r - 1) / 2;
        const bool all = npairs <= prm.n_hypotheses;
        const int nh = all ? (int)npairs : prm.n_hypotheses;
        int best = 0, pa = 0, pb = 0;
        for (int h = 0; h < nh; ++h) {
            int a, b;
            cl_hypothesis(all, (uint32_t)h, rho, (uint32_t)r, a, b);
            const int pi = R[a] / H, pj = R[a] % H, qi = R[b] / H, qj = R[b] % H;
            const long long len2 = cl_len2(pi, pj, qi, qj);
            int score = 0;
            long long t;
            for (int k = 0; k < r; ++k) score += cl_inlier(pi, pj, qi, qj, len2, prm.inlier_dist_sq, R[k] / H, R[k] % H, t) ? 1 : 0;
            if (score > best) { best = score; pa = a; pb = b; }
        }
        if (best < prm.min_inliers) break;
        const int pi = R[pa] / H, pj = R[pa] % H, qi = R[pb] / H, qj = R[pb] % H;
        const long long len2 = cl_len2(pi, pj, qi, qj), gap2 = (long long)prm.link_dist_sq * len2;
        in.clear();
        for (int k = 0; k < r; ++k) {
            long long t;
            if (cl_inlier(pi, pj, qi, qj, len2, prm.inlier_dist_sq, R[k] / H, R[k] % H, t)) in.push_back({t, k});
        }
        std::sort(in.begin(), in.end());
        size_t rs = 0, rn = 0;      // the kept run: where it begins in `in`, its cells
        for (size_t s = 0; s < in.size();) {
            size_t e = s + 1;
            while (e < in.size() && (in[e].first - in[e - 1].first) * (in[e].first - in[e - 1].first) <= gap2) ++e;
            if (e - s > rn) { rs = s; rn = e - s; }
            s = e;
        }
        if ((long long)rn < prm.min_inliers) break;
        const int first = R[in[rs].second], last = R[in[rs + rn - 1].second];
        cl_put_line(m, c, V, O, total < O ? (int)total : O, first / H, first % H, last / H, last % H);
        ++total; ++lines; ++rho;
        gone.assign(R.size(), 0);
        for (size_t k = rs; k < rs + rn; ++k) gone[in[k].second] = 1;
        size_t n = 0;
        for (size_t k = 0; k < R.size(); ++k) if (!gone[k]) R[n++] = R[k];
        R.resize(n);
    }
    for (size_t k = 0; k < R.size(); ++k, ++total, ++points)
        if (total < O) cc_put_point(m, c, V, O, (int)total, R[k] / H, R[k] % H);
}

inline void cl_instance(const CcMap& m, const LineParams& prm, int V, int O, int32_t* lab, int32_t* n_obstacles, const CcContainer& c, int32_t* dropped, int32_t* info) {
    const ClusterParams cp = {prm.behind_dist, prm.link_dist_sq};
    const int kept = cc_label(m, cp, lab);
    const double u = cc_index_of(m.px, m.ox0, m.res), v = cc_index_of(m.py, m.oy0, m.res);
    long long total = 0;
    int clusters = 0, lines = 0, points = 0, boxes = 0, as_cells = 0;
    std::vector<int> cells;
    for (int key = 0; key < (m.W - 1) * m.H; ++key) {
        if (lab[key] != key) continue;
        ++clusters;
        cc_cells_of(m, lab, key, cells);
        if ((long long)cells.size() < prm.min_inliers) cc_emit_cluster(m, V, O, cells, u, v, c, total, boxes, as_cells);      // rule 2
        else cl_extract(m, prm, V, O, cells, c, total, lines, points);
    }
    cc_finish(total, O, n_obstacles, dropped, info, kept, clusters, lines, points);
}

#if defined(__HIPCC__)

struct LineArgs : CcBatch {
    LineParams prm;
    uint32_t* list;           // [B][size_x * size_y]   the scratch: the cell list of a cluster that does not fit the LDS list
};
static_assert(std::is_trivially_copyable<LineArgs>::value, "a kernel argument");

// The gap rule's bins along t.  A bin is wb = floor(sqrt(link_dist_sq * len2)) wide, so two inliers of one bin are never a break apart, and two inliers with an empty
// bin between them always are (their distance is at least wb + 1): the breaks are the empty bins and those pairs of neighbouring bins whose nearest cells are too far
// apart.  len2 / wb + 1 bins: at most len + 3, and len < 4102 on a map of at most kCcMaxCells cells and kClMaxSize columns or rows.
constexpr int kClMaxBins = 4160;
constexpr int kClBinWords = (kClMaxBins + kCcThreads - 1) / kCcThreads * (kCcThreads / 32);      // a bitmap of the bins, whole chunks of 256
static_assert(kClListCap + kClMaxBins + 2 * kClBinWords <= 2 * kCcMaxSpan, "the list, the bins and their two bitmaps share the words of the column extremes");

// the largest k of the workgroup, in every thread (red: 4 words; every thread calls it; it ends behind a barrier)
__device__ __forceinline__ unsigned long long cl_block_max(unsigned long long k, unsigned long long* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(k, off); k = o > k ? o : k; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    unsigned long long best = red[0];
#pragma unroll
    for (int w = 1; w < kCcThreads / 64; ++w) best = red[w] > best ? red[w] : best;
    __syncthreads();
    return best;
}

// Rule 3 for one cluster by the workgroup.  list: its r cells in scan order, packed (i - imin) << 16 | (j - jmin) -- cross products and t do not see the shift -- in
// LDS or, for a cluster of more than kClListCap cells, in the scratch; the same code either way.
//   score   : thread k scores the hypotheses k, k + 256, ...: each against the whole list, every lane on the same word of it (an LDS broadcast, no bank conflict);
//             the winner is the workgroup's largest (score, -h);
//   gap     : the winner's inliers go into the bins above: the largest t of a bin by atomicMax; a bin is joined to the one before it when one of its inliers is
//             within the gap of that bin's largest t; a run begins at every occupied bin that is not joined; cells per bin, prefix sums, and the run with the most
//             cells, the first on a tie, as the largest (cells, -first bin);
//   emit    : the run's first and last cell by (t, place in the list) are the workgroup's smallest and largest key; the list is compacted in order by ballots.
__device__ __forceinline__ void cl_extract_device(uint32_t* list, int r, const LineParams& prm, const CcMap& m, const CcContainer& c, int V, int O, int imin, int jmin,
                                                  int* s_bin, unsigned* s_joined, unsigned* s_start, int* s_part, int* s_ws, unsigned long long* s_red,
                                                  int& total, int& lines, int& points) {
    const int t = threadIdx.x;
    uint32_t rho = 0;
    while (r > prm.remaining_outliers) {
        const long long npairs = (long long)r * (r - 1) / 2;
        const bool all = npairs <= prm.n_hypotheses;
        const int nh = all ? (int)npairs : prm.n_hypotheses;
        // ---- score
        unsigned long long key = 0;      // score << 32 | ~h; a hypothesis scores 2 at least
        for (int h = t; h < nh; h += kCcThreads) {
            int ia, ib;
            cl_hypothesis(all, (uint32_t)h, rho, (uint32_t)r, ia, ib);
            const uint32_t wp = list[ia], wq = list[ib];
            const int pi = (int)(wp >> 16), pj = (int)(wp & 0xffffu), qi = (int)(wq >> 16), qj = (int)(wq & 0xffffu);
            const long long len2 = cl_len2(pi, pj, qi, qj);
            int score = 0;
            for (int e = 0; e < r; ++e) {
                const uint32_t w = list[e];
                long long tt;
                score += cl_inlier(pi, pj, qi, qj, len2, prm.inlier_dist_sq, (int)(w >> 16), (int)(w & 0xffffu), tt) ? 1 : 0;
            }
            const unsigned long long k = ((unsigned long long)score << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)h);
            key = k > key ? k : key;
        }
        key = cl_block_max(key, s_red);
        if ((int)(key >> 32) < prm.min_inliers) break;
        int ia, ib;
        cl_hypothesis(all, 0xFFFFFFFFu - (uint32_t)key, rho, (uint32_t)r, ia, ib);
        const uint32_t wp = list[ia], wq = list[ib];
        const int pi = (int)(wp >> 16), pj = (int)(wp & 0xffffu), qi = (int)(wq >> 16), qj = (int)(wq & 0xffffu);
        const long long len2 = cl_len2(pi, pj, qi, qj), gap2 = (long long)prm.link_dist_sq * len2;
        const int wb = (int)cl_isqrt(gap2);
        const int nbins = (int)(len2 / wb) + 1, nb = nbins < kClMaxBins ? nbins : kClMaxBins;      // (never above it, see kClMaxBins: the bound of the arrays all the same)
        const int nw = (nb + 31) >> 5;
        // the winner's inlier at place e of the list: its t and its bin
        auto inlier = [&](int e, int& tt, int& bin) -> bool {
            const uint32_t w = list[e];
            long long tl;
            if (!cl_inlier(pi, pj, qi, qj, len2, prm.inlier_dist_sq, (int)(w >> 16), (int)(w & 0xffffu), tl)) return false;
            tt = (int)tl; bin = tt / wb; bin = bin < nb ? bin : nb - 1;
            return true;
        };
        // ---- gap
        for (int e = t; e < nb; e += kCcThreads) s_bin[e] = -1;
        for (int e = t; e < nw; e += kCcThreads) s_joined[e] = 0u;
        __syncthreads();
        for (int e = t; e < r; e += kCcThreads) { int tt, bin; if (inlier(e, tt, bin)) atomicMax(&s_bin[bin], tt); }
        __syncthreads();
        for (int e = t; e < r; e += kCcThreads) {
            int tt, bin;
            if (!inlier(e, tt, bin) || bin == 0) continue;
            const int before = s_bin[bin - 1];
            if (before >= 0 && (long long)(tt - before) * (tt - before) <= gap2) atomicOr(&s_joined[bin >> 5], 1u << (bin & 31));
        }
        __syncthreads();
        for (int b0 = 0; b0 < nb; b0 += kCcThreads) {
            const int bin = b0 + t;
            const bool starts = bin < nb && s_bin[bin] >= 0 && !((s_joined[bin >> 5] >> (bin & 31)) & 1u);
            const unsigned long long mask = __ballot(starts);
            if ((t & 63) == 0) { s_start[(bin >> 5)] = (unsigned)mask; s_start[(bin >> 5) + 1] = (unsigned)(mask >> 32); }
        }
        __syncthreads();
        for (int e = t; e < nb; e += kCcThreads) s_bin[e] = 0;
        __syncthreads();
        for (int e = t; e < r; e += kCcThreads) { int tt, bin; if (inlier(e, tt, bin)) atomicAdd(&s_bin[bin], 1); }
        __syncthreads();
        {      // s_bin[k]: the inliers of the bins 0 .. k
            const int per = (nb + kCcThreads - 1) / kCcThreads, lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
            int sum = 0, all_bins;
            for (int e = lo; e < hi; ++e) sum += s_bin[e];
            int run = cc_block_scan(sum, s_part, all_bins) - sum;
            for (int e = lo; e < hi; ++e) { run += s_bin[e]; s_bin[e] = run; }
        }
        __syncthreads();
        // the first bin behind `bin` at which a run begins, nb when there is none
        auto next_start = [&](int bin) -> int {
            int w = (bin + 1) >> 5;
            unsigned mk = w < nw ? s_start[w] & (~0u << ((bin + 1) & 31)) : 0u;
            while (!mk && ++w < nw) mk = s_start[w];
            return mk ? w * 32 + __builtin_ctz(mk) : nb;
        };
        unsigned long long rkey = 0;      // cells << 32 | ~first bin
        for (int bin = t; bin < nb; bin += kCcThreads) {
            if (!((s_start[bin >> 5] >> (bin & 31)) & 1u)) continue;
            const int cells = s_bin[next_start(bin) - 1] - (bin > 0 ? s_bin[bin - 1] : 0);
            const unsigned long long k = ((unsigned long long)cells << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)bin);
            rkey = k > rkey ? k : rkey;
        }
        rkey = cl_block_max(rkey, s_red);
        if ((int)(rkey >> 32) < prm.min_inliers) break;
        const int bin0 = (int)(0xFFFFFFFFu - (uint32_t)rkey), bin1 = next_start(bin0);      // the run: the inliers of the bins bin0 .. bin1 - 1
        // ---- emit
        unsigned long long kfirst = ~0ull, klast = 0;      // t << 20 | place in the list (below kCcMaxCells = 2^20)
        for (int e = t; e < r; e += kCcThreads) {
            int tt, bin;
            if (!inlier(e, tt, bin) || bin < bin0 || bin >= bin1) continue;
            const unsigned long long k = ((unsigned long long)tt << 20) | (unsigned long long)e;
            kfirst = k < kfirst ? k : kfirst; klast = k > klast ? k : klast;
        }
        kfirst = ~cl_block_max(~kfirst, s_red);
        klast = cl_block_max(klast, s_red);
        const uint32_t wf = list[(int)(kfirst & 0xFFFFFu)], wl = list[(int)(klast & 0xFFFFFu)];
        if (t == 0) cl_put_line(m, c, V, O, total < O ? total : O, imin + (int)(wf >> 16), jmin + (int)(wf & 0xffffu), imin + (int)(wl >> 16), jmin + (int)(wl & 0xffffu));
        ++total; ++lines; ++rho;
        int at = 0;
        for (int e0 = 0; e0 < r; e0 += kCcThreads) {
            const int e = e0 + t;
            int tt, bin;
            const uint32_t w = e < r ? list[e] : 0u;
            const bool stays = e < r && !(inlier(e, tt, bin) && bin >= bin0 && bin < bin1);
            int pre, pre1, tot, tot1;
            fo_scan_flags(stays, false, s_ws, pre, pre1, tot, tot1);      // (a barrier between the reads above and the writes below)
            if (stays) list[at + pre] = w;
            at += tot;
        }
        __syncthreads();
        r = at;
    }
    for (int e = t; e < r; e += kCcThreads) {
        const uint32_t w = list[e];
        cc_put_point(m, c, V, O, total + e < O ? total + e : O, imin + (int)(w >> 16), jmin + (int)(w & 0xffffu));
    }
    total += r; points += r;
}

// One workgroup (256 threads) per instance: keep, link and rank by cc_label_device (mpc_costmap_clusters.hpp), then the clusters one after the other in rank order.
// Count, first cell and bounding box of 256 clusters at a time by cc_chunk_stats, as costmap_clusters_kernel has them.
//   small  : fewer than min_inliers cells.  Column extremes by LDS atomicMin / atomicMax, cc_wrap by one thread for the vertex count and the robot test, again to write
//            the vertices; a cluster that contains the robot is swept in scan order by the workgroup: the shapes and the bytes of costmap_clusters_kernel.
//   lines  : the cells in scan order into the list by ordered ballots, then cl_extract_device.
__global__ __launch_bounds__(kCcThreads) __attribute__((amdgpu_waves_per_eu(4))) void costmap_lines_kernel(LineArgs a) {
    __shared__ int s_cnt[kCcThreads], s_first[kCcThreads], s_imax[kCcThreads], s_jmin[kCcThreads], s_jmax[kCcThreads];
    __shared__ int s_part[kCcThreads];
    __shared__ int s_ext[2 * kCcMaxSpan];
    int* const s_lo = s_ext;
    int* const s_hi = s_ext + kCcMaxSpan;
    uint32_t* const s_list = reinterpret_cast<uint32_t*>(s_ext);
    int* const s_bin = s_ext + kClListCap;
    unsigned* const s_joined = reinterpret_cast<unsigned*>(s_bin + kClMaxBins);
    unsigned* const s_start = s_joined + kClBinWords;
    __shared__ unsigned long long s_red[kCcThreads / 64];
    __shared__ int s_ws[8];
    __shared__ int s_shape[1];
    __shared__ int s_nlist;
    const int b = blockIdx.x, t = threadIdx.x;
    const int W = a.size_x, H = a.size_y, ncol = W - 1, nrow = H - 1, O = a.O, V = a.V;
    const int ncell = W * H, nscan = ncol > 0 && nrow > 0 ? ncol * H : 0;
    int32_t* lab = a.lab + (size_t)b * ncell;
    uint32_t* glist = a.list + (size_t)b * ncell;
    CcMap m;
    CcContainer c;
    cc_view(a, b, m, c);
    const double u = cc_index_of(m.px, m.ox0, m.res), v = cc_index_of(m.py, m.oy0, m.res);
    int kept, nclusters;
    cc_label_device(m, a.prm.behind_dist, a.prm.link_dist_sq, lab, s_ext, s_ws, &s_nlist, kept, nclusters);
    int total = 0, lines = 0, points = 0;      // workgroup-uniform
    for (int r0 = 0; r0 < nclusters; r0 += kCcThreads) {
        const int nc = nclusters - r0 < kCcThreads ? nclusters - r0 : kCcThreads;
        cc_chunk_stats(lab, nscan, H, r0, nc, s_cnt, s_first, s_imax, s_jmin, s_jmax);
        for (int k = 0; k < nc; ++k) {
            const int cnt = s_cnt[k], first = s_first[k], imax = s_imax[k], jmin = s_jmin[k], jmax = s_jmax[k];
            const int imin = first / H, want = -2 - (r0 + k), pbeg = imin * H, pend = (imax + 1) * H;
            if (cnt >= a.prm.min_inliers) {
                // ---- lines
                uint32_t* const list = cnt <= kClListCap ? s_list : glist;
                cc_sweep_cluster(lab, want, pbeg, pend, 0, kCcNoStop, s_ws, [&](int p, int place) {
                    const int i = p / H, j = p - i * H;
                    list[place] = ((uint32_t)(i - imin) << 16) | (uint32_t)(j - jmin);
                });
                __syncthreads();
                if (cnt <= kClListCap) cl_extract_device(s_list, cnt, a.prm, m, c, V, O, imin, jmin, s_bin, s_joined, s_start, s_part, s_ws, s_red, total, lines, points);
                else cl_extract_device(glist, cnt, a.prm, m, c, V, O, imin, jmin, s_bin, s_joined, s_start, s_part, s_ws, s_red, total, lines, points);
                __syncthreads();
                continue;
            }
            // ---- small (rule 2).  A map of at most kClMaxSize columns: the span of a cluster fits the words of the column extremes.
            if (cnt == 1) {
                if (t == 0) cc_put_point(m, c, V, O, total < O ? total : O, imin, first - imin * H);
                ++total;
                continue;
            }
            const int w = imax - imin + 1;
            for (int e = t; e < w; e += kCcThreads) { s_lo[e] = 0x7fffffff; s_hi[e] = -1; }
            __syncthreads();
            for (int p = pbeg + t; p < pend; p += kCcThreads) {
                if (cc_ld(lab + p) != want) continue;
                const int i = p / H, j = p - i * H;
                atomicMin(&s_lo[i - imin], j); atomicMax(&s_hi[i - imin], j);
            }
            __syncthreads();
            if (t == 0) {
                bool inside = false;
                const int nv = cc_wrap(s_lo, s_hi, w, imin, V, u, v, inside, nullptr, nullptr, 0);
                int kind = nv > V ? kCcKindBox : kCcKindHull;
                if (nv < 3) inside = false;
                if (kind == kCcKindBox) inside = cc_in_box(imin, imax, jmin, jmax, u, v);
                if (inside) kind = kCcKindCells;
                cc_put_shape(m, c, V, O, total, kind, nv, w, s_lo, s_hi, imin, imax, first - imin * H, jmin, jmax, u, v);
                s_shape[0] = kind;
            }
            __syncthreads();
            if (s_shape[0] == kCcKindCells) {      // workgroup-uniform
                cc_sweep_cluster(lab, want, pbeg, pend, total, O, s_ws, [&](int p, int place) { cc_put_point(m, c, V, O, place, p / H, p % H); });
                total += cnt;
            } else ++total;
            __syncthreads();
        }
        __syncthreads();
    }
    if (t == 0) cc_finish(total, O, a.n_obstacles + b, a.dropped ? a.dropped + b : nullptr, a.info ? a.info + 4 * b : nullptr, kept, nclusters, lines, points);
}

#endif  // __HIPCC__

}  // namespace mpc
