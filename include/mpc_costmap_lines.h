/* mpc_costmap_lines.h -- costmap -> line segments that follow the walls, for a batch of planner instances on the device: the third costmap step for the one slot of the
 * fleet cycle, beside mpc_costmap_to_obstacles* (one point per lethal cell) and mpc_costmap_to_polygons* (one convex shape per cluster, include/mpc_costmap_clusters.h).
 * Convex hulls overreach concave clusters -- an L-shaped wall becomes a triangle --; lines follow the walls: an L becomes two segments and the free corner stays free.
 * The reference's shipped demo configures costmap_converter::CostmapToLinesDBSRANSAC (cfg/diff_drive/costmap_converter_params.yaml: ransac_inlier_distance 0.15,
 * ransac_min_inliers 10, ransac_no_iterations 1500, ransac_remainig_outliers 3).  costmap_converter is not part of the reference's tree and its plugins stay out of
 * scope; the rule below is OURS, deterministic and in integer arithmetic: where the converter samples at random, its hypotheses are a fixed function of (h, rho, r).
 * It is stated in full in mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp.
 *
 * The functions live in the same library as include/mpc_hip.h's and are built with it; they are declared here, apart from that header, whose set of declarations and
 * mpc_version stay as they are.  Callers that load the library at run time find them with dlsym under the names below.  mpc_last_costmap_ms
 * (include/mpc_costmap_clusters.h) reports this step too.
 *
 *     ... -> mpc_fleet_pool_device
 *  -> [next cycle] mpc_costmap_to_obstacles_device  (one point per lethal cell)
 *               or mpc_costmap_to_polygons_device   (one point, line or convex polygon per cluster of lethal cells)
 *               or mpc_costmap_to_lines_device      (line segments along the walls of a cluster, points for what is left)
 *  -> mpc_obstacles_from_pool_device (append) -> mpc_controller_step_batch_device ...
 */
#ifndef MPC_COSTMAP_LINES_H
#define MPC_COSTMAP_LINES_H

#include "mpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* behind_robot_dist, link_dist_sq: as in mpc_cluster_params (link_dist_sq in [1, 64]).
 * inlier_dist_sq: a cell belongs to a line when its squared distance from it is at most this, in cells^2; in [0, 64].
 * min_inliers: the fewest cells a line is made of, and the size from which on a cluster is cut into lines; >= 2.
 * n_hypotheses: the pairs of cells tried per line; in [1, 65536].
 * remaining_outliers: extraction ends when no more cells than this are left of a cluster; >= 0. */
typedef struct mpc_line_params {
    double  behind_robot_dist;
    int32_t link_dist_sq;
    int32_t inlier_dist_sq;
    int32_t min_inliers;
    int32_t n_hypotheses;
    int32_t remaining_outliers;
} mpc_line_params;

/* behind_robot_dist = 1.5, link_dist_sq as mpc_cluster_params_defaults has it, inlier_dist_sq = clamp(floor((ransac_inlier_distance / resolution)^2 + 1e-9), 0, 64)
 * (0 when the quotient is not a number), min_inliers = 10, n_hypotheses = 1500, remaining_outliers = 3: the shipped block (9 at 0.15 m and 0.05 m per cell). */
void mpc_line_params_defaults(mpc_line_params* p, double resolution, double cluster_max_distance, double ransac_inlier_distance);

/* Per instance b (cost [B][size_y][size_x], origin [B][2], robot_pose [B][3], as mpc_costmap_to_polygons_device):
 *   1. kept cells and clusters: exactly those of mpc_costmap_to_polygons -- value 254, i < size_x - 1, j < size_y - 1, not (behind the robot and farther than
 *      behind_robot_dist); scan position i * size_y + j; clusters are the connected components under di * di + dj * dj <= link_dist_sq, keyed and emitted in the order of
 *      their first cell; the cells of a cluster are taken in scan order.
 *   2. small clusters: a cluster of fewer than min_inliers cells is emitted exactly as mpc_costmap_to_polygons emits it (point, line, hull, box, robot inside: cells).
 *   3. line extraction for a cluster of m >= min_inliers cells.  R: the remaining cells in scan order, r = |R|; rho: the lines already taken from this cluster.
 *      Repeat while r > remaining_outliers:
 *        hypotheses: hypothesis h is an ordered pair (p, q) = (R[a], R[b]), a != b.  If r (r - 1) / 2 <= n_hypotheses: all pairs a < b in lexicographic order.  Otherwise,
 *          for h = 0 .. n_hypotheses - 1:  a = (mix(2h ^ (rho * 0x9E3779B9)) * r) >> 32,  b' = (mix((2h + 1) ^ (rho * 0x9E3779B9)) * (r - 1)) >> 32,  b = b' + (b' >= a);
 *          mix is the 32-bit "lowbias32" finaliser  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16;  all of it in unsigned 32-bit arithmetic
 *          with 64-bit products.  The hypotheses depend on (h, rho, r) alone: not on the instance, the cluster or the run.
 *        score: in index coordinates, len2 = |q - p|^2, cr = (q - p) x (c - p), t = (c - p) . (q - p).  A cell c of R is an inlier when cr * cr <= inlier_dist_sq * len2
 *          and 0 <= t <= len2.  The score is the number of inliers (p and q count).  The winner is the highest score, ties to the lowest h.  If the winner's score is
 *          < min_inliers: stop.
 *        gap rule (it keeps a line from closing a doorway between two collinear wall pieces that are joined elsewhere in the cluster): order the winner's inliers by
 *          (t, scan position); break the sequence wherever (t[k+1] - t[k])^2 > link_dist_sq * len2; keep the run with the most cells, on a tie the first along t.  If
 *          that run has < min_inliers cells: stop.
 *        emit: a line of 2 vertices, the cell centres of the run's first and last cell, in that order.  Remove the run's cells from R, rho += 1.  The other inliers stay
 *          in R for later rounds.
 *      When the loop ends, every cell left in R is emitted as a point, in scan order: nothing that was kept is left unrepresented.
 *   4. output: slots 0, 1, ... of the mpc_obstacles layout (d_n_vertices [B][O], d_vertices [B][O][V][2], O = cfg.max_obstacles, V = cfg.max_vertices), radius 0 and
 *      velocity (0, 0) for the written slots where d_radius [B][O] / d_velocity [B][O][2] are given; clusters in key order, within a cluster its lines in extraction
 *      order, then its leftover points; n_obstacles[b] = min(total, O), dropped[b] = total - n_obstacles[b],
 *      info[b] = {kept cells, clusters, lines emitted, cells emitted as points by rule 3}.
 * Slots at or above n_obstacles[b], and the vertices behind the valid ones of a written slot, stay byte for byte as they were.  No floating-point arithmetic reaches an
 * output beyond the cell centres, and no endpoint is refined.  The result does not depend on B, on the position in the batch or on the run, and equals a host build of
 * mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp bit for bit.
 * Scratch: 8 bytes per cell and instance (B * size_x * size_y * 8 bytes), the block of mpc_costmap_to_polygons*, owned by the handle: allocated by the first call,
 * reused while it is large enough, replaced by a larger one otherwise (the stream is synchronised then), freed by mpc_destroy.
 * DEVICE pointers, on the solver's stream, no synchronisation.
 * MPC_EINVAL: whatever mpc_costmap_to_polygons_device refuses (a null required pointer, cfg.max_obstacles == 0, cfg.max_vertices < 4, size_x or size_y < 1,
 * size_x * size_y > 2^20, resolution not positive, link_dist_sq outside [1, 64]), size_x or size_y above 4096 (every product of the rule stays inside 64 bits),
 * inlier_dist_sq outside [0, 64], min_inliers < 2, n_hypotheses outside [1, 65536], remaining_outliers < 0; MPC_EBATCH: B above max_batch.  A refused call changes
 * nothing. */
int mpc_costmap_to_lines_device(mpc_solver* s, int32_t B, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution, const double* d_origin,
                                const double* d_robot_pose, const mpc_line_params* params, int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices,
                                double* d_radius, double* d_velocity, int32_t* d_dropped, int32_t* d_info);
/* Same with HOST pointers, staged through the handle's buffers; blocking.  The outputs are cleared first: slots that are not written come back as zeros. */
int mpc_costmap_to_lines(mpc_solver* s, int32_t B, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution, const double* origin,
                         const double* robot_pose, const mpc_line_params* params, int32_t* n_obstacles, int32_t* n_vertices, double* vertices,
                         double* radius, double* velocity, int32_t* dropped, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif
