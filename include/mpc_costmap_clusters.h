/* mpc_costmap_clusters.h -- costmap -> clustered obstacles (points, lines, convex polygons) for a batch of planner instances on the device: what the reference gets from
 * a costmap_converter plugin (updateObstacleContainerWithCostmapConverter, src/mpc_local_planner_ros.cpp:501-541; the shipped demo configures CostmapToPolygonsDBSMCCH
 * with cluster_max_distance 0.4 and cluster_min_pts 2).  costmap_converter is not part of the reference's tree and its plugins stay out of scope; the rule below is OURS,
 * deterministic, and coincides with density clustering plus convex hull at cluster_min_pts <= 2.  It is stated in full in
 * mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp.
 *
 * The functions live in the same library as include/mpc_hip.h's and are built with it; they are declared here, apart from that header, whose set of declarations and
 * mpc_version stay as they are.  Callers that load the library at run time find them with dlsym under the names below.
 *
 * The fleet cycle on device memory, with either costmap step in the one slot it has:
 *     ... -> mpc_fleet_pool_device
 *  -> [next cycle] mpc_costmap_to_obstacles_device  (one point per lethal cell)
 *               or mpc_costmap_to_polygons_device   (one point, line or convex polygon per cluster of lethal cells)
 *  -> mpc_obstacles_from_pool_device (append) -> mpc_controller_step_batch_device ...
 *
 * Which one: a wall of hundreds of cells is hundreds of slots of max_obstacles and hundreds of footprint distances per grid point on the point path, and ONE obstacle
 * and one clearance row as a polygon.  But CONVEX HULLS OVERREACH CONCAVE CLUSTERS: an L-shaped wall becomes a triangle that closes the free corner inside it (the
 * converter's convex-hull variant does the same).  Only a cluster whose shape contains the robot itself is broken up into its cells.
 */
#ifndef MPC_COSTMAP_CLUSTERS_H
#define MPC_COSTMAP_CLUSTERS_H

#include "mpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* behind_robot_dist: as in mpc_costmap_to_obstacles (cells behind the robot and farther away than this are not kept).
 * link_dist_sq: two kept cells belong to one cluster when di * di + dj * dj <= link_dist_sq, in cell indices; in [1, 64].  1: 4-neighbours, 2: 8-neighbours,
 * 64: the shipped cluster_max_distance 0.4 m at 0.05 m per cell. */
typedef struct mpc_cluster_params {
    double  behind_robot_dist;
    int32_t link_dist_sq;
} mpc_cluster_params;

/* behind_robot_dist = 1.5, link_dist_sq = clamp(floor((cluster_max_distance / resolution)^2 + 1e-9), 1, 64) (1 when the quotient is not a number) */
void mpc_cluster_params_defaults(mpc_cluster_params* p, double resolution, double cluster_max_distance);

/* Per instance b (cost [B][size_y][size_x], origin [B][2], robot_pose [B][3], as mpc_costmap_to_obstacles_device):
 *   kept cells : exactly those of mpc_costmap_to_obstacles -- value 254, i < size_x - 1, j < size_y - 1, not (behind the robot and farther than behind_robot_dist) --
 *                in its order: i outer, j inner;
 *   clusters   : the connected components of the kept cells under link_dist_sq, emitted in the order of their first cell;
 *   shape      : one cell: a point.  Collinear cells: a line from the first to the last.  Otherwise the convex hull of the cell centres, counter-clockwise from the
 *                first cell, collinear points dropped; a hull of more than cfg.max_vertices vertices (or a cluster of several rows spanning more than 4096 columns)
 *                is replaced by its bounding box, which contains it;
 *   robot      : a polygon or box that contains the robot position (boundary included) is emitted as its cells instead, one point each; lines and points never are;
 *   output     : slots 0, 1, ... of the mpc_obstacles layout (d_n_vertices [B][O], d_vertices [B][O][V][2], O = cfg.max_obstacles, V = cfg.max_vertices), radius 0 and
 *                velocity (0, 0) for the written slots where d_radius [B][O] / d_velocity [B][O][2] are given; n_obstacles[b] = min(total, O),
 *                dropped[b] = total - n_obstacles[b], info[b] = {kept cells, clusters, hulls replaced by their box, clusters emitted as cells}.
 * Slots at or above n_obstacles[b], and the vertices behind the valid ones of a written slot, stay byte for byte as they were.  The result does not depend on B, on the
 * position in the batch or on the run, and equals a host build of mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp bit for bit.
 * Scratch: 4 bytes per cell and instance (B * size_x * size_y * 4 bytes; 64 MB at 1024 instances of 128 x 128), owned by the handle: allocated by the first call, reused
 * while it is large enough, replaced by a larger one otherwise (the stream is synchronised then), freed by mpc_destroy.
 * DEVICE pointers, on the solver's stream, no synchronisation.
 * MPC_EINVAL: a null required pointer (cost, origin, robot_pose, params, n_obstacles, n_vertices, vertices), cfg.max_obstacles == 0, cfg.max_vertices < 4, size_x or
 * size_y < 1, size_x * size_y > 2^20, resolution not positive, link_dist_sq outside [1, 64]; MPC_EBATCH: B above max_batch.  A refused call changes nothing. */
int mpc_costmap_to_polygons_device(mpc_solver* s, int32_t B, const uint8_t* d_cost, int32_t size_x, int32_t size_y, double resolution, const double* d_origin,
                                   const double* d_robot_pose, const mpc_cluster_params* params, int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices,
                                   double* d_radius, double* d_velocity, int32_t* d_dropped, int32_t* d_info);
/* Same with HOST pointers, staged through the handle's buffers; blocking.  The outputs are cleared first: slots that are not written come back as zeros. */
int mpc_costmap_to_polygons(mpc_solver* s, int32_t B, const uint8_t* cost, int32_t size_x, int32_t size_y, double resolution, const double* origin,
                            const double* robot_pose, const mpc_cluster_params* params, int32_t* n_obstacles, int32_t* n_vertices, double* vertices,
                            double* radius, double* velocity, int32_t* dropped, int32_t* info);

/* Milliseconds the device spent in the most recent costmap step of this handle (mpc_costmap_to_obstacles*, mpc_costmap_to_polygons* or mpc_costmap_to_lines* of include/mpc_costmap_lines.h), between the two events that
 * bracket its launch on the solver's stream; waits for that launch.  0 when there has been none.  (mpc_last_kernel_ms reports the solve launch alone.) */
int mpc_last_costmap_ms(mpc_solver* s, float* ms);

#ifdef __cplusplus
}
#endif
#endif
