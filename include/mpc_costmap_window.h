/* mpc_costmap_window.h -- one shared map -> the local costmap window of every planner instance of a batch, on the device: the step that makes the two arrays the
 * costmap converters, the controller cycle and the feasibility check start from, cost [B][size_y][size_x] and origin [B][2].
 *
 *     mpc_costmap_window_device        (one map on the device, B robot poses -> B windows and their origins)
 *  -> mpc_costmap_scans_device         (optional, include/mpc_costmap_scans.h: B laser scans -> B obstacle layers kept between cycles, combined into the windows)
 *  -> mpc_costmap_to_obstacles_device  (one point per lethal cell)
 *  or mpc_costmap_to_polygons_device   (one point, line or convex polygon per cluster of lethal cells)
 *  or mpc_costmap_to_lines_device      (line segments along the walls of a cluster, points for what is left)
 *  -> mpc_obstacles_from_pool_device (append) -> mpc_plan_inputs_batch_device -> mpc_controller_step_batch_device -> mpc_check_feasibility_device
 *  -> mpc_commands_batch_device -> mpc_plant_step_device (optional, include/mpc_plant.h: simulated robots moved by their commands) -> mpc_fleet_pool_device
 *  -> [next cycle] mpc_costmap_window_device ...
 *
 * In the shipped demos the local costmap is a rolling window (cfg/<robot>/local_costmap_params.yaml: rolling_window true, width / height 5.5, resolution 0.1, a StaticLayer)
 * over one static map (maps/<name>.yaml, 0.05 m per cell).  A fleet shares that map: it is uploaded once, and a window is a gather plus, optionally, an inflation.
 * costmap_2d is not part of the reference's tree; the parts of the rule that restate its published source (getSizeInMetersX, worldToMap, cellDistance, computeCost,
 * InflationLayer::updateCosts) cannot be verified here, the rest is a rule OF OURS: a stateless origin, one frame, and an exact nearest lethal cell in integers,
 * also from the r cells around the window.  It is stated in full in mpc_local_planner_amd/csrc/mpc_costmap_window.hpp.
 *
 * The functions live in the same library as include/mpc_hip.h's and are built with it; they are declared here, apart from that header, whose set of declarations and
 * mpc_version stay as they are.  Callers that load the library at run time find them with dlsym under the names below.  mpc_last_costmap_ms
 * (include/mpc_costmap_clusters.h) reports this step too.
 */
#ifndef MPC_COSTMAP_WINDOW_H
#define MPC_COSTMAP_WINDOW_H

#include "mpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_window_params {
    double  map_origin[2];        /* world coordinates of the lower-left corner of map cell (0, 0) */
    double  map_resolution;
    double  lattice_anchor[2];    /* the window origins lie on anchor + k * resolution; costmap_2d starts at (0, 0) */
    double  inscribed_radius;     /* robot_radius, or the footprint's inscribed radius */
    double  inflation_radius;     /* <= 0: no inflation (the shipped local costmaps have no inflation layer) */
    double  cost_scaling_factor;  /* inflation_layer/cost_scaling_factor, 10 in the shipped files */
    int32_t map_size_x, map_size_y;
    int32_t outside_value;        /* 0 or 255: window cells that fall outside the map */
    int32_t inflate_unknown;      /* 0 / 1 */
} mpc_window_params;

/* map_origin = (0, 0), map_resolution and the map's size as given, lattice_anchor = (0, 0), inscribed_radius = 0, inflation_radius = 0 (no inflation),
 * cost_scaling_factor = 10, outside_value = 0, inflate_unknown = 0. */
void mpc_window_params_defaults(mpc_window_params* p, double map_resolution, int32_t map_size_x, int32_t map_size_y);

/* d_map: ONE map, [map_size_y][map_size_x] bytes in costmap values (0 .. 254, 255 = no information), shared by all B instances, read only.
 * Per instance b (robot_pose [B][3], of which x and y are read; cost [B][size_y][size_x]; origin [B][2]; info [B][4]):
 *   1. origin: sx = ((size_x - 1) + 0.5) * resolution, cx = floor((pose_x - sx / 2 - anchor_x) / resolution), origin_x = anchor_x + cx * resolution; y the same; every
 *      operation rounded on its own.  A pose whose x or y is not finite, or |cx| or |cy| at or above 2^30: every cell outside_value, origin = anchor, info[b][0] = -1.
 *   2. sample: lattice cell (i, j) has its centre at origin + (index + 0.5) * resolution; per axis a coordinate below map_origin is outside, otherwise the map index is
 *      (int)((w - map_origin) / map_resolution), outside when >= map_size; s(i, j) is the map byte, or outside_value for an outside cell.
 *   3. inflation: r = ceil(inflation_radius / resolution), 0 for inflation_radius <= 0; r == 0: cost = s.  Otherwise d2 is the smallest di^2 + dj^2 <= r^2 to a lattice
 *      cell with s == 254, the lattice reaching r cells beyond the window on every side.  None: cost = s.  Otherwise c = table[d2]; s == 255: cost = c when
 *      (inflate_unknown ? c > 0 : c >= 253), else 255; every other s: cost = max(s, c).
 *   4. table[0] = 254; with d = sqrt(d2): 253 when d * resolution <= inscribed_radius, else (unsigned char)(252 * exp(-cost_scaling_factor * (d * resolution -
 *      inscribed_radius))); built on the host inside the call.
 *   5. info[b] = {window cells sampled inside the map, lethal cells in the window, window cells whose value inflation changed, lethal cells in the halo only}.
 * d_cost and d_origin are written in full.  The result does not depend on B, on the position in the batch or on the run, and equals a host build of
 * mpc_local_planner_amd/csrc/mpc_costmap_window.hpp bit for bit.
 * DEVICE pointers, on the solver's stream, no synchronisation.
 * MPC_EINVAL: a null required pointer (s, d_map, params, d_robot_pose, d_cost, d_origin); size_x or size_y below 1 or above 4096, or size_x * size_y > 2^20; a
 * resolution or map_resolution that is not positive and finite; map_size_x or map_size_y below 1, or more than 2^31 - 1 map bytes; r > 32; an outside_value other
 * than 0 or 255; a negative or non-finite inscribed_radius; a negative or non-finite cost_scaling_factor.  MPC_EBATCH: B above max_batch.  A refused call changes
 * nothing. */
int mpc_costmap_window_device(mpc_solver* s, int32_t B, const uint8_t* d_map, const mpc_window_params* params, const double* d_robot_pose, int32_t size_x,
                              int32_t size_y, double resolution, uint8_t* d_cost, double* d_origin, int32_t* d_info);
/* Same with HOST pointers, staged through the handle's buffers; blocking. */
int mpc_costmap_window(mpc_solver* s, int32_t B, const uint8_t* map, const mpc_window_params* params, const double* robot_pose, int32_t size_x, int32_t size_y,
                       double resolution, uint8_t* cost, double* origin, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif
