/* mpc_costmap_scans.h -- the laser-scan obstacle layer of every planner instance of a batch, kept on the device between cycles: the step between
 * mpc_costmap_window_device, which cuts the local costmap from the static map alone, and the costmap converters.
 *
 *     mpc_costmap_window_device        (one map on the device, B robot poses -> B windows and their origins)
 *  -> mpc_costmap_scans_device         (B laser scans -> B obstacle layers rolled, cleared, marked, and combined into the windows)
 *  -> mpc_costmap_to_obstacles_device | mpc_costmap_to_polygons_device | mpc_costmap_to_lines_device -> ... (include/mpc_costmap_window.h has the whole cycle)
 *
 * Both shipped local costmaps (cfg/<robot>/local_costmap_params.yaml) list two plugins, a costmap_2d::StaticLayer and a costmap_2d::ObstacleLayer; the obstacle
 * layer's settings are in cfg/<robot>/costmap_common_params.yaml (obstacle_range 3.0, raytrace_range 4.0 / 3.5, track_unknown_space true, combination_method 1, one
 * LaserScan source that marks and clears).  costmap_2d is not part of the reference's tree; the parts of the rule that restate its published source (ROS navigation
 * 1.17: obstacle_layer.cpp, costmap_2d.cpp / .h raytraceLine, bresenham2D, updateOrigin, worldToMap, costmap_layer.cpp updateWithMax / updateWithOverwrite, and
 * laser_geometry's range test) cannot be verified here.  The rest is a rule OF OURS: an integer roll on the window's lattice, a ray that is walked in full and
 * whose writes outside the window are dropped, a step count in integers, a disc where costmap_2d clears the footprint polygon.  Marks are NOT inflated: the shipped
 * local costmaps have no inflation layer, and a window cut with inflation_radius > 0 keeps its inflation of the static map while the marks of this step stay bare.
 * The rule is stated in full in mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp.
 *
 * The functions live in the same library as include/mpc_hip.h's and are built with it; they are declared here, apart from that header, whose set of declarations and
 * mpc_version stay as they are.  Callers that load the library at run time find them with dlsym under the names below.  mpc_last_costmap_ms
 * (include/mpc_costmap_clusters.h) reports this step too.
 */
#ifndef MPC_COSTMAP_SCANS_H
#define MPC_COSTMAP_SCANS_H

#include "mpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpc_scan_params {
    double  lattice_anchor[2];       /* the same anchor as mpc_window_params: both steps must put the window on the same lattice */
    double  sensor_pose[3];          /* x, y, yaw of the scanner in the robot frame, one for the whole batch */
    double  angle_min, angle_increment;
    double  range_min, range_max;    /* a range is used when range_min <= range < range_max */
    double  obstacle_range, raytrace_range;
    double  footprint_clear_radius;  /* <= 0: none */
    int32_t marking, clearing, inf_is_valid;
    int32_t track_unknown;           /* 1: an untouched layer cell is 255 (no information); 0: it is 0 */
    int32_t combination_method;      /* 0 overwrite, 1 maximum (the shipped files) */
} mpc_scan_params;

/* lattice_anchor = (0, 0), sensor_pose = (0, 0, 0), angle_min = -pi, angle_increment = 2 pi / 360, range_min = 0, range_max = 30, obstacle_range = 2.5,
 * raytrace_range = 3.0 (costmap_2d's defaults), footprint_clear_radius = 0 (none), marking = clearing = 1, inf_is_valid = 0, track_unknown = 0,
 * combination_method = 1. */
void mpc_scan_params_defaults(mpc_scan_params* p);

/* d_layer [B][size_y][size_x] and d_layer_cell [B][2] belong to the caller and are the layer's whole state: the handle keeps none.  d_layer_cell[b] is the lattice
 * index (cx, cy) of the window origin d_layer[b] was last written for.  With def = track_unknown ? 255 : 0, per instance b (robot_pose [B][3], all three read;
 * ranges [B][n_beams], float; keep [B] or NULL; cost [B][size_y][size_x] or NULL; info [B][4] or NULL):
 *   1. origin: rule 1 of include/mpc_costmap_window.h with this call's lattice_anchor, keeping the integer indices (cx, cy).  A pose whose x, y or yaw is not
 *      finite, or |cx| or |cy| at or above 2^30: the layer is def throughout, layer_cell = {0, 0}, cost is left as it was, info = {-1, 0, 0, 0}.
 *   2. roll: keep != NULL and keep[b] != 0: new(x, y) = old(x + cx - layer_cell_x, y + cy - layer_cell_y), def where that lies outside the old layer (a shift of a
 *      window or more empties it).  Otherwise the layer starts as def throughout and layer_cell[b] is not read.  Then layer_cell[b] = (cx, cy).
 *   3. beams: beam k points along wrap(((yaw + sensor_yaw) + angle_min) + k * angle_increment), from the sensor at pose_xy + R(wrap(yaw)) * sensor_xy; its range is
 *      ranges[b][k] as a double, +inf read as range_max - 1e-4 when inf_is_valid.  A NaN, a range below range_min or at or above range_max drops the beam, and so
 *      does an angle that wrap() cannot bring into [-pi, pi) (a heading beyond 2^50 or so).
 *   4. clear (clearing != 0, every kept beam): costmap_2d's Bresenham walk from the sensor's lattice cell to the endpoint's, cells floor((w - origin) / resolution),
 *      at most R = max(0, ceil(raytrace_range / resolution)) cells long; every visited cell inside the window becomes 0.  A sensor whose own cell lies outside the
 *      window clears nothing.
 *   5. mark (marking != 0, after all clearing): an endpoint closer to the sensor than obstacle_range (squared distances, strictly less) whose cell lies in the window
 *      becomes 254.  Then, footprint_clear_radius > 0: layer cells whose centre lies within that distance of (pose_x, pose_y) become 0.
 *   6. combine (cost != NULL), per cell with layer value l and window value s: l == 255: s stays; combination_method 1: s = l when s == 255 or s < l;
 *      combination_method 0: s = l.
 *   7. info[b] = {beams kept, layer cells equal to 254 after the call, layer cells equal to 0 after the call, window cells the combination changed}.
 * The result does not depend on the order of the beams, on B, on the position in the batch or on the run, and equals a host build of
 * mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp bit for bit.
 * DEVICE pointers, on the solver's stream, no synchronisation.
 * MPC_EINVAL: a null required pointer (s, params, d_robot_pose, d_ranges, d_layer, d_layer_cell); n_beams below 1 or above 4096; size_x or size_y below 1, or
 * size_x * size_y above 65536 (the layer of an instance stays in the LDS of one workgroup); a resolution that is not positive and finite; a range parameter
 * (range_min, range_max, obstacle_range, raytrace_range) that is negative or not finite; R above 4096, or range_max / resolution at or above 2^15; an angle or a
 * sensor pose that is not finite; a footprint_clear_radius that is not a number; a combination_method other than 0 or 1.  MPC_EBATCH: B above max_batch.  A refused
 * call changes nothing. */
int mpc_costmap_scans_device(mpc_solver* s, int32_t B, const mpc_scan_params* params, const double* d_robot_pose, const float* d_ranges, int32_t n_beams,
                             const int32_t* d_keep, int32_t size_x, int32_t size_y, double resolution, uint8_t* d_layer, int32_t* d_layer_cell, uint8_t* d_cost,
                             int32_t* d_info);
/* Same with HOST pointers, staged through the handle's buffers; blocking. */
int mpc_costmap_scans(mpc_solver* s, int32_t B, const mpc_scan_params* params, const double* robot_pose, const float* ranges, int32_t n_beams, const int32_t* keep,
                      int32_t size_x, int32_t size_y, double resolution, uint8_t* layer, int32_t* layer_cell, uint8_t* cost, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif
