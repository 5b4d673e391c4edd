/* mpc_plant.h -- the plant step: every robot of a batch moved by its command on the device, the last arrow of the fleet's control cycle.
 *
 *     mpc_scan_cast_device             (include/mpc_scan_cast.h: one map, B poses, the fleet's pool -> B laser scans)
 *  -> mpc_costmap_window_device        (the same map, the same poses -> B windows and their origins)
 *  -> mpc_costmap_scans_device         (the B scans -> B obstacle layers, combined into the windows)
 *  -> mpc_costmap_to_obstacles_device | mpc_costmap_to_polygons_device | mpc_costmap_to_lines_device -> ... -> mpc_controller_step_batch_device
 *  -> mpc_commands_batch_device        (include/mpc_hip.h: the solves -> cmd [B][3])
 *  -> mpc_plant_step_device            (cmd, the map, the pool -> the next B poses, and which robots stalled)
 *  -> mpc_fleet_pool_device            (include/mpc_fleet.h: the new poses -> the pool the next cycle's cast and plant step see)
 *
 * In every demo of the reference the plant is the `position` model of the Stage simulator: ex/stage/robots/ declare drive "diff", "car" with wheelbase 0.4, or "omni",
 * and a size and origin that give the footprint; the ex/stage/ world files set interval_sim 100, the floorplan has boundary 1, the robots obstruct each other.  Stage
 * is not part of the reference's tree: what restates its position model (the target velocity of the drives, the pose sum, the restored pose and the stall flag on a
 * collision) is stated from memory of its source and cannot be verified here.  The rest is a rule OF OURS: the velocity and acceleration bounds, the rear-axle car (the
 * reference's simple_car model as a plant), and the collision test, an exact test of the footprint's OUTLINE against the map's cells and the pool's bodies.
 * DECLARED LIMITS, and so visible deviations from Stage: the outline only -- a body wholly inside the footprint is not seen; every robot is tested against the others
 * where they stood when the call began, where Stage moves its models one after the other; no odom_error, the pose is the true one (Stage's localization "gps"); pool
 * entries are not moved; z is ignored.  The rule is stated in full in mpc_local_planner_amd/csrc/mpc_plant.hpp.
 *
 * The functions live in the same library as include/mpc_hip.h's and are built with it; they are declared here, apart from that header, whose set of declarations and
 * mpc_version stay as they are.  Callers that load the library at run time find them with dlsym under the names below.  mpc_last_costmap_ms
 * (include/mpc_costmap_clusters.h) reports this step too.
 */
#ifndef MPC_PLANT_H
#define MPC_PLANT_H

#include "mpc_fleet.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPC_DRIVE_DIFF = 0, MPC_DRIVE_OMNI = 1, MPC_DRIVE_CAR_STAGE = 2, MPC_DRIVE_CAR_REAR = 3 };

typedef struct mpc_plant_params {
    double  map_origin[2], map_resolution;      /* as mpc_cast_params: the world position of the corner of cell (0, 0); read when a map is given */
    double  interval;                           /* seconds per sub-step (Stage: interval_sim / 1000) */
    double  wheelbase;                          /* the car drives */
    double  v_min[3], v_max[3];                 /* box on the body velocity (vx, vy, w); -inf / +inf: none */
    double  a_max[3];                           /* bound on |dv| / interval per component; +inf: none */
    double  footprint[16][2];                   /* robot frame, the closed outline */
    int32_t n_footprint;                        /* 0: no collision test; else 2 .. 16 (2: one open segment) */
    int32_t n_substeps;                         /* 1 .. 64 sub-steps per call */
    int32_t drive;                              /* MPC_DRIVE_DIFF 0, _OMNI 1, _CAR_STAGE 2, _CAR_REAR 3 */
    int32_t map_size_x, map_size_y, block_threshold, unknown_blocks;   /* as mpc_cast_params */
    int32_t outside_blocks;                     /* a footprint vertex off the map stalls the robot (Stage: boundary 1) */
} mpc_plant_params;

/* map_origin = (0, 0), the given map geometry, interval = 0.1, wheelbase = 0.4, v_min = -inf, v_max = a_max = +inf, the footprint zeroed with n_footprint = 0,
 * n_substeps = 1, drive = MPC_DRIVE_DIFF, block_threshold = 254, unknown_blocks = 0, outside_blocks = 1. */
void mpc_plant_params_defaults(mpc_plant_params* p, double map_resolution, int32_t map_size_x, int32_t map_size_y);

/* Per instance b (map [map_size_y][map_size_x] bytes, shared, or NULL: no map test; cmd [B][3] as mpc_commands_batch* writes it; pool: NULL or a host struct
 * (include/mpc_fleet.h) laid out with V = cfg.max_vertices, velocity not read; self_index [B] or NULL; pose [B][3] in / out; vel [B][3] in / out or NULL; stall [B] or
 * NULL; info [B][4] or NULL), for sub-step m = 0 .. n_substeps - 1:
 *   1. validity: a pose, command or given velocity component that is not finite, a heading or (car drives) a steering angle that does not wrap into [-pi, pi), or a
 *      target velocity that is not finite (the rear-axle car at a quarter turn): the instance does not move, pose and vel are not written, stall = 0,
 *      info = {-1, -1, -1, -1}.
 *   2. target velocity from cmd = (c0, c1, c2): diff (c0, 0, c2); omni (c0, c1, c2); car, Stage: phi = wrap(c2), (c0 cos phi, 0, c0 sin phi / wheelbase); car, rear
 *      axle: (c0, 0, c0 (sin phi / cos phi) / wheelbase).
 *   3. bounds: per component v = v_prev + clamp(target - v_prev, -+ a_max * interval), then clamped to [v_min, v_max].  vel NULL: v_prev is the target, nothing is kept
 *      between calls.  Otherwise vel is read at the start and receives the bounded velocity of the last sub-step, whether or not that sub-step moved.
 *   4. move: (dx, dy, da) = v * interval, one Euler step in the frame at the start of the sub-step: x' = x + (dx cos th - dy sin th), y' = y + (dx sin th + dy cos th),
 *      th' = wrap(th + da).  A th' that does not wrap, or an x' or y' that is not finite, blocks the sub-step with reason -4.
 *   5. collision (n_footprint >= 2): the footprint's vertices are placed at the candidate pose; edge j runs from vertex j to vertex j + 1, the closed loop for
 *      n_footprint >= 3 and the one segment for 2.  With a map: a vertex whose cell is off the map gives reason -3 with outside_blocks and is ignored without; otherwise
 *      the edge is followed from its first vertex across every cell boundary it crosses, as mpc_scan_cast follows a beam, for its length: a blocking cell gives reason
 *      -2.  With a pool: entry p (what mpc_scan_cast skips is skipped) blocks when the ray from the edge's first vertex along the edge meets it within the edge's length.
 *      If nothing blocks, the pose becomes the candidate; otherwise the pose stays, the sub-step is counted in stall, and the next sub-step is tried from the
 *      unchanged pose.
 *   6. outputs: pose is written once, at the end, and only when a sub-step moved; stall[b] = the number of blocked sub-steps; info[b] = {sub-steps moved, the first
 *      blocked sub-step or -1, its reason or -1, the lowest edge j that shows that reason (the lowest vertex for -3; -1 for -4 or none)}.  The reason is the first that
 *      applies of -4, -3, -2, then the lowest pool p.
 * The result does not depend on the order of edges or entries, on B, on the position in the batch or on the run, and equals a host build of
 * mpc_local_planner_amd/csrc/mpc_plant.hpp bit for bit.
 * DEVICE pointers (pool: a host struct with device pointers inside), on the solver's stream, no synchronisation: d_cmd comes straight from mpc_commands_batch_device,
 * d_pose goes straight into mpc_fleet_pool_device and the next cycle.
 * MPC_EINVAL: a null required pointer (s, params, d_cmd, d_pose); n_substeps outside 1 .. 64; an interval that is not positive and finite; drive outside 0 .. 3; for a
 * car drive a wheelbase that is not positive and finite; n_footprint below 0, of 1 or above 16, or a footprint vertex that is not finite; with a map: map_size_x or
 * map_size_y below 1 or their product above 2^31 - 1, a map_resolution that is not positive and finite, a map_origin that is not finite, block_threshold outside
 * 1 .. 254, a footprint edge longer than 350 cells of the map; an a_max that is negative or not a number, or v_min <= v_max not holding; pool->P < 0, or pool->P > 0
 * without n_vertices and vertices.  MPC_EBATCH: B above max_batch.  A refused call changes nothing. */
int mpc_plant_step_device(mpc_solver* s, int32_t B, const uint8_t* d_map, const mpc_plant_params* params, const double* d_cmd, const mpc_pool* pool,
                          const int32_t* d_self_index, double* d_pose, double* d_vel, int32_t* d_stall, int32_t* d_info);
/* Same with HOST pointers (pool: host pointers inside), staged through the handle's buffers; blocking. */
int mpc_plant_step(mpc_solver* s, int32_t B, const uint8_t* map, const mpc_plant_params* params, const double* cmd, const mpc_pool* pool, const int32_t* self_index,
                   double* pose, double* vel, int32_t* stall, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif
