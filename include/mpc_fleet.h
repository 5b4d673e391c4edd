/* mpc_fleet.h -- obstacles that are not in the costmap, for a batch of planner instances on the device: the counterpart of
 * MpcLocalPlannerROS::updateObstacleContainerWithCustomObstacles (src/mpc_local_planner_ros.cpp:543-617) for a fleet.  Every instance of a launch gets, behind what its
 * container already holds (mpc_costmap_to_obstacles_device), the entries of a shared POOL of obstacles that lie within reach of it -- tracked agents, or the other robots of
 * the same fleet (mpc_fleet_pool*) -- each with its centroid velocity, which a solver created with enable_dynamic_obstacles follows along k * dt * v.
 *
 * The functions live in the same library as include/mpc_hip.h's and are built with it; they are declared here, apart from that header, whose set of declarations and
 * mpc_version (900) stay as they are.  Callers that load the library at run time find them with dlsym under the names below.
 *
 * The fleet cycle on device memory:
 *     mpc_controller_step_batch_device -> mpc_check_feasibility_device -> mpc_commands_batch_device
 *  -> mpc_plant_step_device            (optional, include/mpc_plant.h: simulated robots moved by their commands, stalled by the map and by this pool)
 *  -> mpc_fleet_pool_device            (poses and first plan intervals of this cycle -> pool entries)
 *  -> [next cycle] mpc_costmap_to_obstacles_device -> mpc_obstacles_from_pool_device (append) -> mpc_controller_step_batch_device ...
 */
#ifndef MPC_FLEET_H
#define MPC_FLEET_H

#include "mpc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* P obstacles in the planning frame, laid out like ONE instance of mpc_obstacles with V = cfg.max_vertices.  The struct itself is read on the host at the call; the
 * pointers inside are DEVICE pointers for the _device variant and HOST pointers for the other. */
typedef struct mpc_pool {
    int32_t P;
    const int32_t* n_vertices;        /* [P]        valid vertices of entry p; an entry with n_vertices < 1 is skipped */
    const double*  vertices;          /* [P][V][2] */
    const double*  radius;            /* [P] or NULL (NULL = all 0) */
    const double*  velocity;          /* [P][2] or NULL (NULL = all static) */
} mpc_pool;

/* reach: the culling radius.  An entry is a candidate when the squared distance of the robot position to its nearest valid vertex is at most reach * reach.  It is NOT a
 * clearance: radii are not subtracted, and nothing is said about the footprint.  The caller chooses it at least cutoff_dist plus the distance robot and agent can close
 * within one horizon (both speeds x the horizon's duration): what lies farther cannot get a clearance row before the next cycle's call sees it again.
 * min_speed: an entry whose speed sqrt(vx^2 + vy^2) is below it is handed on as static, velocity (0, 0).  Default 0.001: teb_local_planner's
 * Obstacle::setCentroidVelocity(TwistWithCovariance, Quaternion), which :612-614 call, is believed to use that threshold (it is not part of the reference's tree).
 * append: non-zero: the entries go behind the n_obstacles[b] the container holds; zero: the container is filled from slot 0. */
typedef struct mpc_pool_params {
    double  reach;
    double  min_speed;
    int32_t append;
} mpc_pool_params;

/* reach = cfg.cutoff_dist of the handle, min_speed = 0.001, append = 1 */
void mpc_pool_params_defaults(const mpc_solver* s, mpc_pool_params* p);

/* Per instance b, seen from (robot_pose[b][0], robot_pose[b][1]):
 *   candidates: the entries p with n_vertices[p] >= 1, p != self_index[b] (self_index NULL or -1: none is the robot itself), every valid vertex at a finite squared
 *               distance, and the nearest one within reach (inclusive);
 *   free = cfg.max_obstacles - base slots are left, base = n_obstacles[b] clamped to [0, max_obstacles] (append) or 0.  If the candidates do not all fit, the `free`
 *               NEAREST are taken -- ordered by (squared distance to the nearest vertex, p): ties go to the lower pool index;
 *   the taken entries are written in increasing p at slots base, base + 1, ...: n_vertices, the valid vertices, radius, velocity;
 *   n_obstacles[b] = base + taken, dropped[b] = candidates - taken, n_taken[b] = taken (both nullable).
 * Slots below base and at or above the new n_obstacles[b] stay byte for byte as they were.  d_radius / d_velocity may be NULL when the pool has no radius / velocity
 * (a pool that carries one needs the container's array: MPC_EINVAL).  The result does not depend on B, on the position in the batch or on the run, and equals a host
 * build of the same header (mpc_local_planner_amd/csrc/mpc_fleet_obstacles.hpp) bit for bit.
 * DEVICE pointers (pool: a host struct with device pointers inside), on the solver's stream, no synchronisation.
 * MPC_EINVAL: a null required pointer (pool, its n_vertices / vertices unless P == 0, robot_pose, params, n_obstacles, n_vertices, vertices), cfg.max_obstacles == 0, P < 0,
 * reach negative or not finite; MPC_EBATCH: B above max_batch.  A refused call changes nothing. */
int mpc_obstacles_from_pool_device(mpc_solver* s, int32_t B, const mpc_pool* pool, const double* d_robot_pose, const int32_t* d_self_index, const mpc_pool_params* params,
                                   int32_t* d_n_obstacles, int32_t* d_n_vertices, double* d_vertices, double* d_radius, double* d_velocity, int32_t* d_dropped, int32_t* d_n_taken);
/* Same with HOST pointers (pool: host pointers inside), staged through the handle's buffers; blocking.  The container arrays are in / out. */
int mpc_obstacles_from_pool(mpc_solver* s, int32_t B, const mpc_pool* pool, const double* robot_pose, const int32_t* self_index, const mpc_pool_params* params,
                            int32_t* n_obstacles, int32_t* n_vertices, double* vertices, double* radius, double* velocity, int32_t* dropped, int32_t* n_taken);

/* A pool made of the fleet itself: robot b becomes pool entry pool_offset + b -- n_vertices 1, the vertex (robot_pose[b][0], robot_pose[b][1]), the radius
 * d_robot_radius[b] (or the scalar robot_radius when that array is NULL), and the velocity of the first interval of its own plan,
 * ((x[b][1][0] - x[b][0][0]) / dt[b], (x[b][1][1] - x[b][0][1]) / dt[b]): the constant-velocity model of stage_inequality_se2.cpp:177-189 fed with what the robot is
 * about to do.  x [B][cfg.n][3] and dt [B] are the outputs of the solve (x NULL: velocity (0, 0)); status [B] (nullable): an instance whose solve did not end in
 * MPC_CONVERGED gets (0, 0), and so does one with dt <= 0 or with one of the five numbers not finite.  The pool arrays have room for pool_offset + B entries;
 * pool_radius / pool_velocity may be NULL.  Pools of several handles or shards are concatenated by pool_offset; self_index[b] = pool_offset + b excludes a robot from its own view.
 * DEVICE pointers, on the solver's stream, no synchronisation.  MPC_EINVAL: robot_pose, pool_n_vertices or pool_vertices NULL, x without dt, pool_offset < 0;
 * MPC_EBATCH: B above max_batch. */
int mpc_fleet_pool_device(mpc_solver* s, int32_t B, const double* d_robot_pose, const double* d_x, const double* d_dt, const int32_t* d_status, double robot_radius,
                          const double* d_robot_radius, int32_t pool_offset, int32_t* d_pool_n_vertices, double* d_pool_vertices, double* d_pool_radius, double* d_pool_velocity);
/* Same with HOST pointers (staged; blocking).  Only the entries pool_offset .. pool_offset + B - 1 of the pool arrays are touched. */
int mpc_fleet_pool(mpc_solver* s, int32_t B, const double* robot_pose, const double* x, const double* dt, const int32_t* status, double robot_radius,
                   const double* robot_radius_per_robot, int32_t pool_offset, int32_t* pool_n_vertices, double* pool_vertices, double* pool_radius, double* pool_velocity);

#ifdef __cplusplus
}
#endif
#endif
