"""ctypes mirror of the C ABI: for every header under include/, its structs, its enum values and, in a prototype table, its functions.
HEADERS, below the tables, says which table and which mirrors belong to which header.

Pure data definitions -- shared by the product binding (mpc_local_planner_amd/_lib.py)
and by tests.  No solver code here.
"""
from __future__ import annotations

import ctypes as C

MODEL_UNICYCLE = 0
MODEL_SIMPLE_CAR = 1
MODEL_SIMPLE_CAR_FRONT = 2
MODEL_KINEMATIC_BICYCLE = 3

COLLOC_FORWARD = 0
COLLOC_MIDPOINT = 1
COLLOC_CRANK_NICOLSON = 2

OBJ_MIN_TIME = 0
OBJ_QUADRATIC = 1
OBJ_MIN_TIME_VIA_POINTS = 2

FP64 = 0
FP32 = 1
MIXED = 2

STATUS_NAMES = {0: "converged", 1: "max_iter", 2: "linesearch_failed", 3: "linsolve_failed", 4: "numerical_error", 5: "time_limit"}

MPC_OK = 0
MPC_EINVAL = -1
MPC_ENODEV = -2
MPC_ENOMEM = -3
MPC_EHIP = -4
MPC_EBATCH = -5

INF = 1e30

COST_LEFT_SUM, COST_TRAPEZOIDAL = 0, 1
MU_ADAPTIVE, MU_MONOTONE = 0, 1          # enum mpc_mu_strategy
LS_DEFAULT, LS_MERIT, LS_FILTER = 0, 1, 2   # enum mpc_line_search
STAGE_AUTO, STAGE_LDS, STAGE_GLOBAL = 0, 1, 2      # enum mpc_stage_data: where a solve keeps its factorisation data

CAND_REFERENCE = 0
CAND_TRAVEL = 1
CAND_TRAVEL_REVERSE = 2
CAND_BLEND = 3
CAND_BLEND_REVERSE = 4
CAND_HERMITE_FF, CAND_HERMITE_RR, CAND_HERMITE_FR, CAND_HERMITE_RF = 5, 6, 7, 8
MAX_CANDIDATES = 4


class MpcConfig(C.Structure):
    """struct mpc_config (include/mpc_hip.h); field-for-field."""
    _fields_ = [
        ("model", C.c_int32),
        ("model_params", C.c_double * 4),
        ("n", C.c_int32),
        ("dt_ref", C.c_double),
        ("dt_free", C.c_int32),
        ("dt_lb", C.c_double),
        ("dt_ub", C.c_double),
        ("xf_fixed", C.c_int32 * 3),
        ("collocation", C.c_int32),
        ("objective", C.c_int32),
        ("Q", C.c_double * 3),
        ("R", C.c_double * 2),
        ("integral_form", C.c_int32),
        ("has_Qf", C.c_int32),
        ("Qf", C.c_double * 3),
        ("u_lb", C.c_double * 2),
        ("u_ub", C.c_double * 2),
        ("du_lb", C.c_double * 2),
        ("du_ub", C.c_double * 2),
        ("max_iter", C.c_int32),
        ("tol", C.c_double),
        ("mu_init", C.c_double),
        ("precision", C.c_int32),
        ("min_obstacle_dist", C.c_double),
        ("force_inclusion_dist", C.c_double),
        ("cutoff_dist", C.c_double),
        ("footprint_kind", C.c_int32),
        ("footprint_radius", C.c_double),
        ("max_obstacles", C.c_int32),
        ("max_vertices", C.c_int32),
        ("max_obstacle_rows", C.c_int32),
        ("mu_init_warm", C.c_double),
        ("terminal_ball", C.c_int32),
        ("terminal_ball_S", C.c_double * 3),
        ("terminal_ball_gamma", C.c_double),
        ("vp_position_weight", C.c_double),
        ("vp_orientation_weight", C.c_double),
        ("via_points_ordered", C.c_int32),
        ("max_via_points", C.c_int32),
        ("footprint_n_vertices", C.c_int32),
        ("footprint_vertices", C.c_double * 32),
        ("enable_dynamic_obstacles", C.c_int32),
        ("footprint_params", C.c_double * 4),
        ("n_candidates", C.c_int32),
        ("candidate_kind", C.c_int32 * 4),
        ("candidate_max_iter", C.c_int32 * 4),
        ("candidate_blend", C.c_int32),
        ("dual_warm_start", C.c_int32),
        ("mu_init_dual", C.c_double),
        ("candidate_param", C.c_double * 4),
        ("hessian_mode", C.c_int32),
        ("hybrid_cost_minimum_time", C.c_int32),
        ("cost_integration", C.c_int32),
        ("mu_strategy", C.c_int32), ("stage_data", C.c_int32), ("two_wave_min_batch", C.c_int32), ("line_search", C.c_int32),
        ("Q_offdiag", C.c_double * 3),
        ("R_offdiag", C.c_double),
        ("Qf_offdiag", C.c_double * 3),
        ("terminal_ball_S_offdiag", C.c_double * 3),
        ("acceptable_tol", C.c_double),
        ("acceptable_iter", C.c_int32),
        ("max_time_us", C.c_int32),
    ]


class MpcObstacles(C.Structure):
    """struct mpc_obstacles (include/mpc_hip.h): raw addresses (host or device)."""
    _fields_ = [
        ("n_obstacles", C.c_void_p),
        ("n_vertices", C.c_void_p),
        ("vertices", C.c_void_p),
        ("radius", C.c_void_p),
        ("velocity", C.c_void_p),
    ]


class MpcEvalOut(C.Structure):
    """struct mpc_eval_out (include/mpc_hip.h): raw addresses (host or device), each nullable."""
    _fields_ = [
        ("objective", C.c_void_p),
        ("eq_violation", C.c_void_p),
        ("ineq_violation", C.c_void_p),
        ("clearance", C.c_void_p),
        ("closest", C.c_void_p),
    ]


class MpcCycleParams(C.Structure):
    """struct mpc_cycle_params (include/mpc_hip.h): the controller / grid options of mpc_controller_step_batch*; field-for-field."""
    _fields_ = [
        ("n_ref", C.c_int32),
        ("outer_iterations", C.c_int32),
        ("adapt", C.c_int32),
        ("n_min", C.c_int32),
        ("n_max", C.c_int32),
        ("dt_hyst_ratio", C.c_double),
        ("warm_start", C.c_int32),
        ("force_reinit_num_steps", C.c_int32),
        ("force_reinit_new_goal_dist", C.c_double),
        ("force_reinit_new_goal_angular", C.c_double),
        ("initial_plan_estimate_orientation", C.c_int32),
        ("prefer_x_feedback", C.c_int32),
        ("reference_reinit_sampling", C.c_int32),
        ("period", C.c_double),
    ]


# enum mpc_reinit_cause: the bits of reinit_out[b] (0 = warm start from the slot's previous solution)
REINIT_FIRST, REINIT_NUM_STEPS, REINIT_GOAL_DIST, REINIT_GOAL_ANGULAR, REINIT_RESET, REINIT_PLAN_GUESS = 1, 2, 4, 8, 16, 32


class MpcPlanParams(C.Structure):
    """struct mpc_plan_params (include/mpc_hip.h): the plugin options and costmap geometry of mpc_plan_inputs_batch*; field-for-field."""
    _fields_ = [
        ("global_plan_prune_distance", C.c_double),
        ("max_global_plan_lookahead_dist", C.c_double),
        ("global_plan_viapoint_sep", C.c_double),
        ("xy_goal_tolerance", C.c_double),
        ("yaw_goal_tolerance", C.c_double),
        ("global_plan_overwrite_orientation", C.c_int32),
        ("moving_average_length", C.c_int32),
        ("costmap_size_x", C.c_int32),
        ("costmap_size_y", C.c_int32),
        ("resolution", C.c_double),
    ]


# enum mpc_plan_flag: the bits of flags[b] of mpc_plan_inputs_batch*
PLAN_GOAL_REACHED, PLAN_EMPTY, PLAN_TRUNCATED, PLAN_VIA_DROPPED, PLAN_GOAL_INJECTED = 1, 2, 4, 8, 16
# enum mpc_cmd_result: result[b] of mpc_commands_batch*
CMD_SUCCESS, CMD_GOAL_REACHED, CMD_PLAN_EMPTY, CMD_SOLVE_FAILED, CMD_INFEASIBLE, CMD_NOT_FINITE = 0, 1, 2, 3, 4, 5


# ---- the functions, one table per header: name -> (restype, argtypes), the one statement of the C ABI on the Python side.  A host / device pair shares one signature
# object.  HEADERS (below the tables) ties each table and each struct mirror to its header; _lib.load() binds every table of it to the one library, and tests/test_abi.py
# holds every row to its header's declaration and every mirror to the C compiler's layout.  PROTOTYPES is include/mpc_hip.h alone, and _lib.EXPORTS is its names.
_p = C.c_void_p      # a raw address (host numpy buffer or device pointer) or the opaque mpc_solver*
_i, _d, _rc = C.c_int32, C.c_double, C.c_int
_SOLVE = (_rc, [_p, _i] + [_p] * 7 + [_p] + [_p] * 5)      # s, B, x0, xf, u_prev, dt_prev, x_init, u_init, dt_init, const mpc_obstacles*, x_out, u_out, dt_out, status, iters
_STEP = [_p, _i] + [_p] * 7 + [_p] + [_i] * 4 + [_d] + [_p] * 5      # s, B, the seven inputs, obstacles, outer_iterations, adapt, n_min, n_max, dt_hyst_ratio, the five outputs
# s, B, p, plan, n_plan, plan_stride, x_feedback, feedback_age, reset, u_prev, dt_prev, obstacles, x_out, u_out, dt_out, status, iters, reinit_out
_CYCLE = [_p, _i, C.POINTER(MpcCycleParams), _p, _p, _i] + [_p] * 5 + [_p] + [_p] * 6
# s, B, cost, size_x, size_y, resolution, origin, robot_pose, behind_robot_dist, n_obstacles, n_vertices, vertices, dropped
_COSTMAP = (_rc, [_p, _i, _p, _i, _i, _d, _p, _p, _d, _p, _p, _p, _p])
# s, B, x, cost, size_x, size_y, resolution, origin, footprint_spec, n_spec, inscribed_radius, min_resolution_collision_check_angular, look_ahead_idx, feasible
_FEASIBLE = (_rc, [_p, _i, _p, _p, _i, _i, _d, _p, _p, _i, _d, _d, _i, _p])
_EVALUATE = (_rc, [_p, _i] + [_p] * 7 + [_p, C.POINTER(MpcEvalOut)])      # s, B, x0, xf, u_prev, dt_prev, x, u, dt, const mpc_obstacles*, const mpc_eval_out*
# s, B, p, global_plan, n_global, gstride, robot_pose, plan_begin, plan, n_plan, plan_stride, n_via, via, goal_idx, flags
_PLAN_INPUTS = (_rc, [_p, _i, C.POINTER(MpcPlanParams), _p, _p, _i, _p, _p, _p, _p, _i] + [_p] * 4)
_COMMANDS = (_rc, [_p, _i] + [_p] * 9)      # s, B, u_out, status, feasible, plan_flags, cmd, result, reset_next, u_prev_next, infeasible_count

PROTOTYPES = {
    "mpc_config_defaults": (None, [C.POINTER(MpcConfig)]),                                      # cfg
    "mpc_create": (_rc, [C.POINTER(MpcConfig), _i, _i, C.POINTER(C.c_void_p)]),                  # cfg, max_batch, device, out
    "mpc_reset": (_rc, [_p]),                                                                   # s
    "mpc_destroy": (None, [_p]),                                                                # s
    "mpc_solve_batch": _SOLVE, "mpc_solve_batch_device": _SOLVE,
    "mpc_step_batch": (_rc, _STEP + [_p]),                                                      # ..., n_grid_out
    "mpc_step_batch_device": (_rc, _STEP),
    "mpc_cycle_params_defaults": (None, [C.POINTER(MpcCycleParams)]),                           # p
    "mpc_controller_step_batch": (_rc, _CYCLE + [_p]),                                          # ..., n_grid_out
    "mpc_controller_step_batch_device": (_rc, _CYCLE),
    "mpc_controller_state": (_rc, [_p, _i, _p, _p, _p]),                                        # s, B, seq, empty, last_goal
    "mpc_set_grid_sizes": (_rc, [_p, _p, _i]),                                                  # s, n_grid, B
    "mpc_set_parameter_sets": (_rc, [_p, _i, _p, _i, _p]),                                      # s, n_sets, sets, B, set_of
    "mpc_set_via_points": (_rc, [_p, _i, _p, _p]),                                              # s, B, n_via, via
    "mpc_set_via_points_device": (_rc, [_p, _p, _p]),                                          # s, n_via, via
    "mpc_costmap_to_obstacles": _COSTMAP, "mpc_costmap_to_obstacles_device": _COSTMAP,
    "mpc_last_candidates": (_rc, [_p, _i, _p, _p]),                                             # s, B, winner, iters_total
    "mpc_last_rows_dropped": (_rc, [_p, _i, _p]),                                               # s, B, rows_dropped
    "mpc_check_feasibility": _FEASIBLE, "mpc_check_feasibility_device": _FEASIBLE,
    "mpc_evaluate_batch": _EVALUATE, "mpc_evaluate_batch_device": _EVALUATE,
    "mpc_plan_params_defaults": (None, [C.POINTER(MpcPlanParams)]),                             # p
    "mpc_plan_inputs_batch": _PLAN_INPUTS, "mpc_plan_inputs_batch_device": _PLAN_INPUTS,
    "mpc_commands_batch": _COMMANDS, "mpc_commands_batch_device": _COMMANDS,
    "mpc_grid_update_device": (_rc, [_p, _i, _p, _p, _p, _p, _i, _i, _i, _d]),                  # s, B, x0_new, x, u, dt, adapt, n_min, n_max, dt_hyst_ratio
    "mpc_get_grid_sizes": (_rc, [_p, _i, _p]),                                                  # s, B, n_grid
    "mpc_synchronize": (_rc, [_p]),                                                             # s
    "mpc_last_kernel_ms": (_rc, [_p, C.POINTER(C.c_float)]),                                    # s, ms
    "mpc_lds_bytes": (_rc, [_p, C.POINTER(C.c_int64)]),                                         # s, bytes
    "mpc_occupancy": (_rc, [_p, _i, C.POINTER(_i), C.POINTER(C.c_int64)]),                      # s, B, workgroups_per_cu, lds_bytes
    "mpc_last_error": (C.c_char_p, []),
    "mpc_version": (_i, []),
}


class MpcPool(C.Structure):
    """struct mpc_pool (include/mpc_fleet.h): P obstacles laid out like one instance of mpc_obstacles; raw addresses (host or device)."""
    _fields_ = [
        ("P", C.c_int32),
        ("n_vertices", C.c_void_p),
        ("vertices", C.c_void_p),
        ("radius", C.c_void_p),
        ("velocity", C.c_void_p),
    ]


class MpcPoolParams(C.Structure):
    """struct mpc_pool_params (include/mpc_fleet.h); field-for-field."""
    _fields_ = [
        ("reach", C.c_double),
        ("min_speed", C.c_double),
        ("append", C.c_int32),
    ]


# ---- include/mpc_fleet.h
# s, B, pool, robot_pose, self_index, params, n_obstacles, n_vertices, vertices, radius, velocity, dropped, n_taken
_FROM_POOL = (_rc, [_p, _i, C.POINTER(MpcPool), _p, _p, C.POINTER(MpcPoolParams)] + [_p] * 7)
# s, B, robot_pose, x, dt, status, robot_radius, robot_radius per robot, pool_offset, pool_n_vertices, pool_vertices, pool_radius, pool_velocity
_FLEET_POOL = (_rc, [_p, _i, _p, _p, _p, _p, _d, _p, _i, _p, _p, _p, _p])

FLEET_PROTOTYPES = {
    "mpc_pool_params_defaults": (None, [_p, C.POINTER(MpcPoolParams)]),                         # s, p
    "mpc_obstacles_from_pool": _FROM_POOL, "mpc_obstacles_from_pool_device": _FROM_POOL,
    "mpc_fleet_pool": _FLEET_POOL, "mpc_fleet_pool_device": _FLEET_POOL,
}


class MpcClusterParams(C.Structure):
    """struct mpc_cluster_params (include/mpc_costmap_clusters.h); field-for-field."""
    _fields_ = [
        ("behind_robot_dist", C.c_double),
        ("link_dist_sq", C.c_int32),
    ]


# ---- include/mpc_costmap_clusters.h
# s, B, cost, size_x, size_y, resolution, origin, robot_pose, params, n_obstacles, n_vertices, vertices, radius, velocity, dropped, info
_TO_POLYGONS = (_rc, [_p, _i, _p, _i, _i, _d, _p, _p, C.POINTER(MpcClusterParams)] + [_p] * 7)

CLUSTER_PROTOTYPES = {
    "mpc_cluster_params_defaults": (None, [C.POINTER(MpcClusterParams), _d, _d]),               # p, resolution, cluster_max_distance
    "mpc_costmap_to_polygons": _TO_POLYGONS, "mpc_costmap_to_polygons_device": _TO_POLYGONS,
    "mpc_last_costmap_ms": (_rc, [_p, C.POINTER(C.c_float)]),                                   # s, ms
}


class MpcLineParams(C.Structure):
    """struct mpc_line_params (include/mpc_costmap_lines.h); field-for-field."""
    _fields_ = [
        ("behind_robot_dist", C.c_double),
        ("link_dist_sq", C.c_int32),
        ("inlier_dist_sq", C.c_int32),
        ("min_inliers", C.c_int32),
        ("n_hypotheses", C.c_int32),
        ("remaining_outliers", C.c_int32),
    ]


# ---- include/mpc_costmap_lines.h
# s, B, cost, size_x, size_y, resolution, origin, robot_pose, params, n_obstacles, n_vertices, vertices, radius, velocity, dropped, info
_TO_LINES = (_rc, [_p, _i, _p, _i, _i, _d, _p, _p, C.POINTER(MpcLineParams)] + [_p] * 7)

LINE_PROTOTYPES = {
    "mpc_line_params_defaults": (None, [C.POINTER(MpcLineParams), _d, _d, _d]),                 # p, resolution, cluster_max_distance, ransac_inlier_distance
    "mpc_costmap_to_lines": _TO_LINES, "mpc_costmap_to_lines_device": _TO_LINES,
}


class MpcWindowParams(C.Structure):
    """struct mpc_window_params (include/mpc_costmap_window.h); field-for-field."""
    _fields_ = [
        ("map_origin", C.c_double * 2),
        ("map_resolution", C.c_double),
        ("lattice_anchor", C.c_double * 2),
        ("inscribed_radius", C.c_double),
        ("inflation_radius", C.c_double),
        ("cost_scaling_factor", C.c_double),
        ("map_size_x", C.c_int32),
        ("map_size_y", C.c_int32),
        ("outside_value", C.c_int32),
        ("inflate_unknown", C.c_int32),
    ]


# ---- include/mpc_costmap_window.h
# s, B, map, params, robot_pose, size_x, size_y, resolution, cost, origin, info
_WINDOW = (_rc, [_p, _i, _p, C.POINTER(MpcWindowParams), _p, _i, _i, _d, _p, _p, _p])

WINDOW_PROTOTYPES = {
    "mpc_window_params_defaults": (None, [C.POINTER(MpcWindowParams), _d, _i, _i]),             # p, map_resolution, map_size_x, map_size_y
    "mpc_costmap_window": _WINDOW, "mpc_costmap_window_device": _WINDOW,
}


# ---- the boundary, whole: header under include/ -> (its prototype table, {C struct: its mirror}).  A new header is one row here.
HEADERS = {
    "mpc_hip.h": (PROTOTYPES, {"mpc_config": MpcConfig, "mpc_obstacles": MpcObstacles, "mpc_eval_out": MpcEvalOut, "mpc_cycle_params": MpcCycleParams,
                               "mpc_plan_params": MpcPlanParams}),
    "mpc_fleet.h": (FLEET_PROTOTYPES, {"mpc_pool": MpcPool, "mpc_pool_params": MpcPoolParams}),
    "mpc_costmap_clusters.h": (CLUSTER_PROTOTYPES, {"mpc_cluster_params": MpcClusterParams}),
    "mpc_costmap_lines.h": (LINE_PROTOTYPES, {"mpc_line_params": MpcLineParams}),
    "mpc_costmap_window.h": (WINDOW_PROTOTYPES, {"mpc_window_params": MpcWindowParams}),
}


class MpcScanParams(C.Structure):
    """struct mpc_scan_params (include/mpc_costmap_scans.h); field-for-field."""
    _fields_ = [
        ("lattice_anchor", C.c_double * 2),
        ("sensor_pose", C.c_double * 3),
        ("angle_min", C.c_double),
        ("angle_increment", C.c_double),
        ("range_min", C.c_double),
        ("range_max", C.c_double),
        ("obstacle_range", C.c_double),
        ("raytrace_range", C.c_double),
        ("footprint_clear_radius", C.c_double),
        ("marking", C.c_int32),
        ("clearing", C.c_int32),
        ("inf_is_valid", C.c_int32),
        ("track_unknown", C.c_int32),
        ("combination_method", C.c_int32),
    ]


# ---- include/mpc_costmap_scans.h
# s, B, params, robot_pose, ranges, n_beams, keep, size_x, size_y, resolution, layer, layer_cell, cost, info
_SCANS = (_rc, [_p, _i, C.POINTER(MpcScanParams), _p, C.POINTER(C.c_float), _i, _p, _i, _i, _d, _p, _p, _p, _p])

SCAN_PROTOTYPES = {
    "mpc_scan_params_defaults": (None, [C.POINTER(MpcScanParams)]),                             # p
    "mpc_costmap_scans": _SCANS, "mpc_costmap_scans_device": _SCANS,
}

# Headers that came after tests/test_abi.py pinned HEADERS to its five tables and their 52 functions: the same row, bound by _lib.load() in the same loop, and held to
# its header by the same comparator in the header's own test module (tests/test_costmap_scans_abi.py).
LATER_HEADERS = {
    "mpc_costmap_scans.h": (SCAN_PROTOTYPES, {"mpc_scan_params": MpcScanParams}),
}


class MpcCastParams(C.Structure):
    """struct mpc_cast_params (include/mpc_scan_cast.h); field-for-field."""
    _fields_ = [
        ("map_origin", C.c_double * 2),
        ("map_resolution", C.c_double),
        ("sensor_pose", C.c_double * 3),
        ("angle_min", C.c_double),
        ("angle_increment", C.c_double),
        ("range_max", C.c_double),
        ("map_size_x", C.c_int32),
        ("map_size_y", C.c_int32),
        ("block_threshold", C.c_int32),
        ("unknown_blocks", C.c_int32),
        ("hit_point", C.c_int32),
        ("miss_is_inf", C.c_int32),
    ]


# ---- include/mpc_scan_cast.h
# s, B, map, params, robot_pose, pool, self_index, n_beams, ranges, hit, info
_CAST = (_rc, [_p, _i, _p, C.POINTER(MpcCastParams), _p, C.POINTER(MpcPool), _p, _i, C.POINTER(C.c_float), _p, _p])

CAST_PROTOTYPES = {
    "mpc_cast_params_defaults": (None, [C.POINTER(MpcCastParams), _d, _i, _i]),                  # p, map_resolution, map_size_x, map_size_y
    "mpc_scan_cast": _CAST, "mpc_scan_cast_device": _CAST,
}

# The registry that stays open: tests/test_abi.py pins HEADERS and tests/test_costmap_scans_abi.py pins LATER_HEADERS to the rows they were written for, so a header
# that comes after them is a row HERE, bound by _lib.load() in the same loop; its own test module holds the row to its header and does not count the others.  A row's
# mirrors are the structs its declarations name that mpc_hip.h does not have: the header's own and, for this one, mpc_fleet.h's pool.
OPEN_HEADERS = {
    "mpc_scan_cast.h": (CAST_PROTOTYPES, {"mpc_cast_params": MpcCastParams, "mpc_pool": MpcPool}),
}


DRIVE_DIFF, DRIVE_OMNI, DRIVE_CAR_STAGE, DRIVE_CAR_REAR = 0, 1, 2, 3      # MPC_DRIVE_* of include/mpc_plant.h


class MpcPlantParams(C.Structure):
    """struct mpc_plant_params (include/mpc_plant.h); field-for-field."""
    _fields_ = [
        ("map_origin", C.c_double * 2),
        ("map_resolution", C.c_double),
        ("interval", C.c_double),
        ("wheelbase", C.c_double),
        ("v_min", C.c_double * 3),
        ("v_max", C.c_double * 3),
        ("a_max", C.c_double * 3),
        ("footprint", (C.c_double * 2) * 16),
        ("n_footprint", C.c_int32),
        ("n_substeps", C.c_int32),
        ("drive", C.c_int32),
        ("map_size_x", C.c_int32),
        ("map_size_y", C.c_int32),
        ("block_threshold", C.c_int32),
        ("unknown_blocks", C.c_int32),
        ("outside_blocks", C.c_int32),
    ]


# ---- include/mpc_plant.h
# s, B, map, params, cmd, pool, self_index, pose, vel, stall, info
_PLANT = (_rc, [_p, _i, _p, C.POINTER(MpcPlantParams), _p, C.POINTER(MpcPool), _p, _p, _p, _p, _p])

PLANT_PROTOTYPES = {
    "mpc_plant_params_defaults": (None, [C.POINTER(MpcPlantParams), _d, _i, _i]),                # p, map_resolution, map_size_x, map_size_y
    "mpc_plant_step": _PLANT, "mpc_plant_step_device": _PLANT,
}

OPEN_HEADERS["mpc_plant.h"] = (PLANT_PROTOTYPES, {"mpc_plant_params": MpcPlantParams, "mpc_pool": MpcPool})


def _diag_offdiag(w, dim):
    """a weight given as its diagonal or as a full dim x dim matrix -> (diagonal, off-diagonal terms (0,1)[, (0,2), (1,2)] of the symmetric part)"""
    rows = [list(r) if hasattr(r, "__len__") else None for r in w]
    if rows and rows[0] is not None:
        m = [[0.5 * (float(rows[i][j]) + float(rows[j][i])) for j in range(dim)] for i in range(dim)]
        return [m[i][i] for i in range(dim)], ([m[0][1], m[0][2], m[1][2]] if dim == 3 else [m[0][1]])
    return [float(v) for v in w], [0.0] * (3 if dim == 3 else 1)


def make_config(model=MODEL_UNICYCLE, model_params=(0.5, 1.0), n=20, dt_ref=0.3, dt_free=True, dt_lb=0.0, dt_ub=10.0,
                xf_fixed=(True, True, True), objective=OBJ_MIN_TIME, Q=(0, 0, 0), R=(0, 0), integral_form=False, Qf=None,
                u_lb=(-0.2, -0.3), u_ub=(0.4, 0.3), du_lb=(-INF, -INF), du_ub=(INF, INF), max_iter=100, tol=1e-8,
                mu_init=0.1, precision=FP64, min_obstacle_dist=0.5, force_inclusion_dist=0.5, cutoff_dist=2.0,
                footprint_kind=0, footprint_radius=0.0, max_obstacles=0, max_vertices=1, max_obstacle_rows=4, mu_init_warm=0.0, collocation=COLLOC_FORWARD,
                terminal_ball_S=None, terminal_ball_gamma=1.0, vp_position_weight=1e-3, vp_orientation_weight=0.0,
                via_points_ordered=False, max_via_points=0, footprint_params=(0.0, 0.0, 0.0, 0.0),
                enable_dynamic_obstacles=False, footprint_vertices=(), candidates=(), candidate_max_iter=(), candidate_blend=0, dual_warm_start=False, mu_init_dual=0.0, candidate_param=(), hessian_mode=0,
                hybrid_cost_minimum_time=False, cost_integration=COST_LEFT_SUM, acceptable_tol=0.0, acceptable_iter=0, mu_strategy=0, max_cpu_time=0.0, stage_data=STAGE_AUTO, two_wave_min_batch=0, line_search=LS_DEFAULT) -> MpcConfig:
    """Q, R, Qf, terminal_ball_S: the diagonal (3 / 2 / 3 / 3 values) or the full matrix (nested 3 x 3 / 2 x 2; its symmetric part is used)."""
    c = MpcConfig()
    c.model = model
    mp = list(model_params) + [0.0] * 4
    for i in range(4):
        c.model_params[i] = mp[i]
    c.n = n
    c.dt_ref = dt_ref
    c.dt_free = int(bool(dt_free))
    c.dt_lb, c.dt_ub = dt_lb, dt_ub
    Qd, Qo = _diag_offdiag(Q, 3)
    Qfd, Qfo = _diag_offdiag(Qf if Qf is not None else (0, 0, 0), 3)
    Rd, Ro = _diag_offdiag(R, 2)
    for i in range(3):
        c.xf_fixed[i] = int(bool(xf_fixed[i]))
        c.Q[i], c.Q_offdiag[i] = Qd[i], Qo[i]
        c.Qf[i], c.Qf_offdiag[i] = Qfd[i], Qfo[i]
    c.R_offdiag = Ro[0]
    c.collocation = collocation
    c.objective = objective
    c.integral_form = int(bool(integral_form))
    c.has_Qf = int(Qf is not None)
    for j in range(2):
        c.R[j] = Rd[j]
        c.u_lb[j], c.u_ub[j] = u_lb[j], u_ub[j]
        c.du_lb[j], c.du_ub[j] = du_lb[j], du_ub[j]
    c.max_iter = max_iter
    c.tol = tol
    c.mu_init = mu_init
    c.precision = precision
    c.min_obstacle_dist, c.force_inclusion_dist, c.cutoff_dist = min_obstacle_dist, force_inclusion_dist, cutoff_dist
    c.footprint_kind, c.footprint_radius = footprint_kind, footprint_radius
    c.max_obstacles, c.max_vertices, c.max_obstacle_rows = max_obstacles, max_vertices, max_obstacle_rows
    c.mu_init_warm = mu_init_warm
    c.terminal_ball = int(terminal_ball_S is not None)
    Sd, So = _diag_offdiag(terminal_ball_S if terminal_ball_S is not None else (0, 0, 0), 3)
    for i in range(3):
        c.terminal_ball_S[i], c.terminal_ball_S_offdiag[i] = Sd[i], So[i]
    c.terminal_ball_gamma = terminal_ball_gamma
    c.vp_position_weight, c.vp_orientation_weight = vp_position_weight, vp_orientation_weight
    c.via_points_ordered, c.max_via_points = int(bool(via_points_ordered)), max_via_points
    for i in range(4):
        c.footprint_params[i] = footprint_params[i]
    c.enable_dynamic_obstacles = int(bool(enable_dynamic_obstacles))
    fv = []
    for row in footprint_vertices:          # flat (x0, y0, x1, ...) or nested ((x0, y0), ...)
        fv.extend([float(v) for v in row] if hasattr(row, "__len__") else [float(row)])
    c.footprint_n_vertices = len(fv) // 2
    for i, x in enumerate(fv[:32]):
        c.footprint_vertices[i] = x
    # candidate initial trajectories: kinds (CAND_*) in priority order, per-candidate iteration caps (0 / missing -> max_iter)
    c.n_candidates = len(candidates)
    for i, k in enumerate(candidates[:MAX_CANDIDATES]):
        c.candidate_kind[i] = int(k)
        c.candidate_max_iter[i] = int(candidate_max_iter[i]) if i < len(candidate_max_iter) else 0
        c.candidate_param[i] = float(candidate_param[i]) if i < len(candidate_param) else 0.0
    c.candidate_blend = int(candidate_blend)
    c.dual_warm_start = int(bool(dual_warm_start))
    c.mu_init_dual = float(mu_init_dual)
    c.hessian_mode = int(hessian_mode)
    c.mu_strategy = int(mu_strategy)          # MU_ADAPTIVE (0, default) | MU_MONOTONE
    c.stage_data = int(stage_data)            # STAGE_AUTO (0, default) | STAGE_LDS | STAGE_GLOBAL
    c.line_search = int(line_search)          # LS_DEFAULT (0) | LS_MERIT | LS_FILTER
    c.two_wave_min_batch = int(two_wave_min_batch)      # 0: the default threshold (4096 instances per launch), negative: never the two-waves-per-SIMD kernel
    c.hybrid_cost_minimum_time = int(bool(hybrid_cost_minimum_time))
    c.cost_integration = int(cost_integration)
    c.acceptable_tol, c.acceptable_iter = float(acceptable_tol), int(acceptable_iter)      # 0 = Ipopt's defaults (1e-6, 15), negative = off
    # solver/ipopt/max_cpu_time (seconds; <= 0 = none; beyond the int32 range of microseconds, ~2147 s, = none: same rule as include/mpc_params.hpp)
    c.max_time_us = int(max_cpu_time * 1e6 + 0.5) if max_cpu_time and 0 < max_cpu_time and max_cpu_time * 1e6 + 0.5 < 2147483647.0 else 0
    return c


def config_carlike_min_time(n=50, **kw) -> MpcConfig:
    """BASELINE.json config 2: mpc_local_planner_examples/cfg/carlike/mpc_local_planner_params.yaml:7-16,46-65."""
    d = dict(model=MODEL_SIMPLE_CAR, model_params=(0.4,), n=n, dt_ref=0.3, dt_free=True, dt_lb=0.0, dt_ub=10.0,
             xf_fixed=(True, True, True), objective=OBJ_MIN_TIME, u_lb=(-0.2, -1.4), u_ub=(0.4, 1.4),
             du_lb=(-0.5, -0.5), du_ub=(0.5, 0.5))
    d.update(kw)
    return make_config(**d)


def config_unicycle_quadratic(n=20, **kw) -> MpcConfig:
    """BASELINE.json config 1: .../cfg/diff_drive/mpc_local_planner_params_quadratic_form.yaml:7-14,33-41,53-61."""
    d = dict(model=MODEL_UNICYCLE, model_params=(0.0,), n=n, dt_ref=0.3, dt_free=False,
             xf_fixed=(False, False, False), objective=OBJ_QUADRATIC, Q=(2.0, 2.0, 0.25), R=(0.1, 0.05),
             Qf=(10.0, 10.0, 0.5), u_lb=(-0.2, -0.3), u_ub=(0.4, 0.3), du_lb=(-0.2, -0.2), du_ub=(0.2, 0.2),
             min_obstacle_dist=0.2, force_inclusion_dist=0.5, cutoff_dist=2.5)
    d.update(kw)
    return make_config(**d)


def config_bicycle_min_time(n=120, **kw) -> MpcConfig:
    """BASELINE.json config 5; lr = lf = 1.0 (src/controller.cpp:366-369)."""
    return make_config(model=MODEL_KINEMATIC_BICYCLE, model_params=(1.0, 1.0), n=n, dt_ref=0.3, dt_free=True,
                       xf_fixed=(True, True, True), objective=OBJ_MIN_TIME, u_lb=(-0.2, -1.5), u_ub=(0.4, 1.5),
                       du_lb=(-0.5, -0.5), du_ub=(0.5, 0.5), **kw)
