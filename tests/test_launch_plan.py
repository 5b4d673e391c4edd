"""CPU test of the launch plan (mpc_launch_plan.hpp) and of the configuration checks of mpc_create (mpc_problem.hpp::config_error), compiled for the host with g++
by a tests-only harness (tests/host_harness/launch_plan_host.cpp): for every configuration the kernel level, the form per precision, the dynamic LDS of every kernel a
handle launches, the two-wave choice at 4095 / 4096 instances and the pool size on a fake device, or the text mpc_create refuses it with.  The table was recorded from
the decision code of mpc_capi.hip before the plan existed; it changes only when a rule does."""
import ctypes as C

import pytest

from mpc_local_planner_amd import _abi as A
import _harness

CANDS = dict(candidates=(A.CAND_REFERENCE, A.CAND_HERMITE_FF, A.CAND_HERMITE_FR), candidate_max_iter=(40, 40, 40), candidate_param=(0.0, 2.0, 1.5))
LINE_MOVING = dict(footprint_kind=2, footprint_params=(0.0, 0.0, 0.4, 0.0), enable_dynamic_obstacles=True, max_obstacles=3, max_vertices=1, max_obstacle_rows=4)
CASES = {
    "config1_unicycle_quadratic_n20": lambda: A.config_unicycle_quadratic(20),
    "config2_carlike_n50": lambda: A.config_carlike_min_time(50),
    "config3_unicycle_n80_16polygons": lambda: A.config_unicycle_quadratic(80, max_obstacles=16, max_vertices=6, max_obstacle_rows=4, max_iter=60),
    "config4_carlike_n50_candidates": lambda: A.config_carlike_min_time(50, **CANDS),
    "config5_bicycle_n120_fp32": lambda: A.config_bicycle_min_time(120, precision=A.FP32, tol=1e-4),
    "config5_bicycle_n120_fp64": lambda: A.config_bicycle_min_time(120),
    "carlike_n20": lambda: A.config_carlike_min_time(20),
    "carlike_n24": lambda: A.config_carlike_min_time(24),
    "carlike_n12": lambda: A.config_carlike_min_time(12),
    "carlike_n120_fp32": lambda: A.config_carlike_min_time(120, precision=A.FP32),
    "bicycle_n120_mixed": lambda: A.config_bicycle_min_time(120, precision=A.MIXED),
    "bicycle_n200_mixed": lambda: A.config_bicycle_min_time(200, precision=A.MIXED),
    "bicycle_n200_mixed_global": lambda: A.config_bicycle_min_time(200, precision=A.MIXED, stage_data=A.STAGE_GLOBAL),
    "bicycle_n120_mixed_lds": lambda: A.config_bicycle_min_time(120, precision=A.MIXED, stage_data=A.STAGE_LDS),
    "carlike_n50_lds": lambda: A.config_carlike_min_time(50, stage_data=A.STAGE_LDS),
    "carlike_n50_global": lambda: A.config_carlike_min_time(50, stage_data=A.STAGE_GLOBAL),
    "carlike_n20_global": lambda: A.config_carlike_min_time(20, stage_data=A.STAGE_GLOBAL),
    "carlike_n20_lds": lambda: A.config_carlike_min_time(20, stage_data=A.STAGE_LDS),
    "bicycle_n120_lds": lambda: A.config_bicycle_min_time(120, stage_data=A.STAGE_LDS),
    "bicycle_n120_fp32_lds": lambda: A.config_bicycle_min_time(120, precision=A.FP32, stage_data=A.STAGE_LDS),
    "bicycle_n120_fp32_global": lambda: A.config_bicycle_min_time(120, precision=A.FP32, stage_data=A.STAGE_GLOBAL),
    "bicycle_n300_fp64": lambda: A.config_bicycle_min_time(300),
    "carlike_n80_fp32": lambda: A.config_carlike_min_time(80, precision=A.FP32),
    "carlike_n50_via_points": lambda: A.config_carlike_min_time(50, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=8),
    "unicycle_quadratic_n20_offdiag": lambda: A.config_unicycle_quadratic(20, Q=((2.0, 0.3, 0.0), (0.3, 2.0, 0.0), (0.0, 0.0, 0.25))),
    "unicycle_quadratic_n20_trapezoid_dt_free": lambda: A.config_unicycle_quadratic(20, dt_free=True, integral_form=True, cost_integration=A.COST_TRAPEZOIDAL),
    "unicycle_quadratic_n20_integral_dt_free": lambda: A.config_unicycle_quadratic(20, dt_free=True, integral_form=True),
    "unicycle_quadratic_n20_hybrid": lambda: A.config_unicycle_quadratic(20, hybrid_cost_minimum_time=True),
    "unicycle_quadratic_n20_ball": lambda: A.config_unicycle_quadratic(20, terminal_ball_S=(1.0, 1.0, 0.1)),
    "carlike_n20_convexified": lambda: A.config_carlike_min_time(20, hessian_mode=1),
    "carlike_n50_crank_nicolson": lambda: A.config_carlike_min_time(50, collocation=A.COLLOC_CRANK_NICOLSON),
    "carlike_n30_point_obstacles": lambda: A.config_carlike_min_time(30, max_obstacles=8, max_vertices=4, max_obstacle_rows=4),
    "carlike_n30_line_moving_obstacles": lambda: A.config_carlike_min_time(30, **LINE_MOVING),
    "carlike_n120_line_moving_obstacles": lambda: A.config_carlike_min_time(120, **LINE_MOVING),
    "carlike_n120_line_moving_obstacles_lds": lambda: A.config_carlike_min_time(120, stage_data=A.STAGE_LDS, **LINE_MOVING),
    "carlike_n20_two_wave_min_batch_-1": lambda: A.config_carlike_min_time(20, two_wave_min_batch=-1),
    "carlike_n20_two_wave_min_batch_0": lambda: A.config_carlike_min_time(20, two_wave_min_batch=0),
    "carlike_n20_two_wave_min_batch_1": lambda: A.config_carlike_min_time(20, two_wave_min_batch=1),
    "carlike_n20_fp32": lambda: A.config_carlike_min_time(20, precision=A.FP32),
    "carlike_n20_dual_warm_start": lambda: A.config_carlike_min_time(20, dual_warm_start=True),
    # rejected
    "reject_n2": lambda: A.config_carlike_min_time(2),
    "reject_stage_data_7": lambda: A.config_carlike_min_time(50, stage_data=7),
    "reject_mixed_with_obstacles": lambda: A.config_carlike_min_time(30, precision=A.MIXED, max_obstacles=4),
    "reject_lds_form_n250": lambda: A.config_bicycle_min_time(250, stage_data=A.STAGE_LDS),
    "reject_n700": lambda: A.config_carlike_min_time(700),
    "reject_precision_5": lambda: A.config_carlike_min_time(20, precision=5),
    "reject_line_search_9": lambda: A.config_carlike_min_time(20, line_search=9),
    "reject_dt_ref_outside_bounds": lambda: A.config_carlike_min_time(20, dt_lb=0.5),
}

# level, gs64, gs32, mpc_lds_bytes | fp64 launch of 4095 instances: global form, two waves, LDS | of 4096: the same | fp32 launch of 4096: global form, LDS |
# pool blocks per XCD (256 CUs, 8 XCCs, 4 workgroups per CU), block bytes, kept-multiplier words | the kernel that sizes the pool: global form, LDS   (-1: no launch of that precision)
TABLE = {
    'config1_unicycle_quadratic_n20': (0, 0, 0, 16848, 0, 0, 16848, 0, 1, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'config2_carlike_n50': (0, 0, 0, 40128, 0, 0, 40128, 0, 0, 40128, -1, -1, 0, 0, 554, 0, 40128),
    'config3_unicycle_n80_16polygons': (0, 1, 0, 33200, 1, 0, 33200, 1, 0, 33200, -1, -1, 256, 65024, 884, 1, 33200),
    'config4_carlike_n50_candidates': (0, 0, 0, 40128, 0, 0, 40128, 0, 0, 40128, -1, -1, 0, 0, 554, 0, 40128),
    'config5_bicycle_n120_fp32': (0, 0, 1, 17552, -1, -1, -1, -1, -1, -1, 1, 17552, 256, 36352, 1324, 1, 17552),
    'config5_bicycle_n120_fp64': (0, 1, 0, 34928, 1, 0, 34928, 1, 0, 34928, -1, -1, 256, 72704, 1324, 1, 34928),
    'carlike_n20': (0, 0, 0, 16848, 0, 0, 16848, 0, 1, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'carlike_n24': (0, 0, 0, 19952, 0, 0, 19952, 0, 1, 19952, -1, -1, 0, 0, 268, 0, 19952),
    'carlike_n12': (0, 0, 0, 10640, 0, 0, 10640, 0, 1, 10640, -1, -1, 0, 0, 136, 0, 10640),
    'carlike_n120_fp32': (0, 0, 1, 17072, -1, -1, -1, -1, -1, -1, 1, 17072, 256, 36352, 1324, 1, 17072),
    'bicycle_n120_mixed': (0, 0, 0, 95408, 0, 0, 95408, 0, 0, 95408, 0, 47792, 0, 0, 1324, 0, 95408),
    'bicycle_n200_mixed': (0, 0, 1, 158128, 0, 0, 158128, 0, 0, 158128, 1, 28752, 256, 59392, 2204, 0, 158128),
    'bicycle_n200_mixed_global': (0, 1, 1, 57328, 1, 0, 57328, 1, 0, 57328, 1, 28752, 256, 118784, 2204, 1, 57328),
    'bicycle_n120_mixed_lds': (0, 0, 0, 95408, 0, 0, 95408, 0, 0, 95408, 0, 47792, 0, 0, 1324, 0, 95408),
    'carlike_n50_lds': (0, 0, 0, 40128, 0, 0, 40128, 0, 0, 40128, -1, -1, 0, 0, 554, 0, 40128),
    'carlike_n50_global': (0, 1, 0, 14928, 1, 0, 14928, 1, 0, 14928, -1, -1, 256, 33152, 554, 1, 14928),
    'carlike_n20_global': (0, 1, 0, 6768, 1, 0, 6768, 1, 0, 6768, -1, -1, 256, 15104, 224, 1, 6768),
    'carlike_n20_lds': (0, 0, 0, 16848, 0, 0, 16848, 0, 0, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'bicycle_n120_lds': (0, 0, 0, 95408, 0, 0, 95408, 0, 0, 95408, -1, -1, 0, 0, 1324, 0, 95408),
    'bicycle_n120_fp32_lds': (0, 0, 0, 47792, -1, -1, -1, -1, -1, -1, 0, 47792, 0, 0, 1324, 0, 47792),
    'bicycle_n120_fp32_global': (0, 0, 1, 17552, -1, -1, -1, -1, -1, -1, 1, 17552, 256, 36352, 1324, 1, 17552),
    'bicycle_n300_fp64': (0, 1, 0, 85328, 1, 0, 85328, 1, 0, 85328, -1, -1, 256, 176384, 3304, 1, 85328),
    'carlike_n80_fp32': (0, 0, 0, 31792, -1, -1, -1, -1, -1, -1, 0, 31792, 0, 0, 884, 0, 31792),
    'carlike_n50_via_points': (1, 0, 0, 41984, 0, 0, 41984, 0, 0, 41984, -1, -1, 0, 0, 554, 0, 41984),
    'unicycle_quadratic_n20_offdiag': (2, 0, 0, 17488, 0, 0, 17488, 0, 0, 17488, -1, -1, 0, 0, 224, 0, 17488),
    'unicycle_quadratic_n20_trapezoid_dt_free': (2, 0, 0, 17488, 0, 0, 17488, 0, 0, 17488, -1, -1, 0, 0, 224, 0, 17488),
    'unicycle_quadratic_n20_integral_dt_free': (1, 0, 0, 17488, 0, 0, 17488, 0, 0, 17488, -1, -1, 0, 0, 224, 0, 17488),
    'unicycle_quadratic_n20_hybrid': (0, 0, 0, 16848, 0, 0, 16848, 0, 1, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'unicycle_quadratic_n20_ball': (1, 0, 0, 17488, 0, 0, 17488, 0, 0, 17488, -1, -1, 0, 0, 224, 0, 17488),
    'carlike_n20_convexified': (1, 0, 0, 17488, 0, 0, 17488, 0, 0, 17488, -1, -1, 0, 0, 224, 0, 17488),
    'carlike_n50_crank_nicolson': (0, 0, 0, 40928, 0, 0, 40928, 0, 0, 40928, -1, -1, 0, 0, 554, 0, 40928),
    'carlike_n30_point_obstacles': (0, 0, 0, 32144, 0, 0, 32144, 0, 0, 32144, -1, -1, 256, 2048, 334, 0, 32144),
    'carlike_n30_line_moving_obstacles': (1, 0, 0, 40400, 0, 0, 40400, 0, 0, 40400, -1, -1, 256, 2048, 334, 0, 40400),
    'carlike_n120_line_moving_obstacles': (1, 1, 0, 42800, 1, 0, 42800, 1, 0, 42800, -1, -1, 256, 134400, 1324, 1, 42800),
    'carlike_n120_line_moving_obstacles_lds': (1, 0, 0, 157040, 0, 0, 157040, 0, 0, 157040, -1, -1, 256, 7808, 1324, 0, 157040),
    'carlike_n20_two_wave_min_batch_-1': (0, 0, 0, 16848, 0, 0, 16848, 0, 0, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'carlike_n20_two_wave_min_batch_0': (0, 0, 0, 16848, 0, 0, 16848, 0, 1, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'carlike_n20_two_wave_min_batch_1': (0, 0, 0, 16848, 0, 1, 16848, 0, 1, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'carlike_n20_fp32': (0, 0, 0, 8512, -1, -1, -1, -1, -1, -1, 0, 8512, 0, 0, 224, 0, 8512),
    'carlike_n20_dual_warm_start': (0, 0, 0, 16848, 0, 0, 16848, 0, 1, 16848, -1, -1, 0, 0, 224, 0, 16848),
    'reject_n2': 'mpc_create: n out of range [3,4096]',
    'reject_stage_data_7': 'mpc_create: unknown stage_data',
    'reject_mixed_with_obstacles': 'mpc_create: MPC_MIXED is implemented for problems without clearance rows and via-points (their association would be redone by the refinement phase)',
    'reject_lds_form_n250': 'mpc_create: the working set of one instance (n, max_obstacles, max_vertices, precision) does not fit in the 160 KB of LDS of a compute unit (about n <= 215 grid points in fp64 without obstacles; n <= 590 with the factorisation data in global memory)',
    'reject_n700': 'mpc_create: the working set of one instance (n, max_obstacles, max_vertices, precision) does not fit in the 160 KB of LDS of a compute unit (about n <= 215 grid points in fp64 without obstacles; n <= 590 with the factorisation data in global memory)',
    'reject_precision_5': 'mpc_create: unknown precision',
    'reject_line_search_9': 'mpc_create: unknown line_search',
    'reject_dt_ref_outside_bounds': 'mpc_create: dt_ref must lie in [dt_lb, dt_ub] on the variable grid',
}


@pytest.fixture(scope="module")
def plan():
    lib = C.CDLL(_harness.shared("launch_plan_host"))
    lib.plan_row.restype = C.c_int
    return lib


def test_the_table_covers_every_configuration():
    assert sorted(TABLE) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_plan_matches_the_table(plan, name):
    cfg = CASES[name]()
    out = (C.c_int64 * 17)()
    err = C.create_string_buffer(512)
    rc = plan.plan_row(C.byref(cfg), out, err, 512)
    got = err.value.decode() if rc else tuple(out)
    assert got == TABLE[name]
