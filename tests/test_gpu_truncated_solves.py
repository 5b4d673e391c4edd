"""-m gpu: the device's iterate after 1, 2 and 4 interior-point iterations against the refined dense oracle, through mpc_solve_batch alone.

Every other GPU test of the solver compares answers after the loop has converged (the stop test is the KKT residual: a slightly wrong Newton step costs iterations and
lands on the same point) or two device forms with each other bit for bit (an old error is carried forward unchanged).  Here mpc_config.max_iter = cap makes the kernel
return its cap-th iterate with status max_iter (mpc_solve_kernel.hpp writes x, u and dt of candidate 0 whatever the status), and that iterate is held to the REFERENCE of
tests/_truncated.py: the numpy dense interior-point method with every KKT solve refined in extended precision.  The yardstick per instance is e_cpu[i], the largest
distance of an fp64 CPU solver (unrefined dense LU, the C oracle's banded LU, the host build of the kernel core) to that reference -- what a change of linear algebra
alone moves the iterate by; tests/test_truncated_reference.py shows it stays below 1e-10 on every instance, so no instance is undecidable and none is left out:

    status == 1 and iters == cap everywhere,  e_dev[i] <= K * max(e_cpu[i], 1e-13)          (fp32: e_dev[i] <= K32 * max(e_cpu32[i], 1e-6))

and, not a measurement: K * max(e_cpu[i], 1e-13) <= 1e-9 for every fp64 case.

The ABI cannot show whether a given factorisation took the partitioned sweeps.  The cases rest on the static rule pit_enabled() (mpc_wave_pit.inc: n >= 40, kernel level
< 2, not the two-wave kernel) and on the barrier parameter of the first iterations (mu_init = 0.1) being far above pit_floor() (max(tol, 1e-6); 1e-4 with clearance
rows), below which the serial sweeps take over.  The level-2 case therefore runs the SERIAL sweeps at n = 43, the fixed_layout cases the compile-time n = 50 layout with
its lane-parallel combine inertia, the ragged case both sides of the threshold in one launch.

The endgame_* families are the other side of that rule: WARM cases (tests/_truncated.py) -- the second control cycle of the cold problem, every solver started from cycle 1's
unshifted solution through x_init / u_init / dt_init, the barrier parameter started at mpc_config.mu_init (mu_init_warm = 0, dual_warm_start off) a factor 4 BELOW the floor
(the serial sweeps on the layouts built for the partitioned ones: n = 40, 43, 65, the fixed n = 50 layout, the global form, the ragged launch) or a factor 4 ABOVE it (the
partitioned sweeps where mu / s^2 is largest).  tests/test_truncated_reference.py section (f) asserts that every counted iteration stayed on its side by a factor 2, and
tests/test_gpu_dev_variants.py reads the sweeps that ran off the prof library's counters.  Below the floor the CPU solvers themselves spread past 1e-10 by the fourth
iteration on every seed tried, so those cases (and carlike n = 43 above) have caps (1, 2); the steps of all of them are short (fraction to the boundary 1e-5 .. 1e-3 of a
Newton step 1e4 .. 1e5 long), which the yardstick already reflects.

K and K32 are measured, not chosen: the next power of two at or above 4 x the worst e_dev[i] / max(e_cpu[i], floor) seen on the MI355X, per family (the factor 4 covers
other seeds and another compiler's contraction choices).  Measured (worst ratio over the family's cases, instances and caps):

    family       case                                       cap 1   cap 2   cap 4   worst e_dev   worst K x yardstick
    serial       serial_carlike_n3                           0.00    0.63    0.92   2.6e-13       3.7e-11
    serial       serial_carlike_n4                           0.01    0.93    0.23   9.3e-14       5.7e-12
    serial       serial_carlike_n8                           0.02    0.02    0.03   6.7e-15       4.7e-12
    serial       serial_carlike_n39                          0.19    0.20    1.58   1.0e-12       5.1e-12
    serial       serial_unicycle_n8                          0.00    0.04    0.04   3.8e-15       8.0e-13
    serial       serial_bicycle_n8                           0.01    0.01    0.02   1.7e-14       6.4e-11
    serial       -> worst ratio 1.58, x 4 = 6.33, K = 8  
    partitioned  pit_carlike_n40                             0.34    0.57    0.58   2.9e-13       3.2e-11
    partitioned  pit_carlike_n41                             0.18    1.22    1.29   1.8e-13       1.9e-11
    partitioned  pit_carlike_n42                             0.10    2.19    1.96   2.4e-13       7.0e-12
    partitioned  pit_carlike_n43                             0.36    9.45    9.74   1.1e-12       2.6e-11
    partitioned  pit_carlike_n65                             0.22    1.96    2.26   1.9e-12       1.5e-10
    partitioned  pit_unicycle_n43                            0.04    0.02    0.16   1.6e-14       6.4e-12
    partitioned  pit_bicycle_n43                             0.25    1.45    3.98   4.1e-13       2.0e-11
    partitioned  -> worst ratio 9.74, x 4 = 38.98, K = 64
    fixed_layout fixed_carlike_n50                           0.17    0.46    0.43   4.6e-14       7.5e-13
    fixed_layout fixed_carlike_n50_dt_prev0                  0.20    0.25    0.92   9.2e-14       1.6e-12
    fixed_layout -> worst ratio 0.92, x 4 = 3.69, K = 4  
    forms        global_carlike_n8                           0.02    0.02    0.03   6.7e-15       3.8e-11
    forms        global_carlike_n43                          0.36    9.45    9.74   1.1e-12       2.6e-11
    forms        global_carlike_n50                          0.17    0.46    0.43   4.6e-14       1.2e-11
    forms        two_wave_carlike_n8                         0.02    0.02    0.03   6.7e-15       3.8e-11
    forms        two_wave_carlike_n24                        0.16    0.25    2.97   7.5e-13       4.9e-11
    forms        ragged_carlike_39_40_43_50                  0.19    0.46    1.58   1.0e-12       4.1e-11
    forms        -> worst ratio 9.74, x 4 = 38.98, K = 64
    clearance    obst_unicycle_points_n43                    0.03    0.02    0.02   2.7e-15       2.5e-14
    clearance    obst_unicycle_polygons_n43                  0.03    0.03    0.02   3.2e-15       3.0e-14
    clearance    -> worst ratio 0.03, x 4 = 0.13, K = 0.25
    level1       level1_carlike_line_moving_n43              0.35    1.83    1.42   1.8e-13       2.8e-11
    level1       level1_unicycle_integral_free_dt_n43        0.58    7.01   13.28   1.3e-12       7.6e-11
    level1       -> worst ratio 13.28, x 4 = 53.13, K = 64
    level2       level2_unicycle_full_weights_ball_n43       0.04    0.03    0.02   4.0e-15       2.5e-14
    level2       -> worst ratio 0.04, x 4 = 0.16, K = 0.25
    collocation  colloc_carlike_midpoint_n43                 0.36    0.34    0.81   7.2e-13       5.1e-11
    collocation  colloc_carlike_crank_nicolson_n43           0.77    0.95    3.08   7.1e-12       3.7e-11
    collocation  -> worst ratio 3.08, x 4 = 12.30, K = 16
    algorithm    algo_mu_monotone_carlike_n43                   -    9.45    9.74   1.1e-12       2.6e-11
    algorithm    algo_ls_merit_carlike_n43                      -    4.79   10.16   2.2e-12       2.6e-11
    algorithm    -> worst ratio 10.16, x 4 = 40.63, K = 64
    fp32         fp32_carlike_n8                             1.00    1.00    1.00   8.3e-03       6.6e-02
    fp32         fp32_carlike_n43                            1.09    1.07    1.15   1.2e-03       9.7e-03
    fp32         -> worst ratio 1.15, x 4 = 4.61, K32 = 8
    endgame_serial    endgame_serial_carlike_n40_below              0.88    0.78       -   9.2e-14       7.6e-11
    endgame_serial    endgame_serial_carlike_n43_below              1.12    1.08       -   1.1e-13       1.4e-11
    endgame_serial    endgame_serial_carlike_n65_below              0.76    0.83       -   3.7e-13       1.7e-10
    endgame_serial    endgame_serial_bicycle_n43_below              0.18    1.09       -   1.3e-12       1.4e-10
    endgame_serial    -> worst ratio 1.12, x 4 = 4.48, K = 8
    endgame_pit       endgame_pit_carlike_n43_above                 0.35    0.34       -   3.7e-14       1.7e-12
    endgame_pit       endgame_pit_carlike_n65_above                 0.15    0.22    0.94   1.8e-12       4.3e-11
    endgame_pit       endgame_pit_bicycle_n43_above                 0.01    0.55    0.57   3.2e-12       2.3e-11
    endgame_pit       -> worst ratio 0.94, x 4 = 3.76, K = 4
    endgame_fixed     endgame_fixed_carlike_n50_below               1.25    1.34       -   2.8e-13       4.1e-11
    endgame_fixed     endgame_fixed_carlike_n50_above               0.71    0.78    0.99   9.9e-14       5.8e-11
    endgame_fixed     -> worst ratio 1.34, x 4 = 5.36, K = 8
    endgame_forms     endgame_global_carlike_n50_below              1.25    1.34       -   2.8e-13       4.1e-11
    endgame_forms     endgame_ragged_carlike_39_40_43_50_below      1.62    1.62       -   1.6e-13       1.7e-10
    endgame_forms     endgame_global_carlike_n50_above              0.71    0.78    0.99   9.9e-14       5.8e-11
    endgame_forms     endgame_ragged_carlike_39_40_43_50_above      0.59    0.78    0.99   1.6e-13       1.2e-10
    endgame_forms     -> worst ratio 1.62, x 4 = 6.48, K = 8
    endgame_clearance endgame_obst_unicycle_points_n43_below        0.00    0.00    0.08   8.1e-15       5.0e-14
    endgame_clearance endgame_obst_unicycle_points_n43_above        0.00    0.00    0.00   4.4e-16       5.0e-14
    endgame_clearance -> worst ratio 0.08, x 4 = 0.32, K = 0.5
    endgame_control   endgame_control_carlike_n8_below              0.42    1.08       -   5.6e-13       4.1e-12
    endgame_control   -> worst ratio 1.08, x 4 = 4.32, K = 8

(columns: worst e_dev[i] / max(e_cpu[i], floor) over the 12 instances at each cap.  Every fp64 bound K x yardstick is at or below 1.7e-10: no family needs a bound of its own.
The partitioned sweeps show about ten times the spread of the CPU solvers from the second iteration on -- the combines eliminate I - W P+ without exchanges -- and stay
below 2.3e-12 in absolute terms; the fixed-dt unicycle cases sit at the rounding of the outputs, 30 times below the floor.
The endgame_* rows: no ratio above 1.62 on either side of the floor -- the device sits inside the CPU solvers' own spread, the partitioned sweeps just above the floor (0.94)
no worse than the serial ones below it, and the n = 8 control (1.08) like the long grids: nothing here needed a second look, and no K comes near the partitioned family's 64.)
"""
import numpy as np
import pytest

import _truncated as T

pytestmark = pytest.mark.gpu

K = {
    "serial": 8, "partitioned": 64, "fixed_layout": 4, "forms": 64, "clearance": 0.25, "level1": 64, "level2": 0.25, "collocation": 16, "algorithm": 64,
    "endgame_serial": 8, "endgame_pit": 4, "endgame_fixed": 8, "endgame_forms": 8, "endgame_clearance": 0.5, "endgame_control": 8,
}
K32 = 8
BOUND_FP64 = 1e-9          # K * max(e_cpu, floor) must stay at or below this for every fp64 case and instance


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as pkg
    return pkg


def device_iterate(m, name, cap):
    """one handle per (case, cap), alive for its launch only"""
    cs = T.CASES[name]
    x0, xf, up, dtp, obstacles, ng = T.inputs(name)
    s = m.BatchSolver(T.abi_config(name, cap), max_batch=T.B)
    try:
        if cs.n_grid is not None:
            s.set_grid_sizes(ng)
        return s.solve(x0, xf, up, dtp, init=T.guess(name), obstacles=obstacles)
    finally:
        s.close()


def yardstick(name, cap):
    """(per-instance yardstick, factor) of a case"""
    cs = T.CASES[name]
    if cs.fp32:
        return np.maximum(T.e_cpu32(name, cap), T.FLOOR32), K32
    return np.maximum(T.e_cpu(name, cap), T.FLOOR), K[cs.family]


@pytest.mark.parametrize("name,cap", T.CASE_CAPS)
def test_device_iterate_after_cap_iterations_against_the_refined_dense_oracle(m, name, cap):
    cs = T.CASES[name]
    r = device_iterate(m, name, cap)
    ref, ng = T.reference(name, cap), T.inputs(name)[5]
    e_dev = T.dist_batch((r.x, r.u, r.dt), ref, ng)
    yard, k = yardstick(name, cap)
    ratio = e_dev / yard
    print(f"[truncated, device] {name} cap {cap}: e_dev max {e_dev.max():.2e}, yardstick max {yard.max():.2e}, e_dev / yardstick per instance " + " ".join(f"{v:.2f}" for v in ratio)
          + f"; worst {ratio.max():.2f}, K {k}")
    assert (r.status == 1).all(), r.status
    assert (r.iters == cap).all(), r.iters
    assert (e_dev <= k * yard).all(), (name, cap, e_dev, k * yard)
    if not cs.fp32:
        assert (k * yard <= BOUND_FP64).all(), (name, cap, k * yard)
