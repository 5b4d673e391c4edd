"""Developer tool: the head-on scenario of tests/test_gpu_fleet_obstacles.py on the C oracle (CPU), with and without the other robot as a moving obstacle.

    python tests/tools/fleet_head_on_oracle.py [cycles]

Two unicycles (in-code defaults: u in [-0.2, 0.4] x [-0.3, 0.3], no rate limits; n = 16, dt_ref 0.3, dt free in [0, 10], minimum time, goal fixed; tol 1e-6, 100
iterations), A: (0, 0, 0) -> (4, 0, 0), B: (4, 0.1, pi) -> (0, 0.1, pi).  Circular footprint r = 0.2, min_obstacle_dist 0.25, force_inclusion_dist 0.5, cutoff_dist 2.5,
dynamic obstacles, circle obstacles of radius 0.2, max_obstacle_rows 4.  Period 0.2 s, dt_prev 0.2, u_prev = the applied control, plant = the exact unicycle arc; a failed
solve gives a zero command and a cold start next cycle; warm start from the previous outputs while all converge.  The other robot enters as ONE obstacle at its current
position with the velocity of the first interval of its own converged plan -- the pool-fill rule of include/mpc_fleet.h, restated here with numpy.

Recorded (70 cycles): minimum centre distance 0.6391 m with the obstacle (0 failed solves of 140, final goal distances 0.083 / 0.083 m), 0.1000 m without (9 failed
solves, 0.012 / 0.068 m).  The thresholds of the GPU test (0.4 m = 2 r, 0.15 m) are conditions these figures meet with a wide margin."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle import c_oracle, se2_nlp as R      # noqa: E402

START = np.array([(0.0, 0.0, 0.0), (4.0, 0.1, math.pi)])
GOAL = np.array([(4.0, 0.0, 0.0), (0.0, 0.1, math.pi)])
PERIOD, RADIUS = 0.2, 0.2


def plant(pose, u):
    out = pose.copy()
    for b, (v, w) in enumerate(u):
        x, y, th = pose[b]
        if abs(w) < 1e-12:
            out[b] = (x + v * PERIOD * math.cos(th), y + v * PERIOD * math.sin(th), th)
        else:
            out[b] = (x + v / w * (math.sin(th + w * PERIOD) - math.sin(th)), y - v / w * (math.cos(th + w * PERIOD) - math.cos(th)), th + w * PERIOD)
    return out


def run(cycles, with_obstacle):
    cfg = R.OcpConfig(model=R.MODEL_UNICYCLE, model_params=(0.0,), n=16, dt_ref=0.3)
    cfg.enable_dynamic_obstacles, cfg.min_obstacle_dist, cfg.force_inclusion_dist, cfg.cutoff_dist = True, 0.25, 0.5, 2.5
    cfg.footprint_kind, cfg.footprint_params = R.FOOTPRINT_CIRCLE, (RADIUS,)
    ocfg, obst = c_oracle.from_nlp_config(cfg, max_iter=100, tol=1e-6), c_oracle.obst_from_nlp_config(cfg, 4, 1, 4)
    B = 2
    pose, u_prev, dt_prev, init = START.copy(), np.zeros((B, 2)), np.full(B, PERIOD), None
    ob = (np.zeros(B, np.int32), np.zeros((B, 4), np.int32), np.zeros((B, 4, 1, 2)), np.zeros((B, 4)), np.zeros((B, 4, 2)))
    closest, failed = math.inf, 0
    for _ in range(cycles):
        x, u, dt, st, _ = c_oracle.solve_batch(ocfg, pose, GOAL, u_prev, dt_prev, init, obstacles=ob, obst=obst)
        ok = st == 0
        failed += int((~ok).sum())
        u0 = np.where(ok[:, None], u[:, 0], 0.0)
        pose, u_prev = plant(pose, u0), u0
        init = (x, u, dt) if ok.all() else None
        closest = min(closest, math.hypot(pose[0, 0] - pose[1, 0], pose[0, 1] - pose[1, 1]))
        if with_obstacle:
            vel = np.where(ok[:, None] & (dt > 0)[:, None], (x[:, 1, :2] - x[:, 0, :2]) / dt[:, None], 0.0)
            for b in range(B):
                o = 1 - b
                ob[0][b], ob[1][b, 0], ob[2][b, 0, 0], ob[3][b, 0], ob[4][b, 0] = 1, 1, pose[o, :2], RADIUS, vel[o]
    return closest, failed, np.hypot(pose[:, 0] - GOAL[:, 0], pose[:, 1] - GOAL[:, 1])


if __name__ == "__main__":
    cycles = int(sys.argv[1]) if len(sys.argv) > 1 else 70
    for with_obstacle in (True, False):
        closest, failed, goal = run(cycles, with_obstacle)
        print(f"{'with' if with_obstacle else 'without'} the other robot as an obstacle: minimum centre distance {closest:.4f} m, {failed} failed solves of {2 * cycles}, "
              f"final goal distances {goal[0]:.3f} / {goal[1]:.3f} m")
