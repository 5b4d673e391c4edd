"""developer tool: per-iteration trace (census of non-finite LDS words after every sweep, the sweeps' roots, line-search lines) of ONE workgroup, which the `nancheck`
variant of the library prints from the kernel:
    python scripts/dev/variants.py nancheck:3 python scripts/dev/nancheck_trace.py golden      instance 3 of the car-like golden fixture (n = 50)
    python scripts/dev/variants.py nancheck:6 python scripts/dev/nancheck_trace.py config3     instance 6 of the config-3-shaped batch (unicycle quadratic, n = 80, 16 polygons)
Pipe through `grep "ls:\\|ls FAILED\\|status"` for the line-search lines alone."""
import sys, os, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import mpc_local_planner_amd as m
if (sys.argv[1] if len(sys.argv) > 1 else "golden") == "golden":
    g = np.load(os.path.join(ROOT, "tests", "golden", "carlike_min_time_n50.npz"))
    s = m.BatchSolver(m.config_carlike_min_time(50), max_batch=8)
    r = s.solve(g["x0"], g["xf"], g["u_prev"], g["dt_prev"])
else:
    n, B, O, V, M = 80, 256, 16, 6, 4
    x0, xf, up, dtp, obs = m.workloads.unicycle_obstacle_inputs(B, n_obst=O, max_vertices=V)
    s = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=O, max_vertices=V, max_obstacle_rows=M), max_batch=B)
    r = s.solve(x0, xf, up, dtp, obstacles=obs)
print("status", r.status[:12].tolist(), "iters", r.iters[:12].tolist())
