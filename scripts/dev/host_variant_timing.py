"""developer tool (GPU): what the host-pointer entry points other than mpc_solve_batch cost per call with the library named by MPC_HIP_LIB (default: the in-tree one) --
evaluate, plan_inputs, commands, controller_step, check_feasibility and costmap_to_obstacles at B = 64 and B = 4096, the last two on a 64 x 64 map.  A host clock around
the synchronous call, after one warm-up call of the kind at that B (the first call allocates or grows the staging); the median, minimum and maximum over REPS calls.
One process per library; to compare two libraries run them alternately, several rounds each (profiles/r15_capi_staging.md), and hold one's median to the other's spread.
Prints one JSON line and a checksum of everything the calls returned, which two libraries that compute the same must share.

    MPC_HIP_LIB=/path/to/libmpc_hip.so python scripts/dev/host_variant_timing.py [label]"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, STRIDE, GSTRIDE, CELLS, REPS = 20, 16, 128, 64, 15


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit("host_variant_timing.py needs the GPU")
    import mpc_local_planner_amd as m
    digest = hashlib.sha256()
    out = {"label": sys.argv[1] if len(sys.argv) > 1 else "", "library": os.environ.get("MPC_HIP_LIB", "in-tree"), "n": N, "reps": REPS, "ms": {}}

    def timed(name, B, call):
        for a in call():      # warm-up: allocates or grows what the kind needs
            digest.update(np.ascontiguousarray(a).tobytes())
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        out["ms"][f"{name}_B{B}"] = {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}

    for B in (64, 4096):
        s = m.BatchSolver(m.config_carlike_min_time(N), max_batch=B)
        so = m.BatchSolver(m.config_carlike_min_time(N, max_obstacles=3, max_vertices=1, max_obstacle_rows=4), max_batch=B)
        x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0))
        r = s.solve(x0, xf, up, dtp)
        timed("evaluate", B, lambda: (lambda e: (e.objective, e.eq_violation, e.ineq_violation, e.clearance, e.closest))(s.evaluate(x0, xf, r.x, r.u, r.dt, up, dtp)))
        t = np.linspace(0.0, 1.0, GSTRIDE)[None, :, None]
        gplan = np.ascontiguousarray(x0[:, None, :] + t * (xf - x0)[:, None, :])
        pp = s.plan_params()
        pin = s.plan_inputs(pp, gplan, np.full(B, GSTRIDE, np.int32), x0, STRIDE)
        timed("plan_inputs", B, lambda: (lambda q: (q.plan, q.n_plan, q.plan_begin, q.goal_idx, q.flags))(s.plan_inputs(pp, gplan, np.full(B, GSTRIDE, np.int32), x0, STRIDE)))
        timed("commands", B, lambda: (lambda c: (c.cmd, c.result, c.reset_next, c.u_prev_next, c.infeasible_count))(s.commands(r.u, r.status, plan_flags=pin.flags)))
        cp = s.cycle_params()
        reset = np.ones(B, np.int32)      # every call starts the slots afresh: the same work each time
        timed("controller_step", B, lambda: (lambda q: (q[0].x, q[0].u, q[0].dt, q[0].status, q[1], q[2]))(s.controller_step(cp, pin.plan, pin.n_plan, reset=reset, u_prev=up, dt_prev=dtp)))
        cost = np.zeros((B, CELLS, CELLS), np.uint8)
        cost[:, CELLS // 2, ::3] = 254
        org = np.full((B, 2), -3.2)
        timed("check_feasibility", B, lambda: (s.check_feasibility(r.x, cost, 6.4 / CELLS, org, np.zeros((0, 2)), 0.2),))
        timed("costmap_to_obstacles", B, lambda: so.costmap_to_obstacles(cost, 6.4 / CELLS, org, x0))
        s.close(); so.close()
    out["checksum"] = digest.hexdigest()[:16]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
