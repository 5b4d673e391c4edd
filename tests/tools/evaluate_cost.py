"""Measurement (not a test): what mpc_evaluate_batch_device costs next to the solve launch of the same handle and batch, B = 1024: BASELINE configs[1] (car-like minimum
time, n = 50, no obstacles) and configs[2] (unicycle, n = 80, 16 polygons).  The evaluation runs on the solve's outputs.

Call time: host clock around 200 back-to-back device calls that end in a synchronise (after 20 warm-up calls, five repetitions), next to mpc_last_kernel_ms of five solve
launches.  The handle's stream is private, so a caller cannot bracket the evaluation with events of its own; the kernel time itself comes from a kernel trace of this same
program, in a run of its own:

    python tests/tools/evaluate_cost.py [out.json]
    rocprofv3 --kernel-trace --stats -d DIR -o trace --output-format csv -- python tests/tools/evaluate_cost.py

(mpc::evaluate_kernel in DIR/*kernel_trace.csv: the first 1020 launches are config 2, the next 1020 config 3.)  Prints one JSON line.  profiles/r12_evaluate.md has the figures."""
import json
import sys
import time

import numpy as np
import torch

import mpc_local_planner_amd as m

REPS, WARM = 200, 20
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
out = {}
for name in ("config2_n50", "config3_n80_16polygons"):
    B = 1024
    if name.startswith("config2"):
        x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(B)
        cfg, obst = m.config_carlike_min_time(50), None
    else:
        x0, xf, up, dtp, obst = m.workloads.unicycle_obstacle_inputs(B, n_obst=16, max_vertices=6)
        cfg = m.config_unicycle_quadratic(80, max_obstacles=16, max_vertices=6, max_obstacle_rows=4)
    n = cfg.n
    s = m.BatchSolver(cfg, max_batch=B)
    d = [t(a) for a in (x0, xf, up, dtp)]
    keep = [t(a) for a in obst] if obst is not None else None
    ob = tuple(a.data_ptr() for a in keep) if keep is not None else None
    xo = torch.zeros((B, n, 3), dtype=torch.float64, device="cuda"); uo = torch.zeros((B, n, 2), dtype=torch.float64, device="cuda"); do = torch.zeros(B, dtype=torch.float64, device="cuda")
    st = torch.zeros(B, dtype=torch.int32, device="cuda"); it = torch.zeros(B, dtype=torch.int32, device="cuda")
    ev = torch.zeros((4, B), dtype=torch.float64, device="cuda"); cs = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    solve_ms = []
    for r in range(5):
        s.solve_device(B, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), None, None, None, xo.data_ptr(), uo.data_ptr(), do.data_ptr(), st.data_ptr(), it.data_ptr(), obstacles=ob)
        s.synchronize()
        solve_ms.append(s.last_kernel_ms())

    def call():
        s.evaluate_device(B, d[0].data_ptr(), d[1].data_ptr(), xo.data_ptr(), uo.data_ptr(), do.data_ptr(), objective=ev[0].data_ptr(), eq_violation=ev[1].data_ptr(),
                          ineq_violation=ev[2].data_ptr(), clearance=ev[3].data_ptr(), closest=cs.data_ptr(), u_prev=d[2].data_ptr(), dt_prev=d[3].data_ptr(), obstacles=ob)
    for _ in range(WARM):
        call()
    s.synchronize()
    per = []
    for rep in range(5):
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        s.synchronize()
        per.append((time.perf_counter() - t0) / REPS * 1e3)
    s.close()
    out[name] = dict(B=B, n=n, solve_kernel_ms=solve_ms, converged=float((st.cpu().numpy() == 0).mean()), evaluate_call_ms=per,
                     evaluate_over_solve=float(np.median(per) / np.median(solve_ms[1:])), clearance_min=float(ev[3].min().item()))
print(json.dumps(out))
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write(json.dumps(out, indent=1))
