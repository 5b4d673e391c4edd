"""Measurement (not a test): wall time per control cycle of mpc_controller_step_batch_device against the best loop a caller can write for the same decisions
on the ABI without it -- the re-initialisation decision on the host from the goals it supplies, the batch split into a cold launch (x_init = NULL) and a warm launch
(previous solutions) of mpc_solve_batch_device with gathers in front and scatters behind, mpc_grid_update_device on the warm part.

Workload: BASELINE configs[1] (car-like, minimum time, n = 50), B = 1024, a 20-cycle closed loop (next start = x[b][1], u_prev = u[b][0]) in which 5 % of the
instances get a goal jump of 1.5 m per cycle.  Grid adaptation off and re-initialisations sampled at dt_ref, so that a re-initialised 2-pose plan is the device cold
start on both sides and the caller's loop needs no per-instance grid sizes.  Both sides see the same inputs; the answers are compared bit for bit in every cycle.

    python tests/tools/controller_cycle_time.py [--batch 1024] [--cycles 20] [--repeats 5]

Prints one JSON line: median wall ms per cycle of both loops, launches (kernels and copies enqueued by the caller) per cycle, and whether the answers are equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    import mpc_local_planner_amd as m
    B, n, per = args.batch, 50, 0.1
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    x0h, xfh, _, _ = m.workloads.carlike_min_time_inputs(B)
    rng = np.random.default_rng(5)
    jumps = [rng.uniform(size=B) < 0.05 for _ in range(args.cycles)]          # which instances get a new goal in which cycle
    jumps[0][:] = False

    def goals_of(cyc, goal):
        g = goal.copy()
        g[jumps[cyc], 1] += 1.5
        return g

    def controller_loop(record):
        s = m.BatchSolver(m.config_carlike_min_time(n), max_batch=B)
        p = s.cycle_params(n_ref=n, adapt=0, reference_reinit_sampling=0, period=per)
        pose, goal = torch.from_numpy(x0h).to(dev), xfh.copy()
        plan = torch.zeros((B, 2, 3), **f64); n_plan = torch.full((B,), 2, dtype=torch.int32, device=dev)
        up, dtp = torch.zeros((B, 2), **f64), torch.zeros(B, **f64)
        x, u, dt = torch.zeros((B, n, 3), **f64), torch.zeros((B, n, 2), **f64), torch.zeros(B, **f64)
        st, it, ri = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
        times = []
        for cyc in range(args.cycles):
            goal = goals_of(cyc, goal)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan[:, 0] = pose; plan[:, 1] = torch.from_numpy(goal).to(dev)                  # 2 launches + 1 copy
            torch.cuda.synchronize()
            s.controller_step_device(B, p, plan.data_ptr(), n_plan.data_ptr(), 2, None, None, None, up.data_ptr(), dtp.data_ptr(), x.data_ptr(), u.data_ptr(), dt.data_ptr(),
                                     st.data_ptr(), it.data_ptr(), ri.data_ptr())             # prepare + solve + 3 copies
            s.synchronize()
            times.append(time.perf_counter() - t0)
            record.append((x.cpu().numpy(), u.cpu().numpy(), dt.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()))
            pose, up = x[:, 1].clone(), u[:, 0].clone()
            dtp.fill_(per)
        s.close()
        return times, 8

    def caller_loop(record):
        s = m.BatchSolver(m.config_carlike_min_time(n), max_batch=B)
        pose, goal, last = torch.from_numpy(x0h).to(dev), xfh.copy(), None
        up, dtp = torch.zeros((B, 2), **f64), torch.zeros(B, **f64)
        x, u, dt = torch.zeros((B, n, 3), **f64), torch.zeros((B, n, 2), **f64), torch.zeros(B, **f64)
        st, it = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        times, launches = [], 0
        for cyc in range(args.cycles):
            goal = goals_of(cyc, goal)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            # the decision of src/controller.cpp:152-158 on the host, from the goals the caller supplies
            if last is None:
                cold = np.ones(B, bool)
            else:
                d = goal - last
                cold = (np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) > 1.0) | (np.abs((d[:, 2] + np.pi) % (2 * np.pi) - np.pi) > 0.5 * np.pi)
            xf = torch.from_numpy(goal).to(dev)
            launches = 1
            for part, warm in ((np.nonzero(cold)[0], False), (np.nonzero(~cold)[0], True)):
                if part.size == 0:
                    continue
                k = int(part.size)
                idx = torch.from_numpy(part).to(dev)
                g = [t.index_select(0, idx) for t in (pose, xf, up, dtp)]
                o = [torch.empty((k, n, 3), **f64), torch.empty((k, n, 2), **f64), torch.empty(k, **f64), torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, dtype=torch.int32, device=dev)]
                init = [None, None, None]
                launches += 1 + 4 + 1 + 5
                if warm:
                    init = [t.index_select(0, idx) for t in (x, u, dt)]
                    launches += 3
                torch.cuda.synchronize()
                if warm:
                    s.grid_update_device(k, g[0].data_ptr(), init[0].data_ptr(), init[1].data_ptr(), init[2].data_ptr(), adapt=False)      # (variable grid without adaptation: nothing moves)
                s.solve_device(k, g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), *(t.data_ptr() if t is not None else None for t in init),
                               o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr())
                s.synchronize()
                for dst, src in zip((x, u, dt, st, it), o):
                    dst.index_copy_(0, idx, src)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            record.append((x.cpu().numpy(), u.cpu().numpy(), dt.cpu().numpy(), st.cpu().numpy(), it.cpu().numpy()))
            pose, up, last = x[:, 1].clone(), u[:, 0].clone(), goal
            dtp.fill_(per)
        s.close()
        return times, launches

    best = {"controller": [], "caller": []}
    equal, conv, launches = True, 0.0, {}
    for rep in range(args.repeats):
        ra, rb = [], []
        ta, launches["controller"] = controller_loop(ra)
        tb, launches["caller"] = caller_loop(rb)
        best["controller"].append(float(np.median(ta[1:])))
        best["caller"].append(float(np.median(tb[1:])))
        equal = equal and all(a.tobytes() == b.tobytes() for ca, cb in zip(ra, rb) for a, b in zip(ca, cb))
        conv = float(np.mean(ra[-1][3] == 0))
    print(json.dumps({"workload": f"carlike_n{n}_B{B}_{args.cycles}_cycles_5pct_goal_jumps", "repeats": args.repeats,
                      "controller_step_batch_device_ms_per_cycle": [round(1e3 * v, 4) for v in best["controller"]],
                      "caller_loop_on_the_previous_abi_ms_per_cycle": [round(1e3 * v, 4) for v in best["caller"]],
                      "launches_per_cycle": launches, "answers_equal": bool(equal), "converged_last_cycle": conv}))


if __name__ == "__main__":
    main()
