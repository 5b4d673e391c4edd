"""developer tool: what mpc_plan_inputs_batch_device and mpc_commands_batch_device cost next to the same work on one host thread (profiles/r14_plan_inputs.md).

B = 1024 robots, global plans of 2048 poses at 0.05 m spacing (gentle arcs), robots at random arc positions along them, a 6 m costmap, look-ahead 1.5 m and 3 m.
The handle's stream is private to the library, so the device figure is a host clock around R back-to-back calls that ends in mpc_synchronize, divided by R, after a
warm-up; repeated, with the spread printed.  The host figures: the facade's functions (tests/host_harness/plan_inputs_host.cpp, pin_facade -- it copies the plan into a
vector per call, as the harness has no persistent plan) and the host build of the device's own header (pin_batch, no copy), one thread.  Needs an MI355X; fails without one.

    python scripts/dev/plan_inputs_timing.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

B, NPOSE, STEP, STRIDE, MAX_VIA = 1024, 2048, 0.05, 96, 4
WARM, R, REPEATS = 20, 200, 7


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit("plan_inputs_timing.py needs the GPU")
    import _plan_inputs_cases as K
    import mpc_local_planner_amd as m
    from mpc_local_planner_amd import _abi as A
    rng = np.random.default_rng(41)
    s = STEP * np.arange(NPOSE)
    radius = rng.uniform(15.0, 60.0, B) * rng.choice([-1.0, 1.0], B)
    g = np.ascontiguousarray(np.stack([np.column_stack([r * np.sin(s / r), r * (1.0 - np.cos(s / r)), s / r]) for r in radius]))
    at = rng.integers(0, NPOSE, B)
    robot = np.ascontiguousarray(g[np.arange(B), at] + np.column_stack([rng.uniform(-0.2, 0.2, (B, 2)), rng.uniform(-0.3, 0.3, B)]))
    ng = np.full(B, NPOSE, np.int32)
    solver = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=20, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=MAX_VIA), max_batch=B)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = {"B": B, "poses": NPOSE, "spacing": STEP, "plan_stride": STRIDE, "calls_per_window": R, "windows": REPEATS, "cases": []}
    for look in (1.5, 3.0):
        p = K.params(max_global_plan_lookahead_dist=look, global_plan_viapoint_sep=0.5, costmap_size_x=120, costmap_size_y=120)
        dg, dn, dr = T(g), T(ng), T(robot)
        plan, n_plan, n_via, via, gi, fl = (T(a) for a in K.blank_outputs(B, STRIDE, MAX_VIA))
        begin0 = np.zeros(B, np.int32)
        windows = {}
        # the first call of a cycle prunes from the plan's start (begin = 0: the scan runs up to the robot); a steady-state call starts at the front of the cycle before
        for name, fresh in (("from the plan's start", True), ("from the last front", False)):
            db = T(begin0)
            torch.cuda.synchronize()
            call = lambda: solver.plan_inputs_device(B, p, dg.data_ptr(), dn.data_ptr(), NPOSE, dr.data_ptr(), None if fresh else db.data_ptr(), plan.data_ptr(), n_plan.data_ptr(),
                                                     STRIDE, n_via.data_ptr(), via.data_ptr(), gi.data_ptr(), fl.data_ptr())
            for _ in range(WARM):
                call()
            solver.synchronize()
            ms = []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                for _ in range(R):
                    call()
                solver.synchronize()
                ms.append((time.perf_counter() - t0) / R * 1e3)
            windows[name] = {"ms_per_call_median": float(np.median(ms)), "ms_per_call_min": float(min(ms)), "ms_per_call_max": float(max(ms))}
        sel = n_plan.cpu().numpy()
        # the commands kernel on the same batch
        du, dst = torch.zeros((B, 20, 2), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        cmd, res = torch.zeros((B, 3), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ccall = lambda: solver.commands_device(B, du.data_ptr(), dst.data_ptr(), None, fl.data_ptr(), cmd.data_ptr(), res.data_ptr())
        for _ in range(WARM):
            ccall()
        solver.synchronize()
        cms = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            for _ in range(R):
                ccall()
            solver.synchronize()
            cms.append((time.perf_counter() - t0) / R * 1e3)
        # one host thread: the facade's functions, and the host build of the device's header
        h = K.harness()
        hp, hn, hnv, hv, hgi, hfl = K.blank_outputs(B, STRIDE, MAX_VIA)
        host = {}
        for name in ("facade", "host build of the header"):
            best = []
            for _ in range(3):
                hb = begin0.copy()
                t0 = time.perf_counter()
                if name == "facade":
                    for b in range(B):
                        h.pin_facade(C.byref(p), K.d_(g[b]), NPOSE, K.d_(robot[b]), K.i_(hb[b:b + 1]), K.d_(hp[b]), K.i_(hn[b:b + 1]), STRIDE, MAX_VIA, K.i_(hnv[b:b + 1]), K.d_(hv[b]),
                                     K.i_(hgi[b:b + 1]), K.i_(hfl[b:b + 1]))
                else:
                    h.pin_batch(B, C.byref(p), K.d_(g), K.i_(ng), NPOSE, K.d_(robot), K.i_(hb), K.d_(hp), K.i_(hn), STRIDE, MAX_VIA, K.i_(hnv), K.d_(hv), K.i_(hgi), K.i_(hfl))
                best.append((time.perf_counter() - t0) * 1e3)
            host[name] = {"ms_per_batch_min": float(min(best)), "ms_per_batch_max": float(max(best))}
        assert hn.tobytes() == sel.tobytes()          # the timed device calls computed what the host computes
        out["cases"].append({"look_ahead": look, "selected_poses_mean": float(sel.mean()), "device_plan_inputs": windows,
                             "device_commands_ms_per_call_median": float(np.median(cms)), "host_one_thread": host})
        print(json.dumps(out["cases"][-1]), flush=True)
    solver.close()
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
