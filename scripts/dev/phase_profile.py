"""developer tool: per-phase cycle counters of the solve kernel, on the `prof` variant of the library (scripts/dev/variants.py builds it next to the product library):
    python scripts/dev/variants.py prof python scripts/dev/phase_profile.py [carlike50|bicycle120|unicycle80] [lds|global|auto] [B]"""
import sys, os, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import mpc_local_planner_amd as m
from mpc_local_planner_amd import _lib, _abi as A
from variants import COL, GLUE, PHASES, PROF_COLUMNS, read_profile
what = sys.argv[1] if len(sys.argv) > 1 else "carlike50"
mode = {"lds": A.STAGE_LDS, "global": A.STAGE_GLOBAL, "auto": A.STAGE_AUTO}[sys.argv[2] if len(sys.argv) > 2 else "auto"]
B = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
obstacles = None
if what == "carlike50":
    cfg = m.config_carlike_min_time(50, stage_data=mode); inp = m.workloads.carlike_min_time_inputs(B)
elif what == "bicycle120":
    cfg = m.config_bicycle_min_time(120, stage_data=mode); inp = m.workloads.bicycle_min_time_inputs(B)
else:
    x0, xf, up, dtp, obstacles = m.workloads.unicycle_obstacle_inputs(B, n_obst=16, max_vertices=6, lateral=(0.15, 0.8)); inp = (x0, xf, up, dtp)
    cfg = m.config_unicycle_quadratic(80, max_obstacles=16, max_vertices=6, max_obstacle_rows=4, max_iter=60, stage_data=mode)
s = m.BatchSolver(cfg, max_batch=B)
r = s.solve(*inp, obstacles=obstacles)
r = s.solve(*inp, obstacles=obstacles)
print(what, sys.argv[2:] , "kernel ms", s.last_kernel_ms(), "lds", s.lds_bytes(), "converged", (r.status == 0).mean(), "iters", r.iters.mean())
buf = read_profile(_lib.load(), min(B, 4096))
print("tick rate GHz ~", (buf[:, COL["ticks"]] / (buf[:, COL["wall100MHz"]] / 100e6)).mean() / 1e9)
tot = dict(zip(PROF_COLUMNS, buf.sum(0).astype(float)))
it, nfac, ntrial = tot["iters"], tot["nfac"], tot["ntrial"]
print("per iteration (ticks):", {k: round(v / it) for k, v in tot.items() if k not in ("wall100MHz", "iters", "nfac", "ntrial", "spare")})
print("phases + glue per iteration:", round(sum(tot[k] for k in PHASES + GLUE) / it), "of", round(tot["ticks"] / it), "ticks; glue alone", round(sum(tot[k] for k in GLUE) / it))
print("factorisations per iteration", nfac / it, "trials per iteration", ntrial / it)
print("per-sweep ticks: backward", tot["backward"] / nfac, "forward", tot["forward"] / it, "trial", tot["trial"] / max(1, ntrial))
