#!/usr/bin/env python
"""Developer tool (GPU box): per-phase cycle counters of the solve kernel on the config-3 workload (unicycle n = 80, 16 polygons), with and without its obstacles, on the
`prof` variant of the library:  python scripts/dev/variants.py prof python scripts/gpu_phase_profile_config3.py"""
import sys, os, numpy as np
import torch
torch.zeros(1, device="cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts", "dev")]
import mpc_local_planner_amd as m
from mpc_local_planner_amd import _lib
from variants import PROF_COLUMNS, read_profile
n, B, O, V, M = 80, 2048, 16, 6, 4
x0, xf, up, dtp, obs = m.workloads.unicycle_obstacle_inputs(B, n_obst=O, max_vertices=V)
for tag, kw, ob in (("with obstacles", dict(max_obstacles=O, max_vertices=V, max_obstacle_rows=M), obs), ("without", {}, None)):
    s = m.BatchSolver(m.config_unicycle_quadratic(n, **kw), max_batch=B)
    r = s.solve(x0, xf, up, dtp, obstacles=ob)
    r = s.solve(x0, xf, up, dtp, obstacles=ob)
    print(tag, "kernel ms", s.last_kernel_ms(), "iters", r.iters.mean(), "conv", (r.status == 0).mean())
    t = dict(zip(PROF_COLUMNS, read_profile(_lib.load(), B).sum(0).astype(float)))
    it = t["iters"]
    print("  per iteration ticks:", {k: round(v / it) for k, v in t.items() if k not in ("wall100MHz", "iters", "nfac", "ntrial", "spare")}, "fac/it", round(t["nfac"] / it, 3), "trials/it", round(t["ntrial"] / it, 3))
    s.close()
