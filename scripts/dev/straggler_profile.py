"""developer tool: where the slowest reference-path solves of the config-2 batch spend their time, on the `prof` variant of the library:
    python scripts/dev/variants.py prof python scripts/dev/straggler_profile.py"""
import sys, os, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import mpc_local_planner_amd as m
from mpc_local_planner_amd import _lib
from variants import COL, PROF_COLUMNS, read_profile
B = 1024
inp = m.workloads.carlike_min_time_inputs(B, seed=20260924)
s = m.BatchSolver(m.config_carlike_min_time(50), max_batch=B)
r = s.solve(*inp); r = s.solve(*inp)
print("kernel ms", s.last_kernel_ms(), "status", np.bincount(r.status, minlength=4))
buf = read_profile(_lib.load(), B)
counters = PROF_COLUMNS[COL["kkt"]:COL["spare"]]
order = np.argsort(-buf[:, COL["ticks"]])
print("slowest 12 (ticks, us, iters, nfac, ntrial, status):")
for i in order[:12]:
    b = dict(zip(PROF_COLUMNS, buf[i].tolist()))
    print(int(i), b["ticks"], round(b["wall100MHz"] / 100.0, 1), b["iters"], b["nfac"], b["ntrial"], int(r.status[i]), {k: b[k] for k in counters})
slow = r.iters >= 100
for nm, sel in (("100-iteration solves", slow), ("the rest", ~slow)):
    t = dict(zip(PROF_COLUMNS, buf[sel].sum(0).astype(float)))
    print(nm, int(sel.sum()), "ticks/iter", round(t["ticks"] / t["iters"]), "fac/iter", round(t["nfac"] / t["iters"], 2), "trials/iter", round(t["ntrial"] / t["iters"], 2), {k: round(t[k] / t["iters"]) for k in counters})
