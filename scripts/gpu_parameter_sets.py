"""Measurements of parameter sets (mpc_set_parameter_sets) on one MI355X, in one process per part, alternating the variants.

  --part bench  plain bench.py of a base tree (the parent commit with its library built) and of this tree, alternated in ABBA order: ms_per_step of each
                run and whether the --dump-outputs files of the two are byte-identical
  --part table  config 2 (car-like minimum time, n = 50) at B = 1024: the handle alone, then the same handle with 16 sets that all equal its configuration,
                alternated launch by launch; kernel ms from mpc_last_kernel_ms; outputs compared
  --part fleet  config 2 with 16 distinct sets of 64 instances (speed limit, wheelbase, rate limits): one launch of one handle against 16 handles enqueued back
                to back on their own streams and then synchronised; wall ms per cycle and the device memory each variant holds

Usage: python scripts/gpu_parameter_sets.py --part table [--launches 30]
       python scripts/gpu_parameter_sets.py --part bench --base-tree DIR [--rounds 4 --steps 10 --warmup 2] [--dump-dir DIR]"""
from __future__ import annotations

import argparse
import filecmp
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def part_bench(args):
    out = args.dump_dir or tempfile.mkdtemp(prefix="parameter_sets_bench_")
    runs = {"base": [], "branch": []}
    trees = {"base": args.base_tree, "branch": ROOT}
    for r in range(args.rounds):
        # ABBA: the variant that runs first alternates from round to round, so that a drift within the pair (clocks, temperature) does not favour one of them
        for pos, name in enumerate(("base", "branch") if r % 2 == 0 else ("branch", "base")):
            d = os.path.join(out, f"{name}_{r}")
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup), "--dump-outputs", d]
            p = subprocess.run(["timeout", "-k", "10", "300"] + cmd, cwd=trees[name], capture_output=True, text=True)
            if p.returncode != 0:
                print(f"{name} round {r}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
                raise SystemExit(1)
            line = json.loads([s for s in p.stdout.splitlines() if s.startswith("{")][-1])
            runs[name].append((line["ms_per_step"], d, pos))
            print(f"round {r} {name:6s} (runs {'first' if pos == 0 else 'second'}) ms_per_step {line['ms_per_step']:.4f}  value {line['value']:.1f} {line.get('unit', '')}", flush=True)
    for name in runs:
        ms = np.array([v for v, _, _ in runs[name]])
        print(f"{name:6s} ms_per_step: mean {ms.mean():.4f}  min {ms.min():.4f}  max {ms.max():.4f}  spread {ms.max() - ms.min():.4f}")
    for pos in (0, 1):
        ms = np.array([v for name in runs for v, _, q in runs[name] if q == pos])
        print(f"runs {'first' if pos == 0 else 'second'} in their pair, either variant: mean {ms.mean():.4f}")
    b, n = runs["base"][-1][1], runs["branch"][-1][1]
    files = sorted(os.listdir(b))
    same = files == sorted(os.listdir(n)) and all(filecmp.cmp(os.path.join(b, f), os.path.join(n, f), shallow=False) for f in files)
    print(f"--dump-outputs of the last rounds byte-identical: {same} ({', '.join(files)})")


def _inputs_device(torch, dev, inputs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in inputs]


class _Out:
    def __init__(self, torch, dev, B, n):
        self.x = torch.empty((B, n, 3), dtype=torch.float64, device=dev)
        self.u = torch.empty((B, n, 2), dtype=torch.float64, device=dev)
        self.dt = torch.empty(B, dtype=torch.float64, device=dev)
        self.st = torch.empty(B, dtype=torch.int32, device=dev)
        self.it = torch.empty(B, dtype=torch.int32, device=dev)

    def launch(self, s, B, d, lo=0):
        x0, xf, up, dtp = d
        s.solve_device(B, x0[lo:].data_ptr(), xf[lo:].data_ptr(), up[lo:].data_ptr(), dtp[lo:].data_ptr(), None, None, None,
                       self.x[lo:].data_ptr(), self.u[lo:].data_ptr(), self.dt[lo:].data_ptr(), self.st[lo:].data_ptr(), self.it[lo:].data_ptr())

    def host(self):
        return [t.cpu().numpy() for t in (self.x, self.u, self.dt, self.st, self.it)]


def part_table(args):
    import torch
    import mpc_local_planner_amd as m
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    B, n = 1024, 50
    d = _inputs_device(torch, dev, m.workloads.carlike_min_time_inputs(B))
    s = m.BatchSolver(m.config_carlike_min_time(n), max_batch=B)
    out = _Out(torch, dev, B, n)
    same_sets = [m.config_carlike_min_time(n) for _ in range(16)]
    set_of = np.random.default_rng(3).integers(0, 16, B)
    ms = {"alone": [], "16 equal sets": []}
    res = {}
    for i in range(args.warmup + args.launches):
        for name in ms:
            if name == "alone":
                s.set_parameter_sets(None)
            else:
                s.set_parameter_sets(same_sets, set_of)
            out.launch(s, B, d)
            s.synchronize()
            if i >= args.warmup:
                ms[name].append(s.last_kernel_ms())
            res[name] = out.host()
    for name, v in ms.items():
        v = np.array(v)
        print(f"config 2, B = {B}, {name:14s}: kernel ms over {len(v)} launches: median {np.median(v):.4f}  mean {v.mean():.4f}  min {v.min():.4f}  max {v.max():.4f}")
    a, b = np.median(ms["alone"]), np.median(ms["16 equal sets"])
    print(f"median ratio (16 equal sets / alone): {b / a:.4f}")
    print(f"outputs identical (x, u, dt, status, iters of the last launches): {all(np.array_equal(p, q) for p, q in zip(res['alone'], res['16 equal sets']))}")
    s.close()


def _fleet_sets(m, n, K):
    sets = []
    for k in range(K):
        c = m.config_carlike_min_time(n)
        c.u_ub[0] = 0.3 + 0.02 * k                     # speed limit
        c.model_params[0] = 0.3 + 0.02 * k             # wheelbase
        for j in range(2):
            c.du_lb[j], c.du_ub[j] = -(0.35 + 0.03 * k), 0.35 + 0.03 * k      # rate limits
        sets.append(c)
    return sets


def part_fleet(args):
    import torch
    import mpc_local_planner_amd as m
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    K, per, n = 16, 64, 50
    B = K * per
    sets = _fleet_sets(m, n, K)
    inputs = m.workloads.carlike_min_time_inputs(B)
    # instances sorted by robot: robot k holds instances [k per, (k + 1) per) -- the 16 handles then read contiguous slices of the same device arrays
    d = _inputs_device(torch, dev, inputs)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    one = m.BatchSolver(m.config_carlike_min_time(n), max_batch=B)
    one.set_parameter_sets(sets, np.repeat(np.arange(K), per))
    free1 = torch.cuda.mem_get_info(dev)[0]
    many = [m.BatchSolver(sets[k], max_batch=per) for k in range(K)]
    free2 = torch.cuda.mem_get_info(dev)[0]
    o1, o2 = _Out(torch, dev, B, n), _Out(torch, dev, B, n)

    def cycle_one():
        o1.launch(one, B, d)
        one.synchronize()

    def cycle_many():
        for k, h in enumerate(many):
            o2.launch(h, per, d, lo=k * per)
        for h in many:
            h.synchronize()
    wall = {"one handle, 16 sets, one launch": [], "16 handles, 16 launches on their own streams": []}
    fns = dict(zip(wall, (cycle_one, cycle_many)))
    for i in range(args.warmup + args.launches):
        for name, fn in fns.items():
            t = time.perf_counter()
            fn()
            if i >= args.warmup:
                wall[name].append((time.perf_counter() - t) * 1e3)
    for name, v in wall.items():
        v = np.array(v)
        print(f"{name:46s}: wall ms per cycle over {len(v)} cycles: median {np.median(v):.4f}  mean {v.mean():.4f}  min {v.min():.4f}  max {v.max():.4f}")
    print(f"device memory: one handle {(free0 - free1) / 2**20:.1f} MiB, 16 handles {(free1 - free2) / 2**20:.1f} MiB (torch.cuda.mem_get_info deltas)")
    r1, r2 = o1.host(), o2.host()
    print(f"outputs identical (x, u, dt, status, iters): {all(np.array_equal(p, q) for p, q in zip(r1, r2))}; converged {np.mean(r1[3] == 0):.4f}; "
          f"iterations mean {r1[4].mean():.2f} max {r1[4].max()}")
    for h in many:
        h.close()
    one.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("bench", "table", "fleet"), required=True)
    ap.add_argument("--base-tree", default=None)
    ap.add_argument("--dump-dir", default=None, help="--part bench: where the --dump-outputs files go (default: a new temporary directory)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=30)
    args = ap.parse_args()
    print("command:", " ".join([os.path.basename(sys.executable)] + sys.argv), flush=True)
    if args.part == "bench":
        if not args.base_tree:
            ap.error("--part bench needs --base-tree")
        part_bench(args)
    elif args.part == "table":
        part_table(args)
    else:
        part_fleet(args)


if __name__ == "__main__":
    main()
