#!/usr/bin/env python
"""bench.py -- MPC control-cycle solves/sec of the car-like minimum-time NLP (n=50) on MI355X.

One "step" = one pass of the hot path (a full batched NLP solve, cold start exactly as Controller::step does on an empty grid, with the
candidate initial trajectories of DESIGN.md section 5.4 hedging the slow instances) over one batch of synthetic planner inputs that are
already resident in HBM.

  N = 1   workload = BASELINE.json configs[1]: 1024 instances on the GPU at the PARITY-PRESERVING operating point: candidate 0 (the reference's cold
          start) runs the reference's 100 iterations.  With --full, `solver.answers_equal_to_the_reference_path_alone` says for which share of the instances the
          returned trajectory is bit for bit what the reference path alone returns (or that path fails).  Extra legs measured after the timed region (--full):
          the latency-tuned point with candidate 0 capped at 60 iterations and what its hedges cost in solution quality (`hedged_caps_60`), the
          warm-started cycle, the per-GPU share of
          configs[3] (car-like n=50, B=4096), configs[2] (unicycle n=80, 16 polygons, B=4096) on a placement where clearance rows bind and on one
          where they stay inactive (with the share of instances that end with an active row), the per-GPU share of configs[4] (bicycle n=120,
          B=1024) in MPC_MIXED -- the precision that meets the 1e-4 tolerance, hence the leg that counts -- and in plain fp32, the latency of one
          instance at a time, and the CPU baseline.
  N > 1   workload = BASELINE.json configs[3]: 4096 instances per GPU (32768 at N=8), rank r draws its inputs from seed+r; no data-path
          collective inside the timed region.  After it, the per-rank results (status, dt, x -- device resident) are all-gathered over
          RCCL so that every rank holds the whole job's answer; that exchange is timed separately and reported as `gather_ms`.  With --full
          the line carries `per_gpu_reference`: rank 0 alone on the same 4096 instances, timed in the same run before the joint timed region.

`value` counts CONVERGED solves only (a Controller::step that returns false makes the planner reset and command zero,
src/mpc_local_planner_ros.cpp:394-404); `value_all_solves` counts every instance.

A plain run sets up, warms up, times K steps, writes the outputs of the last step (--dump-outputs) and prints the line.  Everything else -- the
parity check against the reference path alone, the check that the last step reproduces the warm-up step, the measured FMA peaks of the roofline
block, the extra legs, the CPU baseline and, for N > 1, rank 0's solo reference -- runs only with --full (--no-legs, --no-cpu-baseline and
--no-parity-check drop parts of it).

--dump-outputs DIR: what the timed path returned in its last step (rank 0's shard for N > 1) as DIR/<name>.npy in float64: x (B, n, 3),
u (B, n, 2), dt (B,), status (B,), iterations (B,).  The inputs are drawn from fixed seeds, so two builds given the same arguments can be
compared output for output.  Above 64 MB in all, a fixed seeded sample of instances is written, with their indices in instance_index.npy.

Contract: python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]   (torchrun for N>1) -> ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_GRID = 50
BATCH_1GPU = 1024              # BASELINE.json configs[1]
BATCH_PER_GPU_MULTI = 4096     # BASELINE.json configs[3]: 32768 over 8 GPUs
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_VECTOR_PEAK_TF = 78.6     # SURVEY.md 8d / AMD spec, vector fp64
FP32_VECTOR_PEAK_TF = 157.3
# candidate initial trajectories of the headline run (include/mpc_hip.h, enum mpc_candidate_kind): the reference cold start first, then three
# Hermite-curve hedges (forward with tangent scales 2 and 3, forward-then-reverse with 1.5) with falling iteration caps (a hedge starts later,
# its cap bounds the launch time).  Chosen with the C oracle over EIGHT seeds of the config-2 distribution (>= 99.3 % converged on each, 99.45 %
# on average; DESIGN.md section 5.4 has the measured sweep).
CAND_KINDS = (0, 5, 5, 7)
# HEADLINE operating point: candidate 0 -- the reference's cold start -- runs the reference's full iteration budget (100,
# src/controller.cpp:390), so every instance the reference path solves keeps exactly that answer; the hedges only serve the rest.  The line carries
# `solver.answers_equal_to_the_reference_path_alone` (checked against a run of the reference path alone on the same inputs).
CAND_CAPS = (100, 45, 40, 35)
# the latency-tuned operating point of rounds 2/3 (candidate 0 capped at 60 iterations: ~7 % of the instances get a hedge's local optimum although the
# reference path would have converged later), reported as the leg `hedged_caps_60`
CAND_CAPS_HEDGED = (60, 45, 40, 35)
# at 4096 instances per GPU the launch is bound by the total work, not by its slowest instance: longer hedge caps cost nothing there and lift the converged
# fraction (profiles/r02_candidate_sweep_B4096.log: 99.95 % instead of 99.2 % at the same 10.1 ms)
CAND_CAPS_LARGE_BATCH = (100, 60, 50, 40)
CAND_PARAMS = (0.0, 2.0, 3.0, 1.5)
CAND5_KINDS, CAND5_CAPS, CAND5_PARAMS = (0, 1, 2, 5), (60, 50, 45, 40), (0.0, 0.0, 0.0, 2.0)      # config-5 legs (bicycle, n = 120)


def algorithmic_bytes_per_solve(n: int, s: int = 8, obstacle_scalars: int = 0) -> int:
    """B_alg = s * (2*P(n) + 9 + O), P(n) = 5n - 1 scalars per trajectory (read guess + write solution)
    + x0(3) + xf(3) + u_prev(2) + dt_prev(1) + obstacle scalars."""
    return s * (2 * (5 * n - 1) + 9 + obstacle_scalars)


def cpu_baseline(n):
    """Times the C oracle (oracle/mpc_oracle.c, banded-LU interior point, OpenMP over instances) on a bounded
    sample of the same workload on the host cores.  Checker/baseline only: nothing here feeds the GPU path.
    The thread count is the one that gives the highest throughput in a short pilot (containers often expose more logical
    CPUs than their CPU quota lets them run; oversubscribing costs the oracle up to 2x).  Single candidate (the reference path)."""
    from oracle import c_oracle as CO, se2_nlp as R
    import mpc_local_planner_amd.workloads as W
    CO.build()
    oc = CO.from_nlp_config(R.config_carlike_min_time(n))
    logical = CO.num_threads()
    pilot = 2048
    x0, xf, up, dtp = W.carlike_min_time_inputs(pilot)
    CO.solve_batch(oc, x0[:64], xf[:64], up[:64], dtp[:64])      # untimed: library load + OpenMP team start-up
    best, cores, nt = 0.0, logical, logical
    while nt >= 4:
        t = time.perf_counter()
        CO.solve_batch(oc, x0, xf, up, dtp, nthreads=nt)
        rate = pilot / (time.perf_counter() - t)
        if rate > best:
            best, cores = rate, nt
        nt //= 2
    sample2 = int(min(64 * BATCH_1GPU, max(pilot, best * 5.0)))
    x0, xf, up, dtp = W.carlike_min_time_inputs(sample2)
    t = time.perf_counter()
    out = CO.solve_batch(oc, x0, xf, up, dtp, nthreads=cores)
    dt = time.perf_counter() - t
    conv = float((out[3] == 0).mean())
    return {"value": sample2 * conv / dt, "value_all_solves": sample2 / dt, "unit": "solves/s", "cores": cores, "kind": "port",
            "converged_frac": conv,
            "sample": f"{sample2} instances drawn from the config-2 distribution (seed {W.SEED_CONFIG2}), cold start, one candidate (the reference "
                      f"path), tol 1e-8, max 100 iterations, mean {float(out[4].mean()):.1f} iterations, {dt:.2f} s wall on {cores} OpenMP threads "
                      f"(best of a pilot over {logical}, {logical}/2, ... threads; the host exposes {logical} logical CPUs)"}


def active_row_fraction(x, obs, d_min, n_inst=512, tol=1e-4):
    """share of instances whose solution has a clearance row at its bound: min over grid points 1..n-2 and polygons of the point-to-polygon
    distance (teb semantics: distance to the closed edge loop) <= d_min + tol.  Host-side numpy on a sample of the batch (reporting only)."""
    no, nv, verts = obs
    B = min(n_inst, x.shape[0])
    act = 0
    for b in range(B):
        p = x[b, 1:-1, :2]                                     # (n-2, 2)
        best = np.full(p.shape[0], np.inf)
        for o in range(int(no[b])):
            k = int(nv[b, o]); v = verts[b, o, :k]
            a, c = v, np.roll(v, -1, axis=0)
            ab = c - a                                         # (k, 2)
            t = np.clip(((p[:, None, :] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1)[None], 0.0, 1.0)
            q = a[None] + t[..., None] * ab[None]
            best = np.minimum(best, np.sqrt(((p[:, None, :] - q) ** 2).sum(-1)).min(1))
        act += int(best.min() <= d_min + tol)
    return act / B


def measured_traffic(key):
    """HBM bytes per launch of the solve kernel from the rocprofv3 PMC passes (FETCH_SIZE x2 on gfx950 + WRITE_SIZE, in bytes),
    as recorded by scripts/summarize_profile.py for this exact workload; None when no matching record is committed."""
    path = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    try:
        rec = json.load(open(path))
    except (OSError, ValueError):
        return None
    rec = rec.get(key) if isinstance(rec.get(key), dict) else (rec if rec.get("key") == key else None)
    return rec.get("bytes_per_launch") if rec else None


def measured_counters(key):
    """PMC means per launch of the solve kernel recorded by scripts/summarize_profile.py for this workload (profiles/pmc_counters.json), or None."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "pmc_counters.json")))
    except (OSError, ValueError):
        return None
    return rec.get(key)


def workgroups_per_cu(solver, B):
    """resident one-wave workgroups per CU of the kernel a launch of B instances selects: the runtime's occupancy calculation on that instantiation (registers, LDS)"""
    return solver.occupancy(B)[0]


def executed_work(key, kernel_ms, convention_flops_per_launch=None, n_simd=1024, clock_hz=2.4e9):
    """What the SIMDs actually issued, from the committed counter pass of the same workload: SQ_INSTS_VALU wave-instructions x 4 cycles of a SIMD's vector issue
    slot each, over kernel time x 1024 SIMDs -- the share of the chip's vector issue slots the launch fills, whatever the instruction computes and however many of its
    64 lanes work (the serial sweeps use 12, the partitioned ones 44+).  Next to it the counters that say why the rest idles."""
    c = measured_counters(key)
    if not c or "SQ_INSTS_VALU" not in c:
        return None
    k_s = (c.get("kernel_avg_ns", kernel_ms * 1e6)) * 1e-9
    out = {"valu_issue_slot_frac": c["SQ_INSTS_VALU"] * 4.0 / (k_s * clock_hz * n_simd), "sq_insts_valu_per_launch": c["SQ_INSTS_VALU"],
           "kernel_ms_in_that_pass": k_s * 1e3, "source": "profiles/" + str(c.get("source"))}
    out["issue_slot_frac"] = out["valu_issue_slot_frac"]
    # 64 lane-slots per issued VALU wave-instruction over the reference-convention flops of the launch (914 per stage and iteration for the car-like model, central-
    # difference Jacobians included, which the kernel never computes): how many lane-slots the kernel spends per flop of the convention the valu_frac numbers are quoted in
    if convention_flops_per_launch:
        out["lane_slots_per_flop"] = c["SQ_INSTS_VALU"] * 64.0 / convention_flops_per_launch
    if c.get("SQ_WAVE_CYCLES"):
        out["valu_busy_frac_of_wave_cycles"] = c.get("SQ_ACTIVE_INST_VALU", 0.0) / c["SQ_WAVE_CYCLES"]
        out["wait_any_frac_of_wave_cycles"] = c.get("SQ_WAIT_ANY", 0.0) / c["SQ_WAVE_CYCLES"] if c.get("SQ_WAIT_ANY") else None
        out["wait_inst_frac_of_wave_cycles"] = c.get("SQ_WAIT_INST_ANY", 0.0) / c["SQ_WAVE_CYCLES"] if c.get("SQ_WAIT_INST_ANY") else None
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, arrays, limit=DUMP_LIMIT_BYTES, seed=0):
    """--dump-outputs: `arrays` (name -> numpy array, leading dimension = instance) as dirname/<name>.npy in float64.  Above `limit` bytes in all, the
    same fixed seeded sample of instances from every array (rows in ascending order), their indices in instance_index.npy.  Returns the names written."""
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    B = next(iter(arrays.values())).shape[0]
    per_instance = sum(a[0].nbytes for a in arrays.values())
    if B * per_instance > limit:
        keep = max(1, limit // (per_instance + 8))
        idx = np.sort(np.random.default_rng(seed).choice(B, size=keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
        arrays["instance_index"] = idx.astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), np.ascontiguousarray(a))
    return sorted(arrays)


class Leg:
    """one solver + device-resident inputs/outputs of one workload"""

    def __init__(self, m, torch, dev, cfg, B, inputs, obstacles=None):
        self.m, self.torch, self.dev, self.B, self.n = m, torch, dev, B, int(cfg.n)
        self.solver = m.BatchSolver(cfg, max_batch=B, device=dev.index)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.inp = [T(a) for a in inputs]
        n = self.n
        self.xo = torch.empty((B, n, 3), dtype=torch.float64, device=dev)
        self.uo = torch.empty((B, n, 2), dtype=torch.float64, device=dev)
        self.do = torch.empty(B, dtype=torch.float64, device=dev)
        self.st = torch.empty(B, dtype=torch.int32, device=dev)
        self.it = torch.empty(B, dtype=torch.int32, device=dev)
        self.ob = None
        if obstacles is not None:
            self.ob_t = [T(a) for a in obstacles]
            self.ob = tuple(t.data_ptr() for t in self.ob_t)

    def step(self, init=None, inp=None, st=None, it=None):
        i = self.inp if inp is None else inp
        xi, ui, di = (None, None, None) if init is None else (t.data_ptr() for t in init)
        self.solver.solve_device(self.B, i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(), xi, ui, di,
                                 self.xo.data_ptr(), self.uo.data_ptr(), self.do.data_ptr(), (st if st is not None else self.st).data_ptr(),
                                 (it if it is not None else self.it).data_ptr(), obstacles=self.ob)

    def sync(self):
        self.solver.synchronize()
        self.torch.cuda.synchronize()

    def timed(self, steps, warmup, **kw):
        for _ in range(warmup):
            self.step(**kw)
        self.sync()
        k_ms = []
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(**kw)
            self.solver.synchronize()          # a control cycle ends when its commands are available
            k_ms.append(self.solver.last_kernel_ms())
        self.sync()
        return time.perf_counter() - t0, float(np.mean(k_ms))

    def stats(self, st=None, it=None):
        status = (self.st if st is None else st).cpu().numpy()
        iters = (self.it if it is None else it).cpu().numpy()
        win, tot = self.solver.last_candidates(self.B)
        ok = status == 0
        return {"converged_frac": float(ok.mean()), "iters_mean": float(iters.mean()), "iters_p50": float(np.percentile(iters, 50)),
                "iters_p99": float(np.percentile(iters, 99)), "iters_max": int(iters.max()),
                "iters_total_mean": float(tot.mean()), "winner_histogram": np.bincount(win + 1, minlength=2).tolist()}, ok

    def close(self):
        self.solver.close()


def leg_summary(leg, steps, warmup, bytes_per_solve, flops_per_iter, peak_tf, traffic_key):
    elapsed, k_ms = leg.timed(steps, warmup)
    s, ok = leg.stats()
    B = leg.B
    bpl = bytes_per_solve * B
    gbs = bpl / (k_ms * 1e-3) / 1e9
    tf = B * s["iters_total_mean"] * flops_per_iter / (k_ms * 1e-3) / 1e12
    ex = executed_work(traffic_key, k_ms, B * s["iters_total_mean"] * flops_per_iter)
    return {"value": B * s["converged_frac"] * steps / elapsed, "value_all_solves": B * steps / elapsed, "unit": "solves/s", "batch": B,
            "ms_per_step": elapsed / steps * 1e3, "solver": s, "lds_bytes_per_instance": leg.solver.occupancy(B)[1], "workgroups_per_cu": workgroups_per_cu(leg.solver, B),
            "roofline": {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                         "traffic": measured_traffic(traffic_key), "kernel": "mpc_ipm_wave_kernel", "kernel_ms": k_ms,
                         "algorithmic_bytes_per_launch": bpl, "valu_frac": tf / peak_tf, "waves_per_simd": workgroups_per_cu(leg.solver, B) / 4.0,
                         "issue_slot_frac": (ex or {}).get("issue_slot_frac"), "lane_slots_per_flop": (ex or {}).get("lane_slots_per_flop"),
                         "executed": ex,
                         "valu": {"achieved_tflops": tf, "peak_tflops": peak_tf, "frac": tf / peak_tf, "flops_per_iteration": flops_per_iter}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="instances per GPU (default: 1024 at N=1 = configs[1], 4096 at N>1 = configs[3])")
    ap.add_argument("--n", type=int, default=N_GRID)
    ap.add_argument("--candidates", type=str, default=",".join(str(k) for k in CAND_KINDS), help="candidate kinds in priority order; '0' = the single reference solve")
    ap.add_argument("--caps", type=str, default="", help="per-candidate iteration caps (default: %s up to 1024 instances per GPU, %s at 4096)" % (CAND_CAPS, CAND_CAPS_LARGE_BATCH))
    ap.add_argument("--params", type=str, default=",".join(str(k) for k in CAND_PARAMS), help="per candidate: tangent scale of the Hermite kinds")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-legs", action="store_true", help="skip the extra legs (warm start, other configs)")
    ap.add_argument("--no-parity-check", action="store_true", help="skip the reference-path-alone run behind solver.answers_equal_to_the_reference_path_alone (profiling runs: keeps the kernel statistics of rocprofv3 to the headline launches)")
    ap.add_argument("--force-dist", action="store_true", help="developer check on a one-GPU box: take the N > 1 code path (process group, barriers, RCCL "
                    "all-gather of the results) with a world of one rank")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure: parity and reproducibility checks, measured FMA peaks, the extra "
                    "legs, the CPU baseline, rank 0's solo reference at N > 1")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the outputs of the last timed step as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    import torch
    import torch.distributed as dist
    import mpc_local_planner_amd as m
    from mpc_local_planner_amd import sharding

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    torch.zeros(1, device=dev)
    multi = world > 1 or args.force_dist
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        dist.init_process_group(backend="nccl", device_id=dev, rank=rank, world_size=world)

    n = args.n
    B = args.batch if args.batch > 0 else (BATCH_PER_GPU_MULTI if multi else BATCH_1GPU)
    kinds = tuple(int(k) for k in args.candidates.split(","))
    caps = (tuple(int(k) for k in args.caps.split(",")) if args.caps else (CAND_CAPS_LARGE_BATCH if B >= 4096 else CAND_CAPS))[:len(kinds)]
    pars = tuple(float(k) for k in args.params.split(","))[:len(kinds)]
    ckw = dict(candidates=kinds, candidate_max_iter=caps, candidate_param=pars) if len(kinds) > 1 else {}
    # the warm-start leg has its own solver: its handle keeps the multipliers of every instance's last converged solve (dual_warm_start) and the
    # next cycle starts from them at mu0 = 1e-3; the headline solver does not write them
    cfg = m.config_carlike_min_time(n=n, **ckw)
    cfg_warm = m.config_carlike_min_time(n=n, mu_init_warm=1e-2, dual_warm_start=True, mu_init_dual=1e-3, **ckw)
    # independent planner instances per rank: seed + rank (no scatter needed)
    leg = Leg(m, torch, dev, cfg, B, m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank)))

    # warm-up outside run_sharded_job: the reference copy of the last warm-up step's results is taken between the two -- the timed steps solve the same inputs and have to
    # reproduce them bit for bit (the candidate rule is timing independent); the LAST step is compared after the timed region
    for _ in range(args.warmup):
        leg.step()
    leg.sync()
    ref_out = (leg.xo.clone(), leg.uo.clone(), leg.do.clone(), leg.st.clone(), leg.it.clone()) if args.full and args.warmup > 0 else None
    # The timed region and, for N > 1, everything around it -- rank 0's solo reference (the denominator for scaling efficiency, measured in THIS run: same box, same clocks,
    # same warm-up state), the barriers, the maximum over the ranks, the RCCL all-gather of the results AFTER the timed region and the check that every rank's slice of the
    # gathered arrays is what it computed -- is ONE function that the CPU test suite drives under gloo at world 8 (tests/test_multi_gpu_cpu.py): sharding.run_sharded_job
    kernel_ms = []

    class _Timed:
        def step_wait(self):
            leg.step()
            leg.solver.synchronize()          # a control cycle ends when its commands are available
            kernel_ms.append(leg.solver.last_kernel_ms())

        def sync(self):
            leg.sync()

        def results(self):
            return leg.st, leg.do, leg.xo
    job = sharding.run_sharded_job(_Timed(), args.steps, 0, rank, world, B * world, device=dev, solo_reference=args.full, force_gather=args.force_dist)
    kernel_ms = kernel_ms[-args.steps:]          # (with --full, rank 0's solo reference ran the same steps before the timed ones)
    elapsed, solo_elapsed = job["elapsed"], job["solo_elapsed"]
    sstat, ok = leg.stats()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"x": leg.xo.cpu().numpy(), "u": leg.uo.cpu().numpy(), "dt": leg.do.cpu().numpy(), "status": leg.st.cpu().numpy(),
                                         "iterations": leg.it.cpu().numpy()})
    reproducible = None
    if ref_out is not None:
        reproducible = bool(all(torch.equal(a_, b_) for a_, b_ in zip(ref_out, (leg.xo, leg.uo, leg.do, leg.st, leg.it))))

    # ---- N > 1: every rank ends with the whole job's results (RCCL all-gather of HBM-resident arrays), outside the timed region
    gather = None
    n_conv_total = job["converged_total"]
    if multi:
        g_st, g_dt, g_x = job["gathered"]
        nbytes = (g_st.numel() * 4 + g_dt.numel() * 8 + g_x.numel() * 8)
        gather = {"ms": job["gather_ms"], "bytes_per_rank_received": nbytes, "what": "status, dt_out, x_out of all ranks (RCCL all_gather, device resident), first call "
                  "(includes communicator warm-up); NOT part of ms_per_step"}

    line = None
    if rank == 0:
        total = B * world * args.steps
        k_ms = float(np.mean(kernel_ms))
        conv_frac_job = n_conv_total / (B * world)
        bytes_per_launch = algorithmic_bytes_per_solve(n) * B
        achieved_gbs = bytes_per_launch / (k_ms * 1e-3) / 1e9
        flops_per_iter = 914.0 * (n - 1)               # SURVEY.md 8d convention
        from mpc_local_planner_amd import _lib as mlib
        # the FMA-rate micro-benchmark takes launches of its own: --full only (without it the measured-peak fields are None)
        pk64, pk32 = (mlib.measured_fma_peak(local_rank, True), mlib.measured_fma_peak(local_rank, False)) if args.full else (None, None)
        fp64_tf = B * sstat["iters_total_mean"] * flops_per_iter / (k_ms * 1e-3) / 1e12
        fp64_useful_tf = B * sstat["iters_mean"] * flops_per_iter / (k_ms * 1e-3) / 1e12
        ex_h = executed_work(f"carlike_n{n}_B{B}_c{len(kinds)}", k_ms, B * sstat["iters_total_mean"] * flops_per_iter)
        wl = ("BASELINE.json configs[1]: carlike (Ackermann) minimum-time MPC, n=50 grid points, batch=1024 instances on 1 MI355X" if (world == 1 and B == BATCH_1GPU and n == N_GRID) else
              (f"BASELINE.json configs[3]: carlike minimum-time MPC, n=50, batch={B * world} sharded across {world} MI355X ({B} per GPU)" if (B == BATCH_PER_GPU_MULTI and n == N_GRID) else
               f"carlike minimum-time MPC, n={n}, batch={B} per GPU (non-default size)"))
        line = {
            "metric": "MPC solves/sec (batched control cycles) at N=50 carlike",
            "value": total * conv_frac_job / elapsed, "value_all_solves": total / elapsed,
            "unit": "solves/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": wl + "; cold start (Controller::step on an empty grid), tol 1e-8; value counts converged solves only",
                       "n": n, "batch_per_gpu": B, "global_batch": B * world,
                       "candidates": {"kinds": list(kinds), "max_iter": list(caps), "param": list(pars),
                                      "rule": "lowest-index candidate that converges within its cap supplies the result (index 0 = the reference cold start)"},
                       "parallelism": f"instances sharded over {world} GPU(s), no data-path collective in the timed region",
                       "lds_bytes_per_instance": leg.solver.occupancy(B)[1], "workgroups_per_cu": workgroups_per_cu(leg.solver, B),
                       "seed": m.workloads.SEED_CONFIG2},
            "solver": dict(sstat, converged_frac_job=conv_frac_job, last_step_reproduces_the_warmup_step_bit_for_bit=reproducible),
            "roofline": {"bound": "hbm", "achieved": achieved_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved_gbs / HBM_PEAK_GBS, "traffic": measured_traffic(f"carlike_n{n}_B{B}_c{len(kinds)}"),
                         "kernel": "mpc_ipm_wave_kernel",
                         "kernel_ms": k_ms,
                         "algorithmic_bytes_per_launch": bytes_per_launch,
                         "note": "latency/FP64-issue bound by construction (SURVEY.md 8d): compulsory traffic is ~4 KB per solve; the numbers that say how the chip is used are the valu_* scalars below",
                         # the fp64 vector side, as top-level scalars (the nested dict below keeps the detail): reference-convention flops (914 per
                         # stage and iteration) of ALL candidates' iterations / of the winners' only, over the data-sheet peak and over the FMA rate measured in this run
                         "valu_frac": fp64_tf / FP64_VECTOR_PEAK_TF, "valu_useful_frac": fp64_useful_tf / FP64_VECTOR_PEAK_TF,
                         "valu_peak_measured_tflops": (pk64[0] if pk64 else None), "valu_frac_of_measured_peak": (fp64_tf / pk64[0] if pk64 else None),
                         "waves_per_simd": workgroups_per_cu(leg.solver, B) / 4.0,
                         "issue_slot_frac": (ex_h or {}).get("issue_slot_frac"), "lane_slots_per_flop": (ex_h or {}).get("lane_slots_per_flop"),
                         "executed": ex_h,
                         "fp64_valu": {"achieved_tflops": fp64_tf, "peak_tflops": FP64_VECTOR_PEAK_TF,
                                       "frac": fp64_tf / FP64_VECTOR_PEAK_TF,
                                       "useful_tflops": fp64_useful_tf, "useful_frac": fp64_useful_tf / FP64_VECTOR_PEAK_TF,
                                       "flops_per_iteration": flops_per_iter,
                                       "peak_measured_tflops": (pk64[0] if pk64 else None), "frac_of_measured_peak": (fp64_tf / pk64[0] if pk64 else None),
                                       "fp32_peak_measured_tflops": (pk32[0] if pk32 else None),
                                       "peak_measured_how": "csrc/mpc_ubench.hip: 8 independent v_fma_f64 (v_pk_fma_f32) chains per lane, 8 waves per SIMD on every CU, best of 3 launches of ~10 ms",
                                       "note": "frac counts the iterations of ALL candidates of an instance as work; useful_frac only those of the candidate that supplied the result"}},
        }
        if gather is not None:
            line["gather"] = gather
        if multi and solo_elapsed is not None:
            line["per_gpu_reference"] = {"value": B * float(ok.mean()) * args.steps / solo_elapsed, "unit": "solves/s", "ms_per_step": solo_elapsed / args.steps * 1e3,
                                         "what": "rank 0 alone on the same %d instances, %d steps, measured in this run right before the joint timed region (the other ranks wait "
                                                 "at a barrier): the denominator for scaling efficiency, not the N = 1 headline (1024 instances, latency bound)" % (B, args.steps)}

    # ---- parity statement of the headline (every N; outside the timed region): the same inputs through the REFERENCE PATH ALONE (one candidate, the
    # reference's 100 iterations).  An instance counts as "equal" when the reference path converges and the headline returns candidate 0's trajectory,
    # bit for bit the reference path's, or when the reference path does not converge (then a hedge may answer).
    st_r = dt_r = None
    if args.full and len(kinds) > 1 and not args.no_parity_check:
        win_h, _ = leg.solver.last_candidates(B)
        lr = Leg(m, torch, dev, m.config_carlike_min_time(n=n), B, m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank)))
        lr.step(); lr.sync()
        dt_r = lr.do.cpu().numpy(); st_r = lr.st.cpu().numpy()
        conv_r = lr.st == 0
        same_traj = ((lr.xo == leg.xo).flatten(1).all(1) & (lr.uo == leg.uo).flatten(1).all(1) & (lr.do == leg.do)).cpu().numpy()
        equal = np.where(st_r == 0, (win_h == 0) & same_traj, True)
        if rank == 0:
            line["solver"]["answers_equal_to_the_reference_path_alone"] = float(equal.mean())
            line["solver"]["reference_path_alone_converged_frac"] = float((st_r == 0).mean())
            line["solver"]["parity_note"] = ("candidate 0 = the reference's cold start with the reference's iteration budget (%d); 1.0 = every instance that path solves is answered with "
                                             "exactly its trajectory (bit for bit), hedges answer only instances it leaves unsolved" % caps[0])
        lr.close()

    # ---- extra legs (--full, N = 1 only; after the timed region)
    if args.full and not multi and not args.no_legs:
        legs = {}
        if len(kinds) > 1 and st_r is not None:
            # the latency-tuned operating point of rounds 2/3: candidate 0 capped at 60 iterations.  Faster, but instances the reference path would still
            # have solved get a hedge's answer -- a different local optimum in most of them; what that costs in solution quality is reported here:
            # objective(hedge's answer) - objective(reference path's answer), objective = (n - 1) dt
            capsh = CAND_CAPS_HEDGED[:len(kinds)]
            lh = Leg(m, torch, dev, m.config_carlike_min_time(n=n, candidates=kinds, candidate_max_iter=capsh, candidate_param=pars), B,
                     m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank)))
            legs["hedged_caps_60"] = leg_summary(lh, max(2, args.steps // 2), 1, algorithmic_bytes_per_solve(n), 914.0 * (n - 1), FP64_VECTOR_PEAK_TF, f"carlike_n{n}_B{B}_c{len(kinds)}")
            legs["hedged_caps_60"]["candidate_max_iter"] = list(capsh)
            wh, _ = lh.solver.last_candidates(B)
            dt_h = lh.do.cpu().numpy().copy(); st_h = lh.st.cpu().numpy().copy()
            lh.close()
            sel = (wh > 0) & (st_h == 0) & (st_r == 0)
            dobj = (n - 1) * (dt_h[sel] - dt_r[sel])
            legs["hedged_caps_60"]["answers_equal_to_the_reference_path_alone"] = float(np.where(st_r == 0, wh == 0, True).mean())
            legs["hedged_caps_60"]["hedge_vs_reference_path"] = {
                "instances_answered_by_a_hedge": int((wh > 0).sum()), "of_which_the_100_iteration_reference_path_solves": int(sel.sum()),
                "objective_hedge_minus_reference": ({"min": float(dobj.min()), "p10": float(np.percentile(dobj, 10)), "median": float(np.median(dobj)), "p90": float(np.percentile(dobj, 90)),
                                                     "max": float(dobj.max()), "same_within_1e-6": float((np.abs(dobj) < 1e-6).mean()), "hedge_better": float((dobj < -1e-6).mean()),
                                                     "hedge_worse": float((dobj > 1e-6).mean())} if sel.any() else None),
                "unit": "seconds of travel time ((n-1) dt); negative = the hedge's local optimum is FASTER than the reference path's"}
        # warm start, reported separately: the plant advances one controller period (0.2 s) with u_0, the previous solution is
        # the initial guess with x0 overwritten (full_discretization_grid_base_se2.cpp:101-110; variable grid: no shifting)
        per, Lw = 0.2, float(cfg.model_params[0])
        lw = Leg(m, torch, dev, cfg_warm, B, m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank)))
        lw.step(); lw.sync()
        assert torch.equal(lw.xo, leg.xo) and torch.equal(lw.st, leg.st)
        leg.close()
        leg = lw
        dx0, dxf = leg.inp[0], leg.inp[1]
        u0 = leg.uo[:, 0, :].clone()
        x1 = dx0.clone()
        x1[:, 0] += per * u0[:, 0] * torch.cos(dx0[:, 2]); x1[:, 1] += per * u0[:, 0] * torch.sin(dx0[:, 2])
        x1[:, 2] = torch.remainder(dx0[:, 2] + per * u0[:, 0] * torch.tan(u0[:, 1]) / Lw + np.pi, 2 * np.pi) - np.pi
        init = (leg.xo.clone(), leg.uo.clone(), leg.do.clone())
        dper = torch.full((B,), per, dtype=torch.float64, device=dev)
        st2 = torch.empty_like(leg.st); it2 = torch.empty_like(leg.it)
        # every timed warm cycle follows an (untimed) repeat of the cold cycle, so that the handle holds the multipliers of the COLD solution --
        # what a closed loop has at this point -- and not those of an earlier repetition of the same warm solve
        tw, kms = 0.0, []
        for k in range(args.warmup + args.steps):
            leg.step(); leg.sync()
            t1 = time.perf_counter()
            leg.step(init=init, inp=[x1, dxf, u0, dper], st=st2, it=it2)
            leg.solver.synchronize()
            if k >= args.warmup:
                tw += time.perf_counter() - t1; kms.append(leg.solver.last_kernel_ms())
        kw_ms = float(np.mean(kms))
        s2, ok2 = leg.stats(st2, it2)
        it2n = it2.cpu().numpy()
        legs["warm_start"] = {"value": B * float(ok2.mean()) * args.steps / tw, "value_all_solves": B * args.steps / tw, "unit": "solves/s", "ms_per_step": tw / args.steps * 1e3, "kernel_ms": kw_ms,
                              "converged_frac": float(ok2.mean()), "converged_frac_of_previously_converged": float(ok2[ok].mean()), "iters_mean": float(it2n[ok].mean()),
                              "iters_p99": float(np.percentile(it2n[ok], 99)),
                              "init": "previous solution with x0 advanced one 0.2 s period under u_0 as candidate 0, started from the multipliers the handle kept from the cold cycle "
                                      "(dual_warm_start: every inequality multiplier max(previous, mu0 / slack), mu0 = 1e-3); the hedges start cold from their own seeds"}
        leg.close()
        # configs[3] share on one GPU (what every rank of the N = 8 run does)
        caps4 = (tuple(int(k) for k in args.caps.split(",")) if args.caps else CAND_CAPS_LARGE_BATCH)[:len(kinds)]
        cfg4 = m.config_carlike_min_time(n=n, candidates=kinds, candidate_max_iter=caps4, candidate_param=pars) if len(kinds) > 1 else cfg
        l4 = Leg(m, torch, dev, cfg4, BATCH_PER_GPU_MULTI, m.workloads.carlike_min_time_inputs(BATCH_PER_GPU_MULTI))
        legs["config4_share_B4096"] = leg_summary(l4, max(2, args.steps // 2), 1, algorithmic_bytes_per_solve(n), 914.0 * (n - 1), FP64_VECTOR_PEAK_TF, f"carlike_n{n}_B4096_c{len(kinds)}")
        legs["config4_share_B4096"]["candidate_max_iter"] = list(caps4)
        l4.close()
        # configs[2]: unicycle quadratic form, n = 80, 16 polygon obstacles, B = 4096.  SURVEY 8d asks for polygons IN the corridor: the leg that counts
        # puts them 0.15 .. 0.8 m beside the start-goal line with d_min = 0.2 (rows start violated and bind at the solution; the share of instances with
        # an active row is reported); the placement of round 2 (0.3 .. 1.5 m: rows carried but inactive) is the second leg.  max_iter 60: the launch is
        # bound by its slowest instance below 2048 instances, and the mean is 28 iterations.
        n3, B3, O, V, M = 80, 4096, 16, 6, 4
        for tag, lateral in (("config3_unicycle_n80_16polygons_B4096", (0.15, 0.8)), ("config3_rows_inactive_placement_B4096", (0.3, 1.5))):
            x0, xf, up, dtp, obs = m.workloads.unicycle_obstacle_inputs(B3, n_obst=O, max_vertices=V, lateral=lateral)
            l3 = Leg(m, torch, dev, m.config_unicycle_quadratic(n3, max_obstacles=O, max_vertices=V, max_obstacle_rows=M, max_iter=60), B3, (x0, xf, up, dtp), obstacles=obs)
            osc = int(np.mean([(2 * obs[1][b] + 2).sum() for b in range(64)]))       # sum(2 V_j + 2) obstacle scalars per instance
            legs[tag] = leg_summary(l3, max(2, args.steps // 2), 1, algorithmic_bytes_per_solve(n3, 8, osc), (18 + 342 + 418 + 100) * (n3 - 1) + 60 * 2 * (n3 - 2),
                                    FP64_VECTOR_PEAK_TF, "unicycle_n80_B4096")
            xs = l3.xo.cpu().numpy(); ok3 = l3.st.cpu().numpy() == 0
            legs[tag]["placement"] = f"polygons {lateral[0]} .. {lateral[1]} m beside the start-goal line, min_obstacle_dist 0.2"
            legs[tag]["instances_with_an_active_clearance_row"] = active_row_fraction(xs[ok3], tuple(a[ok3] for a in obs), 0.2)
            legs[tag]["max_iter"] = 60
            l3.close()
        # configs[4] share: kinematic bicycle, n = 120, fp32, 1024 per GPU
        n5, B5 = 120, 1024
        # candidate set chosen ON THE DEVICE in fp32 (tests/tools/gpu_candidate_sweep_config5.py, profiles/r02_candidate_sweep_config5.log): the reference cold
        # start, then the reference's own no-initial-plan guess (heading = direction of travel), its reverse-driving twin and one Hermite seed.  On these
        # 5-40 m problems the reference cold start alone converges for 72 %, this set for 99.8 % (6 draws: see the log); the headline's Hermite set at
        # caps 100, which this leg ran before, reached 97.9 % in 20 ms.
        c5kw = dict(candidates=CAND5_KINDS, candidate_max_iter=CAND5_CAPS, candidate_param=CAND5_PARAMS) if len(kinds) > 1 else {}
        f5 = (24 + 486 + 418 + 100) * (n5 - 1)
        # r05: the leg that counts is plain fp64 -- the reference's arithmetic, 1022 of 1024 answers within 1e-4 of the fp64 oracle's candidate rule
        # (tests/test_gpu_closed_loop.py::test_config5_candidates_vs_oracle_rule_fp64_and_mixed, floor 95 %).  It became affordable when the factorisation data
        # left LDS (mpc_config.stage_data, MPC_STAGE_AUTO: four workgroups per CU instead of one).  MPC_MIXED (fp32 main phase + fp64 refinement: within 1e-7 of
        # ITS fp64 optimum, but the fp32 phase picks another basin in ~19 % of the instances) and plain fp32 -- the precision BASELINE.json names, which does NOT
        # meet the 1e-4 tolerance (median 2e-4 .. 5e-3 from the fp64 result) -- are reported next to it.
        c5d = m.config_bicycle_min_time(n5, precision=0, **c5kw)
        l5d = Leg(m, torch, dev, c5d, B5, m.workloads.bicycle_min_time_inputs(B5))
        legs["config5_share_bicycle_n120_fp64_B1024"] = leg_summary(l5d, max(2, args.steps // 2), 1, algorithmic_bytes_per_solve(n5, 8), f5, FP64_VECTOR_PEAK_TF, "bicycle_n120_fp64_B1024")
        legs["config5_share_bicycle_n120_fp64_B1024"]["dtype"] = "f64"
        legs["config5_share_bicycle_n120_fp64_B1024"]["parity"] = ("not measured in this run (bench.py may call the oracle only as its CPU baseline): the share of answers within 1e-4 of the fp64 oracle's "
                                                                   "candidate rule on these 1024 instances is asserted >= 0.95 by tests/test_gpu_closed_loop.py::test_config5_candidates_vs_oracle_rule_fp64_and_mixed (GPUTEST); "
                                                                   "the leg that counts for BASELINE configs[4]")
        l5d.close()
        if len(kinds) > 1:
            # the same leg at the PARITY-PRESERVING operating point of the headline: candidate 0 -- the reference's cold start -- runs the reference's 100 iterations, so every instance
            # that path solves within the reference's budget is answered by it (lowest converged index wins); the hedges keep their caps.  The launch lasts as long as 100 iterations of a wave.
            caps100 = (100,) + tuple(CAND5_CAPS[1:])
            l5p = Leg(m, torch, dev, m.config_bicycle_min_time(n5, precision=0, candidates=CAND5_KINDS, candidate_max_iter=caps100, candidate_param=CAND5_PARAMS), B5, m.workloads.bicycle_min_time_inputs(B5))
            el, kms = l5p.timed(max(2, args.steps // 2), 1)
            s5, _ = l5p.stats()
            legs["config5_share_bicycle_n120_fp64_B1024_reference_path_at_100_iterations"] = {
                "value": B5 * s5["converged_frac"] * max(2, args.steps // 2) / el, "unit": "solves/s", "batch": B5, "ms_per_step": el / max(2, args.steps // 2) * 1e3, "kernel_ms": kms,
                "caps": list(caps100), "solver": s5, "answered_by_the_reference_path": s5["winner_histogram"][1] / B5,
                "what": "the fp64 leg above with candidate 0 at the reference's iteration budget instead of 60: the share of answers that are the reference path's own rises, the launch lasts 100 iterations"}
            l5p.close()
        c5m = m.config_bicycle_min_time(n5, precision=2, **c5kw)
        l5m = Leg(m, torch, dev, c5m, B5, m.workloads.bicycle_min_time_inputs(B5))
        legs["config5_share_bicycle_n120_mixed_B1024"] = leg_summary(l5m, max(2, args.steps // 2), 1, algorithmic_bytes_per_solve(n5, 8), f5, FP32_VECTOR_PEAK_TF, "bicycle_n120_mixed_B1024")
        legs["config5_share_bicycle_n120_mixed_B1024"]["dtype"] = "f32 main phase + f64 refinement"
        legs["config5_share_bicycle_n120_mixed_B1024"]["parity"] = "refines to ITS OWN fp64 optimum; the share of answers that are the fp64 oracle rule's is asserted >= 0.6 by the same GPU test (the fp32 phase picks another basin in about one instance of five)"
        # (no counter pass is committed for this leg and the next: they carry throughput and solver statistics only, no roofline block -- VERDICT r05 item 8)
        legs["config5_share_bicycle_n120_mixed_B1024"]["kernel_ms_both_phases"] = legs["config5_share_bicycle_n120_mixed_B1024"].pop("roofline")["kernel_ms"]
        l5m.close()
        c5 = m.config_bicycle_min_time(n5, precision=1, tol=1e-4, **c5kw)
        l5 = Leg(m, torch, dev, c5, B5, m.workloads.bicycle_min_time_inputs(B5))
        legs["config5_share_bicycle_n120_fp32_B1024"] = leg_summary(l5, max(2, args.steps // 2), 1, algorithmic_bytes_per_solve(n5, 4), f5, FP32_VECTOR_PEAK_TF, "bicycle_n120_fp32_B1024")
        legs["config5_share_bicycle_n120_fp32_B1024"]["dtype"] = "f32"
        legs["config5_share_bicycle_n120_fp32_B1024"]["parity"] = "plain fp32 does NOT meet the 1e-4 tolerance against the fp64 result (DESIGN.md section 6); reported because BASELINE configs[4] names fp32"
        legs["config5_share_bicycle_n120_fp32_B1024"]["kernel_ms"] = legs["config5_share_bicycle_n120_fp32_B1024"].pop("roofline")["kernel_ms"]
        l5.close()
        # (r06) an EXTENDED kernel level on a grid whose LDS record fits once per CU: car-like minimum time, n = 80, the shipped car-like file's line footprint, three obstacles beside
        # the path of which one crosses it (stage_inequality_se2.cpp:164-189).  The factorisation data in the global block (MPC_STAGE_AUTO) against everything in LDS.
        from mpc_local_planner_amd import _abi as mabi
        nE, BE = 80, 1024
        x0e, xfe, upe, dtpe, obe = m.workloads.carlike_moving_obstacle_inputs(BE)
        ext = {}
        for tag, mode in (("lds_form", mabi.STAGE_LDS), ("auto", mabi.STAGE_AUTO)):
            le = Leg(m, torch, dev, m.config_carlike_min_time(nE, footprint_kind=2,      # MPC_FOOTPRINT_LINE
                                                            footprint_params=(0.0, 0.0, 0.4, 0.0), enable_dynamic_obstacles=True,
                                                            min_obstacle_dist=0.27, force_inclusion_dist=0.5, cutoff_dist=2.5, max_obstacles=3, max_vertices=1, max_obstacle_rows=4, stage_data=mode),
                     BE, (x0e, xfe, upe, dtpe), obstacles=obe)
            el, kms = le.timed(max(2, args.steps // 2), 1)
            se, oke = le.stats()
            ext[tag] = {"value": BE * float(oke.mean()) * max(2, args.steps // 2) / el, "unit": "solves/s", "kernel_ms": kms, "converged_frac": float(oke.mean()), "iters_mean": se["iters_mean"],
                        "workgroups_per_cu": workgroups_per_cu(le.solver, BE), "lds_bytes_per_instance": le.solver.occupancy(BE)[1], "checksum_dt": float(le.do.sum().item())}
            le.close()
        ext["same_answers"] = bool(ext["lds_form"]["checksum_dt"] == ext["auto"]["checksum_dt"])
        ext["what"] = "car-like minimum time, n = 80, line footprint, 3 obstacles of which one moves across the path, 1024 instances, reference path alone (extended kernel level 1)"
        legs["carlike_n80_line_footprint_moving_obstacle_B1024"] = ext
        # the reference's shipped grid size (grid_size_ref 20 in every example parameter file) at saturation: one wave per SIMD against the two-waves-per-SIMD kernel that
        # mpc_config.two_wave_min_batch selects for launches this large (its 15.6 KB record fits eight times into a CU); the reference path alone, same answers bit for bit
        n20, B20 = 20, 32768
        inp20 = m.workloads.carlike_min_time_inputs(B20, goal_range=(1.0, 6.0 * n20 / 50.0))
        w2 = {}
        for tag, tw in (("one_wave_per_simd", -1), ("two_waves_per_simd", 0)):
            l20 = Leg(m, torch, dev, m.config_carlike_min_time(n20, two_wave_min_batch=tw), B20, inp20)
            el, kms = l20.timed(max(2, args.steps // 2), 1)
            s20, ok20 = l20.stats()
            w2[tag] = {"value": B20 * float(ok20.mean()) * max(2, args.steps // 2) / el, "unit": "solves/s", "kernel_ms": kms, "converged_frac": float(ok20.mean()), "iters_mean": s20["iters_mean"],
                       "workgroups_per_cu": workgroups_per_cu(l20.solver, B20), "lds_bytes_per_instance": l20.solver.occupancy(B20)[1], "checksum_dt": float(l20.do.sum().item())}
            l20.close()
        w2["same_answers"] = bool(w2["one_wave_per_simd"]["checksum_dt"] == w2["two_waves_per_simd"]["checksum_dt"])
        w2["what"] = "car-like minimum time on the reference's shipped grid size n = 20, 32768 instances on one GPU, reference path alone (one candidate), goals 1 .. 2.4 m"
        legs["reference_grid_n20_B32768"] = w2
        # two 1024-instance batches in flight on two handles / streams (a fleet of 2048 in two control groups): the tail of one launch -- the 3 % of reference-path
        # waves that run their 100 iterations while most SIMDs idle -- is filled by the other.  A leg, never the headline: the headline is ONE batch per step.
        la = Leg(m, torch, dev, cfg, B, m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank)))
        lb = Leg(m, torch, dev, cfg, B, m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank) + 1000))
        for _ in range(2):
            la.step(); lb.step()
        la.sync(); lb.sync()
        ksteps = max(2, args.steps // 2)
        t2 = time.perf_counter()
        for _ in range(ksteps):
            la.step(); lb.step()
            la.solver.synchronize(); lb.solver.synchronize()
        la.sync(); lb.sync()
        t2 = time.perf_counter() - t2
        sa, oka = la.stats(); sb_, okb = lb.stats()
        legs["two_batches_in_flight_2x1024"] = {"value": (float(oka.sum()) + float(okb.sum())) * ksteps / t2, "unit": "solves/s", "ms_per_step_of_both": t2 / ksteps * 1e3,
                                                "converged_frac": 0.5 * (sa["converged_frac"] + sb_["converged_frac"]),
                                                "what": "two handles, two streams, one 1024-instance batch each, both launched before either is waited for; same candidates / caps as the headline"}
        la.close(); lb.close()
        # the same 1024-instance batch through the HOST-pointer entry of the boundary (mpc_solve_batch: one pinned staging copy each way + one H2D + one D2H per call): the
        # PCIe-inclusive rate, reported next to `value` (which is measured with the inputs resident in HBM) and never in its place
        sh = m.BatchSolver(cfg, max_batch=B, device=local_rank)
        hin = m.workloads.carlike_min_time_inputs(B, seed=sharding.rank_seed(m.workloads.SEED_CONFIG2, rank))
        rh = sh.solve(*hin)
        th = time.perf_counter()
        kh = max(2, args.steps // 2)
        for _ in range(kh):
            rh = sh.solve(*hin)
        th = time.perf_counter() - th
        sh.close()
        legs["host_pointer_entry_B1024"] = {"value": B * float(np.mean(rh.status == 0)) * kh / th, "unit": "solves/s", "ms_per_step": th / kh * 1e3,
                                            "what": "mpc_solve_batch with host buffers in and out (inputs 72 B, outputs ~2 KB per instance; staging + H2D + kernel + D2H, synchronous)"}
        # B = 1: what ONE move_base instance pays per control cycle -- Controller::step through the host-pointer entry (PCIe and launch included),
        # 256 different config-2 instances solved one at a time, cold start with the headline's candidates (all of them run concurrently here)
        s1 = m.BatchSolver(cfg, max_batch=1, device=local_rank)
        xs = m.workloads.carlike_min_time_inputs(256)
        lat, ok1 = [], []
        for i in range(260):
            j = i % 256
            t1 = time.perf_counter()
            r1 = s1.solve(xs[0][j:j + 1], xs[1][j:j + 1], xs[2][j:j + 1], xs[3][j:j + 1])
            if i >= 4:
                lat.append(time.perf_counter() - t1); ok1.append(int(r1.status[0] == 0))
        s1.close()
        lat = np.asarray(lat) * 1e3
        legs["single_instance_latency_B1"] = {"ms_mean": float(lat.mean()), "ms_p50": float(np.percentile(lat, 50)), "ms_p99": float(np.percentile(lat, 99)), "ms_max": float(lat.max()),
                                              "converged_frac": float(np.mean(ok1)), "unit": "ms per Controller::step-equivalent solve (host pointers in and out)",
                                              "note": "the reference's implied budget is 200 ms (move_base at 5 Hz) / 50 ms (test node at 20 Hz), BASELINE.md section 1"}
        line["legs"] = legs
        line["scaling_reference"] = {"per_gpu_value_at_4096": legs["config4_share_B4096"]["value"],
                                     "note": "bench.py --gpus N>1 runs configs[3] (4096 instances per GPU); its per-GPU reference on one GPU is this leg, not the N=1 headline (1024 instances)"}
    else:
        leg.close()
    if args.full and rank == 0 and not args.no_cpu_baseline and not multi:
        line["cpu_baseline"] = cpu_baseline(n)
    if multi:
        dist.destroy_process_group()
    if rank == 0:
        # the JSON line goes out LAST: RCCL prints a version banner through C stdio, which a pipe would otherwise deliver after python's buffer
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
