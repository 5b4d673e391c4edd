"""GPU tests (-m gpu) of whole Controller::step cycles for a batch (mpc_controller_step_batch*, mpc_local_planner_amd/csrc/mpc_controller_cycle.hpp).

The yardstick is the host facade of ONE robot, include/mpc_controller.hpp: tests/gpu_controller_batch.cpp holds B facade Controllers, each with its own B = 1
handle, next to one handle with max_batch = B driven by mpc_controller_step_batch, in closed loop, and compares x, u, dt, converged, iterations, grid size bit for
bit in every cycle, plus the re-initialisation flags against what the program works out from the facades' public state.  The device variant is held to the host
variant (clearance rows, candidates), and a handle with two parameter sets to two single-set handles.

The yaw of an intermediate plan pose is an atan2: the facade calls the host's libm, the device a correctly rounded routine; they differ by one ulp where libm is off
(0.08 % of arguments, tests/test_controller_cycle_host.py).  The plans of gpu_controller_batch.cpp are fixed: ten such arguments in all."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST, NUM_STEPS, GOAL_DIST, GOAL_ANGULAR, RESET, PLAN_GUESS = 1, 2, 4, 8, 16, 32


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as pkg
    return pkg, torch


@pytest.fixture(scope="module")
def exe(env, tmp_path_factory):
    libdir = os.path.join(ROOT, "mpc_local_planner_amd", "csrc")
    out = str(tmp_path_factory.mktemp("controller_batch") / "gpu_controller_batch")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "gpu_controller_batch.cpp"), "-L" + libdir, "-lmpc_hip", "-Wl,-rpath," + libdir, "-o", out], check=True)
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BATCH_OK" in r.stdout, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("outer", [1, 2])
def test_batched_controller_is_eight_separate_controllers(exe, outer):
    """unicycle, stride 12, n_ref 8, minimum time, variable grid with adaptation (3..12), force_reinit_num_steps 7, 12 cycles in closed loop; per robot: steady goal
    (2 poses), 5-pose curved plan, goal jump of 1.5 m in cycle 4, goal turned by 100 degrees in cycle 5, reset in cycle 3 (re-initialised at its last optimised dt),
    state feedback (fresh on even cycles, stale on odd), 9-pose plan with a heading through +-pi, goal moved by 0.5 m (no re-initialisation; this robot joins in cycle 3,
    so that one launch holds a cold start next to plan guesses and warm starts).  The program itself refuses a run in which a cause did not fire or no launch mixed the
    three start kinds."""
    out = _run(exe, "variable", str(outer))
    last = [l for l in out.splitlines() if l.startswith("compared")][0]
    assert last.startswith("compared 93 robot-cycles, 0 differ; causes seen 63 (all: 63)"), last
    assert int(last.rsplit(":", 1)[1]) >= 1


@pytest.mark.parametrize("dual", [0, 1])
def test_batched_controller_on_the_fixed_grid_is_four_separate_controllers(exe, dual):
    """the same program with dt_free = 0, the quadratic objective, warm-start shifting, B = 4, 8 cycles; with dual_warm_start the per-slot drop of the kept multipliers
    on reset and what the shift does with them equal the facades', whose reset() is mpc_reset on their own handle"""
    out = _run(exe, "fixed", str(dual))
    last = [l for l in out.splitlines() if l.startswith("compared")][0]
    assert last.startswith("compared 32 robot-cycles, 0 differ; causes seen 55 (all: 55)"), last


def _plans(start, goal, mid=None):
    """[B][stride][3] plans from starts, goals and optional in-between poses per robot"""
    B = start.shape[0]
    stride = 2 + max(len(m) for m in mid) if mid else 2
    plan = np.zeros((B, stride, 3)); n_plan = np.zeros(B, np.int32)
    for b in range(B):
        poses = [start[b]] + (list(mid[b]) if mid else []) + [goal[b]]
        plan[b, :len(poses)] = poses
        n_plan[b] = len(poses)
    return plan, n_plan


@pytest.mark.parametrize("n_candidates", [1, 2])
def test_device_variant_equals_host_variant_with_clearance_rows(env, n_candidates):
    """the reference's test-node scenario (unicycle, n = 20, minimum time, point obstacles (-3, 1), (6, 2), (4, .1), start (0, 0, 0), goal (5, 2, 0)) at B = 4 with four
    slightly different goals, 6 cycles in closed loop with a goal jump in cycle 3: mpc_controller_step_batch_device on torch tensors against mpc_controller_step_batch"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    B, n, cycles = 4, 20, 6
    kw = dict(model=A.MODEL_UNICYCLE, n=n, dt_ref=0.3, dt_free=True, objective=A.OBJ_MIN_TIME, max_obstacles=3, max_vertices=1, max_obstacle_rows=4, min_obstacle_dist=0.5)
    if n_candidates == 2:
        kw.update(candidates=(A.CAND_REFERENCE, A.CAND_HERMITE_FF), candidate_max_iter=(100, 100), candidate_param=(0.0, 2.0))
    hs, ds = m.BatchSolver(A.make_config(**kw), max_batch=B), m.BatchSolver(A.make_config(**kw), max_batch=B)
    p = hs.cycle_params(n_ref=n, adapt=1, n_min=3, n_max=n, force_reinit_num_steps=4, period=0.1)
    obst = (np.full(B, 3, np.int32), np.ones((B, 3), np.int32), np.tile(np.array([[-3.0, 1.0], [6.0, 2.0], [4.0, 0.1]])[None, :, None, :], (B, 1, 1, 1)))
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_obst = [T(a) for a in obst]
    pose = np.zeros((B, 3)); goal = np.array([[5.0, 2.0, 0.0]]) + np.arange(B)[:, None] * np.array([[0.05, -0.03, 0.02]])
    mid = [[], [(1.5, 0.4, 0.0), (3.0, 1.5, 0.0)], [], [(2.0, 1.0, 0.3)]]
    up, dtp = np.zeros((B, 2)), np.zeros(B)
    dx, du, dd = torch.zeros((B, n, 3), dtype=torch.float64, device=dev), torch.zeros((B, n, 2), dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.float64, device=dev)
    dst, dit, dri = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    kinds = set()
    for cyc in range(cycles):
        if cyc == 3:
            goal[2, 1] -= 1.2
        plan, n_plan = _plans(pose, goal, mid)
        r, ri, ng = hs.controller_step(p, plan, n_plan, u_prev=up, dt_prev=dtp, obstacles=obst)
        dp, dn, dup, ddtp = T(plan), T(n_plan), T(up), T(dtp)
        torch.cuda.synchronize()
        ds.controller_step_device(B, p, dp.data_ptr(), dn.data_ptr(), plan.shape[1], None, None, None, dup.data_ptr(), ddtp.data_ptr(), dx.data_ptr(), du.data_ptr(), dd.data_ptr(),
                                  dst.data_ptr(), dit.data_ptr(), dri.data_ptr(), obstacles=[t.data_ptr() for t in d_obst])
        ds.synchronize()
        for name, host, device in (("x", r.x, dx), ("u", r.u, du), ("dt", r.dt, dd), ("status", r.status, dst), ("iters", r.iters, dit), ("reinit", ri, dri), ("n_grid", ng, ds.grid_sizes(B))):
            device = device.cpu().numpy() if hasattr(device, "cpu") else device
            assert host.tobytes() == device.tobytes(), (cyc, name)
        kinds |= set(ri.tolist())
        print(f"cycle {cyc}: reinit {ri.tolist()} n {ng.tolist()} iters {r.iters.tolist()} status {r.status.tolist()}")
        pose, up, dtp = r.x[:, 1, :].copy(), r.u[:, 0, :].copy(), np.full(B, 0.1)
    assert 0 in kinds and any(k & GOAL_DIST for k in kinds) and any(k & PLAN_GUESS for k in kinds) and (FIRST | NUM_STEPS) in kinds
    seq, empty, last_goal = ds.controller_state(B)
    assert seq.tolist() == [cycles] * B and empty.tolist() == [0] * B and last_goal.tobytes() == goal.tobytes()
    hs.close(); ds.close()


def test_parameter_sets_give_each_instance_its_own_dt_ref(env):
    """two parameter sets with different dt_ref in one handle: the re-initialisation (time axis of the plan, dt of the guess) and the grid adaptation of every instance use its
    own dt_ref -- bit for bit what two single-set handles return"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    B, stride, n_ref, cycles = 4, 12, 8, 7
    cfgs = [A.make_config(model=A.MODEL_UNICYCLE, n=stride, dt_ref=dt_ref) for dt_ref in (0.3, 0.2)]
    set_of = np.array([0, 1, 1, 0], np.int32)
    fleet = m.BatchSolver(cfgs[0], max_batch=B)
    fleet.set_parameter_sets(cfgs, set_of)
    singles = [m.BatchSolver(c, max_batch=B) for c in cfgs]
    p = fleet.cycle_params(n_ref=n_ref, adapt=1, n_min=3, n_max=stride, period=0.1)
    pose = np.zeros((B, 3)); goal = np.array([[2.0, 0.5, 0.3], [2.0, 1.0, 0.4], [1.5, -0.5, -0.2], [2.0, 1.0, 0.4]])
    mid = [[], [(0.5, 0.2, 0.0), (1.0, 0.6, 0.0), (1.5, 0.7, 0.0)], [], [(0.5, 0.2, 0.0), (1.0, 0.6, 0.0), (1.5, 0.7, 0.0)]]
    up, dtp = np.zeros((B, 2)), np.zeros(B)
    sizes = set()
    for cyc in range(cycles):
        if cyc == 4:
            goal[:, 1] += 1.5                         # every robot re-initialises, at its own last optimised dt, over its own (n_ref - 1) dt_ref
        plan, n_plan = _plans(pose, goal, mid)
        r, ri, ng = fleet.controller_step(p, plan, n_plan, u_prev=up, dt_prev=dtp)
        for k, s in enumerate(singles):
            idx = np.nonzero(set_of == k)[0]
            rk, rik, ngk = s.controller_step(p, plan[idx], n_plan[idx], u_prev=up[idx], dt_prev=dtp[idx])
            for name, a, b in (("x", r.x[idx], rk.x), ("u", r.u[idx], rk.u), ("dt", r.dt[idx], rk.dt), ("status", r.status[idx], rk.status), ("iters", r.iters[idx], rk.iters),
                               ("reinit", ri[idx], rik), ("n_grid", ng[idx], ngk)):
                assert np.ascontiguousarray(a).tobytes() == b.tobytes(), (cyc, k, name)
        assert (ri != 0).all() == (cyc in (0, 4))
        sizes |= set(ng.tolist())
        print(f"cycle {cyc}: reinit {ri.tolist()} n {ng.tolist()} dt {r.dt.tolist()}")
        pose, up, dtp = r.x[:, 1, :].copy(), r.u[:, 0, :].copy(), np.full(B, 0.1)
    assert len(sizes) > 1                             # the adaptation moved a grid
    assert not np.array_equal(r.x[1], r.x[3])         # same plan, different dt_ref: different answers
    fleet.close()
    for s in singles:
        s.close()


def test_controller_call_errors_are_named(env):
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    s = m.BatchSolver(A.make_config(n=12), max_batch=2)
    seq, empty, goal = s.controller_state(2)          # before any controller call
    assert seq.tolist() == [0, 0] and empty.tolist() == [1, 1] and not goal.any()
    plan, n_plan = _plans(np.zeros((2, 3)), np.array([[1.0, 0.0, 0.0]] * 2))
    for kw, arg, code, text in (({"n_ref": 2}, {}, A.MPC_EINVAL, "n_ref must be in [3, cfg.n]"), ({"n_ref": 13}, {}, A.MPC_EINVAL, "n_ref must be in [3, cfg.n]"),
                                ({}, {"x_feedback": np.zeros((2, 3))}, A.MPC_EINVAL, "x_feedback and feedback_age must be given together"),
                                ({}, {"n_plan": np.array([2, 3], np.int32)}, A.MPC_EINVAL, "n_plan[1] = 3 is not in [2, plan_stride]")):
        with pytest.raises(m.MpcError) as ei:
            s.controller_step(s.cycle_params(**kw), plan, arg.pop("n_plan", n_plan), **arg)
        assert ei.value.code == code and text in str(ei.value), str(ei.value)
    big, nb = _plans(np.zeros((3, 3)), np.array([[1.0, 0.0, 0.0]] * 3))
    with pytest.raises(m.MpcError) as ei:
        s.controller_step(s.cycle_params(), big, nb)
    assert ei.value.code == A.MPC_EBATCH
    assert s.controller_state(2)[1].tolist() == [1, 1]      # a refused call changes nothing
    s.close()
