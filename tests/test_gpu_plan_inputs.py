"""GPU tests (-m gpu) of mpc_plan_inputs_batch* and mpc_commands_batch* (mpc_local_planner_amd/csrc/mpc_plan_inputs.hpp): what the reference's plugin runs around
Controller::step, for a batch on the device.

The yardstick is the host build of the same header (tests/host_harness/plan_inputs_host.cpp through tests/_plan_inputs_cases.py), which tests/test_plan_inputs_host.py holds
to the facade: the device has to equal it BIT FOR BIT in every output.  The plans aim at where the lane-parallel scans can go wrong -- lengths 1, 2, 63, 64, 65, 128, 129, the
pruned front, the nearest pose, the break of the nearest scan and the last selected pose in lanes 0, 63 and 64, a begin off the chunk grid, a plan that ends inside a chunk,
every scripted plan of the CPU test -- not at the workload.  Then: results do not depend on the batch; host and device entry points agree; the commands against a numpy
restatement of src/mpc_local_planner_ros.cpp:394-452; a closed loop of six robots whose plan inputs, step, feasibility check and commands stay on device pointers against
the same loop through the host harness and the host entry points; argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import _plan_inputs_cases as K
from test_plan_inputs_host import _commands_numpy, commands_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as pkg
    return pkg, torch


@pytest.fixture(scope="module")
def solver(env):
    """unicycle, minimum time with via-points (cfg.max_via_points = K.MAX_VIA), room for the largest scripted batch"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    s = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=12, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=K.MAX_VIA), max_batch=128)
    yield s
    s.close()


@pytest.fixture(scope="module")
def host_results():
    """the host build's outputs of every scripted group, computed once and left unchanged"""
    K.harness()
    return {g.name: K.host_batch(g.p, *g.arrays(), g.plan_stride) for g in K.groups()}


def _device(s, torch, p, g, ng, robot, begin, plan_stride, max_via=K.MAX_VIA, with_begin=True):
    """mpc_plan_inputs_batch_device on torch tensors: the tuple of K.host_batch"""
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B = len(ng)
    plan, n_plan, n_via, via, gi, fl = (T(a) for a in K.blank_outputs(B, plan_stride, max_via))
    dg, dn, dr, db = T(g), T(ng), T(robot), T(begin)
    torch.cuda.synchronize()
    s.plan_inputs_device(B, p, dg.data_ptr(), dn.data_ptr(), g.shape[1], dr.data_ptr(), db.data_ptr() if with_begin else None, plan.data_ptr(), n_plan.data_ptr(), plan_stride,
                         n_via.data_ptr(), via.data_ptr(), gi.data_ptr(), fl.data_ptr())
    s.synchronize()
    return tuple(t.cpu().numpy() for t in (db, plan, n_plan, n_via, via, gi, fl))


NAMES = ("plan_begin", "plan", "n_plan", "n_via", "via", "goal_idx", "flags")


def _assert_same(a, b, what, rows=None):
    for name, x, y in zip(NAMES, a, b):
        x = x if rows is None else x[rows]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, name)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_group(env, solver, host_results):
    m, torch = env
    groups = K.groups()
    assert len(groups[0].inst) >= 36 and {len(q[1]) for q in groups[0].inst} >= {1, 2, 63, 64, 65, 128, 129}
    for g in groups:
        out = _device(solver, torch, g.p, *g.arrays(), g.plan_stride)
        _assert_same(host_results[g.name], out, g.name)
    flags = np.concatenate([host_results[g.name][6] for g in groups])
    assert all((flags & bit).any() for bit in (1, 4, 8, 16))          # reached, truncated, dropped, injected all occur (the empty plan: next test)


def test_empty_plans_and_a_null_begin_on_the_device(env, solver):
    m, torch = env
    p = K.params()
    g = np.ascontiguousarray(np.tile(K.line(70, 0.05)[None], (4, 1, 1)))
    ng, begin = np.array([0, 70, 70, -3], np.int32), np.array([0, 70, 12, 0], np.int32)
    robot = np.tile(np.array([[1.0, 0.1, 0.2]]), (4, 1))
    host = K.host_batch(p, g, ng, robot, begin, 40)
    assert host[6].tolist() == [2, 2, 0, 2]
    _assert_same(host, _device(solver, torch, p, g, ng, robot, begin, 40), "empty plans next to a full one")
    zero = np.zeros(4, np.int32)
    out = _device(solver, torch, p, g, ng, robot, begin, 40, with_begin=False)          # no persistent front: counts as 0, nothing written back
    _assert_same(K.host_batch(p, g, ng, robot, zero, 40)[1:], out[1:], "begin NULL")
    assert out[0].tolist() == begin.tolist()


def test_results_do_not_depend_on_the_batch(env, solver, host_results):
    """the main group alone (B = 1 each, a sample), in the batch, and in reversed order"""
    m, torch = env
    g = K.groups()[0]
    B = len(g.inst)
    rev = list(range(B))[::-1]
    out = _device(solver, torch, g.p, *g.arrays(rev), g.plan_stride)
    _assert_same(host_results["main"], out, "reversed order", rows=rev)
    for b in range(0, B, 3):
        arr = g.arrays([b])
        wide = np.full((1, g.arrays()[0].shape[1], 3), 777.0)          # the same gstride as in the batch
        wide[0, :arr[0].shape[1]] = arr[0][0]
        one = _device(solver, torch, g.p, wide, arr[1], arr[2], arr[3], g.plan_stride)
        _assert_same(host_results["main"], one, f"alone: {g.inst[b][0]}", rows=[b])


def test_host_and_device_entry_points_agree(env, solver, host_results):
    m, torch = env
    g = K.groups()[0]
    gl, ng, robot, begin = g.arrays()
    r = solver.plan_inputs(g.p, gl, ng, robot, g.plan_stride, plan_begin=begin, via_points=True)
    h = host_results["main"]
    n = h[2]
    assert r.plan_begin.tobytes() == h[0].tobytes() and r.n_plan.tobytes() == n.tobytes() and r.n_via.tobytes() == h[3].tobytes()
    assert r.goal_idx.tobytes() == h[5].tobytes() and r.flags.tobytes() == h[6].tobytes()
    for b in range(len(ng)):          # the wrapper starts from zeroed arrays, the harness from its own filler: compare what the call writes
        assert r.plan[b, :n[b]].tobytes() == h[1][b, :n[b]].tobytes() and not r.plan[b, n[b]:].any(), b
        assert r.via[b, :h[3][b]].tobytes() == h[4][b, :h[3][b]].tobytes(), b
    # the commands pair, on every combination
    u, st, fe, fl = commands_cases()
    full = np.zeros((len(st), solver.n, 2)); full[:, :2] = u
    cnt0 = (np.arange(len(st), dtype=np.int32) % 3)
    hc = solver.commands(full, st, fe, fl, infeasible_count=cnt0)
    dc = _device_commands(solver, torch, full, st, fe, fl, cnt0)
    for name, a, b in zip(("cmd", "result", "reset_next", "u_prev_next", "infeasible_count"), (hc.cmd, hc.result, hc.reset_next, hc.u_prev_next, hc.infeasible_count), dc):
        assert a.tobytes() == b.tobytes(), name


def _device_commands(s, torch, u, st, fe, fl, cnt, calls=1):
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B = len(st)
    du, dst, dfe, dfl, dcnt = T(u), T(st), T(fe), T(fl), T(cnt)
    cmd, up = torch.full((B, 3), -7.0, dtype=torch.float64, device=dev), torch.full((B, 2), -7.0, dtype=torch.float64, device=dev)
    res, rs = torch.full((B,), -1, dtype=torch.int32, device=dev), torch.full((B,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    for _ in range(calls):
        s.commands_device(B, du.data_ptr(), dst.data_ptr(), ptr(dfe), ptr(dfl), cmd.data_ptr(), res.data_ptr(), rs.data_ptr(), up.data_ptr(), ptr(dcnt))
    s.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (cmd, res, rs, up, dcnt))


def test_commands_equal_the_restatement_on_every_combination(env, solver):
    """status converged or not x feasible or not x each plan flag x a control that is not finite, B = 126 (two blocks of the one-lane-per-instance kernel, the second
    partly filled); infeasible_count over three calls"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    u, st, fe, fl = commands_cases()
    B = len(st)
    assert 64 < B <= 128
    s = m.BatchSolver(A.make_config(n=5), max_batch=B)
    full = np.zeros((B, 5, 2)); full[:, :2] = u
    cnt0 = (np.arange(B, dtype=np.int32) % 3)
    expect = [_commands_numpy(tuple(u[b, 0]), int(st[b]), int(fe[b]), int(fl[b]), int(cnt0[b])) for b in range(B)]
    cmd, res, rs, up, cnt = _device_commands(s, torch, full, st, fe, fl, cnt0)
    for b in range(B):
        assert (tuple(cmd[b]), int(res[b]), int(rs[b]), tuple(up[b]), int(cnt[b])) == expect[b], b
    cnt3 = _device_commands(s, torch, full, st, fe, fl, cnt0, calls=3)[4]
    for b in range(B):
        c = int(cnt0[b])
        for _ in range(3):
            c = _commands_numpy(tuple(u[b, 0]), int(st[b]), int(fe[b]), int(fl[b]), c)[4]
        assert int(cnt3[b]) == c, b
    # feasible, flags and the optional outputs NULL
    cmd, res, rs, up, cnt = _device_commands(s, torch, full, st, None, None, None)
    assert all(int(res[b]) == _commands_numpy(tuple(u[b, 0]), int(st[b]), 1, 0, 0)[1] for b in range(B))
    s.close()


# ---- composition: eight cycles of six robots

B6, N6, STRIDE6, CYCLES, PERIOD = 6, 16, 24, 8, 0.5
SIZE, RES = 60, 0.1                       # a 6 m costmap centred on the robot: the selection's radius is 2.55 m
SPEC = np.array([[0.1, 0.1], [-0.1, 0.1], [-0.1, -0.1], [0.1, -0.1]])
BAD_ROBOT, BAD_CYCLE = 4, 3


def _fleet():
    """global plans [6][gstride][3]: two short ones whose goal is reached within the eight cycles, four long ones (straight, an arc, straight, a diagonal)"""
    plans = [K.line(7, 0.1), K.line(9, 0.1, x0=1.0), K.line(120, 0.1)]
    s = 0.1 * np.arange(150)
    plans.append(np.column_stack([8.0 * np.sin(s / 8.0), 8.0 * (1.0 - np.cos(s / 8.0)), s / 8.0]))
    plans.append(K.line(100, 0.1, x0=-2.0))
    plans.append(np.column_stack([0.07 * np.arange(130), 0.07 * np.arange(130), np.full(130, math.pi / 4.0)]))
    gstride = max(len(q) for q in plans)
    g = np.zeros((B6, gstride, 3))
    for b, q in enumerate(plans):
        g[b, :len(q)] = q
    start = np.array([q[0] for q in plans]) + np.array([[0.0, 0.02, 0.0], [0.05, 0.0, 0.0], [0.0, 0.0, 0.1], [0.0, -0.03, 0.0], [0.0, 0.0, 0.0], [0.0, 0.05, math.pi / 4.0]])
    return np.ascontiguousarray(g), np.array([len(q) for q in plans], np.int32), start


def _costmaps(pose, cyc):
    cost = np.zeros((B6, SIZE, SIZE), np.uint8)
    if cyc == BAD_CYCLE:
        cost[BAD_ROBOT, 20:41, 34] = 254          # a lethal wall 0.4 m ahead of the robot, across its straight plan, for this one cycle
    return cost, np.ascontiguousarray(pose[:, :2] - 0.5 * SIZE * RES)


def _plant(pose, cmd):
    """the one-line unicycle"""
    return pose + PERIOD * np.column_stack([cmd[:, 0] * np.cos(pose[:, 2]), cmd[:, 0] * np.sin(pose[:, 2]), cmd[:, 2]])


def test_closed_loop_on_device_pointers_equals_the_loop_through_the_host(env):
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    cfg = lambda: A.make_config(model=A.MODEL_UNICYCLE, n=N6, dt_ref=0.3, dt_free=True, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=K.MAX_VIA)
    ds, hs = m.BatchSolver(cfg(), max_batch=B6), m.BatchSolver(cfg(), max_batch=B6)
    cp = ds.cycle_params(n_ref=N6, adapt=1, n_min=3, n_max=N6, period=PERIOD)
    pp = K.params(global_plan_viapoint_sep=0.5, costmap_size_x=SIZE, costmap_size_y=SIZE, resolution=RES, yaw_goal_tolerance=0.3)
    g, ng, start = _fleet()
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    f64, i32 = torch.float64, torch.int32
    # device loop state: everything between the plan and the command lives here and is never copied to the host inside the loop
    d_g, d_ng, d_begin = T(g), T(ng), Z((B6,), i32)
    d_plan, d_nplan, d_nvia, d_via, d_flags = Z((B6, STRIDE6, 3), f64), Z((B6,), i32), Z((B6,), i32), Z((B6, K.MAX_VIA, 3), f64), Z((B6,), i32)
    d_x, d_u, d_dt, d_st, d_it, d_ri = Z((B6, N6, 3), f64), Z((B6, N6, 2), f64), Z((B6,), f64), Z((B6,), i32), Z((B6,), i32), Z((B6,), i32)
    d_feas, d_cmd, d_res, d_reset, d_uprev, d_cnt = Z((B6,), i32), Z((B6, 3), f64), Z((B6,), i32), Z((B6,), i32), Z((B6, 2), f64), Z((B6,), i32)
    torch.cuda.synchronize()
    assert ds._lib.mpc_set_via_points_device(ds._h, C.c_void_p(d_nvia.data_ptr()), C.c_void_p(d_via.data_ptr())) == 0
    # baseline state
    h_begin, h_via, h_nvia = np.zeros(B6, np.int32), np.zeros((B6, K.MAX_VIA, 3)), np.zeros(B6, np.int32)
    h_reset, h_uprev, h_cnt = np.zeros(B6, np.int32), np.zeros((B6, 2)), np.zeros(B6, np.int32)
    pose_d, pose_h = start.copy(), start.copy()
    spec = np.ascontiguousarray(SPEC)
    results, reinits = [], []
    for cyc in range(CYCLES):
        dtp = np.full(B6, 0.0 if cyc == 0 else PERIOD)
        # -- device: plan inputs -> step -> feasibility -> commands, all enqueued on the handle's stream
        cost, origin = _costmaps(pose_d, cyc)
        d_pose, d_cost, d_org, d_dtp = T(pose_d), T(cost), T(origin), T(dtp)
        torch.cuda.synchronize()
        ds.plan_inputs_device(B6, pp, d_g.data_ptr(), d_ng.data_ptr(), g.shape[1], d_pose.data_ptr(), d_begin.data_ptr(), d_plan.data_ptr(), d_nplan.data_ptr(), STRIDE6,
                              d_nvia.data_ptr(), d_via.data_ptr(), None, d_flags.data_ptr())
        ds.controller_step_device(B6, cp, d_plan.data_ptr(), d_nplan.data_ptr(), STRIDE6, None, None, d_reset.data_ptr(), d_uprev.data_ptr(), d_dtp.data_ptr(), d_x.data_ptr(),
                                  d_u.data_ptr(), d_dt.data_ptr(), d_st.data_ptr(), d_it.data_ptr(), d_ri.data_ptr())
        rc = ds._lib.mpc_check_feasibility_device(ds._h, B6, C.c_void_p(d_x.data_ptr()), C.c_void_p(d_cost.data_ptr()), SIZE, SIZE, RES, C.c_void_p(d_org.data_ptr()),
                                                  C.c_void_p(spec.ctypes.data), len(spec), 0.1, 0.3, -1, C.c_void_p(d_feas.data_ptr()))
        assert rc == 0, ds._lib.mpc_last_error()
        ds.commands_device(B6, d_u.data_ptr(), d_st.data_ptr(), d_feas.data_ptr(), d_flags.data_ptr(), d_cmd.data_ptr(), d_res.data_ptr(), d_reset.data_ptr(), d_uprev.data_ptr(),
                           d_cnt.data_ptr())
        ds.synchronize()
        cmd_d, res_d, ri_d = d_cmd.cpu().numpy(), d_res.cpu().numpy(), d_ri.cpu().numpy()
        # -- baseline: the host harness for plan inputs and commands, the existing host entry points for the step and the feasibility check
        cost_h, origin_h = _costmaps(pose_h, cyc)
        plan, n_plan, _, _, _, flags = K.blank_outputs(B6, STRIDE6)
        plan[:] = 0.0
        K.harness().pin_batch(B6, C.byref(pp), K.d_(g), K.i_(ng), g.shape[1], K.d_(pose_h), K.i_(h_begin), K.d_(plan), K.i_(n_plan), STRIDE6, K.MAX_VIA, K.i_(h_nvia), K.d_(h_via),
                              None, K.i_(flags))
        hs.set_via_points(h_nvia, h_via)
        r, ri_h, _ = hs.controller_step(cp, plan, n_plan, reset=h_reset, u_prev=h_uprev, dt_prev=dtp)
        feas = hs.check_feasibility(r.x, cost_h, RES, origin_h, spec, 0.1, 0.3, -1)
        cmd_h, res_h = np.zeros((B6, 3)), np.zeros(B6, np.int32)
        K.harness().pin_commands(B6, K.d_(r.u), N6, K.i_(r.status), K.i_(feas), K.i_(flags), K.d_(cmd_h), K.i_(res_h), K.i_(h_reset), K.d_(h_uprev), K.i_(h_cnt))
        print(f"cycle {cyc}: result {res_d.tolist()} reinit {ri_d.tolist()} status {r.status.tolist()} feasible {feas.tolist()} flags {flags.tolist()} n_plan {n_plan.tolist()} "
              f"n_via {h_nvia.tolist()} front {h_begin.tolist()}")
        assert cmd_d.tobytes() == cmd_h.tobytes() and res_d.tobytes() == res_h.tobytes(), cyc
        assert ri_d.tobytes() == ri_h.tobytes(), cyc
        results.append(res_d.copy()); reinits.append(ri_d.copy())
        pose_d, pose_h = _plant(pose_d, cmd_d), _plant(pose_h, cmd_h)
    # what stayed on the device all along equals the baseline's state at the end
    for name, d, h in (("plan_begin", d_begin, h_begin), ("reset_next", d_reset, h_reset), ("u_prev_next", d_uprev, h_uprev), ("infeasible_count", d_cnt, h_cnt), ("n_via", d_nvia, h_nvia)):
        assert d.cpu().numpy().tobytes() == h.tobytes(), name
    results, reinits = np.array(results), np.array(reinits)
    assert (results[-1, :2] == A.CMD_GOAL_REACHED).all() and (results[0] != A.CMD_GOAL_REACHED).all()          # two robots reach their goal
    assert (results == A.CMD_SUCCESS).sum() >= 30
    assert (results[:, 2:] != A.CMD_GOAL_REACHED).all()
    bad = np.argwhere(results == A.CMD_INFEASIBLE)
    assert bad.tolist() == [[BAD_CYCLE, BAD_ROBOT]]                                                            # the feasibility check fails once
    failed = np.isin(results, (A.CMD_SOLVE_FAILED, A.CMD_INFEASIBLE, A.CMD_NOT_FINITE))
    reset_seen = (reinits & A.REINIT_RESET) != 0
    assert not reset_seen[0].any() and np.array_equal(reset_seen[1:], failed[:-1])                             # MPC_REINIT_RESET exactly in the cycle after a failure
    assert reset_seen[BAD_CYCLE + 1, BAD_ROBOT] and reset_seen.sum() == 1
    assert (d_begin.cpu().numpy()[2:5] > 0).all()                                                               # the long plans have been pruned behind the robots
    ds.close(); hs.close()


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solver):
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    lib, h = solver._lib, solver._h
    p = K.params()
    g, ng, robot = np.ascontiguousarray(K.line(8, 0.1)[None]), np.array([8], np.int32), np.zeros((1, 3))
    begin = np.zeros(1, np.int32)
    plan, n_plan, n_via, via, gi, fl = K.blank_outputs(1, 8)
    before = [a.copy() for a in (begin, plan, n_plan, n_via, via, gi, fl)]
    v = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(fn, B=1, pp=p, g_=g, ng_=ng, gstride=8, robot_=robot, plan_=plan, n_plan_=n_plan, stride=8, n_via_=n_via, via_=via, handle=h):
        return fn(handle, B, C.byref(pp) if pp is not None else None, v(g_), v(ng_), gstride, v(robot_), v(begin), v(plan_), v(n_plan_), stride, v(n_via_), v(via_), v(gi), v(fl))

    for fn in (lib.mpc_plan_inputs_batch, lib.mpc_plan_inputs_batch_device):          # (every refusal comes before a pointer is touched: host arrays do for both)
        for kw in (dict(pp=None), dict(g_=None), dict(ng_=None), dict(robot_=None), dict(plan_=None), dict(n_plan_=None)):
            assert call(fn, **kw) == A.MPC_EINVAL and b"null argument" in lib.mpc_last_error(), kw
        assert call(fn, gstride=1) == A.MPC_EINVAL and b"at least 2" in lib.mpc_last_error()
        assert call(fn, stride=1) == A.MPC_EINVAL and b"at least 2" in lib.mpc_last_error()
        assert call(fn, n_via_=None) == A.MPC_EINVAL and b"go together" in lib.mpc_last_error()
        assert call(fn, via_=None) == A.MPC_EINVAL and b"go together" in lib.mpc_last_error()
        assert call(fn, B=129) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
    plain = m.BatchSolver(A.make_config(n=12), max_batch=2)          # max_via_points == 0
    for fn in (lib.mpc_plan_inputs_batch, lib.mpc_plan_inputs_batch_device):
        assert call(fn, handle=plain._h) == A.MPC_EINVAL and b"max_via_points == 0" in lib.mpc_last_error()
    assert call(lib.mpc_plan_inputs_batch, handle=plain._h, n_via_=None, via_=None) == A.MPC_OK          # ... and without them the call is fine
    assert n_plan[0] == 8 and n_via[0] == -1
    n_plan[0] = -1; plan[:] = before[1]; gi[:] = before[5]; fl[:] = before[6]
    u, st = np.zeros((1, 12, 2)), np.zeros(1, np.int32)
    cmd, res = np.full((1, 3), -7.0), np.full(1, -1, np.int32)
    for fn in (lib.mpc_commands_batch, lib.mpc_commands_batch_device):
        for args in ((None, v(st), None, None, v(cmd), v(res)), (v(u), None, None, None, v(cmd), v(res)), (v(u), v(st), None, None, None, v(res)), (v(u), v(st), None, None, v(cmd), None)):
            assert fn(plain._h, 1, *args, None, None, None) == A.MPC_EINVAL and b"null argument" in lib.mpc_last_error()
        assert fn(plain._h, 3, v(u), v(st), None, None, v(cmd), v(res), None, None, None) == A.MPC_EBATCH
    assert cmd.tolist() == [[-7.0] * 3] and res.tolist() == [-1]
    for a, b in zip((begin, plan, n_plan, n_via, via, gi, fl), before):
        assert a.tobytes() == b.tobytes()
    plain.close()
