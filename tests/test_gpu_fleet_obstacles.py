"""GPU tests (-m gpu) of mpc_obstacles_from_pool* and mpc_fleet_pool* (mpc_local_planner_amd/csrc/mpc_fleet_obstacles.hpp, include/mpc_fleet.h): obstacles that are not in
the costmap, for a batch on the device.

The yardstick of the selection is the host build of the same header (tests/host_harness/fleet_obstacles_host.cpp through tests/_fleet_cases.py), which
tests/test_fleet_obstacles_host.py holds to an independent numpy restatement: the device has to equal it BIT FOR BIT in every array, on every scripted case -- pool sizes
around the wave (64), the chunk (256) and the LDS-key limit (2048), B up to 70, ties on a lattice, every free capacity.  Then: results do not depend on the batch; host and
device entry points agree; the argument checks; the pool fill against numpy; a closed loop of four robots on device pointers against the same loop through the host entry
points; and what the feature is for -- two robots driving head-on pass each other instead of through each other.

The closed-loop scenario and its thresholds come from the C oracle on the CPU (tests/tools/fleet_head_on_oracle.py; unicycle, n = 16, dt_ref 0.3, circular footprint
r = 0.2, min_obstacle_dist 0.25, dynamic obstacles, period 0.2 s, 70 cycles): minimum centre distance 0.6391 m with the other robot as an obstacle (no failed solve of 140,
final goal distances 0.083 / 0.083 m), 0.1000 m without.  The test's thresholds are 0.4 m (= 2 r, no overlap) and 0.15 m: conditions the oracle meets with a wide margin,
not figures fitted to the device."""
import ctypes as C
import math

import numpy as np
import pytest

import _fleet_cases as K

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
def solvers(env):
    """one handle per container shape (max_obstacles, max_vertices) of the scripted cases, made on demand"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    made = {}

    def get(O, V):
        if (O, V) not in made:
            made[O, V] = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=O, max_vertices=V, cutoff_dist=2.5), max_batch=128)
        return made[O, V]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def scripted():
    """(case, the host build's result) of every scripted case, computed once and left unchanged"""
    return [(c, K.host_select(c)) for c in K.cases()]


def _params(s, c):
    return s.pool_params(reach=c.reach, min_speed=c.min_speed, append=c.append)


def _device(s, torch, c):
    """mpc_obstacles_from_pool_device on torch tensors: the tuple of K.host_select"""
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
    pool = [T(a) for a in (c.pool_nv, c.pool_v, c.pool_r, c.pool_vel)]
    pose, self_index = T(c.pose), T(c.self_index)
    out = [T(a) for a in c.container()] + [T(np.full(c.B, -1, np.int32)), T(np.full(c.B, -1, np.int32))]
    torch.cuda.synchronize()
    s.obstacles_from_pool_device(c.B, (c.P, *map(ptr, pool)), ptr(pose), ptr(self_index), _params(s, c), *map(ptr, out))
    s.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solvers, scripted):
    m, torch = env
    assert {c.P for c, _ in scripted} >= {0, 1, 5, 63, 64, 65, 255, 256, 257, 1000, 2049} and max(c.B for c, _ in scripted) == 70
    for c, host in scripted:
        assert K.same(_device(solvers(c.O, c.V), torch, c), host) is None, c.name
    assert any(h[5].max() > 0 and c.P > 2048 for c, h in scripted) and any(h[5].max() > 0 and c.P <= 2048 for c, h in scripted)      # the cut with the keys in LDS and recomputed


def test_results_do_not_depend_on_the_batch(env, solvers, scripted):
    """a robot alone, in its batch, and at another position of a batch in another order"""
    m, torch = env
    for c, host in scripted:
        if c.B < 4 or c.P in (0, 1, 5):
            continue
        s = solvers(c.O, c.V)
        rows = np.arange(c.B)[::-1].copy()
        assert K.same(_device(s, torch, c.take(rows)), tuple(None if a is None else np.ascontiguousarray(a[rows]) for a in host)) is None, c.name
        for b in (0, c.B - 1):
            assert K.same(_device(s, torch, c.take(np.array([b]))), tuple(None if a is None else np.ascontiguousarray(a[b:b + 1]) for a in host)) is None, (c.name, b)


def test_host_and_device_entry_points_agree(env, solvers, scripted):
    m, torch = env
    for c, host in scripted:
        if not (c.radius and c.velocity):
            continue          # BatchSolver.obstacles_from_pool always gives the container both arrays
        s = solvers(c.O, c.V)
        pool = (c.pool_nv, c.pool_v, c.pool_r, c.pool_vel)
        got = s.obstacles_from_pool(pool, c.pose, self_index=c.self_index, params=_params(s, c), obstacles=c.container())
        assert K.same(got, host) is None, c.name


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solvers):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    s = solvers(16, 1)
    c = [c for c in K.cases() if c.name == "append"][0]
    pool = A.MpcPool(c.P, c.pool_nv.ctypes.data, c.pool_v.ctypes.data, c.pool_r.ctypes.data, c.pool_vel.ctypes.data)
    p = _params(s, c)
    before = c.container()
    no, nv, vt, rd, vl = c.container()
    dr, tk = np.full(c.B, -1, np.int32), np.full(c.B, -1, np.int32)
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    def call(B=c.B, pool=pool, pose=c.pose, p=p, no=no, nv=nv, vt=vt, rd=rd, vl=vl, fn=lib.mpc_obstacles_from_pool, h=None):
        return fn(h or s._h, B, None if pool is None else C.byref(pool), a(pose), a(c.self_index), None if p is None else C.byref(p), a(no), a(nv), a(vt), a(rd), a(vl), a(dr), a(tk))

    for fn in (lib.mpc_obstacles_from_pool, lib.mpc_obstacles_from_pool_device):          # refused before anything is read: host arrays do for both
        assert call(pool=None, fn=fn) == A.MPC_EINVAL and call(pose=None, fn=fn) == A.MPC_EINVAL and call(p=None, fn=fn) == A.MPC_EINVAL
        assert call(no=None, fn=fn) == A.MPC_EINVAL and call(nv=None, fn=fn) == A.MPC_EINVAL and call(vt=None, fn=fn) == A.MPC_EINVAL
        assert call(pool=A.MpcPool(c.P, None, c.pool_v.ctypes.data, None, None), fn=fn) == A.MPC_EINVAL and call(pool=A.MpcPool(c.P, c.pool_nv.ctypes.data, None, None, None), fn=fn) == A.MPC_EINVAL
        assert call(pool=A.MpcPool(-1, c.pool_nv.ctypes.data, c.pool_v.ctypes.data, None, None), fn=fn) == A.MPC_EINVAL
        for reach in (-0.5, math.nan, math.inf, -math.inf):
            assert call(p=s.pool_params(reach=reach), fn=fn) == A.MPC_EINVAL and b"reach" in lib.mpc_last_error()
        assert call(rd=None, fn=fn) == A.MPC_EINVAL and call(vl=None, fn=fn) == A.MPC_EINVAL and b"container has no array" in lib.mpc_last_error()
        assert call(B=129, fn=fn) == A.MPC_EBATCH
    plain = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5), max_batch=8)          # max_obstacles == 0
    assert call(h=plain._h) == A.MPC_EINVAL and b"max_obstacles = 0" in lib.mpc_last_error()
    # the pool fill
    x, dt, pn, pv = np.zeros((c.B, 5, 3)), np.full(c.B, 0.1), np.full(c.B, -5, np.int32), np.full((c.B, 1, 2), K.SENTINEL)
    for fn in (lib.mpc_fleet_pool, lib.mpc_fleet_pool_device):
        f = lambda B=c.B, pose=c.pose, x=x, dt=dt, off=0, pn=pn, pv=pv: fn(s._h, B, a(pose), a(x), a(dt), None, 0.2, None, off, a(pn), a(pv), None, None)
        assert f(pose=None) == A.MPC_EINVAL and f(pn=None) == A.MPC_EINVAL and f(pv=None) == A.MPC_EINVAL and f(dt=None) == A.MPC_EINVAL and b"x without dt" in lib.mpc_last_error()
        assert f(off=-1) == A.MPC_EINVAL and f(B=129) == A.MPC_EBATCH
    s.synchronize()
    for x_, y_ in zip(before, (no, nv, vt, rd, vl)):
        assert x_.tobytes() == y_.tobytes()
    assert (dr == -1).all() and (tk == -1).all() and (pn == -5).all() and (pv == K.SENTINEL).all()
    plain.close()
    # and the same call goes through once nothing is wrong with it
    assert call() == A.MPC_OK and K.same((no, nv, vt, rd, vl, dr, tk), K.host_select(c)) is None


def test_pool_fill_equals_numpy_bit_for_bit(env):
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    pose, x, dt, status, radius = K.pool_fill_inputs(n=5)
    B = len(pose)
    assert (status != 0).sum() >= 5 and dt[5] == 0.0
    for V, offset, with_x, with_status, per_robot in ((1, 0, True, True, True), (4, 13, True, False, False), (1, 5, False, True, True)):
        s = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=4, max_vertices=V), max_batch=B)
        P = offset + B + 3
        pool = (np.full(P, -5, np.int32), np.full((P, V, 2), K.SENTINEL), np.full(P, K.SENTINEL), np.full((P, 2), K.SENTINEL))
        ref = K.numpy_pool_fill(pose, x if with_x else None, dt, status if with_status else None, radius if per_robot else 0.3, V, offset, pool)
        d = [T(a) for a in pool]
        dx, ddt, dst, drad, dpose = T(x), T(dt), T(status), T(radius), T(pose)
        torch.cuda.synchronize()
        s.fleet_pool_device(B, ptr(dpose), ptr(dx) if with_x else None, ptr(ddt) if with_x else None, ptr(dst) if with_status else None, 0.3, *map(ptr, d), pool_offset=offset,
                            radius_per_robot=ptr(drad) if per_robot else None)
        s.synchronize()
        host = s.fleet_pool(pose, x if with_x else None, dt if with_x else None, status if with_status else None, radius if per_robot else 0.3, pool=pool, pool_offset=offset)
        for name, r, g, h in zip(("n_vertices", "vertices", "radius", "velocity"), ref, d, host):
            assert r.tobytes() == g.cpu().numpy().tobytes() == h.tobytes(), (V, offset, name)
        s.close()


# ---- four unicycles: A and B head-on, offset by 0.1 m; C and D the same routes 20 m away, out of reach of the first pair -----------------------------------------------
START = np.array([(0.0, 0.0, 0.0), (4.0, 0.1, math.pi), (0.0, 20.0, 0.0), (4.0, 20.1, math.pi)])
GOAL = np.array([(4.0, 0.0, 0.0), (0.0, 0.1, math.pi), (4.0, 20.0, 0.0), (0.0, 20.1, math.pi)])
PERIOD, RADIUS, REACH = 0.2, 0.2, 6.0


def _fleet_solver(m):
    from mpc_local_planner_amd import _abi as A
    return m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=16, dt_ref=0.3, tol=1e-6, max_iter=100, footprint_kind=1, footprint_radius=RADIUS, min_obstacle_dist=0.25,
                                       force_inclusion_dist=0.5, cutoff_dist=2.5, enable_dynamic_obstacles=True, max_obstacles=4, max_vertices=1, max_obstacle_rows=4), max_batch=4)


def _plant(pose, u):
    """the exact unicycle arc over one period"""
    out = pose.copy()
    for b, (v, w) in enumerate(u):
        x, y, th = pose[b]
        if abs(w) < 1e-12:
            out[b] = (x + v * PERIOD * math.cos(th), y + v * PERIOD * math.sin(th), th)
        else:
            out[b] = (x + v / w * (math.sin(th + w * PERIOD) - math.sin(th)), y - v / w * (math.cos(th + w * PERIOD) - math.cos(th)), th + w * PERIOD)
    return out


def _host_loop(s, cycles, with_pool=True):
    """solve -> plant -> fleet_pool -> obstacles_from_pool -> next solve through the host entry points: (poses per cycle, statuses per cycle, containers per cycle)"""
    B = len(START)
    pose, u_prev, dt_prev, init = START.copy(), np.zeros((B, 2)), np.full(B, PERIOD), None
    p = s.pool_params(reach=REACH, append=0)
    ob = (np.zeros(B, np.int32), np.zeros((B, 4), np.int32), np.zeros((B, 4, 1, 2)), np.zeros((B, 4)), np.zeros((B, 4, 2)))
    poses, statuses, containers = [pose.copy()], [], []
    for _ in range(cycles):
        r = s.solve(pose, GOAL, u_prev, dt_prev, init, obstacles=ob)
        ok = r.status == 0
        u0 = np.where(ok[:, None], r.u[:, 0], 0.0)          # a failed solve: zero command and a cold start next cycle
        pose, u_prev = _plant(pose, u0), u0
        init = (r.x, r.u, r.dt) if ok.all() else None
        if with_pool:
            pool = s.fleet_pool(pose, r.x, r.dt, r.status, RADIUS)
            ob = s.obstacles_from_pool(pool, pose, self_index=np.arange(B), params=p)[:5]
        poses.append(pose.copy()); statuses.append(r.status.copy()); containers.append(tuple(a.copy() for a in ob))
    return np.array(poses), np.array(statuses), containers


def _device_loop(s, torch, cycles):
    """the same loop with the three calls on device pointers; the plant (the test's simulator) runs on the host from the first controls"""
    dev = torch.device("cuda", 0)
    B, n = len(START), 16
    Z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
    d_pose, d_goal, d_up, d_dtp = Z(B, 3), torch.from_numpy(GOAL).to(dev), Z(B, 2), Z(B)
    bufs = [(Z(B, n, 3), Z(B, n, 2), Z(B)) for _ in range(2)]
    d_st, d_it = Z(B, dtype=torch.int32), Z(B, dtype=torch.int32)
    d_ob = (Z(B, dtype=torch.int32), Z(B, 4, dtype=torch.int32), Z(B, 4, 1, 2), Z(B, 4), Z(B, 4, 2))
    d_pool = (Z(B, dtype=torch.int32), Z(B, 1, 2), Z(B), Z(B, 2))
    d_self = torch.arange(B, dtype=torch.int32, device=dev)
    p = s.pool_params(reach=REACH, append=0)
    pose, u_prev, warm = START.copy(), np.zeros((B, 2)), False
    d_dtp.fill_(PERIOD)
    poses, statuses, containers = [pose.copy()], [], []
    for k in range(cycles):
        out, prev = bufs[k % 2], bufs[(k + 1) % 2]
        d_pose.copy_(torch.from_numpy(pose)); d_up.copy_(torch.from_numpy(u_prev))
        torch.cuda.synchronize()
        s.solve_device(B, d_pose.data_ptr(), d_goal.data_ptr(), d_up.data_ptr(), d_dtp.data_ptr(), *(t.data_ptr() if warm else None for t in prev), *(t.data_ptr() for t in out),
                       d_st.data_ptr(), d_it.data_ptr(), obstacles=tuple(t.data_ptr() for t in d_ob))
        s.synchronize()
        status, u = d_st.cpu().numpy(), out[1].cpu().numpy()
        ok = status == 0
        u0 = np.where(ok[:, None], u[:, 0], 0.0)
        pose, u_prev, warm = _plant(pose, u0), u0, bool(ok.all())
        d_pose.copy_(torch.from_numpy(pose))
        torch.cuda.synchronize()
        s.fleet_pool_device(B, d_pose.data_ptr(), out[0].data_ptr(), out[2].data_ptr(), d_st.data_ptr(), RADIUS, *(t.data_ptr() for t in d_pool))
        s.obstacles_from_pool_device(B, (B, *(t.data_ptr() for t in d_pool)), d_pose.data_ptr(), d_self.data_ptr(), p, *(t.data_ptr() for t in d_ob))
        s.synchronize()
        poses.append(pose.copy()); statuses.append(status.copy()); containers.append(tuple(t.cpu().numpy() for t in d_ob))
    return np.array(poses), np.array(statuses), containers


def test_eight_cycles_on_device_pointers_equal_the_host_entry_points(env):
    m, torch = env
    s = _fleet_solver(m)
    hp, hs, hc = _host_loop(s, 8)
    s.reset()
    dp, ds, dc = _device_loop(s, torch, 8)
    s.close()
    assert hs.tobytes() == ds.tobytes() and hp.tobytes() == dp.tobytes()
    for k, (a, b) in enumerate(zip(hc, dc)):
        n = a[0]
        assert n.tolist() == b[0].tolist() == [1, 1, 1, 1], k          # each robot sees its partner; the other pair is 20 m away, beyond the reach of 6 m
        for x, y in zip(a[1:], b[1:]):
            assert x[:, :1].tobytes() == np.ascontiguousarray(y[:, :1]).tobytes(), k          # (the slots behind n_obstacles are nobody's: the host loop starts each cycle from zeros)
    assert np.abs(hc[-1][4][:, 0]).max() > 0.1          # the partners' velocities arrived


def test_two_robots_head_on_pass_each_other_over_70_cycles(env):
    """with the pool the centres of A and B never come closer than 0.4 m (2 r: no overlap); with empty containers they do; both reach their goals within 0.15 m"""
    m, torch = env
    s = _fleet_solver(m)
    poses, status, _ = _host_loop(s, 70)
    s.reset()
    blind, _, _ = _host_loop(s, 70, with_pool=False)
    s.close()
    dist = lambda p: np.hypot(p[:, 0, 0] - p[:, 1, 0], p[:, 0, 1] - p[:, 1, 1]).min()
    goal = np.hypot(poses[-1, :2, 0] - GOAL[:2, 0], poses[-1, :2, 1] - GOAL[:2, 1])
    print(f"minimum centre distance {dist(poses):.4f} m with the pool, {dist(blind):.4f} m without; goal distances {goal[0]:.3f} / {goal[1]:.3f} m; "
          f"{int((status[:, :2] != 0).sum())} failed solves of {status[:, :2].size}")
    assert dist(poses) >= 0.4
    assert dist(blind) < 0.4
    assert (goal <= 0.15).all()
