"""GPU tests (-m gpu) of mpc_costmap_window* (mpc_local_planner_amd/csrc/mpc_costmap_window.hpp, include/mpc_costmap_window.h): the local costmap window of every robot
of a batch cut from one shared map on the device.

The yardstick is the host build of the same header (tests/host_harness/costmap_window_host.cpp through tests/_window_cases.py), which tests/test_costmap_window_host.py
holds to an independent Python restatement: the device has to equal it BIT FOR BIT in cost, origin and info on every scripted case and on the random maps, over outputs
pre-filled with a poison pattern.  Then: info may be NULL; the host-pointer entry equals the device entry; an instance of a batch of 8 equals the same instance alone;
every refusal leaves the outputs untouched; the step is timed; an inflated window makes the feasibility check's inscribed branch fire; and the window feeds a closed
cycle on device pointers whose every output equals the cycle on windows built by the host build and uploaded."""
import ctypes as C
import math

import numpy as np
import pytest

import _window_cases as Wn

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
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    s = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5), max_batch=8)
    yield s
    s.close()


@pytest.fixture(scope="module")
def scripted():
    """(case, the host build's result) of every scripted case, computed once and left unchanged"""
    return [(c, Wn.host_window(c)) for c in Wn.cases()]


def _device(s, torch, c, with_info=True):
    """mpc_costmap_window_device on torch tensors over poisoned outputs: (cost, origin, info); info None when it is passed as NULL"""
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dmap, dpose = T(c.map), T(c.pose)
    cost, origin, info = (T(a) for a in c.outputs())
    torch.cuda.synchronize()
    s.costmap_window_device(c.B, dmap.data_ptr(), c.struct(), dpose.data_ptr(), c.W, c.H, c.res, cost.data_ptr(), origin.data_ptr(), info.data_ptr() if with_info else None)
    s.synchronize()
    return cost.cpu().numpy(), origin.cpu().numpy(), info.cpu().numpy() if with_info else None


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solver, scripted):
    """cost, origin and info over a poison pattern: what equals the host build was written in full; then the same with info NULL"""
    m, torch = env
    assert len(scripted) >= 20 and max(c.B for c, _ in scripted) <= 8
    for c, host in scripted:
        got = _device(solver, torch, c)
        assert Wn.same(got, host) is None, (c.name, Wn.same(got, host))
        assert solver.last_costmap_ms() > 0.0
        bare = _device(solver, torch, c, with_info=False)
        assert Wn.same(bare[:2], host[:2]) is None and bare[2] is None, c.name
    # the host build leaves no poison either: every cell, origin and count is a value of the rule
    assert all((h[1] != Wn.DPOISON).all() and (h[2] != Wn.IPOISON).all() for _, h in scripted)


def test_random_maps_equal_the_host_build(env, solver):
    m, torch = env
    changed = 0
    for c in Wn.random_cases():
        got, host = _device(solver, torch, c), Wn.host_window(c)
        assert Wn.same(got, host) is None, (c.name, Wn.same(got, host))
        changed += int(host[2][:, 2].clip(0).sum())
    assert changed > 2000


def test_host_pointer_entry_equals_the_device_entry(env, solver, scripted):
    m, torch = env
    for c, host in scripted:
        got = solver.costmap_window(c.map, c.struct(), c.pose, (c.W, c.H), c.res)
        assert Wn.same(got, host) is None, (c.name, Wn.same(got, host))


def test_an_instance_of_a_batch_of_eight_equals_the_same_instance_alone(env, solver, scripted):
    m, torch = env
    by = {c.name: c for c, _ in scripted}
    rng = np.random.default_rng(4)
    for name in ("55 x 55, inflated", "three tiles wide, 2 : 1, r 5", "17 x 16, r 32"):
        c = by[name].with_poses(np.column_stack([rng.uniform(-0.5, 3.5, 8), rng.uniform(-0.5, 2.7, 8), np.zeros(8)]))
        among = _device(solver, torch, c)
        for b in range(8):
            alone = _device(solver, torch, c.take(b))
            assert Wn.same(tuple(np.ascontiguousarray(a[b:b + 1]) for a in among), alone) is None, (name, b)


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solver, scripted):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    c = [c for c, _ in scripted if c.name == "7 x 5, 2 : 1, r 1"][0]
    cost, origin, info = c.outputs()
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)

    def prm(**kw):
        q = c.struct()
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    def call(fn, h=None, B=c.B, map_=c.map, p=c.struct(), pose=c.pose, W=c.W, H=c.H, res=c.res, cost=cost, origin=origin):
        return fn(h or solver._h, B, a(map_), None if p is None else C.byref(p), a(pose), W, H, res, a(cost), a(origin), a(info))

    for fn in (lib.mpc_costmap_window, lib.mpc_costmap_window_device):          # refused before anything is read: host arrays do for both
        for bad in (dict(map_=None), dict(p=None), dict(pose=None), dict(cost=None), dict(origin=None)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"null argument" in lib.mpc_last_error(), bad
        for bad in (dict(W=0), dict(H=0), dict(W=4097, H=1), dict(W=1, H=4097), dict(W=2048, H=1024)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"window geometry" in lib.mpc_last_error(), bad
        for bad in (dict(res=0.0), dict(res=-0.1), dict(res=math.nan), dict(res=math.inf), dict(p=prm(map_resolution=0.0)), dict(p=prm(map_resolution=math.inf))):
            assert call(fn, **bad) == A.MPC_EINVAL and b"positive and finite" in lib.mpc_last_error(), bad
        for bad in (dict(map_size_x=0), dict(map_size_y=-1), dict(map_size_x=65536, map_size_y=32768)):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and b"map size" in lib.mpc_last_error(), bad
        for bad, word in ((dict(inflation_radius=3.25), b"inflation_radius"), (dict(inflation_radius=math.nan), b"inflation_radius"), (dict(inflation_radius=math.inf), b"inflation_radius"),
                          (dict(outside_value=1), b"outside_value"), (dict(outside_value=254), b"outside_value"), (dict(inscribed_radius=-0.1), b"inscribed_radius"),
                          (dict(inscribed_radius=math.nan), b"inscribed_radius"), (dict(cost_scaling_factor=-1.0), b"cost_scaling_factor"),
                          (dict(cost_scaling_factor=math.inf), b"cost_scaling_factor")):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and word in lib.mpc_last_error(), bad
        assert call(fn, B=9) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
    # a refused call changes nothing
    for x, y in zip(c.outputs(), (cost, origin, info)):
        assert x.tobytes() == y.tobytes()
    assert call(lib.mpc_costmap_window, B=0) == A.MPC_OK and (cost == Wn.POISON).all()
    # 3.15 m at 0.1 m is 32 cells: the largest radius that is taken
    assert call(lib.mpc_costmap_window, p=prm(inflation_radius=3.15)) == A.MPC_OK and (cost != Wn.POISON).any() and info[0, 0] == 35


def test_inflation_makes_the_feasibility_check_see_the_inscribed_cells(env):
    """A wall along column 40 of a map at 0.05 m per cell; a robot_radius 0.17 footprint without footprint points drives straight along the wall, 3 cells from it
    (0.15 m <= 0.17 m: the inflated cells under it are 253) and 5 cells from it (int(252 exp(-0.8)) = 113).  mpc_check_feasibility_device reads 253 as a hit for such a
    footprint: the near trajectory is feasible on the uninflated window, infeasible on the inflated one; the far one is feasible on both."""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    n, size, res = 12, 60, 0.05
    s = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=n), max_batch=2)
    grid = np.zeros((100, 100), np.uint8)
    grid[:, 40] = 254
    xs = (np.array([37, 35]) + 0.5) * res                                   # the centres of the columns 3 and 5 cells from the wall
    x = np.zeros((2, n, 3))
    x[:, :, 0], x[:, :, 1], x[:, :, 2] = xs[:, None], np.linspace(2.0, 3.0, n)[None, :], math.pi / 2
    pose = np.ascontiguousarray(x[:, n // 2])
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dmap, dpose, dx = T(grid), T(pose), T(x)
    cost, origin = torch.zeros((2, size, size), dtype=torch.uint8, device=dev), torch.zeros((2, 2), dtype=torch.float64, device=dev)
    info, feas = torch.zeros((2, 4), dtype=torch.int32, device=dev), torch.full((2,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    seen = {}
    for name, inflation in (("plain", 0.0), ("inflated", 0.25)):
        p = s.window_params(0.05, grid.shape, inscribed_radius=0.17, inflation_radius=inflation)
        s.costmap_window_device(2, dmap.data_ptr(), p, dpose.data_ptr(), size, size, res, cost.data_ptr(), origin.data_ptr(), info.data_ptr())
        rc = s._lib.mpc_check_feasibility_device(s._h, 2, C.c_void_p(dx.data_ptr()), C.c_void_p(cost.data_ptr()), size, size, res, C.c_void_p(origin.data_ptr()), None, 0, 0.17,
                                                 0.3, -1, C.c_void_p(feas.data_ptr()))
        assert rc == 0, s._lib.mpc_last_error()
        s.synchronize()
        seen[name] = (feas.cpu().numpy().tolist(), cost.cpu().numpy(), origin.cpu().numpy(), info.cpu().numpy())
    assert seen["plain"][0] == [1, 1] and seen["inflated"][0] == [0, 1]
    # the bytes under the two trajectories, read at the cell the check reads
    for b, (plain, inflated) in enumerate(((0, 253), (0, 113))):
        org = seen["inflated"][2][b]
        i, j = int((xs[b] - org[0]) / res), int((2.5 - org[1]) / res)
        assert seen["plain"][1][b, j, i] == plain and seen["inflated"][1][b, j, i] == inflated, b
    assert (seen["plain"][3][:, 1] == size).all() and (seen["inflated"][3][:, 2] > 9 * size).all()
    s.close()


def test_closed_cycle_on_device_pointers_equals_the_cycle_on_uploaded_host_windows(env):
    """Six robots in one 200 x 200 map at 0.05 m per cell with an L-shaped wall: window -> costmap_to_lines_device -> controller_step_batch_device ->
    check_feasibility_device, everything on device pointers.  The same cycle on a second handle, its windows built by the host build and uploaded: every output of every
    step is identical."""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    B, n, size, res, O, V, stride = 6, 12, 80, 0.05, 32, 4, 16
    grid = np.zeros((200, 200), np.uint8)
    grid[60:141, 100] = 254
    grid[140, 100:161] = 254
    pose = np.array([[4.0, 4.0, 0.0], [4.4, 6.0, 0.5], [6.0, 6.2, -1.0], [5.6, 8.0, math.pi], [2.0, 2.0, 1.0], [7.5, 5.0, math.pi / 2]])
    case = Wn.Case("cycle", grid, pose, (size, size), res, inflation=0.2, inscribed=0.17)
    steps = 0.1 * np.arange(stride)
    plan = np.stack([np.column_stack([p[0] + steps * math.cos(p[2]), p[1] + steps * math.sin(p[2]), np.full(stride, p[2])]) for p in pose])
    n_plan = np.full(B, stride, np.int32)
    cfg = lambda: A.make_config(model=A.MODEL_UNICYCLE, n=n, max_obstacles=O, max_vertices=V, cutoff_dist=2.5)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    f64, i32 = torch.float64, torch.int32
    results = []
    for source in ("device", "host"):
        s = m.BatchSolver(cfg(), max_batch=B)
        cp, lp = s.cycle_params(n_ref=n, period=0.1), s.line_params(res)
        dmap, dpose, dplan, dnplan = T(grid), T(pose), T(plan), T(n_plan)
        cost, origin, info = Z((B, size, size), torch.uint8), Z((B, 2), f64), Z((B, 4), i32)
        ob = [Z((B,), i32), Z((B, O), i32), Z((B, O, V, 2), f64), Z((B, O), f64), Z((B, O, 2), f64)]
        dropped, linfo = Z((B,), i32), Z((B, 4), i32)
        x, u, dt, st, it, ri, feas = Z((B, n, 3), f64), Z((B, n, 2), f64), Z((B,), f64), Z((B,), i32), Z((B,), i32), Z((B,), i32), Z((B,), i32)
        if source == "host":
            hc, ho, hi = Wn.host_window(case)
            cost, origin, info = T(hc), T(ho), T(hi)
        torch.cuda.synchronize()
        if source == "device":
            s.costmap_window_device(B, dmap.data_ptr(), case.struct(), dpose.data_ptr(), size, size, res, cost.data_ptr(), origin.data_ptr(), info.data_ptr())
        obp = tuple(t.data_ptr() for t in ob)
        s.costmap_to_lines_device(B, cost.data_ptr(), size, size, res, origin.data_ptr(), dpose.data_ptr(), lp, *obp, dropped.data_ptr(), linfo.data_ptr())
        s.controller_step_device(B, cp, dplan.data_ptr(), dnplan.data_ptr(), stride, None, None, None, None, None, x.data_ptr(), u.data_ptr(), dt.data_ptr(), st.data_ptr(),
                                 it.data_ptr(), ri.data_ptr(), obstacles=obp)
        rc = s._lib.mpc_check_feasibility_device(s._h, B, C.c_void_p(x.data_ptr()), C.c_void_p(cost.data_ptr()), size, size, res, C.c_void_p(origin.data_ptr()), None, 0, 0.17, 0.3,
                                                 -1, C.c_void_p(feas.data_ptr()))
        assert rc == 0, s._lib.mpc_last_error()
        s.synchronize()
        results.append({k: v.cpu().numpy() for k, v in dict(cost=cost, origin=origin, info=info, n_obstacles=ob[0], n_vertices=ob[1], vertices=ob[2], dropped=dropped, line_info=linfo,
                                                            x=x, u=u, dt=dt, status=st, iters=it, reinit=ri, feasible=feas).items()})
        s.close()
    on_device, on_host = results
    for k in on_device:
        assert on_device[k].tobytes() == on_host[k].tobytes(), k
    print(f"lines per robot {on_device['line_info'][:, 2].tolist()}, obstacles {on_device['n_obstacles'].tolist()}, status {on_device['status'].tolist()}, "
          f"feasible {on_device['feasible'].tolist()}, changed cells {on_device['info'][:, 2].tolist()}")
    assert (on_device["info"][:, 0] == size * size).all() and on_device["line_info"][:, 2].sum() >= 4 and np.isfinite(on_device["x"]).all()
