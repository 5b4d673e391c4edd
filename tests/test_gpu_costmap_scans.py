"""GPU tests (-m gpu) of mpc_costmap_scans* (mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp, include/mpc_costmap_scans.h): the laser-scan obstacle layer of every
robot of a batch, kept on the device between cycles.

The yardstick is the host build of the same header (tests/host_harness/costmap_scans_host.cpp through tests/_scan_cases.py), which tests/test_costmap_scans_host.py
holds to an independent Python restatement: the device has to equal it BIT FOR BIT in layer, layer_cell, cost and info on every scripted case and on the random second
cycles -- every value is a byte or an integer, and the doubles that decide them are stated operation by operation -- with cost, info and the state of every instance
that does not keep its layer pre-filled with a poison pattern.  Then: cost and info may be NULL; the host-pointer entry equals the device entry; an instance of a batch
of 8 equals the same instance alone; every refusal leaves the four outputs untouched; three cycles on device pointers equal three cycles of the host build; and one
closed cycle in which only the scan sees the obstacle: without this step the solved path crosses it, with it the path keeps min_obstacle_dist."""
import ctypes as C
import math

import numpy as np
import pytest

import _scan_cases as Sc

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
    return [(c, Sc.host_scans(c)) for c in Sc.cases()]


def poisoned_state(c):
    """the case's state with the layer and the cell of every instance that does not keep them overwritten by the poison: the rule does not read them"""
    layer, cell, cost, info = c.state()
    for b in range(c.B):
        if c.keep is None or c.keep[b] == 0:
            layer[b], cell[b] = Sc.POISON, Sc.IPOISON
    return layer, cell, cost, info


def _device(s, torch, c, with_cost=True, with_info=True):
    """mpc_costmap_scans_device on torch tensors: (layer, layer_cell, cost, info); cost / info None when the case has none or they are passed as NULL"""
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = lambda t: None if t is None else t.data_ptr()
    layer, cell, cost, info = (T(a) for a in poisoned_state(c))
    if not with_cost:
        cost = None
    if not with_info:
        info = None
    dpose, dranges, dkeep = T(c.pose), T(c.ranges), T(c.keep)
    torch.cuda.synchronize()
    s.costmap_scans_device(c.B, c.struct(), dpose.data_ptr(), dranges.data_ptr(), c.n, P(dkeep), c.W, c.H, c.res, layer.data_ptr(), cell.data_ptr(), P(cost), P(info))
    s.synchronize()
    N = lambda t: None if t is None else t.cpu().numpy()
    return N(layer), N(cell), N(cost), N(info)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solver, scripted):
    """layer, layer_cell, cost and info over the poison: what equals the host build was written in full; then the same with cost NULL and with info NULL"""
    m, torch = env
    assert len(scripted) >= 30 and max(c.B for c, _ in scripted) <= 8
    for c, host in scripted:
        got = _device(solver, torch, c)
        assert Sc.same(got, host) is None, (c.name, Sc.same(got, host))
        assert solver.last_costmap_ms() > 0.0
        bare = _device(solver, torch, c, with_cost=False, with_info=False)
        assert Sc.same(bare[:2], host[:2]) is None and bare[2] is None and bare[3] is None, c.name
    # the host build leaves no poison either: every count is a value of the rule, and so is every layer byte and cell
    assert all(h[3] is None or (h[3] != Sc.IPOISON).all() for _, h in scripted) and all((h[1] != Sc.IPOISON).all() for _, h in scripted)


def test_window_and_info_may_be_null_one_at_a_time(env, solver, scripted):
    m, torch = env
    by = {c.name: (c, h) for c, h in scripted}
    for name in ("55 x 55, carlike, 360 beams", "17 x 16, 64 beams", "rolls under a scan"):
        c, host = by[name]
        no_cost, no_info = _device(solver, torch, c, with_cost=False), _device(solver, torch, c, with_info=False)
        assert no_cost[2] is None and no_cost[3] is not None and Sc.same(no_cost[:2], host[:2]) is None and (no_cost[3][:, :3] == host[3][:, :3]).all() and (no_cost[3][:, 3] == 0).all()
        assert no_info[3] is None and Sc.same(no_info[:3], host[:3]) is None, name


def test_random_second_cycles_equal_the_host_build(env, solver):
    m, torch = env
    marked = 0
    for c in Sc.random_cases():
        got, host = _device(solver, torch, c), Sc.host_scans(c)
        assert Sc.same(got, host) is None, (c.name, Sc.same(got, host))
        marked += int(host[3][:, 1].clip(0).sum())
    assert marked > 500


def test_host_pointer_entry_equals_the_device_entry(env, solver, scripted):
    m, torch = env
    for c, host in scripted:
        layer, cell, cost, info = poisoned_state(c)
        got = solver.costmap_scans(c.struct(), c.pose, c.ranges, (c.W, c.H), c.res, layer=layer, layer_cell=cell, keep=c.keep, cost=cost, want_info=not c.no_info)
        assert Sc.same(got, host) is None, (c.name, Sc.same(got, host))
        assert layer.tobytes() == poisoned_state(c)[0].tobytes()          # the wrapper works on copies
    # a first cycle needs no state
    c, host = [(c, h) for c, h in scripted if c.name == "55 x 55, the demo's, 360 beams"][0]
    got = solver.costmap_scans(c.struct(), c.pose, c.ranges, (c.W, c.H), c.res, cost=c.cost0)
    assert Sc.same(got, host) is None


def test_an_instance_of_a_batch_of_eight_equals_the_same_instance_alone(env, solver, scripted):
    m, torch = env
    by = {c.name: c for c, _ in scripted}
    rng = np.random.default_rng(4)
    for name in ("rolls under a scan", "a pose that is not finite"):
        c = by[name]
        among = _device(solver, torch, c)
        for b in range(8):
            alone = _device(solver, torch, c.take(b))
            assert Sc.same(tuple(np.ascontiguousarray(a[b:b + 1]) for a in among), alone) is None, (name, b)
    c = by["55 x 55, carlike, 360 beams"]
    pose = np.column_stack([rng.uniform(-0.5, 3.5, 8), rng.uniform(-0.5, 2.7, 8), rng.uniform(-3, 3, 8)])
    c = c.variant(pose=pose, ranges=Sc.room_ranges(rng, 8, 360, 0.3, 4.5), cost0=None, layer0=None, cell0=None)
    among = _device(solver, torch, c)
    for b in range(8):
        alone = _device(solver, torch, c.take(b))
        assert Sc.same(tuple(np.ascontiguousarray(a[b:b + 1]) for a in among), alone) is None, b


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solver, scripted):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    c = [c for c, _ in scripted if c.name == "7 x 5, 63 beams"][0]
    layer, cell, cost, info = c.state()
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    fl = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))

    def prm(**kw):
        q = c.struct()
        for k, v in kw.items():
            if k == "sensor_pose":
                v = (C.c_double * 3)(*v)
            setattr(q, k, v)
        return q

    def call(fn, B=c.B, p=c.struct(), pose=c.pose, ranges=c.ranges, n=c.n, W=c.W, H=c.H, res=c.res, layer=layer, cell=cell):
        return fn(solver._h, B, None if p is None else C.byref(p), a(pose), fl(ranges), n, None, W, H, res, a(layer), a(cell), a(cost), a(info))

    for fn in (lib.mpc_costmap_scans, lib.mpc_costmap_scans_device):          # refused before anything is read: host arrays do for both
        for bad in (dict(p=None), dict(pose=None), dict(ranges=None), dict(layer=None), dict(cell=None)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"null argument" in lib.mpc_last_error(), bad
        for bad in (dict(n=0), dict(n=-3), dict(n=4097)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"n_beams" in lib.mpc_last_error(), bad
        for bad in (dict(W=0), dict(H=0), dict(W=257, H=256), dict(W=65537, H=1), dict(W=1 << 20, H=1 << 20)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"layer geometry" in lib.mpc_last_error(), bad
        for bad in (dict(res=0.0), dict(res=-0.1), dict(res=math.nan), dict(res=math.inf)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"positive and finite" in lib.mpc_last_error(), bad
        for field in ("range_min", "range_max", "obstacle_range", "raytrace_range"):
            for v in (-0.1, math.nan, math.inf):
                assert call(fn, p=prm(**{field: v})) == A.MPC_EINVAL and b"at least 0 and finite" in lib.mpc_last_error(), (field, v)
        assert call(fn, p=prm(raytrace_range=409.7)) == A.MPC_EINVAL and b"4096 cells" in lib.mpc_last_error()          # 4097 cells of 0.1 m
        assert call(fn, p=prm(range_max=3276.8)) == A.MPC_EINVAL and b"2^15 cells" in lib.mpc_last_error()
        for bad in (dict(angle_min=math.nan), dict(angle_increment=math.inf), dict(sensor_pose=(math.nan, 0, 0)), dict(sensor_pose=(0, -math.inf, 0)), dict(sensor_pose=(0, 0, math.nan))):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and b"have to be finite" in lib.mpc_last_error(), bad
        assert call(fn, p=prm(footprint_clear_radius=math.nan)) == A.MPC_EINVAL and b"footprint_clear_radius" in lib.mpc_last_error()
        for v in (-1, 2):
            assert call(fn, p=prm(combination_method=v)) == A.MPC_EINVAL and b"combination_method" in lib.mpc_last_error(), v
        assert call(fn, B=9) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
    # a refused call changes nothing
    for x, y in zip(c.state(), (layer, cell, cost, info)):
        assert x.tobytes() == y.tobytes()
    assert call(lib.mpc_costmap_scans, B=0) == A.MPC_OK and (layer == Sc.POISON).all() and (info == Sc.IPOISON).all()
    # 409.6 m at 0.1 m is 4096 cells, and 3276.7 m is below 2^15 of them: the largest that are taken
    assert call(lib.mpc_costmap_scans, p=prm(raytrace_range=409.6, range_max=3276.7)) == A.MPC_OK and (layer != Sc.POISON).all() and info[0, 0] > 0


def test_three_cycles_on_device_pointers_equal_three_cycles_of_the_host_build(env, solver):
    """the state stays in two device tensors that the calls roll in place; the windows of a cycle are fresh.  Six robots, 40 x 33 cells, drifting and turning."""
    m, torch = env
    B, W, H, res, n = 6, 40, 33, 0.05, 90
    rng = np.random.default_rng(17)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    pose = np.column_stack([rng.uniform(-2, 2, B), rng.uniform(-2, 2, B), rng.uniform(-3, 3, B)])
    step = np.column_stack([rng.uniform(-0.12, 0.12, B), rng.uniform(-0.12, 0.12, B), rng.uniform(-0.4, 0.4, B)])
    first = Sc.Case("cycle 0", pose, Sc.room_ranges(rng, B, n, 0.2, 1.5), (W, H), res, angle_min=-2.0, angle_inc=4.0 / n, clear_radius=0.1,
                    cost0=rng.choice(np.array([0, 0, 254, 255], np.uint8), size=(B, H, W)))
    layer, cell, _, _ = poisoned_state(first)
    d_layer, d_cell = T(layer), T(cell)
    host_layer, host_cell, marks = layer, cell, []
    for k in range(3):
        keep = None if k == 0 else np.array([1, 1, 0, 1, 1, 1], np.int32)          # the third robot's controller was reset
        c = first.variant(f"cycle {k}", pose=pose + k * step, ranges=Sc.room_ranges(rng, B, n, 0.2, 1.5), keep=keep, layer0=host_layer, cell0=host_cell,
                          cost0=rng.choice(np.array([0, 0, 254, 255], np.uint8), size=(B, H, W)))
        host = Sc.host_scans(c)
        d_pose, d_ranges, d_keep, d_cost, d_info = T(c.pose), T(c.ranges), None if keep is None else T(keep), T(c.cost0), T(np.full((B, 4), Sc.IPOISON, np.int32))
        torch.cuda.synchronize()
        solver.costmap_scans_device(B, c.struct(), d_pose.data_ptr(), d_ranges.data_ptr(), n, None if keep is None else d_keep.data_ptr(), W, H, res, d_layer.data_ptr(),
                                    d_cell.data_ptr(), d_cost.data_ptr(), d_info.data_ptr())
        solver.synchronize()
        got = tuple(t.cpu().numpy() for t in (d_layer, d_cell, d_cost, d_info))
        assert Sc.same(got, host) is None, (k, Sc.same(got, host))
        host_layer, host_cell = host[0], host[1]
        marks.append(int(host[3][:, 1].sum()))
    assert marks[2] > marks[0] > 50 and (np.abs(host_cell - cell) < 2 ** 20).all()          # the layers accumulate what the scans saw


def _box_ranges(pose, box, angle_min, angle_inc, n):
    """a scan by numpy ray casting: the distance along every beam from the pose to the axis-aligned box (x0, y0, x1, y1), a millimetre inside it; +inf where it misses"""
    th = pose[2] + angle_min + angle_inc * np.arange(n)
    d = np.stack([np.cos(th), np.sin(th)], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (np.array(box[:2]) - pose[:2]) / d, (np.array(box[2:]) - pose[:2]) / d
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    hit = (near <= far) & (near > 0)
    return np.where(hit, near + 1e-3, np.inf).astype(np.float32)


def test_only_the_scan_sees_the_box_and_the_path_goes_round_it(env):
    """An empty static map and an unmapped box, 0.3 m x 0.3 m, 1.25 m ahead of the robot and 0.1 m off its line to the goal.  The chain on device pointers:
    costmap_window_device -> [costmap_scans_device] -> mpc_costmap_to_obstacles_device -> mpc_step_batch_device, four control cycles, the robot moving on to the third
    pose of its path each time.  Without the scans step there is no obstacle and the path crosses the box.  With it every obstacle is a cell of the box's faces and
    every path keeps min_obstacle_dist from every one of them, less the 1e-6 the other clearance tests of this suite allow a converged solve
    (tests/test_gpu_clearance.py), measured by BatchSolver.evaluate's clearance.  The solver carries max_obstacle_rows = 16 clearance rows per pose, the most a handle
    takes: the two faces of the box a robot can see are at most 13 cells, so no row is dropped (asserted) -- with the default 4 rows a wall of cell-sized points is
    crossed between the poses that carry rows, scans or no scans."""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    n, size, res, O, beams, dmin = 20, 80, 0.05, 96, 360, 0.2
    box = (4.25, 4.95, 4.55, 5.25)
    goal = np.array([[6.0, 5.0, 0.0]])
    grid = np.zeros((200, 200), np.uint8)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    V = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    seen = {}
    for with_scans in (False, True):
        s = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=O, max_vertices=1, max_obstacle_rows=16, min_obstacle_dist=dmin), max_batch=1)
        wp = s.window_params(0.05, grid.shape)
        sp = s.scan_params(angle_min=-math.pi, angle_increment=2 * math.pi / beams, range_min=0.05, range_max=10.0, obstacle_range=3.0, raytrace_range=4.0, track_unknown=1)
        dmap, dgoal = T(grid), T(goal)
        cost, origin, layer, cell = Z((1, size, size), u8), Z((1, 2), f64), Z((1, size, size), u8), Z((1, 2), i32)
        keep, sinfo = torch.ones((1,), dtype=i32, device=dev), Z((1, 4), i32)
        ob = [Z((1,), i32), Z((1, O), i32), Z((1, O, 1, 2), f64)]
        dropped = Z((1,), i32)
        x, u, dt, st, it = Z((1, n, 3), f64), Z((1, n, 2), f64), Z((1,), f64), Z((1,), i32), Z((1,), i32)
        pose = np.array([[3.0, 5.0, 0.0]])
        cycles = []
        for k in range(4):
            dpose = T(pose)
            dranges = T(_box_ranges(pose[0], box, -math.pi, 2 * math.pi / beams, beams)[None])
            torch.cuda.synchronize()
            s.costmap_window_device(1, dmap.data_ptr(), wp, dpose.data_ptr(), size, size, res, cost.data_ptr(), origin.data_ptr())
            if with_scans:
                s.costmap_scans_device(1, sp, dpose.data_ptr(), dranges.data_ptr(), beams, keep.data_ptr() if k else None, size, size, res, layer.data_ptr(), cell.data_ptr(),
                                       cost.data_ptr(), sinfo.data_ptr())
            rc = s._lib.mpc_costmap_to_obstacles_device(s._h, 1, V(cost), size, size, res, V(origin), V(dpose), 1.5, V(ob[0]), V(ob[1]), V(ob[2]), V(dropped))
            assert rc == 0, s._lib.mpc_last_error()
            rc = s._lib.mpc_step_batch_device(s._h, 1, V(dpose), V(dgoal), None, None, None, None, None, C.byref(A.MpcObstacles(*(t.data_ptr() for t in ob), None, None)), 3, 0,
                                              3, n, 0.1, V(x), V(u), V(dt), V(st), V(it))
            assert rc == 0, s._lib.mpc_last_error()
            s.synchronize()
            no, nv, vt = (t.cpu().numpy() for t in ob)
            hx, hu, hdt = x.cpu().numpy(), u.cpu().numpy(), dt.cpu().numpy()
            ev = s.evaluate(pose, goal, hx, hu, hdt, obstacles=(no, nv, vt))
            cycles.append(dict(n_obstacles=int(no[0]), points=vt[0, :int(no[0]), 0].copy(), x=hx[0].copy(), status=int(st.cpu().numpy()[0]), clearance=float(ev.clearance[0]),
                               dropped=int(dropped.cpu().numpy()[0]), info=sinfo.cpu().numpy()[0].tolist(), rows_dropped=int(s.last_rows_dropped(1)[0])))
            pose = hx[:, 2].copy()
        s.close()
        seen[with_scans] = cycles
    inside = lambda p: bool(((p[:, 0] > box[0]) & (p[:, 0] < box[2]) & (p[:, 1] > box[1]) & (p[:, 1] < box[3])).any())
    for k, (blind, seeing) in enumerate(zip(seen[False], seen[True])):
        print(f"cycle {k}: without scans: obstacles {blind['n_obstacles']}, status {blind['status']}, crosses the box {inside(blind['x'])}; with: obstacles {seeing['n_obstacles']}, "
              f"info {seeing['info']}, rows dropped {seeing['rows_dropped']}, status {seeing['status']}, clearance {seeing['clearance']:.6f}, crosses {inside(seeing['x'])}")
    assert all(c["n_obstacles"] == 0 and c["status"] == 0 and math.isinf(c["clearance"]) for c in seen[False]) and inside(seen[False][0]["x"])
    for c in seen[True]:
        p = c["points"]
        assert 5 <= c["n_obstacles"] == c["info"][1] <= 16 and c["dropped"] == 0 and c["rows_dropped"] == 0 and c["info"][0] > 0 and c["info"][3] == c["info"][1]
        # every obstacle is the centre of a cell that touches the box
        assert ((p[:, 0] > box[0] - res) & (p[:, 0] < box[2] + res) & (p[:, 1] > box[1] - res) & (p[:, 1] < box[3] + res)).all()
        assert c["status"] == 0 and c["clearance"] >= dmin - 1e-6 and not inside(c["x"]), c
    assert seen[True][3]["n_obstacles"] >= seen[True][0]["n_obstacles"]          # the layer keeps what earlier cycles saw
