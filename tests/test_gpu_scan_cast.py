"""GPU tests (-m gpu) of mpc_scan_cast* (mpc_local_planner_amd/csrc/mpc_scan_cast.hpp, include/mpc_scan_cast.h): the laser scan of every robot of a batch, cast on
the device through one shared map and a pool of other bodies.

The yardstick is the host build of the same header (tests/host_harness/scan_cast_host.cpp through tests/_cast_cases.py), which tests/test_scan_cast_host.py holds to
a Python restatement: the device has to equal it BIT FOR BIT in ranges, hit and info, over poisoned outputs, on every scripted case and on the random scenes.  Then:
hit and info may each be NULL; Rc at the cap of the kernel's LDS, and one above it refused; a pool on either side of the culled list's capacity; an instance of a batch
of eight equals the same instance alone; the host-pointer entry equals the device entry; every refusal leaves the outputs untouched; two cycles cast -> window -> scans
on device pointers equal the host builds chained; one robot in closed loop round a box only its laser sees; two robots that see each other and not themselves."""
import ctypes as C
import math

import numpy as np
import pytest

import _cast_cases as Cc
import _scan_cases as Sc
import _window_cases as Wc

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
    """a handle per max_vertices: the pool is laid out with V = cfg.max_vertices"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    made = {}

    def get(V):
        if V not in made:
            made[V] = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=1, max_vertices=V), max_batch=8)
        return made[V]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def scripted():
    """(case, the host build's result) of every scripted case, computed once and left unchanged"""
    return [(c, Cc.host_cast(c)) for c in Cc.cases()]


def _device(s, torch, c, with_hit=True, with_info=True):
    """mpc_scan_cast_device on torch tensors, the outputs poisoned: (ranges, hit, info); hit / info None when the case has none or they are passed as NULL"""
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = lambda t: None if t is None else t.data_ptr()
    ranges, hit, info = (T(a) for a in c.outputs())
    if not with_hit:
        hit = None
    if not with_info:
        info = None
    dmap, dpose, dself = T(c.grid), T(c.pose), T(c.self_index)
    dnv, dv, dr = (T(a) if c.P else None for a in (c.pnv, c.pv, c.pr))
    torch.cuda.synchronize()
    s.scan_cast_device(c.B, dmap.data_ptr(), c.struct(), dpose.data_ptr(), c.n, ranges.data_ptr(), pool=(c.P, P(dnv), P(dv), P(dr)) if c.P else None, self_index=P(dself),
                       hit=P(hit), info=P(info))
    s.synchronize()
    N = lambda t: None if t is None else t.cpu().numpy()
    return N(ranges), N(hit), N(info)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solvers, scripted):
    """ranges, hit and info over the poison; then the same with hit NULL, with info NULL, and with both"""
    m, torch = env
    assert len(scripted) >= 35 and max(c.B for c, _ in scripted) <= 8 and {c.n for c, _ in scripted} >= {1, 63, 64, 65, 257}
    for c, host in scripted:
        s = solvers(c.V)
        got = _device(s, torch, c)
        assert Cc.same(got, host) is None, (c.name, Cc.same(got, host))
        assert s.last_costmap_ms() > 0.0
        no_hit, no_info, bare = _device(s, torch, c, with_hit=False), _device(s, torch, c, with_info=False), _device(s, torch, c, with_hit=False, with_info=False)
        assert no_hit[1] is None and Cc.same((no_hit[0], host[1], no_hit[2]), host) is None, c.name
        assert no_info[2] is None and Cc.same((no_info[0], no_info[1], host[2]), host) is None, c.name
        assert bare[1] is None and bare[2] is None and bare[0].tobytes() == host[0].tobytes(), c.name
    # the host build leaves no poison: every word is a value of the rule
    assert all((h[0] != Cc.FPOISON).all() and (h[1] is None or (h[1] != Cc.IPOISON).all()) and (h[2] is None or (h[2] != Cc.IPOISON).all()) for _, h in scripted)


def test_random_scenes_equal_the_host_build(env, solvers):
    m, torch = env
    by_pool = 0
    for c in Cc.random_cases():
        got, host = _device(solvers(c.V), torch, c), Cc.host_cast(c)
        assert Cc.same(got, host) is None, (c.name, Cc.same(got, host))
        by_pool += int((host[1] >= 0).sum())
    assert by_pool > 200


def test_rc_at_the_cap_of_the_lds_and_one_above_it(env, solvers):
    """0.0625 m cells: range_max 21.875 m is 350 cells, Rc = 351, the cap; 21.876 m is Rc = 352"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    assert Cc.harness().sch_max_rc() == 351
    c = Cc.Case("Rc at the cap", Cc.room(96, 96), [(2.9, 3.1, 0.4), (0.2, 5.8, -2.0), (7.0, 3.0, 0.0)], 130, res=0.0625, range_max=21.875, pool=Cc.ring_pool(9, (2.9, 3.1), 0.3, 20.0, 5), V=3)
    assert c.Rc == 351
    s = solvers(3)
    got, host = _device(s, torch, c), Cc.host_cast(c)
    assert Cc.same(got, host) is None, Cc.same(got, host)
    assert (host[2][:2, 3] == 4 * 95).all() and host[2][2, 3] == 0 and (host[1] == Cc.MAP).sum() > 200
    with pytest.raises(m.MpcError) as e:
        _device(s, torch, c.variant(range_max=21.876))
    assert e.value.code == A.MPC_EINVAL and "350 cells" in str(e.value)


def test_a_pool_on_either_side_of_the_culled_lists_capacity(env, solvers):
    """512 entries within reach fill the list exactly; with 513 the third chunk does not fit and is read from global memory; 812 the same with a longer tail; 700 entries
    near and far under a short range_max, most of them culled"""
    m, torch = env
    cap = Cc.harness().sch_list_cap()
    assert cap == 512
    centre = (1.23, 0.97, 0.3)
    s = solvers(3)
    for P, hi, range_max in ((cap, 0.9, 3.0), (cap + 1, 0.9, 3.0), (cap + 300, 0.9, 3.0), (700, 9.0, 1.0)):
        c = Cc.Case(f"{P} entries", Cc.room(), [centre, (0.5, 1.5, 2.0)], 70, range_max=range_max, pool=Cc.ring_pool(P, centre, 0.15, hi, P), V=3, self_index=[3, -1])
        got, host = _device(s, torch, c), Cc.host_cast(c)
        assert Cc.same(got, host) is None, (P, Cc.same(got, host))
        assert (host[1] >= 0).sum() > 20 and (host[1][0] != 3).all()


def test_an_instance_of_a_batch_of_eight_equals_the_same_instance_alone(env, solvers):
    m, torch = env
    rng = np.random.default_rng(4)
    pose = np.column_stack([rng.uniform(-0.2, 2.6, 8), rng.uniform(-0.2, 2.2, 8), rng.uniform(-3, 3, 8)])
    pose[5] = (math.nan, 1.0, 0.0)
    c = Cc.Case("eight", Cc.random_rooms(1, seed=9, W=48, H=40)[0][0], pose, 100, range_max=2.0, pool=Cc.ring_pool(20, (1.2, 1.0), 0.1, 1.2, 1), V=3, self_index=np.arange(8))
    s = solvers(3)
    among = _device(s, torch, c)
    assert Cc.same(among, Cc.host_cast(c)) is None
    for b in range(8):
        alone = _device(s, torch, c.take(b))
        assert Cc.same(tuple(np.ascontiguousarray(a[b:b + 1]) for a in among), alone) is None, b


def test_host_pointer_entry_equals_the_device_entry(env, solvers, scripted):
    m, torch = env
    for c, host in scripted:
        got = solvers(c.V).scan_cast(c.grid, c.struct(), c.pose, c.n, pool=c.pool_tuple(), self_index=c.self_index)
        assert Cc.same((got[0], got[1] if host[1] is not None else None, got[2] if host[2] is not None else None), host) is None, c.name


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solvers, scripted):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    solver = solvers(3)
    c = [c for c, _ in scripted if c.name == "63 beams"][0]
    ranges, hit, info = c.outputs()
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    fl = lambda x: None if x is None else x.ctypes.data_as(C.POINTER(C.c_float))
    pool = A.MpcPool(c.P, c.pnv.ctypes.data, c.pv.ctypes.data, c.pr.ctypes.data, None)

    def prm(**kw):
        q = c.struct()
        for k, v in kw.items():
            if k in ("sensor_pose", "map_origin"):
                v = (C.c_double * len(v))(*v)
            setattr(q, k, v)
        return q

    def call(fn, B=c.B, grid=c.grid, p=c.struct(), pose=c.pose, pool=pool, n=c.n, out=ranges):
        return fn(solver._h, B, a(grid), None if p is None else C.byref(p), a(pose), None if pool is None else C.byref(pool), a(c.self_index), n, fl(out), a(hit), a(info))

    for fn in (lib.mpc_scan_cast, lib.mpc_scan_cast_device):          # refused before anything is read: host arrays do for both
        for bad in (dict(grid=None), dict(p=None), dict(pose=None), dict(out=None)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"mpc_scan_cast: null argument" in lib.mpc_last_error(), bad
        for bad in (dict(n=0), dict(n=-3), dict(n=4097)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"n_beams" in lib.mpc_last_error(), bad
        for bad in (dict(map_size_x=0), dict(map_size_y=-1), dict(map_size_x=1 << 16, map_size_y=1 << 15)):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and b"bad map size" in lib.mpc_last_error(), bad
        for field in ("map_resolution", "range_max"):
            for v in (0.0, -0.1, math.nan, math.inf):
                assert call(fn, p=prm(**{field: v})) == A.MPC_EINVAL and b"positive and finite" in lib.mpc_last_error(), (field, v)
        for bad in (dict(angle_min=math.nan), dict(angle_increment=math.inf), dict(sensor_pose=(math.nan, 0, 0)), dict(sensor_pose=(0, 0, -math.inf)), dict(map_origin=(0, math.nan))):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and b"have to be finite" in lib.mpc_last_error(), bad
        assert call(fn, p=prm(range_max=17.6)) == A.MPC_EINVAL and b"350 cells" in lib.mpc_last_error()          # 352 cells of 0.05 m
        for v in (0, -1, 255):
            assert call(fn, p=prm(block_threshold=v)) == A.MPC_EINVAL and b"block_threshold" in lib.mpc_last_error(), v
        assert call(fn, pool=A.MpcPool(-1, None, None, None, None)) == A.MPC_EINVAL and b"P is negative" in lib.mpc_last_error()
        assert call(fn, pool=A.MpcPool(2, None, c.pv.ctypes.data, None, None)) == A.MPC_EINVAL and b"n_vertices and vertices" in lib.mpc_last_error()
        assert call(fn, B=9) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
    # a refused call changes nothing
    for x, y in zip(c.outputs(), (ranges, hit, info)):
        assert x.tobytes() == y.tobytes()
    assert call(lib.mpc_scan_cast, B=0) == A.MPC_OK and (ranges == Cc.FPOISON).all() and (info == Cc.IPOISON).all()
    # what is taken: a pool of no entries, and no pool at all
    assert call(lib.mpc_scan_cast, pool=A.MpcPool(0, None, None, None, None)) == A.MPC_OK and (ranges != Cc.FPOISON).all() and (hit < 0).all()
    assert call(lib.mpc_scan_cast, pool=None) == A.MPC_OK and (hit < 0).all() and (info[:, 1] == 0).all()


def test_two_cycles_on_device_pointers_equal_the_host_builds_chained(env, solvers):
    """cast -> window -> scans on the solver's stream with nothing in between; the ranges never leave the device.  Five robots in a room with boxes, a pool of the
    robots themselves; the layers are kept from the first cycle to the second."""
    m, torch = env
    B, W, H, res, n = 5, 60, 60, 0.05, 120
    s = solvers(1)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    grid, pose = Cc.random_rooms(1, seed=5, W=64, H=48, poses=B)[0]
    step = np.array([[0.06, 0.02, 0.2], [-0.05, 0.04, -0.3], [0.0, -0.07, 0.1], [0.03, 0.03, 0.0], [-0.02, 0.0, 0.5]])
    radius = np.full(B, 0.12)
    dmap, d_layer, d_cell = T(grid), T(np.full((B, H, W), Sc.POISON, np.uint8)), T(np.full((B, 2), Sc.IPOISON, np.int32))
    d_ranges, d_hit, d_cinfo = T(np.full((B, n), Cc.FPOISON, np.float32)), T(np.full((B, n), Cc.IPOISON, np.int32)), T(np.full((B, 4), Cc.IPOISON, np.int32))
    d_cost, d_origin, d_sinfo = T(np.zeros((B, H, W), np.uint8)), T(np.zeros((B, 2))), T(np.zeros((B, 4), np.int32))
    d_nv, d_rad, d_self, d_keep = T(np.ones(B, np.int32)), T(radius), T(np.arange(B, dtype=np.int32)), T(np.ones(B, np.int32))
    host_layer = host_cell = None
    for k in range(2):
        p = pose + k * step
        cc = Cc.Case(f"cycle {k}", grid, p, n, sensor=(-0.1, 0.0, 0.0), angle_min=-1.5, angle_inc=3.0 / n, range_max=2.5, pool=Cc.discs(p[:, :2], radius), self_index=np.arange(B))
        wc = Wc.Case(f"cycle {k}", grid, p, (W, H), res, inflation=0.0)
        h_ranges, h_hit, h_cinfo = Cc.host_cast(cc)
        h_cost, h_origin, _ = Wc.host_window(wc)
        sc = Sc.Case(f"cycle {k}", p, h_ranges, (W, H), res, sensor=cc.sensor, angle_min=cc.angle_min, angle_inc=cc.angle_inc, range_min=0.05, range_max=cc.range_max, obstacle_range=2.0,
                     raytrace_range=2.5, keep=None if k == 0 else 1, layer0=host_layer, cell0=host_cell, cost0=h_cost)
        h_layer, h_cell, h_cost2, h_sinfo = Sc.host_scans(sc)
        d_pose, d_pv = T(p), T(p[:, None, :2].copy())
        torch.cuda.synchronize()
        s.scan_cast_device(B, dmap.data_ptr(), cc.struct(), d_pose.data_ptr(), n, d_ranges.data_ptr(), pool=(B, d_nv.data_ptr(), d_pv.data_ptr(), d_rad.data_ptr()),
                           self_index=d_self.data_ptr(), hit=d_hit.data_ptr(), info=d_cinfo.data_ptr())
        s.costmap_window_device(B, dmap.data_ptr(), wc.struct(), d_pose.data_ptr(), W, H, res, d_cost.data_ptr(), d_origin.data_ptr())
        s.costmap_scans_device(B, sc.struct(), d_pose.data_ptr(), d_ranges.data_ptr(), n, d_keep.data_ptr() if k else None, W, H, res, d_layer.data_ptr(), d_cell.data_ptr(),
                               d_cost.data_ptr(), d_sinfo.data_ptr())
        s.synchronize()
        assert Cc.same(tuple(t.cpu().numpy() for t in (d_ranges, d_hit, d_cinfo)), (h_ranges, h_hit, h_cinfo)) is None, k
        assert Sc.same(tuple(t.cpu().numpy() for t in (d_layer, d_cell, d_cost, d_sinfo)), (h_layer, h_cell, h_cost2, h_sinfo)) is None, k
        assert d_origin.cpu().numpy().tobytes() == h_origin.tobytes() and (h_hit == Cc.MAP).sum() > 100 and h_sinfo[:, 1].min() > 3
        host_layer, host_cell = h_layer, h_cell


def test_only_the_cast_scan_sees_the_box_and_the_path_goes_round_it(env):
    """The scenario of tests/test_gpu_costmap_scans.py::test_only_the_scan_sees_the_box_and_the_path_goes_round_it with the scan no longer made on the host: the
    planner's static map is empty, the map the laser is cast through has a box of 0.3 m x 0.3 m, 1.25 m ahead of the robot and 0.1 m off its line to the goal.  The
    chain on device pointers: scan_cast_device -> costmap_window_device -> costmap_scans_device -> mpc_costmap_to_obstacles_device -> mpc_step_batch_device, four control
    cycles, the robot moving on to the third pose of its path each time (the plant is the caller's).  Every obstacle is the centre of a cell of the box, and every path
    keeps min_obstacle_dist from every one of them, less the 1e-6 the other clearance tests of this suite allow a converged solve."""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    n, size, res, O, beams, dmin = 20, 80, 0.05, 96, 360, 0.2
    box = (2.25, 2.35, 2.55, 2.65)
    goal = np.array([[4.0, 2.4, 0.0]])
    planner_map = np.zeros((96, 96), np.uint8)
    world = planner_map.copy()
    world[47:53, 45:51] = 254
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    f64, i32, u8, f32 = torch.float64, torch.int32, torch.uint8, torch.float32
    V = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=O, max_vertices=1, max_obstacle_rows=16, min_obstacle_dist=dmin), max_batch=1)
    wp = s.window_params(0.05, planner_map.shape)
    cp = s.cast_params(0.05, world.shape, angle_min=-math.pi, angle_increment=2 * math.pi / beams, range_max=10.0)
    sp = s.scan_params(angle_min=-math.pi, angle_increment=2 * math.pi / beams, range_min=0.05, range_max=10.0, obstacle_range=3.0, raytrace_range=4.0, track_unknown=1)
    dplanner, dworld, dgoal = T(planner_map), T(world), T(goal)
    cost, origin, layer, cell = Z((1, size, size), u8), Z((1, 2), f64), Z((1, size, size), u8), Z((1, 2), i32)
    ranges, hit, cinfo = Z((1, beams), f32), Z((1, beams), i32), Z((1, 4), i32)
    keep, sinfo = torch.ones((1,), dtype=i32, device=dev), Z((1, 4), i32)
    ob = [Z((1,), i32), Z((1, O), i32), Z((1, O, 1, 2), f64)]
    dropped = Z((1,), i32)
    x, u, dt, st, it = Z((1, n, 3), f64), Z((1, n, 2), f64), Z((1,), f64), Z((1,), i32), Z((1,), i32)
    pose = np.array([[1.0, 2.4, 0.0]])
    cycles = []
    for k in range(4):
        dpose = T(pose)
        torch.cuda.synchronize()
        s.scan_cast_device(1, dworld.data_ptr(), cp, dpose.data_ptr(), beams, ranges.data_ptr(), hit=hit.data_ptr(), info=cinfo.data_ptr())
        s.costmap_window_device(1, dplanner.data_ptr(), wp, dpose.data_ptr(), size, size, res, cost.data_ptr(), origin.data_ptr())
        s.costmap_scans_device(1, sp, dpose.data_ptr(), ranges.data_ptr(), beams, keep.data_ptr() if k else None, size, size, res, layer.data_ptr(), cell.data_ptr(),
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
                           dropped=int(dropped.cpu().numpy()[0]), cast=cinfo.cpu().numpy()[0].tolist(), info=sinfo.cpu().numpy()[0].tolist(),
                           rows_dropped=int(s.last_rows_dropped(1)[0])))
        pose = hx[:, 2].copy()
    s.close()
    inside = lambda p: bool(((p[:, 0] > box[0]) & (p[:, 0] < box[2]) & (p[:, 1] > box[1]) & (p[:, 1] < box[3])).any())
    for k, c in enumerate(cycles):
        print(f"cycle {k}: cast {c['cast']}, obstacles {c['n_obstacles']}, scans info {c['info']}, rows dropped {c['rows_dropped']}, status {c['status']}, "
              f"clearance {c['clearance']:.6f}, crosses {inside(c['x'])}")
    for c in cycles:
        p = c["points"]
        assert c["cast"][0] > 0 and c["cast"][1] == 0 and c["cast"][0] + c["cast"][2] == beams and c["cast"][3] == 36
        assert 5 <= c["n_obstacles"] == c["info"][1] <= 16 and c["dropped"] == 0 and c["rows_dropped"] == 0 and c["info"][3] == c["info"][1]
        # every obstacle is the centre of a cell of the box
        assert ((p[:, 0] > box[0]) & (p[:, 0] < box[2]) & (p[:, 1] > box[1]) & (p[:, 1] < box[3])).all()
        assert c["status"] == 0 and c["clearance"] >= dmin - 1e-6 and not inside(c["x"]), c
    assert cycles[3]["n_obstacles"] >= cycles[0]["n_obstacles"]          # the layer keeps what earlier cycles saw


def test_two_robots_see_each_other_and_not_themselves(env, solvers):
    """an empty room, two robots 1 m apart facing each other, the pool made of the two as discs of 0.15 m with self_index = (0, 1): each appears in the other's hit words
    and, after the window and scans steps, as marks in the other's layer around where it stands; neither appears in its own"""
    m, torch = env
    s = solvers(1)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    grid, B, n, W, H, res, rad = Cc.room(), 2, 90, 60, 60, 0.05, 0.15
    pose = np.array([[0.7, 1.0, 0.0], [1.7, 1.0, math.pi]])
    cc = Cc.Case("two robots", grid, pose, n, angle_min=-0.75, angle_inc=1.5 / (n - 1), range_max=3.0, pool=Cc.discs(pose[:, :2], [rad, rad]), self_index=[0, 1])
    wc = Wc.Case("two robots", grid, pose, (W, H), res)
    sp = s.scan_params(angle_min=cc.angle_min, angle_increment=cc.angle_inc, range_min=0.0, range_max=cc.range_max, obstacle_range=2.5, raytrace_range=3.0, track_unknown=0)
    dmap, dpose = T(grid), T(pose)
    d_nv, d_pv, d_rad, d_self = T(np.ones(B, np.int32)), T(pose[:, None, :2].copy()), T(np.full(B, rad)), T(np.arange(B, dtype=np.int32))
    ranges, hit = torch.zeros((B, n), dtype=torch.float32, device=dev), torch.zeros((B, n), dtype=torch.int32, device=dev)
    cost, origin = torch.zeros((B, H, W), dtype=torch.uint8, device=dev), torch.zeros((B, 2), dtype=torch.float64, device=dev)
    layer, cell = torch.zeros((B, H, W), dtype=torch.uint8, device=dev), torch.zeros((B, 2), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    s.scan_cast_device(B, dmap.data_ptr(), cc.struct(), dpose.data_ptr(), n, ranges.data_ptr(), pool=(B, d_nv.data_ptr(), d_pv.data_ptr(), d_rad.data_ptr()), self_index=d_self.data_ptr(),
                       hit=hit.data_ptr())
    s.costmap_window_device(B, dmap.data_ptr(), wc.struct(), dpose.data_ptr(), W, H, res, cost.data_ptr(), origin.data_ptr())
    s.costmap_scans_device(B, sp, dpose.data_ptr(), ranges.data_ptr(), n, None, W, H, res, layer.data_ptr(), cell.data_ptr(), cost.data_ptr(), None)
    s.synchronize()
    h, r, L, org = hit.cpu().numpy(), ranges.cpu().numpy(), layer.cpu().numpy(), origin.cpu().numpy()
    assert Cc.same((r, h, None), Cc.host_cast(cc)[:2] + (None,)) is None
    for b, other in ((0, 1), (1, 0)):
        assert (h[b] == other).sum() >= 5 and (h[b] != b).all() and abs(r[b][h[b] == other].min() - (1.0 - rad)) < 1e-3
        ys, xs = np.nonzero(L[b] == Sc.LETHAL)
        wx, wy = org[b, 0] + (xs + 0.5) * res, org[b, 1] + (ys + 0.5) * res
        to_other, to_self = np.hypot(wx - pose[other, 0], wy - pose[other, 1]), np.hypot(wx - pose[b, 0], wy - pose[b, 1])
        assert (to_other < rad + res).sum() >= 3 and (to_self > 0.5).all(), b
