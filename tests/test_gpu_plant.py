"""GPU tests (-m gpu) of mpc_plant_step* (mpc_local_planner_amd/csrc/mpc_plant.hpp, include/mpc_plant.h): every robot of a batch moved by its command on the device,
stalled where its footprint's outline meets the shared map or a body of the pool.

The yardstick is the host build of the same header (tests/host_harness/plant_host.cpp through tests/_plant_cases.py), which tests/test_plant_host.py holds to a
Python restatement: the device has to equal it BIT FOR BIT in pose, vel, stall and info, over poisoned outputs, on every scripted case and on random scenes.  Then:
the nullable outputs may be NULL; the host-pointer entry equals the device entry; a batch of five permuted, and each of its robots alone; a pool of 600 entries with
the blockers on either side of the culled list's capacity and one just inside the culling bound; every refusal leaves the outputs untouched; two robots driven head on
stall on each other; and the fleet's closed loop -- cast, window, scans, obstacles, step, commands, plant step, fleet pool -- runs six cycles on device pointers with no
host step and equals, cycle by cycle, the same loop with the plant done by the host build."""
import ctypes as C
import math

import numpy as np
import pytest

import _cast_cases as Cc
import _plant_cases as Pc

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
    return [(c, Pc.host_step(c)) for c in Pc.cases()]


def _device(s, torch, c, with_stall=True, with_info=True):
    """mpc_plant_step_device on torch tensors, the outputs poisoned: (pose, vel, stall, info); None for what the case has not or what is passed as NULL"""
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    P = lambda t: None if t is None else t.data_ptr()
    pose, vel, stall, info = (T(a) for a in c.state())
    if not with_stall:
        stall = None
    if not with_info:
        info = None
    dmap, dcmd, dself = T(c.grid), T(c.cmd), T(c.self_index)
    dnv, dv, dr = (T(a) if c.P else None for a in (c.pnv, c.pv, c.pr))
    torch.cuda.synchronize()
    s.plant_step_device(c.B, c.struct(), dcmd.data_ptr(), pose.data_ptr(), map_cost=P(dmap), pool=(c.P, P(dnv), P(dv), P(dr)) if c.P else None, self_index=P(dself), vel=P(vel),
                        stall=P(stall), info=P(info))
    s.synchronize()
    N = lambda t: None if t is None else t.cpu().numpy()
    return N(pose), N(vel), N(stall), N(info)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solvers, scripted):
    """pose, vel, stall and info over the poison; then the same with stall NULL, with info NULL, and with both"""
    m, torch = env
    assert len(scripted) >= 40 and max(c.B for c, _ in scripted) <= 8
    for c, host in scripted:
        s = solvers(c.V)
        got = _device(s, torch, c)
        assert Pc.same(got, host) is None, (c.name, Pc.same(got, host))
        assert s.last_costmap_ms() > 0.0
        no_stall, no_info, bare = _device(s, torch, c, with_stall=False), _device(s, torch, c, with_info=False), _device(s, torch, c, with_stall=False, with_info=False)
        assert no_stall[2] is None and Pc.same(no_stall[:2] + (host[2], no_stall[3]), host) is None, c.name
        assert no_info[3] is None and Pc.same(no_info[:3] + (host[3],), host) is None, c.name
        assert bare[2] is None and bare[3] is None and Pc.same(bare[:2] + host[2:], host) is None, c.name
    # the host build leaves no poison in stall and info: every word is a value of the rule, for an invalid instance too
    assert all((h[2] is None or (h[2] != Pc.IPOISON).all()) and (h[3] is None or (h[3] != Pc.IPOISON).all()) for _, h in scripted)


def test_random_scenes_equal_the_host_build(env, solvers):
    m, torch = env
    blocked = moved = 0
    for c in Pc.random_cases(count=20):
        got, host = _device(solvers(c.V), torch, c), Pc.host_step(c)
        assert Pc.same(got, host) is None, (c.name, Pc.same(got, host))
        if host[3] is not None:
            blocked, moved = blocked + int((host[3][:, 1] >= 0).sum()), moved + int(np.maximum(host[3][:, 0], 0).sum())
    assert blocked >= 5 and moved >= 30, (blocked, moved)


def test_host_pointer_entry_equals_the_device_entry(env, solvers, scripted):
    m, torch = env
    for c, host in scripted:
        got = solvers(c.V).plant_step(c.struct(), c.cmd, c.pose, map_cost=c.grid, pool=c.pool_tuple(), self_index=c.self_index, vel=c.vel)
        assert Pc.same((got[0], got[1], got[2] if host[2] is not None else None, got[3] if host[3] is not None else None), host) is None, c.name


def _five():
    """five robots in a room with boxes, a pool round them, velocities kept, clamps on: some run free, some stall"""
    grid, pose = Cc.random_rooms(1, seed=11, W=48, H=40, poses=5)[0]
    rng = np.random.default_rng(12)
    pose[3] = (math.nan, 1.0, 0.0)
    return Pc.Case("five", grid, pose, np.column_stack([rng.uniform(0.3, 1.2, 5), np.zeros(5), rng.uniform(-1, 1, 5)]), vel=rng.uniform(-0.2, 0.2, (5, 3)), a_max=(3.0, 3.0, 4.0),
                   v_max=(1.0, 1.0, 0.8), n_sub=6, interval=0.05, pool=Cc.ring_pool(20, (1.2, 1.0), 0.1, 1.2, 1), V=3, self_index=np.arange(5))


def test_a_batch_of_five_permuted_and_each_robot_alone(env, solvers):
    m, torch = env
    c = _five()
    s = solvers(3)
    among = _device(s, torch, c)
    assert Pc.same(among, Pc.host_step(c)) is None
    assert (among[3][:, 1] >= 0).any() and (among[3][:, 0] > 0).sum() >= 2 and among[3][3].tolist() == [-1] * 4
    order = np.array([3, 0, 4, 2, 1])
    mixed = _device(s, torch, c.take(order))
    assert Pc.same(tuple(np.ascontiguousarray(a[order]) for a in among), mixed) is None
    for b in range(5):
        alone = _device(s, torch, c.take([b]))
        assert Pc.same(tuple(np.ascontiguousarray(a[b:b + 1]) for a in among), alone) is None, b


def _crowd(blockers, seed=0, P=600, near=512):
    """a pool of P discs of 1 cm: the first `near` of them beside the robot's lane, within the culling bound and out of its way, the rest far away; then `blockers`,
    {index: centre}, discs of 10 cm put in their place"""
    rng = np.random.default_rng(seed)
    at = np.empty((P, 2))
    at[:near] = np.column_stack([rng.uniform(0.7, 1.5, near), np.where(rng.random(near) < 0.5, rng.uniform(1.3, 1.6, near), rng.uniform(0.4, 0.7, near))])
    at[near:] = rng.uniform(5.0, 6.0, (P - near, 2))
    rad = np.full(P, 0.01)
    for p, centre in blockers.items():
        at[p], rad[p] = centre, 0.1
    return Cc.discs(at, rad)


def test_a_pool_of_600_on_either_side_of_the_culled_lists_capacity(env, solvers):
    """the car-like footprint from (1, 1, 0) at 1 m/s, four sub-steps of 0.1 s: a disc at (1.75, 1) blocks the second sub-step, one at (1.95, 1) the fourth.  512 small
    discs within the culling bound fill the list exactly (eight chunks of 64), so that an entry from 512 on is tested from global memory.  The lowest blocking p of the
    first blocked sub-step is reported wherever it lies."""
    m, torch = env
    lib = Pc.harness()
    assert lib.plh_list_cap() == 512 and lib.plh_threads() == 64
    s = solvers(1)
    first, second = (1.75, 1.0), (1.95, 1.0)
    for blockers, want in (({100: first}, [1, 1, 100]), ({550: first}, [1, 1, 550]), ({100: second, 550: first}, [1, 1, 550]), ({100: first, 550: first}, [1, 1, 100]),
                           ({511: second, 512: second, 599: second}, [3, 3, 511]), ({512: second, 599: first}, [1, 1, 599]), ({}, [4, -1, -1])):
        c = Pc.Case(f"blockers {sorted(blockers)}", Cc.room(), (1.0, 1.0, 0.0), (1.0, 0.0, 0.0), n_sub=4, pool=_crowd(blockers), self_index=[7])
        kept = [lib.plh_kept(Pc.d_(c.dpar()), Pc.i_(c.ipar()), Pc.d_(c.cmd), Pc.d_(c.pose), None, c.P, c.V, Pc.i_(c.pnv), Pc.d_(c.pv), Pc.d_(c.pr), 7, p) for p in range(c.P)]
        assert sum(kept[:512]) == 511 and kept[7] == 0 and sum(kept[512:]) == sum(p >= 512 for p in blockers), c.name          # (entry 7 is the robot's own)
        got, host = _device(s, torch, c), Pc.host_step(c)
        assert Pc.same(got, host) is None, (c.name, Pc.same(got, host))
        assert host[3][0, :3].tolist() == want, (c.name, host[3])
    # without the robot's own entry the near ones are 512 and fill the list to the brim; one more kept entry and the chunk that holds it goes to the tail as a whole
    for blockers, want in (({550: first}, [1, 1, 550]), ({500: second, 520: first}, [1, 1, 520])):
        c = Pc.Case(f"no self, blockers {sorted(blockers)}", Cc.room(), (1.0, 1.0, 0.0), (1.0, 0.0, 0.0), n_sub=4, pool=_crowd(blockers))
        got, host = _device(s, torch, c), Pc.host_step(c)
        assert Pc.same(got, host) is None and host[3][0, :3].tolist() == want, (c.name, host[3])


def test_an_entry_just_inside_the_culling_bound_blocks_and_one_just_outside_is_dropped(env, solvers):
    """a footprint of one segment along the motion, its tip 0.5 m ahead: after four sub-steps of 0.1 m the tip is 0.9 m from the start, which is the culling radius
    (circumradius + travel) itself.  A disc of 1 cm centred 0.905 m ahead is met in the last sub-step and lies inside the bound by 5 mm; the same disc 0.92 m ahead lies
    outside it and is never met."""
    m, torch = env
    lib = Pc.harness()
    s = solvers(1)
    for ahead, kept, want in ((0.905, 1, [3, 3, 2]), (0.92, 0, [4, -1, -1])):
        pool = Cc.discs([(5.0, 5.0), (5.0, 5.1), (1.0 + ahead, 1.0)], [0.01] * 3)
        c = Pc.Case(f"{ahead} m ahead", None, (1.0, 1.0, 0.0), (1.0, 0.0, 0.0), n_sub=4, footprint=[(0.0, 0.0), (0.5, 0.0)], pool=pool)
        assert lib.plh_kept(Pc.d_(c.dpar()), Pc.i_(c.ipar()), Pc.d_(c.cmd), Pc.d_(c.pose), None, c.P, c.V, Pc.i_(c.pnv), Pc.d_(c.pv), Pc.d_(c.pr), -1, 2) == kept
        got, host = _device(s, torch, c), Pc.host_step(c)
        assert Pc.same(got, host) is None and host[3][0, :3].tolist() == want, (c.name, host[3])


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solvers, scripted):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    solver = solvers(3)
    c = [c for c, _ in scripted if c.name == "origin off zero, sixteen vertices"][0].variant(vel=np.zeros((2, 3)))
    pose, vel, stall, info = c.state()
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    pool = A.MpcPool(c.P, c.pnv.ctypes.data, c.pv.ctypes.data, c.pr.ctypes.data, None)
    inf, nan = math.inf, math.nan

    def prm(**kw):
        q = c.struct()
        for k, v in kw.items():
            if k in ("map_origin", "v_min", "v_max", "a_max"):
                v = (C.c_double * len(v))(*v)
            if k == "vertex":
                q.footprint[v[0]][v[1]] = v[2]
                continue
            setattr(q, k, v)
        return q

    def call(fn, B=c.B, grid=c.grid, p=c.struct(), cmd=c.cmd, pool=pool, out=pose):
        return fn(solver._h, B, a(grid), None if p is None else C.byref(p), a(cmd), None if pool is None else C.byref(pool), a(c.self_index), a(out), a(vel), a(stall), a(info))

    for fn in (lib.mpc_plant_step, lib.mpc_plant_step_device):          # refused before anything is read: host arrays do for both
        for bad in (dict(p=None), dict(cmd=None), dict(out=None)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"mpc_plant_step: null argument" in lib.mpc_last_error(), bad
        for v in (0, -1, 65):
            assert call(fn, p=prm(n_substeps=v)) == A.MPC_EINVAL and b"n_substeps" in lib.mpc_last_error(), v
        for v in (0.0, -0.1, nan, inf):
            assert call(fn, p=prm(interval=v)) == A.MPC_EINVAL and b"interval" in lib.mpc_last_error(), v
        for v in (-1, 4):
            assert call(fn, p=prm(drive=v)) == A.MPC_EINVAL and b"drive has to be" in lib.mpc_last_error(), v
        for v in (0.0, -0.4, nan, inf):
            assert call(fn, p=prm(drive=A.DRIVE_CAR_REAR, wheelbase=v)) == A.MPC_EINVAL and b"wheelbase" in lib.mpc_last_error(), v
            assert call(fn, p=prm(drive=A.DRIVE_OMNI, wheelbase=v), B=0) == A.MPC_OK          # (the other drives do not read it)
        for v in (1, 17, -2):
            assert call(fn, p=prm(n_footprint=v)) == A.MPC_EINVAL and b"n_footprint" in lib.mpc_last_error(), v
        for v in ((0, 0, nan), (15, 1, inf)):
            assert call(fn, p=prm(vertex=v)) == A.MPC_EINVAL and b"footprint vertex" in lib.mpc_last_error(), v
        for bad in (dict(map_size_x=0), dict(map_size_y=-1), dict(map_size_x=1 << 16, map_size_y=1 << 15)):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and b"bad map size" in lib.mpc_last_error(), bad
            assert call(fn, p=prm(**bad), grid=None, B=0) == A.MPC_OK          # (the map's geometry is read with a map)
        for v in (0.0, -0.05, nan, inf):
            assert call(fn, p=prm(map_resolution=v)) == A.MPC_EINVAL and b"map_resolution" in lib.mpc_last_error(), v
        assert call(fn, p=prm(map_origin=(0.0, nan))) == A.MPC_EINVAL and b"map_origin" in lib.mpc_last_error()
        for v in (0, -1, 255):
            assert call(fn, p=prm(block_threshold=v)) == A.MPC_EINVAL and b"block_threshold" in lib.mpc_last_error(), v
        assert call(fn, p=prm(map_resolution=0.0001)) == A.MPC_EINVAL and b"350 cells" in lib.mpc_last_error()          # edges of 6 .. 8 cm are 600 .. 800 cells of 0.1 mm
        for v in ((1.0, -0.1, 1.0), (nan, 1.0, 1.0)):
            assert call(fn, p=prm(a_max=v)) == A.MPC_EINVAL and b"a_max" in lib.mpc_last_error(), v
        for lo, hi in (((0.5, -inf, -inf), (0.4, inf, inf)), ((-inf, -inf, nan), (inf, inf, inf)), ((-inf, -inf, -inf), (inf, nan, inf))):
            assert call(fn, p=prm(v_min=lo, v_max=hi)) == A.MPC_EINVAL and b"v_min" in lib.mpc_last_error(), (lo, hi)
        assert call(fn, pool=A.MpcPool(-1, None, None, None, None)) == A.MPC_EINVAL and b"P is negative" in lib.mpc_last_error()
        assert call(fn, pool=A.MpcPool(2, None, c.pv.ctypes.data, None, None)) == A.MPC_EINVAL and b"n_vertices and vertices" in lib.mpc_last_error()
        assert call(fn, B=9) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
    # a refused call changes nothing
    for x, y in zip(c.state(), (pose, vel, stall, info)):
        assert x.tobytes() == y.tobytes()
    assert call(lib.mpc_plant_step, B=0) == A.MPC_OK and (stall == Pc.IPOISON).all() and pose.tobytes() == c.pose.tobytes()
    # what is taken: a pool of no entries, no pool at all, no map
    assert call(lib.mpc_plant_step, pool=A.MpcPool(0, None, None, None, None)) == A.MPC_OK and (stall != Pc.IPOISON).all() and (info[:, 2] < 0).all()
    assert call(lib.mpc_plant_step, pool=None, grid=None) == A.MPC_OK and (info[:, 0] == c.n_sub).all()


def test_two_robots_driven_head_on_stall_on_each_other(env, solvers):
    """two diff-drive boxes of 0.25 m (ex/stage/robots/diff_drive_robot.inc) 0.8 m apart, facing each other at 0.5 m/s; one sub-step of 0.1 s per call, and behind every
    call mpc_fleet_pool_device makes the pool of the two, discs of 0.125 m, from the new poses.  They close in by 0.1 m a call and then stall, each reporting the
    other's index; neither outline has advanced more than one sub-step's travel into the other's disc.  Every call equals the host build."""
    m, torch = env
    s = solvers(1)
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    half, speed, calls = 0.125, 0.5, 9
    box = [(-half, -half), (half, -half), (half, half), (-half, half)]
    pose0 = np.array([[0.8, 1.0, 0.0], [1.6, 1.0, -math.pi]])
    c = Pc.Case("head on", Cc.room(), pose0, (speed, 0.0, 0.0), footprint=box, pool=Cc.discs(pose0[:, :2], [half, half]), self_index=[0, 1])
    d_map, d_cmd, d_pose, d_self = T(c.grid), T(c.cmd), T(c.pose), T(c.self_index)
    d_nv, d_pv, d_pr, d_vl = T(np.zeros(2, np.int32)), T(np.zeros((2, 1, 2))), T(np.zeros(2)), T(np.zeros((2, 2)))
    d_stall, d_info = T(np.full(2, Pc.IPOISON, np.int32)), T(np.full((2, 4), Pc.IPOISON, np.int32))
    torch.cuda.synchronize()
    s.fleet_pool_device(2, d_pose.data_ptr(), None, None, None, half, d_nv.data_ptr(), d_pv.data_ptr(), d_pr.data_ptr(), d_vl.data_ptr())
    host_pose, log = pose0.copy(), []
    for k in range(calls):
        s.plant_step_device(2, c.struct(), d_cmd.data_ptr(), d_pose.data_ptr(), map_cost=d_map.data_ptr(), pool=(2, d_nv.data_ptr(), d_pv.data_ptr(), d_pr.data_ptr()),
                            self_index=d_self.data_ptr(), stall=d_stall.data_ptr(), info=d_info.data_ptr())
        s.fleet_pool_device(2, d_pose.data_ptr(), None, None, None, half, d_nv.data_ptr(), d_pv.data_ptr(), d_pr.data_ptr(), d_vl.data_ptr())
        s.synchronize()
        host = Pc.host_step(c.variant(pose=host_pose, pool=Cc.discs(host_pose[:, :2], [half, half])))
        got = (d_pose.cpu().numpy(), None, d_stall.cpu().numpy(), d_info.cpu().numpy())
        assert Pc.same(got, host) is None, (k, Pc.same(got, host))
        assert d_pv.cpu().numpy()[:, 0].tobytes() == np.ascontiguousarray(got[0][:, :2]).tobytes()
        host_pose = host[0]
        log.append((got[2].tolist(), got[3][:, 2].tolist()))
    stalled = [k for k, (st, _) in enumerate(log) if st == [1, 1]]
    assert [st for st, _ in log[:3]] == [[0, 0]] * 3 and len(stalled) >= 3 and stalled == list(range(stalled[0], calls)), log
    assert all(who == [1, 0] for _, who in log[stalled[0]:]), log
    # the front of robot 0 against the disc of robot 1 and the other way round: not more than one sub-step's travel inside
    gap = (host_pose[1, 0] - half) - (host_pose[0, 0] + half)
    assert -speed * c.interval - 1e-12 <= gap <= 2 * speed * c.interval, gap
    assert host_pose[0, 0] > pose0[0, 0] + 0.2 and host_pose[1, 0] < pose0[1, 0] - 0.2


def test_the_closed_loop_runs_on_device_pointers_with_no_host_step(env):
    """The scene of tests/test_gpu_scan_cast.py::test_only_the_cast_scan_sees_the_box_and_the_path_goes_round_it: the planner's static map is empty, the map the laser
    is cast through -- and the plant drives on -- has a box of 0.3 m x 0.3 m, 1.25 m ahead of the robot and 0.1 m off its line to the goal.  Six cycles of
    scan_cast_device -> costmap_window_device -> costmap_scans_device -> mpc_costmap_to_obstacles_device -> mpc_step_batch_device -> commands_device ->
    plant_step_device -> fleet_pool_device on the solver's stream: the pose never leaves the device, nothing is uploaded between the first cycle and the last (the
    stream is synchronised once a cycle to copy the results OUT for this test).  The same loop with the plant done by the host build (command and pose read back, the
    new pose uploaded) agrees bit for bit, cycle by cycle.  The stall count is 0 throughout, every solved path keeps min_obstacle_dist from every obstacle less the 1e-6
    that file allows a converged solve, and the robot ends nearer its goal than it began."""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    n, size, res, O, beams, dmin, cycles = 20, 80, 0.05, 96, 360, 0.2, 6
    box = (2.25, 2.35, 2.55, 2.65)
    goal = np.array([[4.0, 2.4, 0.0]])
    start = np.array([[1.0, 2.4, 0.0]])
    planner_map = np.zeros((96, 96), np.uint8)
    world = planner_map.copy()
    world[47:53, 45:51] = 254
    half = 0.1
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    f64, i32, u8, f32 = torch.float64, torch.int32, torch.uint8, torch.float32
    V = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    plant = Pc.Case("closed loop", world, start, (0.0, 0.0, 0.0), vel=np.zeros((1, 3)), a_max=(2.0, 2.0, 3.0), n_sub=3, interval=0.1,
                    footprint=[(-half, -half), (half, -half), (half, half), (-half, half)], pool=Cc.discs(start[:, :2], [half]), self_index=[0])

    def loop(plant_on_host):
        s = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=O, max_vertices=1, max_obstacle_rows=16, min_obstacle_dist=dmin), max_batch=1)
        wp = s.window_params(0.05, planner_map.shape)
        cp = s.cast_params(0.05, world.shape, angle_min=-math.pi, angle_increment=2 * math.pi / beams, range_max=10.0)
        sp = s.scan_params(angle_min=-math.pi, angle_increment=2 * math.pi / beams, range_min=0.05, range_max=10.0, obstacle_range=3.0, raytrace_range=4.0, track_unknown=1)
        pp = plant.struct()
        dplanner, dworld, dgoal, dpose, dvel, dself = T(planner_map), T(world), T(goal), T(start), Z((1, 3), f64), Z((1,), i32)
        cost, origin, layer, cell = Z((1, size, size), u8), Z((1, 2), f64), Z((1, size, size), u8), Z((1, 2), i32)
        ranges, hit, cinfo = Z((1, beams), f32), Z((1, beams), i32), Z((1, 4), i32)
        sinfo = Z((1, 4), i32)
        keep = torch.ones((1,), dtype=i32, device=dev)          # the first cycle starts its layer (NULL), the others keep it
        ob = [Z((1,), i32), Z((1, O), i32), Z((1, O, 1, 2), f64)]
        dropped = Z((1,), i32)
        x, u, dt, st, it = Z((1, n, 3), f64), Z((1, n, 2), f64), Z((1,), f64), Z((1,), i32), Z((1,), i32)
        cmd, result, stall, pinfo = Z((1, 3), f64), Z((1,), i32), Z((1,), i32), Z((1, 4), i32)
        p_nv, p_pv, p_pr, p_vl = Z((1,), i32), Z((1, 1, 2), f64), Z((1,), f64), Z((1, 2), f64)
        pool = lambda: (1, p_nv.data_ptr(), p_pv.data_ptr(), p_pr.data_ptr())
        torch.cuda.synchronize()
        s.fleet_pool_device(1, dpose.data_ptr(), None, None, None, half, p_nv.data_ptr(), p_pv.data_ptr(), p_pr.data_ptr(), p_vl.data_ptr())
        out = []
        for k in range(cycles):
            s.scan_cast_device(1, dworld.data_ptr(), cp, dpose.data_ptr(), beams, ranges.data_ptr(), pool=pool(), self_index=dself.data_ptr(), hit=hit.data_ptr(), info=cinfo.data_ptr())
            s.costmap_window_device(1, dplanner.data_ptr(), wp, dpose.data_ptr(), size, size, res, cost.data_ptr(), origin.data_ptr())
            s.costmap_scans_device(1, sp, dpose.data_ptr(), ranges.data_ptr(), beams, keep.data_ptr() if k else None, size, size, res, layer.data_ptr(), cell.data_ptr(), cost.data_ptr(),
                                   sinfo.data_ptr())
            rc = s._lib.mpc_costmap_to_obstacles_device(s._h, 1, V(cost), size, size, res, V(origin), V(dpose), 1.5, V(ob[0]), V(ob[1]), V(ob[2]), V(dropped))
            assert rc == 0, s._lib.mpc_last_error()
            rc = s._lib.mpc_step_batch_device(s._h, 1, V(dpose), V(dgoal), None, None, None, None, None, C.byref(A.MpcObstacles(*(t.data_ptr() for t in ob), None, None)), 3, 0,
                                              3, n, 0.1, V(x), V(u), V(dt), V(st), V(it))
            assert rc == 0, s._lib.mpc_last_error()
            s.commands_device(1, u.data_ptr(), st.data_ptr(), None, None, cmd.data_ptr(), result.data_ptr())
            before = None
            if plant_on_host:
                s.synchronize()
                before = dpose.cpu().numpy()
                h_pose, h_vel, h_stall, h_info = Pc.host_step(plant.variant(pose=before, cmd=cmd.cpu().numpy(), vel=dvel.cpu().numpy(), pool=Cc.discs(p_pv.cpu().numpy()[:, 0], [half])))
                dpose.copy_(T(h_pose)); dvel.copy_(T(h_vel)); stall.copy_(T(h_stall)); pinfo.copy_(T(h_info))
                torch.cuda.synchronize()
            else:
                s.plant_step_device(1, pp, cmd.data_ptr(), dpose.data_ptr(), map_cost=dworld.data_ptr(), pool=pool(), self_index=dself.data_ptr(), vel=dvel.data_ptr(),
                                    stall=stall.data_ptr(), info=pinfo.data_ptr())
            s.fleet_pool_device(1, dpose.data_ptr(), None, None, None, half, p_nv.data_ptr(), p_pv.data_ptr(), p_pr.data_ptr(), p_vl.data_ptr())
            s.synchronize()
            no, nv, vt = (t.cpu().numpy() for t in ob)
            out.append(dict(pose=dpose.cpu().numpy(), vel=dvel.cpu().numpy(), cmd=cmd.cpu().numpy(), stall=int(stall.cpu().numpy()[0]), info=pinfo.cpu().numpy()[0].tolist(),
                            status=int(st.cpu().numpy()[0]), result=int(result.cpu().numpy()[0]), x=x.cpu().numpy(), u=u.cpu().numpy(), dt=dt.cpu().numpy(), obstacles=(no, nv, vt),
                            cast=cinfo.cpu().numpy()[0].tolist(), pool=p_pv.cpu().numpy().copy()))
        # the start of every cycle's path is the pose the cycle began at: the last cycle's new pose, or the start
        begins = [start] + [c["pose"] for c in out[:-1]]
        for c, at in zip(out, begins):
            ev = s.evaluate(at, goal, c["x"], c["u"], c["dt"], obstacles=c["obstacles"])
            c["clearance"], c["began"] = float(ev.clearance[0]), at
        s.close()
        return out

    on_device, with_host_plant = loop(False), loop(True)
    inside = lambda p: bool(((p[:, 0] > box[0]) & (p[:, 0] < box[2]) & (p[:, 1] > box[1]) & (p[:, 1] < box[3])).any())
    for k, (a, b) in enumerate(zip(on_device, with_host_plant)):
        print(f"cycle {k}: pose {a['pose'][0].tolist()}, cmd {a['cmd'][0].tolist()}, stall {a['stall']}, plant info {a['info']}, status {a['status']}, obstacles "
              f"{int(a['obstacles'][0][0])}, clearance {a['clearance']:.6f}")
        for name in ("cmd", "pose", "vel", "x", "u", "pool"):
            assert a[name].tobytes() == b[name].tobytes(), (k, name, a[name], b[name])
        assert (a["stall"], a["info"], a["status"]) == (b["stall"], b["info"], b["status"]), k
    for k, c in enumerate(on_device):
        assert c["stall"] == 0 and c["info"] == [3, -1, -1, -1] and c["status"] == 0, (k, c["stall"], c["info"], c["status"])
        assert c["cast"][0] > 0 and c["cast"][1] == 0 and int(c["obstacles"][0][0]) >= 1          # the laser sees the box and not the robot's own disc
        assert c["clearance"] >= dmin - 1e-6 and not inside(c["x"][0]), (k, c["clearance"])
        assert c["pool"][0, 0].tobytes() == np.ascontiguousarray(c["pose"][0, :2]).tobytes()
    dist = lambda p: float(np.hypot(*(p[0, :2] - goal[0, :2])))
    assert dist(on_device[-1]["pose"]) < dist(start)
