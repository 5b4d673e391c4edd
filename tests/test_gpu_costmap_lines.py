"""GPU tests (-m gpu) of mpc_costmap_to_lines* (mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp, include/mpc_costmap_lines.h): costmap cells cut into line segments
along the walls for a batch on the device.

The yardstick is the host build of the same header (tests/host_harness/costmap_lines_host.cpp through tests/_line_cases.py), which tests/test_costmap_lines_host.py
holds to an independent Python restatement: the device has to equal it BIT FOR BIT in every array -- containers, counts and info -- on every scripted case, on random
maps and on either side of the kernel's LDS list capacity, with a poison pattern left in everything it does not write.  Then: the host-pointer entry equals the device
entry; the optional outputs may be NULL; the result does not depend on the batch; the scratch grows; the argument checks; and the step feeds a solve on device pointers
round an L-shaped wall whose convex hull would have closed the goal in."""
import ctypes as C
import math

import numpy as np
import pytest

import _cluster_cases as K
import _line_cases as L

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
    """one handle per container shape (max_obstacles, max_vertices) of the cases, made on demand"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    made = {}

    def get(O, V):
        if (O, V) not in made:
            made[O, V] = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=O, max_vertices=V, cutoff_dist=2.5), max_batch=8)
        return made[O, V]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def scripted():
    """(case, the host build's result) of every scripted case, computed once and left unchanged"""
    return [(c, L.host_lines(c)) for c in L.cases()]


def _params(c):
    from mpc_local_planner_amd._abi import MpcLineParams
    return MpcLineParams(c.behind, c.link, c.inl, c.mini, c.nh, c.rem)


def _device(s, torch, c, optional=True):
    """mpc_costmap_to_lines_device on torch tensors: the tuple of L.host_lines; optional False: radius, velocity, dropped and info are NULL and come back as None"""
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    cost, origin, pose = T(c.cost), T(c.origin), T(c.pose)
    out = [T(a) for a in c.container()] + [T(np.full(c.B, -1, np.int32)), T(np.full((c.B, 4), -1, np.int32))]
    if not optional:
        out[3:] = [None] * 4
    torch.cuda.synchronize()
    s.costmap_to_lines_device(c.B, ptr(cost), c.W, c.H, c.res, ptr(origin), ptr(pose), _params(c), *map(ptr, out))
    s.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solvers, scripted):
    """every array, the poison pattern of the slots and vertices that are not written included; then the same with the optional outputs NULL"""
    m, torch = env
    assert len(scripted) >= 26 and max(c.B for c, _ in scripted) <= 8
    for c, host in scripted:
        s = solvers(c.O, c.V)
        got = _device(s, torch, c)
        assert L.same(got, host) is None, (c.name, L.same(got, host))
        for b in range(c.B):          # untouched slots keep the poison
            n = int(got[0][b])
            assert (got[1][b, n:] == L.ISENTINEL).all() and (got[2][b, n:] == L.SENTINEL).all(), c.name
        assert s.last_costmap_ms() > 0.0
        bare = _device(s, torch, c, optional=False)
        assert L.same(bare[:3], host[:3]) is None and bare[3:] == (None,) * 4, c.name


def test_host_pointer_entry_equals_the_device_entry(env, solvers, scripted):
    """mpc_costmap_to_lines clears its outputs first: what the device entry leaves as poison comes back as zeros"""
    m, torch = env
    for c, host in scripted:
        if not (c.radius and c.velocity):
            continue          # BatchSolver.costmap_to_lines always gives the container both arrays
        got = solvers(c.O, c.V).costmap_to_lines(c.cost, c.res, c.origin, c.pose, _params(c))
        want = [a.copy() for a in host]
        want[1][want[1] == L.ISENTINEL] = 0
        for a in want[2:5]:
            a[a == L.SENTINEL] = 0.0
        assert L.same(got, tuple(want)) is None, (c.name, L.same(got, tuple(want)))


def test_random_maps_equal_the_host_build(env, solvers):
    m, torch = env
    lines = 0
    for c in L.random_cases(20, seed=11, size=64):
        got, host = _device(solvers(c.O, c.V), torch, c), L.host_lines(c)
        assert L.same(got, host) is None, (c.name, L.same(got, host))
        lines += int(host[6][0, 2])
    assert lines > 60


def test_a_cluster_on_either_side_of_the_lds_list_capacity_equals_the_host_build(env, solvers):
    """one cell fewer than the kernel's LDS list holds: the list is in LDS; one more: in the handle's scratch"""
    m, torch = env
    below, above = L.capacity_cases()
    for c, cells in ((below, L.list_cap() - 1), (above, L.list_cap() + 1)):
        got, host = _device(solvers(c.O, c.V), torch, c), L.host_lines(c)
        assert host[6][0, :2].tolist() == [cells, 1] and host[6][0, 2] > 10
        assert L.same(got, host) is None, (c.name, L.same(got, host))


def test_results_do_not_depend_on_the_batch(env, solvers, scripted):
    """the same map alone and as entry 5 of 7"""
    m, torch = env
    by = {c.name: (c, h) for c, h in scripted}
    for name in ("doorway", "L", "small U around the robot"):
        c, host = by[name]
        among = _device(solvers(c.O, c.V), torch, c.at(5, 7))
        assert L.same(tuple(np.ascontiguousarray(a[5:6]) for a in among), host) is None, name


def test_scratch_grows_when_a_later_call_needs_more(env, scripted):
    """a fresh handle: a small geometry, a larger one with a larger batch (the scratch grows), then the first again (it is reused)"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    by = {c.name: (c, h) for c, h in scripted}
    s = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=64, max_vertices=8), max_batch=8)
    assert s.last_costmap_ms() == 0.0
    for name in ("6 x 6 blob", "doorway", "pose not a number", "6 x 6 blob", "doorway"):
        c, host = by[name]
        assert (c.O, c.V) == (64, 8)
        assert L.same(_device(s, torch, c), host) is None, name
        assert s.last_costmap_ms() > 0.0
    # the polygon step shares the block
    poly = by["L"][0].polygons()
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = [T(a) for a in poly.container()] + [T(np.full(poly.B, -1, np.int32)), T(np.full((poly.B, 4), -1, np.int32))]
    cost, origin, pose = T(poly.cost), T(poly.origin), T(poly.pose)
    s.costmap_to_polygons_device(poly.B, cost.data_ptr(), poly.W, poly.H, poly.res, origin.data_ptr(), pose.data_ptr(), A.MpcClusterParams(poly.behind, poly.link), *(t.data_ptr() for t in out))
    s.synchronize()
    assert K.same(tuple(t.cpu().numpy() for t in out), K.host_polygons(poly)) is None
    s.close()


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solvers):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    c = [c for c in L.cases() if c.name == "6 x 6 blob"][0]
    s = solvers(c.O, c.V)
    before = c.container()
    no, nv, vt, rd, vl = c.container()
    dr, info = np.full(c.B, -1, np.int32), np.full((c.B, 4), -1, np.int32)
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    p = _params(c)
    big = np.zeros(1, np.uint8)          # a refused call reads nothing

    def call(fn, h=None, B=c.B, cost=c.cost, W=c.W, H=c.H, res=c.res, origin=c.origin, pose=c.pose, p=p, no=no, nv=nv, vt=vt):
        return fn(h or s._h, B, a(cost), W, H, res, a(origin), a(pose), None if p is None else C.byref(p), a(no), a(nv), a(vt), a(rd), a(vl), a(dr), a(info))

    def prm(**kw):
        q = _params(c)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for fn in (lib.mpc_costmap_to_lines, lib.mpc_costmap_to_lines_device):          # refused before anything is read: host arrays do for both
        for bad in (dict(cost=None), dict(origin=None), dict(pose=None), dict(p=None), dict(no=None), dict(nv=None), dict(vt=None)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"null argument" in lib.mpc_last_error(), bad
        for bad in (dict(W=0), dict(H=0), dict(W=2048, H=1024), dict(W=4097, H=2, cost=big), dict(W=2, H=4097, cost=big), dict(res=0.0), dict(res=math.nan)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"geometry" in lib.mpc_last_error(), bad
        for bad, word in ((dict(link_dist_sq=0), b"link_dist_sq"), (dict(link_dist_sq=65), b"link_dist_sq"), (dict(inlier_dist_sq=-1), b"inlier_dist_sq"),
                          (dict(inlier_dist_sq=65), b"inlier_dist_sq"), (dict(min_inliers=1), b"min_inliers"), (dict(n_hypotheses=0), b"n_hypotheses"),
                          (dict(n_hypotheses=65537), b"n_hypotheses"), (dict(remaining_outliers=-1), b"remaining_outliers")):
            assert call(fn, p=prm(**bad)) == A.MPC_EINVAL and word in lib.mpc_last_error(), bad
        assert call(fn, B=9) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
        assert call(fn, h=solvers(16, 3)._h) == A.MPC_EINVAL and b"max_vertices" in lib.mpc_last_error()
    none = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5), max_batch=2)
    assert call(lib.mpc_costmap_to_lines, h=none._h) == A.MPC_EINVAL and b"max_obstacles = 0" in lib.mpc_last_error()
    none.close()
    # a refused call changes nothing
    for x, y in zip(before, (no, nv, vt, rd, vl)):
        assert x.tobytes() == y.tobytes()
    assert (dr == -1).all() and (info == -1).all()
    assert call(lib.mpc_costmap_to_lines, B=0) == A.MPC_OK and (no == L.ISENTINEL).all()
    assert call(lib.mpc_costmap_to_lines) == A.MPC_OK and no.tolist() == [2] and info.tolist() == [[36, 1, 2, 0]]


def test_lines_feed_a_solve_round_an_l_shaped_wall(env):
    """An L-shaped wall on an 80 x 80 map at 0.05 m per cell: mpc_costmap_to_lines_device feeds mpc_solve_batch_device on device pointers, a unicycle at n = 20 drives
    round the end of the wall into its free corner.  The solve converges, and the clearance of its answer to the POINT-path obstacles of the same map (one per cell) is
    at least min_obstacle_dist - 2 sqrt(inlier_dist_sq) resolution: a kept cell lies within 2 sqrt(inlier_dist_sq) cells of an emitted obstacle.  Through
    mpc_costmap_to_polygons_device the same wall is one triangle, and the goal lies strictly inside it: the geometric fact, not a solver outcome."""
    m, torch = env
    dev = torch.device("cuda", 0)
    res, n = 0.05, 20
    cost = np.zeros((1, 80, 80), np.uint8)
    cost[0, 44:61, 30] = 254                                    # the wall x = 1.025 m from y = 0.225 m up to the corner at y = 1.025 m
    cost[0, 60, 30:71] = 254                                    # the wall y = 1.025 m from the corner to x = 3.025 m
    origin = np.array([[-0.5, -2.0]])
    x0 = np.array([[0.0, -0.5, 0.0]]); xf = np.array([[1.525, 0.625, 0.0]])          # the goal: the centre of cell (40, 52)
    up, dtp = np.zeros((1, 2)), np.array([0.2])
    line = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=8, max_vertices=4), max_batch=1)
    pts = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=256, max_vertices=1), max_batch=1)
    prm = line.line_params(res)
    assert (prm.link_dist_sq, prm.inlier_dist_sq, prm.min_inliers, prm.n_hypotheses, prm.remaining_outliers) == (64, 9, 10, 1500, 3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dcost, dorigin, dpose = T(cost), T(origin), T(x0)
    O, V = 8, 4
    ob = [torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, O), dtype=torch.int32, device=dev), torch.zeros((1, O, V, 2), dtype=torch.float64, device=dev),
          torch.zeros((1, O), dtype=torch.float64, device=dev), torch.zeros((1, O, 2), dtype=torch.float64, device=dev)]
    dr, info = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 4), dtype=torch.int32, device=dev)
    dx0, dxf, dup, ddtp = T(x0), T(xf), T(up), T(dtp)
    xo, uo = torch.empty((1, n, 3), dtype=torch.float64, device=dev), torch.empty((1, n, 2), dtype=torch.float64, device=dev)
    do, st, it = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    obp = tuple(t.data_ptr() for t in ob)
    line.costmap_to_lines_device(1, dcost.data_ptr(), 80, 80, res, dorigin.data_ptr(), dpose.data_ptr(), prm, *obp, dr.data_ptr(), info.data_ptr())
    line.solve_device(1, dx0.data_ptr(), dxf.data_ptr(), dup.data_ptr(), ddtp.data_ptr(), None, None, None, xo.data_ptr(), uo.data_ptr(), do.data_ptr(), st.data_ptr(), it.data_ptr(),
                      obstacles=obp)
    line.synchronize()
    assert info.cpu().numpy().tolist() == [[57, 1, 2, 0]] and ob[0].cpu().numpy().tolist() == [2] and dr.cpu().numpy().tolist() == [0]
    assert st.cpu().numpy()[0] == 0, (st.cpu().numpy(), it.cpu().numpy())
    x, u, dt = xo.cpu().numpy(), uo.cpu().numpy(), do.cpu().numpy()
    ob_pts = pts.costmap_to_obstacles(cost, res, origin, x0)
    assert ob_pts[0].tolist() == [57] and ob_pts[3].tolist() == [0]
    c_pts = pts.evaluate(x0, xf, x, u, dt, up, dtp, obstacles=ob_pts[:3]).clearance[0]
    c_line = line.evaluate(x0, xf, x, u, dt, up, dtp, obstacles=tuple(t.cpu().numpy() for t in ob)).clearance[0]
    bound = line.cfg.min_obstacle_dist - 2.0 * math.sqrt(prm.inlier_dist_sq) * res
    print(f"clearance along the converged trajectory: to the lines {c_line!r} m, to the points {c_pts!r} m, bound {bound!r} m; end {x[0, -1].tolist()}, {int(it.cpu().numpy()[0])} iterations")
    assert math.isfinite(c_pts) and c_pts >= bound
    # the polygon step on the same scene: one triangle, the goal strictly inside it
    poly = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=8, max_vertices=8), max_batch=1)
    pob = [torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 8), dtype=torch.int32, device=dev), torch.zeros((1, 8, 8, 2), dtype=torch.float64, device=dev)]
    poly.costmap_to_polygons_device(1, dcost.data_ptr(), 80, 80, res, dorigin.data_ptr(), dpose.data_ptr(), poly.cluster_params(res), *(t.data_ptr() for t in pob))
    poly.synchronize()
    assert pob[0].cpu().numpy().tolist() == [1] and pob[1].cpu().numpy()[0, 0] == 3
    tri = pob[2].cpu().numpy()[0, 0, :3]
    for k in range(3):
        o, a = tri[k], tri[(k + 1) % 3]
        assert (a[0] - o[0]) * (xf[0, 1] - o[1]) - (a[1] - o[1]) * (xf[0, 0] - o[0]) > 0.0
    line.close(); pts.close(); poly.close()
