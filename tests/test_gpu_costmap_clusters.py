"""GPU tests (-m gpu) of mpc_costmap_to_polygons* (mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp, include/mpc_costmap_clusters.h): costmap cells clustered into
points, lines and convex polygons for a batch on the device.

The yardstick is the host build of the same header (tests/host_harness/costmap_clusters_host.cpp through tests/_cluster_cases.py), which
tests/test_costmap_clusters_host.py holds to an independent Python restatement: the device has to equal it BIT FOR BIT in every array -- containers, counts and info -- on
every scripted case, with a poison pattern left in everything it does not write.  Then: the host-pointer entry equals the device entry; the scratch is reused and regrown
across geometries; the argument checks; and the cover is conservative -- along the solver's converged trajectory under the polygon container, the clearance to the point
container of the same map is at least the clearance to the polygons, minus 1e-12 m (geometry: the hull contains the cell centres; the margin is three times the 2.9e-14
relative bound profiles/r12_evaluate.md measured for the evaluation, at 10 m)."""
import ctypes as C
import math

import numpy as np
import pytest

import _cluster_cases as K

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
            made[O, V] = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=O, max_vertices=V, cutoff_dist=2.5), max_batch=8)
        return made[O, V]
    yield get
    for s in made.values():
        s.close()


@pytest.fixture(scope="module")
def scripted():
    """(case, the host build's result) of every scripted case, computed once and left unchanged"""
    return [(c, K.host_polygons(c)) for c in K.cases()]


def _params(c):
    from mpc_local_planner_amd._abi import MpcClusterParams
    return MpcClusterParams(c.behind, c.link)


def _device(s, torch, c):
    """mpc_costmap_to_polygons_device on torch tensors: the tuple of K.host_polygons"""
    dev = torch.device("cuda", 0)
    T = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()
    cost, origin, pose = T(c.cost), T(c.origin), T(c.pose)
    out = [T(a) for a in c.container()] + [T(np.full(c.B, -1, np.int32)), T(np.full((c.B, 4), -1, np.int32))]
    torch.cuda.synchronize()
    s.costmap_to_polygons_device(c.B, ptr(cost), c.W, c.H, c.res, ptr(origin), ptr(pose), _params(c), *map(ptr, out))
    s.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def test_device_equals_the_host_build_bit_for_bit_on_every_scripted_case(env, solvers, scripted):
    """every array, the poison pattern of the slots and vertices that are not written included"""
    m, torch = env
    assert len(scripted) >= 30 and max(c.B for c, _ in scripted) <= 8 and max(max(c.W, c.H) for c, _ in scripted) <= 64
    for c, host in scripted:
        got = _device(solvers(c.O, c.V), torch, c)
        assert K.same(got, host) is None, (c.name, K.same(got, host))
        for b in range(c.B):          # untouched slots keep the poison
            n = int(got[0][b])
            assert (got[1][b, n:] == K.ISENTINEL).all() and (got[2][b, n:] == K.SENTINEL).all(), c.name


def test_random_maps_equal_the_host_build(env, solvers):
    m, torch = env
    for c in K.random_cases(24, seed=11):
        got, host = _device(solvers(c.O, c.V), torch, c), K.host_polygons(c)
        assert K.same(got, host) is None, (c.name, K.same(got, host))


def test_large_maps_equal_the_host_build(env, solvers):
    """more than 2^18 cells: linked through the labels in global memory, not the LDS bitmap; clusters wider than 4096 columns: box and line"""
    m, torch = env
    for c in K.large_cases():
        got, host = _device(solvers(c.O, c.V), torch, c), K.host_polygons(c)
        assert K.same(got, host) is None, (c.name, K.same(got, host))


def test_host_pointer_entry_equals_the_device_entry(env, solvers, scripted):
    """mpc_costmap_to_polygons clears its outputs first: what the device entry leaves as poison comes back as zeros"""
    m, torch = env
    for c, host in scripted:
        if not (c.radius and c.velocity):
            continue          # BatchSolver.costmap_to_polygons always gives the container both arrays
        got = solvers(c.O, c.V).costmap_to_polygons(c.cost, c.res, c.origin, c.pose, cluster_max_distance=math.sqrt(c.link) * c.res, behind_robot_dist=c.behind)
        want = [a.copy() for a in host]
        want[1][want[1] == K.ISENTINEL] = 0
        for a in want[2:5]:
            a[a == K.SENTINEL] = 0.0
        assert K.same(got, tuple(want)) is None, (c.name, K.same(got, tuple(want)))


def test_scratch_is_reused_and_regrown_across_geometries(env, scripted):
    """a fresh handle: a small geometry, a larger one with a larger batch (the scratch grows), then the first again (it is reused)"""
    m, torch = env
    from mpc_local_planner_amd import _abi as A
    by = {c.name: (c, h) for c, h in scripted}
    s = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5, max_obstacles=64, max_vertices=8), max_batch=8)
    assert s.last_costmap_ms() == 0.0
    for name in ("17 x 9", "33 x 33", "U, pose not a number", "17 x 9", "33 x 33"):
        c, host = by[name]
        assert (c.O, c.V) == (64, 8)
        assert K.same(_device(s, torch, c), host) is None, name
        assert s.last_costmap_ms() > 0.0
    s.close()


def test_argument_checks_return_the_stated_codes_and_change_nothing(env, solvers):
    m, torch = env
    from mpc_local_planner_amd import _abi as A, _lib
    lib = _lib.load()
    c = [c for c in K.cases() if c.name == "2 x 2 block"][0]
    s = solvers(c.O, c.V)
    before = c.container()
    no, nv, vt, rd, vl = c.container()
    dr, info = np.full(c.B, -1, np.int32), np.full((c.B, 4), -1, np.int32)
    a = lambda x: None if x is None else C.c_void_p(x.ctypes.data)
    p = _params(c)

    def call(fn, h=None, B=c.B, cost=c.cost, W=c.W, H=c.H, res=c.res, origin=c.origin, pose=c.pose, p=p, no=no, nv=nv, vt=vt):
        return fn(h or s._h, B, a(cost), W, H, res, a(origin), a(pose), None if p is None else C.byref(p), a(no), a(nv), a(vt), a(rd), a(vl), a(dr), a(info))

    for fn in (lib.mpc_costmap_to_polygons, lib.mpc_costmap_to_polygons_device):          # refused before anything is read: host arrays do for both
        for bad in (dict(cost=None), dict(origin=None), dict(pose=None), dict(p=None), dict(no=None), dict(nv=None), dict(vt=None)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"null argument" in lib.mpc_last_error(), bad
        for bad in (dict(W=0), dict(H=0), dict(W=2048, H=1024), dict(W=1 << 20, H=2), dict(res=0.0), dict(res=math.nan)):
            assert call(fn, **bad) == A.MPC_EINVAL and b"geometry" in lib.mpc_last_error(), bad
        for link in (0, -1, 65):
            assert call(fn, p=A.MpcClusterParams(1.5, link)) == A.MPC_EINVAL and b"link_dist_sq" in lib.mpc_last_error()
        assert call(fn, B=9) == A.MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
        assert call(fn, h=solvers(16, 3)._h) == A.MPC_EINVAL and b"max_vertices" in lib.mpc_last_error()
    none = m.BatchSolver(A.make_config(model=A.MODEL_UNICYCLE, n=5), max_batch=2)
    assert call(lib.mpc_costmap_to_polygons, h=none._h) == A.MPC_EINVAL and b"max_obstacles = 0" in lib.mpc_last_error()
    none.close()
    # a refused call changes nothing
    for x, y in zip(before, (no, nv, vt, rd, vl)):
        assert x.tobytes() == y.tobytes()
    assert (dr == -1).all() and (info == -1).all()
    assert call(lib.mpc_costmap_to_polygons, B=0) == A.MPC_OK and (no == K.ISENTINEL).all()
    assert call(lib.mpc_costmap_to_polygons) == A.MPC_OK and no.tolist() == [1] and nv[0, 0] == 4 and info.tolist() == [[4, 1, 0, 0]]


def test_cover_is_conservative_along_the_solved_trajectory(env):
    """Two walls and a blob on an 80 x 80 map, as polygons (two lines and a quadrilateral) and as points (one per cell).  The trajectory the solver converges to under the
    polygon container is evaluated against both: every cell centre lies in its cluster's hull, so the clearance to the points cannot be below the clearance to the
    polygons -- up to the evaluation's rounding, 1e-12 m."""
    m, torch = env
    res = 0.05
    cost = np.zeros((1, 80, 80), np.uint8)
    cost[0, 44:48, 40:42] = 254                                 # a blob whose nearest cell centre is ~0.17 m beside the straight line start -> goal
    cost[0, 20, 10:71] = 254                                    # a wall on either side, about 1 m away
    cost[0, 60, 10:71] = 254
    origin = np.array([[-0.5, -2.0]])
    x0 = np.array([[0.0, 0.0, 0.0]]); xf = np.array([[3.0, 0.1, 0.0]])
    up, dtp = np.zeros((1, 2)), np.array([0.2])
    poly = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=8, max_vertices=8), max_batch=1)
    pts = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=256, max_vertices=1), max_batch=1)
    ob_poly = poly.costmap_to_polygons(cost, res, origin, x0)
    ob_pts = pts.costmap_to_obstacles(cost, res, origin, x0)
    assert ob_poly[6].tolist() == [[130, 3, 0, 0]] and ob_poly[0].tolist() == [3] and sorted(ob_poly[1][0, :3].tolist()) == [2, 2, 4] and ob_poly[5].tolist() == [0]
    assert ob_pts[0].tolist() == [130] and ob_pts[3].tolist() == [0]
    r = poly.solve(x0, xf, up, dtp, obstacles=ob_poly[:5])
    assert r.status[0] == 0
    c_poly = poly.evaluate(x0, xf, r.x, r.u, r.dt, up, dtp, obstacles=ob_poly[:5]).clearance[0]
    c_pts = pts.evaluate(x0, xf, r.x, r.u, r.dt, up, dtp, obstacles=ob_pts[:3]).clearance[0]
    print(f"clearance along the converged trajectory: to the polygons {c_poly!r} m, to the points {c_pts!r} m")
    assert math.isfinite(c_poly) and math.isfinite(c_pts) and c_poly > 0.0
    assert c_pts >= c_poly - 1e-12
    poly.close(); pts.close()
