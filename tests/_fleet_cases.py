"""Shared by tests/test_fleet_obstacles_host.py and tests/test_gpu_fleet_obstacles.py: the host build of mpc_local_planner_amd/csrc/mpc_fleet_obstacles.hpp
(tests/host_harness/fleet_obstacles_host.cpp, g++ -ffp-contract=off) behind ctypes, the scripted cases, and a numpy restatement of the two rules written from
include/mpc_fleet.h, not from the header's code: np.lexsort on (p, key) for the selection, products and sums as separate numpy operations.

A CASE is one call: one pool, one parameter set, B robots with their containers as they are before the call."""
import ctypes as C
import math

import numpy as np

import _harness

_harness.SHARED.setdefault("fleet_obstacles_host", ("libmpc_fleet_obstacles.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
SENTINEL = -7.25          # what unused container slots hold before a call: the call must leave it there
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("fleet_obstacles_host"))
        lib.fob_select.restype, lib.fob_select.argtypes = None, [C.c_int, C.c_int, ip, dp, dp, dp, C.c_int, C.c_int, dp, ip, C.c_double, C.c_double, C.c_int, ip, ip, dp, dp, dp, ip, ip]
        lib.fob_pool.restype, lib.fob_pool.argtypes = None, [C.c_int, dp, dp, C.c_int, dp, ip, C.c_double, dp, C.c_int, C.c_int, ip, dp, dp, dp]
        _lib = lib
    return _lib


def d_(a):
    return None if a is None else a.ctypes.data_as(dp)


def i_(a):
    return None if a is None else a.ctypes.data_as(ip)


class Case:
    """pool: n_vertices [P], vertices [P][V][2], radius [P] or None, velocity [P][2] or None; robots: pose [B][3], self_index [B] or None, n_obstacles [B] before the call"""

    def __init__(self, name, O, V, pool_nv, pool_v, pool_r, pool_vel, pose, n_obstacles=None, self_index=None, reach=2.5, min_speed=0.001, append=1, radius=True, velocity=True):
        f = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
        self.name, self.O, self.V = name, int(O), int(V)
        self.pool_nv = np.ascontiguousarray(pool_nv, dtype=np.int32).reshape(-1)
        self.P = P = len(self.pool_nv)
        self.pool_v, self.pool_r, self.pool_vel = f(pool_v, (P, V, 2)), f(pool_r, (P,)), f(pool_vel, (P, 2))
        self.pose = f(pose, (-1, 3))
        self.B = B = len(self.pose)
        self.self_index = None if self_index is None else np.ascontiguousarray(self_index, dtype=np.int32).reshape(B)
        self.n_obstacles = np.zeros(B, np.int32) if n_obstacles is None else np.ascontiguousarray(n_obstacles, dtype=np.int32).reshape(B)
        self.reach, self.min_speed, self.append = float(reach), float(min_speed), int(append)
        self.radius = radius or pool_r is not None          # does the container have the array?
        self.velocity = velocity or pool_vel is not None

    def container(self):
        """fresh copies of what the container holds before the call: (n_obstacles, n_vertices, vertices, radius or None, velocity or None); the slots a robot already
        uses hold recognisable entries, every other word the sentinel"""
        B, O, V = self.B, self.O, self.V
        nv = np.full((B, O), -3, np.int32)
        vt = np.full((B, O, V, 2), SENTINEL)
        rd = np.full((B, O), SENTINEL) if self.radius else None
        vl = np.full((B, O, 2), SENTINEL) if self.velocity else None
        for b in range(B):
            for o in range(max(0, min(int(self.n_obstacles[b]), O))):
                nv[b, o] = 1
                vt[b, o, 0] = (100.0 + int(self.n_obstacles[b]), 200.0 + o)          # (not the robot's index: a robot's result must not depend on its place in the batch)
                if rd is not None:
                    rd[b, o] = 0.5 + o
                if vl is not None:
                    vl[b, o] = (0.25, -0.5 - o)
        return self.n_obstacles.copy(), nv, vt, rd, vl

    def take(self, rows):
        """the same call for a subset / another order of the robots"""
        c = Case(self.name, self.O, self.V, self.pool_nv, self.pool_v, self.pool_r, self.pool_vel, self.pose[rows], self.n_obstacles[rows],
                 None if self.self_index is None else self.self_index[rows], self.reach, self.min_speed, self.append, self.radius, self.velocity)
        return c


def host_select(case):
    """the case through the host build: (n_obstacles, n_vertices, vertices, radius, velocity, dropped, n_taken)"""
    no, nv, vt, rd, vl = case.container()
    dr, tk = np.full(case.B, -1, np.int32), np.full(case.B, -1, np.int32)
    harness().fob_select(case.B, case.P, i_(case.pool_nv), d_(case.pool_v), d_(case.pool_r), d_(case.pool_vel), case.V, case.O, d_(case.pose), i_(case.self_index), case.reach,
                         case.min_speed, case.append, i_(no), i_(nv), d_(vt), d_(rd), d_(vl), i_(dr), i_(tk))
    return no, nv, vt, rd, vl, dr, tk


def numpy_select(case):
    """the rule of include/mpc_fleet.h restated with numpy, robot by robot"""
    no, nv, vt, rd, vl = case.container()
    dr, tk = np.zeros(case.B, np.int32), np.zeros(case.B, np.int32)
    P, V, O = case.P, case.V, case.O
    valid = np.arange(V)[None, :] < np.minimum(case.pool_nv, V)[:, None]
    reach_sq = np.float64(case.reach) * np.float64(case.reach)
    for b in range(case.B):
        base = min(max(int(no[b]), 0), O) if case.append else 0
        free = O - base
        with np.errstate(all="ignore"):
            dx = case.pose[b, 0] - case.pool_v[:, :, 0]
            dy = case.pose[b, 1] - case.pool_v[:, :, 1]
            qx = dx * dx
            qy = dy * dy
            d = qx + qy
            finite = np.all(np.isfinite(d) | ~valid, axis=1)
            key = np.min(np.where(valid, np.where(np.isnan(d), np.inf, d), np.inf), axis=1, initial=np.inf)
            cand = (case.pool_nv >= 1) & finite & (key <= reach_sq)
        if case.self_index is not None and 0 <= case.self_index[b] < P:
            cand[case.self_index[b]] = False
        idx = np.flatnonzero(cand)
        total = len(idx)
        if total > free:
            order = np.lexsort((idx, key[idx]))          # the last key is the primary one: by key, ties by p
            idx = np.sort(idx[order[:free]])
        for k, p in enumerate(idx):
            o = base + k
            n = min(int(case.pool_nv[p]), V)
            nv[b, o] = n
            vt[b, o, :n] = case.pool_v[p, :n]
            if rd is not None:
                rd[b, o] = case.pool_r[p] if case.pool_r is not None else 0.0
            if vl is not None:
                vel = np.zeros(2)
                if case.pool_vel is not None:
                    sx = case.pool_vel[p, 0] * case.pool_vel[p, 0]
                    sy = case.pool_vel[p, 1] * case.pool_vel[p, 1]
                    with np.errstate(all="ignore"):
                        if np.sqrt(sx + sy) >= case.min_speed:
                            vel = case.pool_vel[p]
                vl[b, o] = vel
        no[b], dr[b], tk[b] = base + len(idx), total - len(idx), len(idx)
    return no, nv, vt, rd, vl, dr, tk


def same(a, b):
    """two result tuples, byte for byte; the name of the first array that differs, or None"""
    for name, x, y in zip(("n_obstacles", "n_vertices", "vertices", "radius", "velocity", "dropped", "n_taken"), a, b):
        if (x is None) != (y is None) or (x is not None and x.tobytes() != y.tobytes()):
            return name
    return None


# ---- the scripted cases ----------------------------------------------------------------------------------------------------------------------------------------------
def random_pool(rng, P, V=1, span=6.0, polygons=False):
    nv = rng.integers(1, V + 1, P).astype(np.int32) if polygons else np.ones(P, np.int32)
    centre = rng.uniform(-span, span, (P, 1, 2))
    v = centre + rng.uniform(-0.4, 0.4, (P, V, 2))
    return nv, v, rng.uniform(0.05, 0.5, P), rng.uniform(-0.5, 0.5, (P, 2))


def lattice_pool(side, step=0.5):
    """side x side points on a lattice around the origin: many exactly equal squared distances from a lattice point or a cell centre"""
    k = (np.arange(side) - side // 2) * step
    v = np.stack(np.meshgrid(k, k, indexing="ij"), axis=-1).reshape(-1, 1, 2)
    P = len(v)
    return np.ones(P, np.int32), v, np.full(P, 0.2), np.tile((0.1, -0.2), (P, 1))


def robots(rng, B, span=4.0):
    return np.column_stack([rng.uniform(-span, span, (B, 2)), rng.uniform(-math.pi, math.pi, B)])


def cases():
    rng = np.random.default_rng(2024)
    out = []
    # pool sizes around the wave (64), the chunk (256) and the LDS-key limit (2048); per robot another fill of the container, so that some take all and some must choose
    for P in (0, 1, 5, 63, 64, 65, 255, 256, 257, 1000, 2049):
        B = 70 if P == 257 else 6
        nv, v, r, vel = random_pool(rng, P)
        out.append(Case(f"P = {P}", 16, 1, nv, v, r, vel, robots(rng, B), n_obstacles=np.arange(B) % 17 - (np.arange(B) % 5 == 4), self_index=(np.arange(B) * 7) % max(P, 1),
                        reach=3.0 if P < 1000 else 1.2))
        if P >= 255:      # everything within reach: the cut is found among P keys
            out.append(Case(f"P = {P}, all within reach", 16, 1, nv, v, r, vel, robots(rng, 4), n_obstacles=(0, 3, 15, 16), reach=30.0))
    # free capacity 0, 1, exact fit, one too many, many too many: nine candidates (the 3 x 3 lattice points around the robot), O = 12
    nv, v, r, vel = lattice_pool(9)
    out.append(Case("free capacity", 12, 1, nv, v, r, vel, np.tile((0.0, 0.0, 0.0), (6, 1)), n_obstacles=(12, 11, 3, 4, 9, 0), reach=0.75))
    # ties: from a lattice point the keys come in groups of 4 and 8 equal values, from a cell centre in groups of 4 and 8 too; the pool index decides
    for side in (16, 32, 46):
        nv, v, r, vel = lattice_pool(side)
        pose = [(0.0, 0.0, 0.0), (0.25, 0.25, 1.0), (0.25, 0.0, 2.0), (-1.0, 0.5, 0.0), (3.75, -3.75, 0.0)]
        out.append(Case(f"lattice {side} x {side}", 16, 1, nv, v, r, vel, pose * 2, n_obstacles=[0] * 5 + [11, 12, 13, 14, 15], reach=4.0))
    nv, v, r, vel = lattice_pool(8)
    out.append(Case("lattice, all keys equal", 6, 1, nv, np.tile((3.0, 4.0), (64, 1, 1)), r, vel, [(0.0, 0.0, 0.0)] * 3, n_obstacles=(0, 2, 6), reach=5.0))
    # a candidate at exactly reach (3-4-5: the key 25 is exact), one just beyond
    v = np.array([(3.0, 4.0), (np.nextafter(3.0, 4.0), 4.0), (-4.0, 3.0), (0.0, np.nextafter(5.0, 6.0))]).reshape(4, 1, 2)
    out.append(Case("exactly at reach", 16, 1, [1] * 4, v, [0.1] * 4, np.zeros((4, 2)), [(0.0, 0.0, 0.0)], reach=5.0))
    out.append(Case("reach 0", 16, 1, [1] * 2, [(1.0, 2.0), (1.0, np.nextafter(2.0, 3.0))], None, None, [(1.0, 2.0, 0.0)], reach=0.0))
    # the fleet as its own pool: self exclusion, with and without self_index
    pose = robots(rng, 20, span=1.5)
    fleet = (np.ones(20, np.int32), pose[:, None, :2].copy(), np.full(20, 0.2), rng.uniform(-0.3, 0.3, (20, 2)))
    out.append(Case("self exclusion", 16, 1, *fleet, pose, self_index=np.arange(20), reach=2.0))
    out.append(Case("self index -1 and out of range", 16, 1, *fleet, pose, self_index=np.where(np.arange(20) % 2, -1, 20 + np.arange(20)), reach=2.0))
    out.append(Case("no self index", 16, 1, *fleet, pose, reach=2.0))
    # entries without vertices, with a negative count, with more vertices than the stride holds
    nv, v, r, vel = random_pool(rng, 40, span=2.0)
    nv[::3] = 0; nv[1::7] = -2; nv[5::11] = 9
    out.append(Case("empty entries", 16, 1, nv, v, r, vel, robots(rng, 5, span=1.0), reach=2.0))
    # vertices that are not finite, among the valid ones (never taken) and behind them (of no account)
    nv, v, r, vel = random_pool(rng, 60, V=4, span=2.0, polygons=True)
    for p, j, val in ((0, 0, math.nan), (3, 1, math.inf), (6, 3, -math.inf), (9, 2, math.nan), (12, 0, 1e200), (15, 1, -1e200)):
        v[p, j, p % 2] = val
    out.append(Case("vertices not finite", 16, 4, nv, v, r, vel, robots(rng, 5, span=1.0), reach=3.0))
    # robot poses that are not finite
    nv, v, r, vel = random_pool(rng, 30, span=1.0)
    out.append(Case("robot pose not finite", 16, 1, nv, v, r, vel, [(math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (-math.inf, math.nan, 0.0), (0.0, 0.0, math.nan), (1e200, 0.0, 0.0)],
                    n_obstacles=(2, 0, 5, 1, 0), reach=5.0))
    # speeds at, just below and just above min_speed
    ms = 0.001
    vel = np.array([(ms, 0.0), (np.nextafter(ms, 0.0), 0.0), (np.nextafter(ms, 1.0), 0.0), (0.0, -ms), (6e-4, 8e-4), (0.0, 0.0), (-0.3, 0.4), (math.nan, 0.0), (0.0, math.inf), (7e-4, 7e-4)])
    out.append(Case("speeds around min_speed", 16, 1, [1] * 10, np.tile((0.5, 0.5), (10, 1, 1)), np.arange(10) * 0.1, vel, [(0.0, 0.0, 0.0)], reach=1.0, min_speed=ms))
    out.append(Case("min_speed 0.25", 16, 1, [1] * 10, np.tile((0.5, 0.5), (10, 1, 1)), np.arange(10) * 0.1, vel * 250.0, [(0.0, 0.0, 0.0)], reach=1.0, min_speed=0.25))
    # append and overwrite on containers that hold entries; counts outside [0, O]
    nv, v, r, vel = random_pool(rng, 50, span=2.0)
    pose = robots(rng, 8, span=1.0)
    held = (0, 1, 7, 15, 16, 40, -3, 10)
    out.append(Case("append", 16, 1, nv, v, r, vel, pose, n_obstacles=held, reach=1.5))
    out.append(Case("overwrite", 16, 1, nv, v, r, vel, pose, n_obstacles=held, reach=1.5, append=0))
    # lines and polygons
    for P in (7, 300):
        nv, v, r, vel = random_pool(rng, P, V=4, polygons=True)
        out.append(Case(f"polygons, P = {P}", 16, 4, nv, v, r, vel, robots(rng, 6), n_obstacles=(0, 0, 5, 12, 15, 16), reach=4.0))
    # pools without radius / velocity, into containers with and without the arrays
    nv, v, r, vel = random_pool(rng, 90, span=2.0)
    pose = robots(rng, 4, span=1.0)
    out.append(Case("pool without radius", 16, 1, nv, v, None, vel, pose, n_obstacles=(0, 4, 14, 16), reach=1.5))
    out.append(Case("pool without velocity", 16, 1, nv, v, r, None, pose, n_obstacles=(0, 4, 14, 16), reach=1.5))
    out.append(Case("pool without either, container with both", 16, 1, nv, v, None, None, pose, n_obstacles=(0, 4, 14, 16), reach=1.5))
    out.append(Case("pool without either, container without", 16, 1, nv, v, None, None, pose, n_obstacles=(0, 4, 14, 16), reach=1.5, radius=False, velocity=False))
    return out


def write_cases(path, case_list):
    """the file the harness's stand-alone program reads (tests/host_harness/fleet_obstacles_host.cpp, FOB_MAIN)"""
    with open(path, "wb") as f:
        for c in case_list:
            no, nv, vt, rd, vl = c.container()
            np.array([c.B, c.P, c.V, c.O, c.pool_r is not None, c.pool_vel is not None, c.self_index is not None, c.append, rd is not None, vl is not None], np.int32).tofile(f)
            np.array([c.reach, c.min_speed]).tofile(f)
            for a in (c.pool_nv, c.pool_v, c.pool_r, c.pool_vel, c.pose, c.self_index, no, nv, vt, rd, vl):
                if a is not None:
                    a.tofile(f)


def read_outputs(path, case_list):
    """the results the stand-alone program wrote, one tuple per case as host_select returns them"""
    out = []
    with open(path, "rb") as f:
        for c in case_list:
            B, O, V = c.B, c.O, c.V
            g = lambda dtype, shape: np.fromfile(f, dtype, int(np.prod(shape))).reshape(shape)
            no, nv, vt = g(np.int32, (B,)), g(np.int32, (B, O)), g(np.float64, (B, O, V, 2))
            rd = g(np.float64, (B, O)) if c.radius else None
            vl = g(np.float64, (B, O, 2)) if c.velocity else None
            out.append((no, nv, vt, rd, vl, g(np.int32, (B,)), g(np.int32, (B,))))
        assert f.read() == b""
    return out


# ---- pool fill ---------------------------------------------------------------------------------------------------------------------------------------------------
def pool_fill_inputs(n=5):
    """(pose [B][3], x [B][n][3], dt [B], status [B], radius [B]) with every branch of the rule: failed statuses, dt = 0 and < 0, numbers that are not finite"""
    rng = np.random.default_rng(77)
    B = 70
    pose = robots(rng, B)
    x = rng.uniform(-3.0, 3.0, (B, n, 3))
    dt = rng.uniform(0.05, 0.5, B)
    status = np.zeros(B, np.int32)
    status[3::9] = (1, 2, 3, 4, 5, 1, 2, 3)[:len(status[3::9])]
    dt[5], dt[6], dt[7], dt[8] = 0.0, -0.1, math.nan, math.inf
    x[10, 0, 0], x[11, 0, 1], x[12, 1, 0], x[13, 1, 1] = math.nan, math.inf, -math.inf, math.nan
    x[14, 0, 2], x[15, 2, 0] = math.nan, math.nan          # a heading and a later state: of no account
    return pose, x, dt, status, rng.uniform(0.1, 0.4, B)


def numpy_pool_fill(pose, x, dt, status, radius, V, pool_offset, pool):
    """the pool-fill rule of include/mpc_fleet.h on copies of the pool arrays (n_vertices, vertices, radius or None, velocity or None)"""
    nv, vt, rd, vl = (None if a is None else a.copy() for a in pool)
    B = len(pose)
    s = slice(pool_offset, pool_offset + B)
    nv[s] = 1
    vt[s, 0] = pose[:, :2]
    if rd is not None:
        rd[s] = radius
    if vl is not None:
        vel = np.zeros((B, 2))
        if x is not None:
            with np.errstate(all="ignore"):
                ok = (dt > 0.0) & np.isfinite(dt) & np.all(np.isfinite(x[:, :2, :2]), axis=(1, 2))
                if status is not None:
                    ok &= status == 0
                e = x[:, 1, :2] - x[:, 0, :2]
                vel[ok] = (e / dt[:, None])[ok]
        vl[s] = vel
    return nv, vt, rd, vl
