"""Shared by tests/test_plant_host.py and tests/test_gpu_plant.py: the host build of mpc_local_planner_amd/csrc/mpc_plant.hpp (tests/host_harness/plant_host.cpp,
g++ -ffp-contract=off) behind ctypes, the scripted cases, and a Python restatement of the rule written from the text of include/mpc_plant.h and of the rule at the top
of the .hpp: Python floats rounded operation by operation, math.sqrt, the wrap and the exact-fma sine and cosine of tests/_scan_cases.py, and -- where the rule CALLS
the scan cast's walk and pool entry instead of restating them -- the restatements of those in tests/_cast_cases.py.

A CASE is one call: one map (or none), one parameter set, B poses and commands, optionally the velocities, a pool and the robots' own indices in it."""
import ctypes as C
import math

import numpy as np

import _cast_cases as Cc
import _harness
import _scan_cases as Sc

_harness.SHARED.setdefault("plant_host", ("libmpc_plant.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip, bp = Sc.dp, Sc.ip, Sc.bp
d_, i_, b_ = Sc.d_, Sc.i_, Sc.b_
LETHAL, UNKNOWN = 254, 255
IPOISON = -77
DIFF, OMNI, CAR_STAGE, CAR_REAR = 0, 1, 2, 3
HEADING, OFF_MAP, MAP = -4, -3, -2
NAMES = ("pose", "vel", "stall", "info")
INF, PI = math.inf, math.pi
finite = math.isfinite
CAR = [(-0.1, -0.125), (0.5, -0.125), (0.5, 0.125), (-0.1, 0.125)]          # ex/stage/robots/carlike_robot.inc:16
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("plant_host"))
        lib.plh_step.restype, lib.plh_step.argtypes = C.c_int, [C.c_int, dp, ip, bp, dp, C.c_int, C.c_int, ip, dp, dp, ip, dp, dp, ip, ip]
        lib.plh_kept.restype, lib.plh_kept.argtypes = C.c_int, [dp, ip, dp, dp, dp, C.c_int, C.c_int, ip, dp, dp, C.c_int, C.c_int]
        lib.plh_list_cap.restype, lib.plh_threads.restype = C.c_int, C.c_int
        _lib = lib
    return _lib


class Case:
    """grid: uint8 (map_size_y, map_size_x) or None.  pool: None or (n_vertices (P,), vertices (P, V, 2), radius (P,) or None).  vel: (B, 3) or None.  no_stall /
    no_info: the output is NULL."""

    def __init__(self, name, grid, pose, cmd, vel=None, res=0.05, origin=(0.0, 0.0), interval=0.1, wheelbase=0.4, v_min=(-INF,) * 3, v_max=(INF,) * 3, a_max=(INF,) * 3,
                 footprint=CAR, n_sub=1, drive=DIFF, threshold=254, unknown_blocks=0, outside_blocks=1, pool=None, V=1, self_index=None, no_stall=False, no_info=False):
        self.name = name
        self.grid = None if grid is None else np.ascontiguousarray(grid, dtype=np.uint8)
        self.pose = np.array(np.asarray(pose, float).reshape(-1, 3))
        self.B = self.pose.shape[0]
        self.cmd = np.array(np.broadcast_to(np.asarray(cmd, float), (self.B, 3)), order="C")
        self.vel = None if vel is None else np.array(np.broadcast_to(np.asarray(vel, float), (self.B, 3)), order="C")
        self.res, self.origin, self.interval, self.wheelbase = float(res), tuple(map(float, origin)), float(interval), float(wheelbase)
        self.v_min, self.v_max, self.a_max = (tuple(map(float, v)) for v in (v_min, v_max, a_max))
        self.footprint = [(float(x), float(y)) for x, y in footprint]
        self.nf, self.n_sub, self.drive = len(self.footprint), int(n_sub), int(drive)
        self.threshold, self.unknown_blocks, self.outside_blocks = int(threshold), int(unknown_blocks), int(outside_blocks)
        self.V = int(V)
        if pool is None:
            self.pnv, self.pv, self.pr = np.zeros((0,), np.int32), np.zeros((0, self.V, 2)), None
        else:
            self.pnv = np.ascontiguousarray(pool[0], dtype=np.int32).reshape(-1)
            self.pv = np.ascontiguousarray(np.asarray(pool[1], float).reshape(self.pnv.shape[0], self.V, 2))
            self.pr = None if len(pool) < 3 or pool[2] is None else np.ascontiguousarray(np.asarray(pool[2], float).reshape(-1))
        self.P = int(self.pnv.shape[0])
        self.self_index = None if self_index is None else np.array(np.broadcast_to(np.asarray(self_index, np.int32), (self.B,)))
        self.no_stall, self.no_info = bool(no_stall), bool(no_info)

    @property
    def shape(self):
        return (1, 1) if self.grid is None else self.grid.shape

    def pool_tuple(self):
        return None if self.P == 0 else (self.pnv, self.pv, self.pr)

    def blocking(self):
        g = self.grid
        return ((g >= self.threshold) & (g <= LETHAL)) | ((g == UNKNOWN) & bool(self.unknown_blocks))

    def dpar(self):
        flat = [v for q in self.footprint for v in q] + [0.0] * (32 - 2 * self.nf)
        return np.array(self.origin + (self.res, self.interval, self.wheelbase) + self.v_min + self.v_max + self.a_max + tuple(flat))

    def ipar(self):
        return np.array([self.nf, self.n_sub, self.drive, self.shape[1], self.shape[0], self.threshold, self.unknown_blocks, self.outside_blocks], np.int32)

    def struct(self):
        """the mpc_plant_params of the case"""
        from mpc_local_planner_amd._abi import MpcPlantParams
        tri = lambda v: (C.c_double * 3)(*v)
        fp = ((C.c_double * 2) * 16)(*((C.c_double * 2)(*q) for q in self.footprint))
        return MpcPlantParams((C.c_double * 2)(*self.origin), self.res, self.interval, self.wheelbase, tri(self.v_min), tri(self.v_max), tri(self.a_max), fp, self.nf, self.n_sub,
                              self.drive, self.shape[1], self.shape[0], self.threshold, self.unknown_blocks, self.outside_blocks)

    def state(self):
        """(pose, vel or None, stall or None, info or None) as they are before a call: copies of the in / out arrays, the outputs poisoned"""
        return (self.pose.copy(), None if self.vel is None else self.vel.copy(), None if self.no_stall else np.full(self.B, IPOISON, np.int32),
                None if self.no_info else np.full((self.B, 4), IPOISON, np.int32))

    def variant(self, name=None, **kw):
        """the same case with some constructor arguments replaced"""
        args = dict(grid=self.grid, pose=self.pose, cmd=self.cmd, vel=self.vel, res=self.res, origin=self.origin, interval=self.interval, wheelbase=self.wheelbase,
                    v_min=self.v_min, v_max=self.v_max, a_max=self.a_max, footprint=self.footprint, n_sub=self.n_sub, drive=self.drive, threshold=self.threshold,
                    unknown_blocks=self.unknown_blocks, outside_blocks=self.outside_blocks, pool=self.pool_tuple(), V=self.V, self_index=self.self_index,
                    no_stall=self.no_stall, no_info=self.no_info)
        args.update(kw)
        return Case(name or self.name, **args)

    def take(self, order, name=None):
        """the instances `order` (indices) of the case, in that order"""
        order = np.asarray(order).reshape(-1)
        return self.variant(name or f"{self.name} {order.tolist()}", pose=self.pose[order], cmd=self.cmd[order], vel=None if self.vel is None else self.vel[order],
                            self_index=None if self.self_index is None else self.self_index[order])


def host_step(c):
    """the host build: (pose, vel or None, stall or None, info or None)"""
    pose, vel, stall, info = c.state()
    r = harness().plh_step(c.B, d_(c.dpar()), i_(c.ipar()), b_(c.grid), d_(c.cmd), c.P, c.V, i_(c.pnv), d_(c.pv), d_(c.pr), i_(c.self_index), d_(pose), d_(vel), i_(stall), i_(info))
    assert r >= 1, (c.name, r)
    return pose, vel, stall, info


def same(a, b):
    """None when the two results are the same bytes, else the first array that differs"""
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            if x is not y:
                return f"{NAMES[k]}: one is missing"
            continue
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            return f"{NAMES[k]} differs: {x.tolist()} / {y.tolist()}"
    return None


# ---- the restatement
class _Edge:
    """what tests/_cast_cases.py's walk reads of a case: the edge's length in the place of range_max, the return at the entry"""
    hit_point = 0

    def __init__(self, res, length):
        self.res, self.range_max = res, length


def _clamp_step(target, v, lim):
    d = target - v
    if d > lim:
        d = lim
    if d < -lim:
        d = -lim
    return v + d


def target_velocity(c, cmd):
    """rule 2: (vx, vy, w), or None when the steering angle does not wrap"""
    c0, c1, c2 = cmd
    if c.drive == DIFF:
        return [c0, 0.0, c2]
    if c.drive == OMNI:
        return [c0, c1, c2]
    phi = Sc.wrap(c2)
    if not -PI <= phi < PI:
        return None
    s, cs = Sc.sincos(phi)
    if c.drive == CAR_STAGE:
        return [c0 * cs, 0.0, (c0 * s) / c.wheelbase]
    tangent = s / cs if cs != 0.0 else (math.nan if s == 0.0 else math.copysign(INF, s) * math.copysign(1.0, cs))
    return [c0, 0.0, (c0 * tangent) / c.wheelbase]


def python_step(c, trace=None):
    """the restatement: (pose, vel or None, stall or None, info or None).  trace, a list, receives per instance a dict: valid, target, v (per sub-step), keys (per
    sub-step: None or (reason, edge))"""
    pose, vel, stall, info = c.state()
    blocking = None if c.grid is None else c.blocking()
    H, W = c.shape
    dt, res = c.interval, c.res
    edges = 1 if c.nf == 2 else c.nf
    for b in range(c.B):
        x, y, th0 = (float(v) for v in c.pose[b])
        cmd = [float(v) for v in c.cmd[b]]
        v = None if c.vel is None else [float(q) for q in c.vel[b]]
        t = dict(valid=False, target=None, v=[], keys=[])
        if trace is not None:
            trace.append(t)
        ok = all(finite(q) for q in [x, y, th0] + cmd + (v or []))
        th = Sc.wrap(th0) if ok else math.nan
        target = target_velocity(c, cmd) if -PI <= th < PI else None
        if target is None or not all(finite(q) for q in target):
            if stall is not None:
                stall[b] = 0
            if info is not None:
                info[b] = (-1, -1, -1, -1)
            continue
        t.update(valid=True, target=list(target))
        if v is None:
            v = list(target)
        me = -1 if c.self_index is None else int(c.self_index[b])
        moved = stalled = 0
        first = reason = edge = -1
        for m in range(c.n_sub):
            for k in range(3):
                w = _clamp_step(target[k], v[k], c.a_max[k] * dt)
                if w < c.v_min[k]:
                    w = c.v_min[k]
                if w > c.v_max[k]:
                    w = c.v_max[k]
                v[k] = w
            t["v"].append(list(v))
            dx, dy, da = v[0] * dt, v[1] * dt, v[2] * dt
            sn, cs = Sc.sincos(th)
            xc, yc = x + (dx * cs - dy * sn), y + (dx * sn + dy * cs)
            thc = Sc.wrap(th + da)
            key = None          # (reason + 4, edge): the smallest blocks
            if not (-PI <= thc < PI and finite(xc) and finite(yc)):
                key = (HEADING + 4, 0)
            elif c.nf >= 2:
                found = []
                s2, c2 = Sc.sincos(thc)
                w_ = [(xc + (c2 * fx - s2 * fy), yc + (s2 * fx + c2 * fy)) for fx, fy in c.footprint]
                on = []
                for j, (wx, wy) in enumerate(w_):
                    u, vv = (wx - c.origin[0]) / res, (wy - c.origin[1]) / res
                    inside = blocking is not None and finite(u) and finite(vv) and 0 <= math.floor(u) < W and 0 <= math.floor(vv) < H
                    on.append((u, vv) if inside else None)
                    if blocking is not None and not inside and c.outside_blocks:
                        found.append((OFF_MAP + 4, j))
                for j in range(edges):
                    (ax, ay), (bx, by) = w_[j], w_[(j + 1) % c.nf]
                    ex, ey = bx - ax, by - ay
                    length = math.sqrt(ex * ex + ey * ey)
                    ux, uy = (1.0, 0.0) if length == 0.0 else (ex / length, ey / length)
                    if on[j] is not None:
                        u, vv = on[j]
                        if Cc.walk(_Edge(res, length), blocking, u, vv, math.floor(u), math.floor(vv), ux, uy) < INF:
                            found.append((MAP + 4, j))
                    for p in range(c.P):
                        tp = None if p == me else Cc.pool_entry(c, p, ax, ay, ux, uy)
                        if tp is not None and tp <= length:
                            found.append((p + 4, j))
                key = min(found) if found else None
            t["keys"].append(None if key is None else (key[0] - 4, -1 if key[0] == 0 else key[1]))
            if key is None:
                x, y, th, moved = xc, yc, thc, moved + 1
            else:
                if first < 0:
                    first, reason, edge = m, key[0] - 4, (-1 if key[0] == 0 else key[1])
                stalled += 1
        if moved:
            pose[b] = (x, y, th)
        if vel is not None:
            vel[b] = v
        if stall is not None:
            stall[b] = stalled
        if info is not None:
            info[b] = (moved, first, reason, edge)
    return pose, vel, stall, info


# ---- the scripted cases
room, discs = Cc.room, Cc.discs


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    R = room()                                  # 48 x 40 cells of 0.05 m: 2.4 m x 2.0 m, a ring of lethal cells; the free space is x in [0.05, 2.35), y in [0.05, 1.95)
    free = np.zeros((40, 48), np.uint8)
    at = (1.0, 1.0, 0.0)
    for name, drive in (("diff", DIFF), ("omni", OMNI), ("car, Stage", CAR_STAGE), ("car, rear axle", CAR_REAR)):
        add(f"drive: {name}", R, [at, (0.8, 1.2, 2.5)], (0.4, 0.2, 0.3), drive=drive)
        add(f"drive: {name}, three sub-steps, the velocity kept", R, [at, (0.8, 1.2, -2.5)], (0.4, 0.2, 0.3), vel=[(0.1, 0.0, 0.0), (0.0, 0.1, -0.2)], drive=drive, n_sub=3)
    add("the acceleration clamp binds", R, at, (0.4, 0.0, 0.3), vel=(0.0, 0.0, 0.0), a_max=(1.0, 1.0, 1.0))
    add("the acceleration clamp binds, then no longer", R, at, (0.4, 0.0, 0.3), vel=(0.0, 0.0, 0.0), a_max=(1.0, 1.0, 1.0), n_sub=6)
    add("the acceleration clamp does not bind", R, at, (0.4, 0.0, 0.3), vel=(0.35, 0.0, 0.25), a_max=(1.0, 1.0, 1.0))
    add("the velocity clamp binds", R, at, (0.4, 0.0, -0.3), v_min=(-0.25, -INF, -0.2), v_max=(0.25, INF, 0.2))
    add("the velocity clamp does not bind", R, at, (0.4, 0.0, -0.3), v_min=(-1.0, -INF, -1.0), v_max=(1.0, INF, 1.0))
    add("no velocity kept", R, at, (0.4, 0.0, 0.3), n_sub=2)
    # the front of the car 0.5 m ahead of the pose, at 2.12 m; the wall's cells are x in [2.35, 2.4): four sub-steps of 0.05 m fit (2.32), the fifth does not (2.37)
    add("straight into a wall", R, (1.62, 1.0, 0.0), (0.5, 0.0, 0.0), n_sub=8)
    add("a vertex off the map, outside_blocks 1", free, (1.72, 1.0, 0.0), (1.0, 0.0, 0.0), n_sub=4, outside_blocks=1)
    add("a vertex off the map, outside_blocks 0", free, (1.72, 1.0, 0.0), (1.0, 0.0, 0.0), n_sub=4, outside_blocks=0)
    # cells of 0.5 m, the blocking cell (4, 2): x in [2, 2.5), y in [1, 1.5).  interval 0.125 and 4 m/s: the candidate is (1.0, 1.25, 0) exactly, the segment's far end at
    # x = 2.0 exactly: the walk reaches the boundary at its full length and does not enter; the same segment listed from the other end begins in the blocking cell
    g = np.zeros((8, 8), np.uint8)
    g[2, 4] = LETHAL
    add("an edge that ends on the boundary of a blocking cell", g, (0.5, 1.25, 0.0), (4.0, 0.0, 0.0), res=0.5, interval=0.125, footprint=[(0.0, 0.0), (1.0, 0.0)])
    add("the same edge from its other end", g, (0.5, 1.25, 0.0), (4.0, 0.0, 0.0), res=0.5, interval=0.125, footprint=[(1.0, 0.0), (0.0, 0.0)])
    add("the same edge in a closed outline", g, (0.5, 1.25, 0.0), (4.0, 0.0, 0.0), res=0.5, interval=0.125, footprint=[(0.0, 0.0), (1.0, 0.0), (0.0, 0.25)])
    twice = [(0.0, -0.1), (0.3, -0.1), (0.3, -0.1), (0.3, 0.1), (0.0, 0.1)]
    add("a zero-length edge", R, at, (0.5, 0.0, 0.2), n_sub=3, footprint=twice)
    add("a zero-length edge inside a disc", R, at, (0.5, 0.0, 0.0), n_sub=1, footprint=[(0.3, 0.0), (0.3, 0.0)], pool=discs([(1.36, 1.0)], [0.02]))
    add("no footprint", R, (1.6, 1.0, 0.0), (1.0, 0.0, 0.0), n_sub=8, footprint=[], pool=discs([(1.9, 1.0)], [0.1]))
    add("a footprint of one segment", R, (1.62, 1.0, 0.0), (0.5, 0.0, 0.0), n_sub=8, footprint=[(0.0, 0.0), (0.5, 0.0)])
    add("a disc blocks", R, at, (1.0, 0.0, 0.0), n_sub=4, pool=discs([(1.75, 1.0)], [0.1]))
    add("a segment blocks", R, at, (1.0, 0.0, 0.0), n_sub=4, pool=([2], [[(1.62, 0.8), (1.62, 1.2), (0, 0)]], None), V=3)
    add("a polygon blocks", R, at, (1.0, 0.0, 0.0), n_sub=4, pool=([3], [[(1.65, 0.9), (1.9, 1.0), (1.65, 1.1)]], None), V=3)
    add("a tie between two pool entries", R, at, (1.0, 0.0, 0.0), n_sub=4, pool=discs([(0.2, 0.2), (1.75, 1.0), (1.75, 1.0)], [0.05, 0.1, 0.1]))
    add("map and pool both block", R, (1.62, 1.0, 0.0), (0.5, 0.0, 0.0), n_sub=8, pool=discs([(2.4, 1.0)], [0.06]))
    me = discs([(1.0, 1.0), (0.2, 0.2)], [0.3, 0.05])          # entry 0 stands where the robots do
    add("self_index skipped", R, [at, at, at], (1.0, 0.0, 0.0), n_sub=2, pool=me, self_index=[0, -1, 1])
    nan = math.nan
    add("a pose, a command and a velocity that are not finite", R, [(nan, 1.0, 0.0), (1.0, INF, 0.0), (1.0, 1.0, -INF), at, at, at, at],
        [(0.4, 0.0, 0.1)] * 3 + [(nan, 0.0, 0.1), (0.4, 0.0, INF), (0.4, 0.0, 0.1), (0.4, 0.0, 0.1)], vel=[(0.1, 0.0, 0.0)] * 5 + [(0.1, nan, 0.0), (0.1, 0.0, 0.0)], n_sub=2)
    add("a heading that does not wrap", R, [(1.0, 1.0, 1e18), at], (0.4, 0.0, 0.1), n_sub=2)
    # 1e19 rad/s for 0.1 s: the multiple of 2 pi nearest to 1e18 is rounded by more than a turn, the difference is -121.7
    assert not -PI <= Sc.wrap(0.0 + 1e19 * 0.1) < PI
    add("a turn so large that the new heading does not wrap", R, [at, at], [(0.4, 0.0, 1e19), (0.4, 0.0, 0.1)], n_sub=3)
    add("a steering angle that does not wrap", R, [at, at], [(0.4, 0.0, 1e18), (0.4, 0.0, 0.1)], drive=CAR_STAGE, n_sub=2)
    add("no stall, no info", R, [at, (1.6, 1.0, 0.0)], (1.0, 0.0, 0.0), n_sub=4, no_stall=True, no_info=True)
    add("no map", None, [(1.6, 1.0, 0.0), (50.0, -3.0, 1.0)], (1.0, 0.0, 0.0), n_sub=8, pool=discs([(2.5, 1.0)], [0.1]))
    add("unknown cells block", np.full((40, 48), UNKNOWN, np.uint8), at, (1.0, 0.0, 0.0), unknown_blocks=1)
    add("unknown cells pass", np.full((40, 48), UNKNOWN, np.uint8), at, (1.0, 0.0, 0.0), unknown_blocks=0)
    add("a threshold below 254", np.full((40, 48), 100, np.uint8), [at, at], (1.0, 0.0, 0.0), threshold=100)
    add("origin off zero, sixteen vertices", R, [(0.2, 0.1, 3.0), (-0.3, -0.2, -1.0)], (0.3, 0.1, 0.4), origin=(-1.013, -0.927), drive=OMNI, n_sub=5,
        footprint=[(0.2 * math.cos(2 * PI * k / 16), 0.15 * math.sin(2 * PI * k / 16)) for k in range(16)], pool=Cc.ring_pool(9, (0.2, 0.1), 0.3, 0.8, 5), V=3)
    assert max(c.B for c in out) <= 8 and {c.nf for c in out} >= {0, 2, 3, 4, 16}
    return out


def random_cases(count=60, seed=29):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        W, H, B, V = int(rng.integers(24, 49)), int(rng.integers(24, 49)), int(rng.integers(1, 5)), int(rng.integers(1, 5))
        res = float(rng.choice([0.05, 0.1]))
        grid = rng.choice(np.array([0, 0, 100, 253, LETHAL, UNKNOWN], np.uint8), size=(H, W), p=[0.6, 0.374, 0.005, 0.005, 0.008, 0.008])
        origin = (float(rng.choice([0.0, -0.513])), float(rng.choice([0.0, 0.207])))
        pose = np.column_stack([origin[0] + rng.uniform(-0.05, 1.05, B) * W * res, origin[1] + rng.uniform(-0.05, 1.05, B) * H * res, rng.uniform(-4, 4, B)])
        kind = int(rng.integers(0, 6))
        if kind == 0:
            fp = []
        elif kind == 1:
            fp = [(-0.1, 0.0), (0.2, 0.05)]
        elif kind == 2:
            fp = CAR
        else:
            nv = int(rng.integers(3, 9))
            ang = np.sort(rng.uniform(0, 2 * PI, nv))
            rad = rng.uniform(0.05, 0.25, nv)
            fp = list(zip(rad * np.cos(ang), rad * np.sin(ang)))
        P = int(rng.integers(0, 13))
        pool = None
        if P:
            nv = rng.integers(0, V + 1, P).astype(np.int32)
            pv = np.stack([origin[0] + rng.uniform(0, W * res, (P, V)), origin[1] + rng.uniform(0, H * res, (P, V))], 2)
            pv[:, 1:] = pv[:, :1] + rng.uniform(-0.3, 0.3, (P, V - 1, 2))
            for p in np.flatnonzero(rng.random(P) < 0.4):          # some of the bodies right next to a robot
                pv[p] += pose[int(rng.integers(0, B)), :2] + rng.uniform(-0.3, 0.3, 2) - pv[p, 0]
            pool = (nv, pv, None if rng.random() < 0.2 else rng.uniform(-0.05, 0.2, P))
        lim = lambda lo, hi: tuple(float(rng.choice([INF, rng.uniform(lo, hi)])) for _ in range(3))
        v_max = lim(0.3, 1.5)
        out.append(Case(f"random {k}", grid if rng.random() < 0.9 else None, pose, np.column_stack([rng.uniform(-1.5, 1.5, B), rng.uniform(-0.5, 0.5, B), rng.uniform(-1.2, 1.2, B)]),
                        vel=None if rng.random() < 0.4 else rng.uniform(-0.5, 0.5, (B, 3)), res=res, origin=origin, interval=float(rng.choice([0.1, 0.05, 0.025])),
                        wheelbase=float(rng.choice([0.4, 0.25])), v_min=tuple(-v for v in lim(0.3, 1.5)), v_max=v_max, a_max=lim(0.5, 4.0), footprint=fp,
                        n_sub=int(rng.integers(1, 9)), drive=int(rng.integers(0, 4)), threshold=int(rng.choice([254, 253, 100])), unknown_blocks=int(rng.integers(0, 2)),
                        outside_blocks=int(rng.integers(0, 2)), pool=pool, V=V, self_index=None if rng.random() < 0.3 else rng.integers(-1, max(P, 1), B),
                        no_stall=rng.random() < 0.15, no_info=rng.random() < 0.1))
    return out


# ---- the file format of the stand-alone program (tests/host_harness/plant_host.cpp, -DPLH_MAIN)
def write_cases(path, cs):
    with open(path, "wb") as f:
        for c in cs:
            np.array([c.B, c.P, c.V, c.grid is not None, c.pr is not None, c.self_index is not None, c.vel is not None, not c.no_stall, not c.no_info], np.int32).tofile(f)
            c.ipar().tofile(f)
            c.dpar().tofile(f)
            if c.grid is not None:
                c.grid.tofile(f)
            c.cmd.tofile(f)
            c.pose.tofile(f)
            if c.vel is not None:
                c.vel.tofile(f)
            c.pnv.tofile(f)
            c.pv.tofile(f)
            if c.pr is not None:
                c.pr.tofile(f)
            if c.self_index is not None:
                c.self_index.tofile(f)


def read_outputs(path, cs):
    out = []
    with open(path, "rb") as f:
        for c in cs:
            pose = np.fromfile(f, np.float64, 3 * c.B).reshape(c.B, 3)
            vel = None if c.vel is None else np.fromfile(f, np.float64, 3 * c.B).reshape(c.B, 3)
            stall = None if c.no_stall else np.fromfile(f, np.int32, c.B)
            out.append((pose, vel, stall, None if c.no_info else np.fromfile(f, np.int32, 4 * c.B).reshape(c.B, 4)))
        assert f.read() == b""
    return out
