"""Shared by tests/test_scan_cast_host.py and tests/test_gpu_scan_cast.py: the host build of mpc_local_planner_amd/csrc/mpc_scan_cast.hpp
(tests/host_harness/scan_cast_host.cpp, g++ -ffp-contract=off) behind ctypes, the scripted cases, and a Python restatement of the rule written from the text of
include/mpc_scan_cast.h and of the rule at the top of the .hpp: Python floats rounded operation by operation, math.sqrt, and the wrap and the exact-fma sine and
cosine of tests/_scan_cases.py.

A CASE is one call: one map, one parameter set, B poses, optionally a pool and the robots' own indices in it."""
import ctypes as C
import math

import numpy as np

import _harness
import _scan_cases as Sc

_harness.SHARED.setdefault("scan_cast_host", ("libmpc_scan_cast.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip, bp, fp = Sc.dp, Sc.ip, Sc.bp, Sc.fp
d_, i_, b_, f_ = Sc.d_, Sc.i_, Sc.b_, Sc.f_
LETHAL, UNKNOWN = 254, 255
FPOISON, IPOISON = np.float32(-7.25), -77
MAP, MISS = -2, -1
NAMES = ("ranges", "hit", "info")
INF = math.inf
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("scan_cast_host"))
        lib.sch_cast.restype, lib.sch_cast.argtypes = C.c_int, [C.c_int, dp, ip, bp, dp, C.c_int, C.c_int, ip, dp, dp, ip, C.c_int, fp, ip, ip, dp]
        lib.sch_lds_bytes.restype, lib.sch_lds_bytes.argtypes = C.c_size_t, [C.c_int]
        lib.sch_list_cap.restype, lib.sch_max_rc.restype = C.c_int, C.c_int
        _lib = lib
    return _lib


class Case:
    """grid: uint8 (map_size_y, map_size_x).  pool: None or (n_vertices (P,), vertices (P, V, 2), radius (P,) or None).  no_hit / no_info: the output is NULL."""

    def __init__(self, name, grid, pose, n, res=0.05, origin=(0.0, 0.0), sensor=(0.0, 0.0, 0.0), angle_min=-math.pi, angle_inc=None, range_max=3.0, threshold=254,
                 unknown_blocks=0, hit_point=1, miss_is_inf=1, pool=None, V=1, self_index=None, no_hit=False, no_info=False):
        self.name = name
        self.grid = np.ascontiguousarray(grid, dtype=np.uint8)
        self.pose = np.array(np.asarray(pose, float).reshape(-1, 3))
        self.B, self.n = self.pose.shape[0], int(n)
        self.res, self.origin, self.sensor = float(res), tuple(map(float, origin)), tuple(map(float, sensor))
        self.angle_min, self.angle_inc, self.range_max = float(angle_min), float(2 * math.pi / self.n if angle_inc is None else angle_inc), float(range_max)
        self.threshold, self.unknown_blocks, self.hit_point, self.miss_is_inf = int(threshold), int(unknown_blocks), int(hit_point), int(miss_is_inf)
        self.V = int(V)
        if pool is None:
            self.pnv, self.pv, self.pr = np.zeros((0,), np.int32), np.zeros((0, self.V, 2)), None
        else:
            self.pnv = np.ascontiguousarray(pool[0], dtype=np.int32).reshape(-1)
            self.pv = np.ascontiguousarray(np.asarray(pool[1], float).reshape(self.pnv.shape[0], self.V, 2))
            self.pr = None if len(pool) < 3 or pool[2] is None else np.ascontiguousarray(np.asarray(pool[2], float).reshape(-1))
        self.P = int(self.pnv.shape[0])
        self.self_index = None if self_index is None else np.array(np.broadcast_to(np.asarray(self_index, np.int32), (self.B,)))
        self.no_hit, self.no_info = bool(no_hit), bool(no_info)

    @property
    def Rc(self):
        return int(math.ceil(self.range_max / self.res)) + 1

    @property
    def miss(self):
        return np.float32(INF) if self.miss_is_inf else np.float32(self.range_max)

    def pool_tuple(self):
        return None if self.P == 0 else (self.pnv, self.pv, self.pr)

    def blocking(self):
        """the map cells that block, a bool array"""
        g = self.grid
        return ((g >= self.threshold) & (g <= LETHAL)) | ((g == UNKNOWN) & bool(self.unknown_blocks))

    def dpar(self):
        return np.array(self.origin + (self.res,) + self.sensor + (self.angle_min, self.angle_inc, self.range_max))

    def ipar(self):
        return np.array([self.grid.shape[1], self.grid.shape[0], self.threshold, self.unknown_blocks, self.hit_point, self.miss_is_inf], np.int32)

    def struct(self):
        """the mpc_cast_params of the case"""
        from mpc_local_planner_amd._abi import MpcCastParams
        return MpcCastParams((C.c_double * 2)(*self.origin), self.res, (C.c_double * 3)(*self.sensor), self.angle_min, self.angle_inc, self.range_max, self.grid.shape[1],
                             self.grid.shape[0], self.threshold, self.unknown_blocks, self.hit_point, self.miss_is_inf)

    def outputs(self):
        """(ranges, hit or None, info or None), poisoned"""
        return (np.full((self.B, self.n), FPOISON, np.float32), None if self.no_hit else np.full((self.B, self.n), IPOISON, np.int32),
                None if self.no_info else np.full((self.B, 4), IPOISON, np.int32))

    def variant(self, name=None, **kw):
        """the same case with some constructor arguments replaced"""
        args = dict(grid=self.grid, pose=self.pose, n=self.n, res=self.res, origin=self.origin, sensor=self.sensor, angle_min=self.angle_min, angle_inc=self.angle_inc,
                    range_max=self.range_max, threshold=self.threshold, unknown_blocks=self.unknown_blocks, hit_point=self.hit_point, miss_is_inf=self.miss_is_inf,
                    pool=self.pool_tuple(), V=self.V, self_index=self.self_index, no_hit=self.no_hit, no_info=self.no_info)
        args.update(kw)
        return Case(name or self.name, **args)

    def take(self, b):
        return self.variant(f"{self.name} [{b}]", pose=self.pose[b], self_index=None if self.self_index is None else self.self_index[b:b + 1])


def host_cast(c, chord=False):
    """the host build: (ranges, hit or None, info or None)[, chord (B, n) in metres]"""
    ranges, hit, info = c.outputs()
    ch = np.zeros((c.B, c.n)) if chord else None
    r = harness().sch_cast(c.B, d_(c.dpar()), i_(c.ipar()), b_(c.grid), d_(c.pose), c.P, c.V, i_(c.pnv), d_(c.pv), d_(c.pr), i_(c.self_index), c.n, f_(ranges), i_(hit), i_(info),
                           d_(ch))
    assert r == c.Rc, (c.name, r, c.Rc)
    return (ranges, hit, info) + ((ch,) if chord else ())


def same(a, b):
    """None when the two results are the same bytes, else the first array that differs"""
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            if x is not y:
                return f"{NAMES[k]}: one is missing"
            continue
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            diff = np.argwhere(x.view(np.int32) != y.view(np.int32))[:3].tolist() if x.shape == y.shape else (x.shape, y.shape)
            return f"{NAMES[k]} differs at {diff}: {[(x[tuple(d)], y[tuple(d)]) for d in diff] if x.shape == y.shape else ''}"
    return None


# ---- the restatement
PI = math.pi
finite = math.isfinite


def _cross(c, i, u, inv):
    return INF if c == 0.0 else (float(i + 1 if c > 0.0 else i) - u) * inv


def walk(c, blocking, u, v, i, j, dc, ds, trace=None):
    """rule 2 from the sensor's cell (i, j), on the map: r_map or inf.  trace: a dict that receives ties, steps, t_in, t_out"""
    H, W = blocking.shape
    if blocking[j, i]:
        return 0.0
    inv_x = 1.0 / dc if dc != 0.0 else 0.0
    inv_y = 1.0 / ds if ds != 0.0 else 0.0
    while True:
        tx, ty = _cross(dc, i, u, inv_x), _cross(ds, j, v, inv_y)
        t_in = tx if tx <= ty else ty
        if trace is not None:
            trace["ties"] += tx == ty
            trace["steps"] += 1
        if not t_in * c.res < c.range_max:
            return INF
        if tx <= ty:
            i += 1 if dc > 0.0 else -1
        else:
            j += 1 if ds > 0.0 else -1
        if not (0 <= i < W and 0 <= j < H):
            return INF
        if blocking[j, i]:
            t_out = min(_cross(dc, i, u, inv_x), _cross(ds, j, v, inv_y))
            if trace is not None:
                trace.update(t_in=t_in, t_out=t_out, cell=(i, j))
            return ((t_in + t_out) * 0.5 if c.hit_point else t_in) * c.res


def pool_entry(c, p, sx, sy, dc, ds):
    """rule 3: the t of pool entry p along the beam, None when it returns nothing"""
    nv = min(int(c.pnv[p]), c.V)
    q = [(float(x), float(y)) for x, y in c.pv[p, :max(nv, 0)]]
    if nv < 1 or not all(finite(x) and finite(y) for x, y in q):
        return None
    if nv == 1:
        rad = 0.0 if c.pr is None else float(c.pr[p])
        if not finite(rad) or not rad > 0.0:
            return None
        dx, dy = q[0][0] - sx, q[0][1] - sy
        bq = dx * dc + dy * ds
        cq = (dx * dx + dy * dy) - rad * rad
        if cq <= 0.0:
            return 0.0
        if bq <= 0.0:
            return None
        disc = bq * bq - cq
        if disc < 0.0 or math.isnan(disc):
            return None
        t = bq - math.sqrt(disc)
        return t if t >= 0.0 else None
    best = None
    for j in range(1 if nv == 2 else nv):
        (ax, ay), (bx, by) = q[j], q[(j + 1) % nv]
        ex, ey, wx, wy = bx - ax, by - ay, ax - sx, ay - sy
        den = dc * ey - ds * ex
        if den == 0.0 or math.isnan(den):
            continue
        t, s = (wx * ey - wy * ex) / den, (wx * ds - wy * dc) / den
        if t >= 0.0 and 0.0 <= s <= 1.0 and (best is None or t < best):
            best = t
    return best


def python_cast(c, trace=None):
    """the restatement: (ranges, hit or None, info or None).  trace, a list, receives per instance a dict: valid, on_map, beams [dict(k, dir, r_map, r_pool, ties, ...)]"""
    ranges, hit, info = c.outputs()
    blocking = c.blocking()
    H, W = blocking.shape
    for b in range(c.B):
        px, py, yaw = (float(v) for v in c.pose[b])
        t = dict(valid=False, on_map=False, beams=[])
        if trace is not None:
            trace.append(t)
        heading = Sc.wrap(yaw) if finite(px) and finite(py) and finite(yaw) else math.nan
        h_row = np.full(c.n, MISS, np.int32)
        ranges[b] = c.miss
        if not -PI <= heading < PI:
            if hit is not None:
                hit[b] = h_row
            if info is not None:
                info[b] = (-1, 0, 0, 0)
            continue
        t["valid"] = True
        sn, cs = Sc.sincos(heading)
        sx = px + (cs * c.sensor[0] - sn * c.sensor[1])
        sy = py + (sn * c.sensor[0] + cs * c.sensor[1])
        u, v = (sx - c.origin[0]) / c.res, (sy - c.origin[1]) / c.res
        on_map = finite(u) and finite(v) and 0 <= math.floor(u) < W and 0 <= math.floor(v) < H
        t.update(on_map=on_map, sensor=(sx, sy), uv=(u, v))
        i0, j0 = (math.floor(u), math.floor(v)) if on_map else (0, 0)
        me = -1 if c.self_index is None else int(c.self_index[b])
        for k in range(c.n):
            th = Sc.wrap(((yaw + c.sensor[2]) + c.angle_min) + float(k) * c.angle_inc)
            if not -PI <= th < PI:
                continue
            ds, dc = Sc.sincos(th)
            bt = dict(k=k, dir=(dc, ds), ties=0, steps=0)
            r_map = walk(c, blocking, u, v, i0, j0, dc, ds, bt) if on_map else INF
            r_pool, who = INF, -1
            for p in range(c.P):
                tp = None if p == me else pool_entry(c, p, sx, sy, dc, ds)
                if tp is not None and tp < r_pool:
                    r_pool, who = tp, p
            r = r_map if r_map <= r_pool else r_pool
            if r < c.range_max:
                ranges[b, k] = np.float32(r)
                h_row[k] = MAP if r_map <= r_pool else who
            bt.update(r_map=r_map, r_pool=r_pool)
            t["beams"].append(bt)
        if hit is not None:
            hit[b] = h_row
        if info is not None:
            Rc = c.Rc
            n_cells = int(blocking[max(j0 - Rc, 0):j0 + Rc + 1, max(i0 - Rc, 0):i0 + Rc + 1].sum()) if on_map else 0
            info[b] = (int((h_row == MAP).sum()), int((h_row >= 0).sum()), int((h_row == MISS).sum()), n_cells)
    return ranges, hit, info


# ---- the scripted cases
def room(W=48, H=40, wall=LETHAL):
    """free inside, one ring of `wall` cells around it"""
    g = np.zeros((H, W), np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = wall
    return g


def discs(centres, radii):
    centres = np.asarray(centres, float).reshape(-1, 1, 2)
    return np.ones(centres.shape[0], np.int32), centres, np.asarray(radii, float).reshape(-1)


def ring_pool(P, centre, lo, hi, seed, V=3):
    """P entries around `centre` at distances lo .. hi: discs, segments and triangles in turn"""
    rng = np.random.default_rng(seed)
    ang, dist = rng.uniform(-math.pi, math.pi, P), rng.uniform(lo, hi, P)
    at = np.stack([centre[0] + dist * np.cos(ang), centre[1] + dist * np.sin(ang)], 1)
    nv = np.array([1 + (p % 3) for p in range(P)], np.int32)
    pv = at[:, None, :] + rng.uniform(-0.06, 0.06, (P, V, 2))
    return nv, pv, rng.uniform(0.01, 0.05, P)


def tie_pose():
    """a pose on a map of resolution 0.5 whose one beam, heading pi / 4, reaches the upper right corner of cell (3, 0) with the same crossing parameter on both axes: the
    sine and cosine of rule 1 differ in the last place there, and so do their reciprocals; v is chosen one place off the middle so that the two products round alike"""
    s, c = Sc.sincos(math.pi / 4)
    for dy in (0.5, 0.5 - 2.0 ** -53, 0.5 + 2.0 ** -53, 0.5 - 2.0 ** -52, 0.5 + 2.0 ** -52):
        v = 1.0 - dy
        if (1.0 - v) * (1.0 / s) == 0.5 * (1.0 / c) and 1.0 - v == dy:
            return (0.5 * 3.5, 0.5 * v, math.pi / 4)
    raise AssertionError("no tie found")


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    R = room()
    centre = (1.23, 0.97, 0.3)
    rng = np.random.default_rng(28)
    # the beam counts around the wave (64) and beyond the workgroup (256)
    for n in (1, 63, 64, 65, 257):
        add(f"{n} beams", R, [centre, (0.4, 1.6, -2.0)], n, pool=ring_pool(7, centre, 0.2, 1.0, n), V=3, self_index=[-1, 2])
    add("the demo's laser", R, [centre, (2.0, 0.3, 2.0)], 640, sensor=(-0.1, 0.0, 0.0), angle_min=-math.radians(58.0) / 2, angle_inc=math.radians(58.0) / 639, range_max=6.5)
    # along an axis: yaw 0 and angle_min 0 give sine 0 and cosine 1 exactly; the sensor in the middle of cell (20, 20), the wall's cells 47 and 39
    axis = Case("a beam along an axis", R, (1.025, 1.025, 0.0), 4, angle_min=0.0, angle_inc=math.pi / 2, hit_point=0)
    out.append(axis)
    g = np.zeros((4, 8), np.uint8)
    g[0, 4] = LETHAL          # the cell the x step enters at the corner; (3, 1), which a y step would enter, and (4, 1) beyond the corner are free
    add("a tie at a cell corner", g, tie_pose(), 1, res=0.5, angle_min=0.0, angle_inc=0.0, range_max=3.0, hit_point=0)
    add("the sensor's own cell blocking", R, [(0.02, 1.0, 0.5), (2.39, 1.99, -1.0)], 12)
    add("the sensor off the map", R, [(-1.0, 1.0, 0.0), (1.0, 2.5, -1.5), (1e9, 1.0, 0.0)], 16, pool=discs([(-0.5, 1.0)], [0.1]))
    add("a ray leaving the map", np.zeros((40, 48), np.uint8), centre, 24, range_max=6.0)
    # +x from u = 20.5: the wall's cell 47 is entered at 26.5 cells = 1.325 m, its middle lies at 27 cells
    d_in = 26.5 * 0.05
    add("a return just inside range_max", R, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=0, range_max=math.nextafter(d_in, INF))
    add("a return just beyond range_max", R, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=0, range_max=d_in)
    add("the midpoint beyond range_max while the entry is inside", R, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=1, range_max=d_in + 0.01)
    add("the entry inside range_max, reported at the entry", R, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=0, range_max=d_in + 0.01)
    # +x from cell 20: a column of 100 at cell 25, of 255 at cell 30, the wall at 47
    g = room()
    g[1:-1, 25], g[1:-1, 30] = 100, UNKNOWN
    add("unknown cells pass, threshold 254", g, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=0)
    add("unknown cells block", g, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=0, unknown_blocks=1)
    add("a threshold below 254", g, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, hit_point=0, threshold=100)
    add("a disc around the sensor", R, centre, 16, pool=discs([(1.3, 1.0)], [0.3]))
    add("a disc behind the sensor", R, (1.025, 1.025, 0.0), 1, angle_min=0.0, angle_inc=0.0, pool=discs([(0.5, 1.025)], [0.2]))
    # +x from (0.5, 0.5): d = (1, 0.25) and radius 0.25 give bq = 1, cq = 1 and a discriminant of exactly 0; with the centre 1e-15 higher the sum d . d moves by two places and the ray passes
    add("a tangent ray", R, (0.5, 0.5, 0.0), 1, angle_min=0.0, angle_inc=0.0, pool=discs([(1.5, 0.75)], [0.25]))
    add("a ray just past the tangent", R, (0.5, 0.5, 0.0), 1, angle_min=0.0, angle_inc=0.0, pool=discs([(1.5, 0.75 + 1e-15)], [0.25]))
    add("self_index honoured", R, [centre, centre, centre], 16, pool=discs([(1.23, 0.97), (1.6, 1.3)], [0.2, 0.1]), self_index=[0, -1, 1])
    add("a segment parallel to the beam", R, (0.5, 0.5, 0.0), 1, angle_min=0.0, angle_inc=0.0, pool=([2], [[(1.0, 0.5), (1.5, 0.5)]], None), V=2)
    tri = [(1.0, 0.2), (1.6, 0.5), (1.0, 0.8)]          # the edge from the last vertex back to the first is the one the beam meets first
    add("a polygon's closing edge", R, (0.5, 0.5, 0.0), 1, angle_min=0.0, angle_inc=0.0, pool=([3], [tri], None), V=3)
    add("the same vertices as an open pair", R, (0.5, 0.5, 0.0), 1, angle_min=0.0, angle_inc=0.0, pool=([2], [tri], None), V=3)
    add("a pool entry nearer than the wall and one behind it", R, [(1.025, 1.025, 0.0)], 2, angle_min=0.0, angle_inc=math.pi, pool=discs([(1.8, 1.025), (-0.6, 1.025)], [0.1, 0.1]))
    add("a map/pool tie", R, (0.02, 1.0, 0.5), 6, pool=discs([(0.02, 1.0)], [0.1]))
    add("a pose that is not finite", R, [(math.nan, 1.0, 0.0), (1.0, math.inf, 0.0), (1.0, 1.0, math.nan), (1.0, 1.0, -math.inf), (1.0, 1.0, 1e18), centre], 9,
        pool=discs([(1.3, 1.0)], [0.05]))
    for mi in (0, 1):
        add(f"miss_is_inf {mi}", np.zeros((40, 48), np.uint8), centre, 5, range_max=1.5, miss_is_inf=mi)
    # a blocking cell at bit 63 and at bit 64 of a bitmap row: range_max 3.0 is Rc = 61, the row begins 61 cells left of the sensor's cell
    for bit in (63, 64):
        g = np.zeros((40, 48), np.uint8)
        g[20, 20 + bit - 61] = LETHAL
        add(f"a blocking cell at bit {bit}", g, (1.025, 1.025, 0.0), 3, angle_min=-0.01, angle_inc=0.01, hit_point=0)
    # what the pool can hold that is not a body: no vertices, numbers that are not finite, a point without a radius
    odd_nv = np.array([0, 1, 1, 2, 1, 3, -2], np.int32)
    odd_v = np.array([[(1.5, 1.0)] * 3, [(math.nan, 1.0)] * 3, [(1.5, 1.0)] * 3, [(1.5, 0.5), (1.5, math.inf), (0, 0)], [(1.5, 1.0)] * 3, [(1.6, 0.6), (1.7, 1.4), (1.9, 1.0)], [(1.4, 1.0)] * 3])
    add("pool entries that are skipped", R, centre, 32, pool=(odd_nv, odd_v, [0.1, 0.1, math.nan, 0.1, 0.0, 5.0, 0.1]), V=3)
    add("no hit, no info", R, [centre, (0.4, 1.6, -2.0)], 40, pool=ring_pool(5, centre, 0.2, 1.0, 3), V=3, no_hit=True, no_info=True)
    add("origin off zero, a sensor off the axis", R, [(0.3, 0.1, 3.0), (-0.9, -0.4, -3.1)], 90, origin=(-1.013, -0.927), sensor=(-0.1, 0.05, -2.0), res=0.05, range_max=2.0)
    assert {c.n for c in out} >= {1, 63, 64, 65, 257} and max(c.B for c in out) <= 8 and max(max(c.grid.shape) for c in out) <= 96
    return out


def random_cases(count=40, seed=28):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        W, H, B, n, V = int(rng.integers(8, 65)), int(rng.integers(8, 65)), int(rng.integers(1, 5)), int(rng.integers(1, 91)), int(rng.integers(1, 5))
        res = float(rng.choice([0.05, 0.1]))
        grid = rng.choice(np.array([0, 0, 50, 100, 253, LETHAL, UNKNOWN], np.uint8), size=(H, W), p=[0.5, 0.38, 0.02, 0.02, 0.02, 0.04, 0.02])
        origin = (float(rng.choice([0.0, -0.513])), float(rng.choice([0.0, 0.207])))
        pose = np.column_stack([origin[0] + rng.uniform(-0.1, 1.1, B) * W * res, origin[1] + rng.uniform(-0.1, 1.1, B) * H * res, rng.uniform(-4, 4, B)])
        P = int(rng.integers(0, 13))
        pool = None
        if P:
            nv = rng.integers(0, V + 1, P).astype(np.int32)
            pv = np.stack([origin[0] + rng.uniform(0, W * res, (P, V)), origin[1] + rng.uniform(0, H * res, (P, V))], 2)
            pv[:, 1:] = pv[:, :1] + rng.uniform(-0.3, 0.3, (P, V - 1, 2))
            pool = (nv, pv, None if rng.random() < 0.2 else rng.uniform(-0.05, 0.2, P))
        out.append(Case(f"random {k}", grid, pose, n, res=res, origin=origin, sensor=(float(rng.choice([0.0, -0.1])), 0.0, float(rng.choice([0.0, 0.5]))),
                        angle_min=float(rng.uniform(-3.5, 0)), angle_inc=float(rng.uniform(0.01, 0.1)), range_max=float(rng.choice([0.7, 2.0, 6.5])),
                        threshold=int(rng.choice([254, 253, 100])), unknown_blocks=int(rng.integers(0, 2)), hit_point=int(rng.integers(0, 2)), miss_is_inf=int(rng.integers(0, 2)),
                        pool=pool, V=V, self_index=None if rng.random() < 0.3 else rng.integers(-1, max(P, 1), B)))
    return out


def random_rooms(count=20, seed=28, W=64, H=48, poses=8):
    """rooms for the tests that are independent of the rule: a ring of walls, a few boxes and single cells inside; (grid, poses in free cells)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        g = room(W, H)
        for _ in range(int(rng.integers(2, 6))):
            x, y, w, h = int(rng.integers(2, W - 12)), int(rng.integers(2, H - 12)), int(rng.integers(1, 10)), int(rng.integers(1, 10))
            g[y:y + h, x:x + w] = LETHAL
        for _ in range(6):
            g[int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1))] = LETHAL
        free = np.argwhere(g == 0)
        at = free[rng.choice(len(free), poses, replace=False)]
        pose = np.column_stack([(at[:, 1] + rng.uniform(0.05, 0.95, poses)) * 0.05, (at[:, 0] + rng.uniform(0.05, 0.95, poses)) * 0.05, rng.uniform(-3.1, 3.1, poses)])
        out.append((g, pose))
    return out


# ---- the file format of the stand-alone program (tests/host_harness/scan_cast_host.cpp, -DSCH_MAIN)
def write_cases(path, cs):
    with open(path, "wb") as f:
        for c in cs:
            np.array([c.B, c.P, c.V, c.n, c.pr is not None, c.self_index is not None, not c.no_hit, not c.no_info], np.int32).tofile(f)
            c.ipar().tofile(f)
            c.dpar().tofile(f)
            c.grid.tofile(f)
            c.pose.tofile(f)
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
            ranges = np.fromfile(f, np.float32, c.B * c.n).reshape(c.B, c.n)
            hit = None if c.no_hit else np.fromfile(f, np.int32, c.B * c.n).reshape(c.B, c.n)
            out.append((ranges, hit, None if c.no_info else np.fromfile(f, np.int32, 4 * c.B).reshape(c.B, 4)))
        assert f.read() == b""
    return out
