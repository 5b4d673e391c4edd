"""Shared by tests/test_costmap_scans_host.py and tests/test_gpu_costmap_scans.py: the host build of mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp
(tests/host_harness/costmap_scans_host.cpp, g++ -ffp-contract=off) behind ctypes, the scripted cases, and a Python restatement of the rule written from the text of
include/mpc_costmap_scans.h and of the rule at the top of the .hpp, not from the header's code: the walk and the step count in Python integers (the step count by an
integer square root, where the header bisects), the roll by slices, the combination by numpy masks, every floating-point operation a Python float operation rounded on
its own, and the sine and cosine operation by operation with an exact fused multiply-add made from integer ratios (no math.sin, no math.fma).

A CASE is one call: one parameter set, B poses and scans, one window geometry, and the state (layer, layer_cell) and the window (cost) as they are before it."""
import ctypes as C
import math

import numpy as np

import _harness

_harness.SHARED.setdefault("costmap_scans_host", ("libmpc_costmap_scans.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip, bp, fp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_float)
d_ = lambda a: None if a is None else a.ctypes.data_as(dp)
i_ = lambda a: None if a is None else a.ctypes.data_as(ip)
b_ = lambda a: None if a is None else a.ctypes.data_as(bp)
f_ = lambda a: None if a is None else a.ctypes.data_as(fp)
LETHAL, UNKNOWN = 254, 255
POISON, IPOISON = 0xA5, -77
NAMES = ("layer", "layer_cell", "cost", "info")
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("costmap_scans_host"))
        lib.csh_scans.restype, lib.csh_scans.argtypes = C.c_int, [C.c_int, dp, ip, dp, fp, C.c_int, ip, C.c_int, C.c_int, C.c_double, bp, ip, bp, ip]
        lib.csh_sincos.restype, lib.csh_sincos.argtypes = None, [C.c_double, dp, dp]
        lib.csh_wrap.restype, lib.csh_wrap.argtypes = C.c_double, [C.c_double]
        lib.csh_steps.restype, lib.csh_steps.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int]
        lib.csh_origin_agrees.restype, lib.csh_origin_agrees.argtypes = C.c_int, [C.c_double, C.c_int, C.c_double, C.c_double, dp, ip]
        _lib = lib
    return _lib


class Case:
    """keep None: NULL.  layer0 / cell0 None: the poison.  cost0 None: the poison, or no window at all with no_cost.  no_info: info NULL."""

    def __init__(self, name, pose, ranges, size, res, anchor=(0.0, 0.0), sensor=(0.0, 0.0, 0.0), angle_min=-math.pi, angle_inc=None, range_min=0.1, range_max=10.0,
                 obstacle_range=3.0, raytrace_range=4.0, clear_radius=0.0, marking=1, clearing=1, inf_is_valid=0, track_unknown=1, method=1, keep=None, layer0=None,
                 cell0=None, cost0=None, no_cost=False, no_info=False):
        self.name = name
        self.pose = np.array(np.asarray(pose, float).reshape(-1, 3))
        self.B, (self.W, self.H) = self.pose.shape[0], (int(size[0]), int(size[1]))
        self.ranges = np.array(np.asarray(ranges, np.float32).reshape(self.B, -1))
        self.n = self.ranges.shape[1]
        self.res, self.anchor, self.sensor = float(res), tuple(map(float, anchor)), tuple(map(float, sensor))
        self.angle_min, self.angle_inc = float(angle_min), float(2 * math.pi / self.n if angle_inc is None else angle_inc)
        self.range_min, self.range_max, self.obstacle_range, self.raytrace_range, self.clear_radius = map(float, (range_min, range_max, obstacle_range, raytrace_range, clear_radius))
        self.marking, self.clearing, self.inf_is_valid, self.track_unknown, self.method = int(marking), int(clearing), int(inf_is_valid), int(track_unknown), int(method)
        self.keep = None if keep is None else np.array(np.broadcast_to(np.asarray(keep, np.int32), (self.B,)))          # np.array: a writable copy
        shape = (self.B, self.H, self.W)
        self.layer0 = np.full(shape, POISON, np.uint8) if layer0 is None else np.array(np.broadcast_to(np.asarray(layer0, np.uint8), shape))
        self.cell0 = np.full((self.B, 2), IPOISON, np.int32) if cell0 is None else np.ascontiguousarray(np.asarray(cell0, np.int32).reshape(self.B, 2))
        self.cost0 = None if no_cost else np.full(shape, POISON, np.uint8) if cost0 is None else np.array(np.broadcast_to(np.asarray(cost0, np.uint8), shape))
        self.no_info = bool(no_info)

    @property
    def default(self):
        return UNKNOWN if self.track_unknown else 0

    @property
    def R(self):
        return max(0, int(math.ceil(self.raytrace_range / self.res)))

    def dpar(self):
        return np.array(self.anchor + self.sensor + (self.angle_min, self.angle_inc, self.range_min, self.range_max, self.obstacle_range, self.raytrace_range, self.clear_radius))

    def ipar(self):
        return np.array([self.marking, self.clearing, self.inf_is_valid, self.track_unknown, self.method], np.int32)

    def struct(self):
        """the mpc_scan_params of the case"""
        from mpc_local_planner_amd._abi import MpcScanParams
        return MpcScanParams((C.c_double * 2)(*self.anchor), (C.c_double * 3)(*self.sensor), self.angle_min, self.angle_inc, self.range_min, self.range_max, self.obstacle_range,
                             self.raytrace_range, self.clear_radius, self.marking, self.clearing, self.inf_is_valid, self.track_unknown, self.method)

    def state(self):
        """(layer, layer_cell, cost or None, info or None) as they are before a call: copies; info a poison"""
        return (self.layer0.copy(), self.cell0.copy(), None if self.cost0 is None else self.cost0.copy(), None if self.no_info else np.full((self.B, 4), IPOISON, np.int32))

    def variant(self, name=None, **kw):
        """the same case with some constructor arguments replaced"""
        args = dict(pose=self.pose, ranges=self.ranges, size=(self.W, self.H), res=self.res, anchor=self.anchor, sensor=self.sensor, angle_min=self.angle_min,
                    angle_inc=self.angle_inc, range_min=self.range_min, range_max=self.range_max, obstacle_range=self.obstacle_range, raytrace_range=self.raytrace_range,
                    clear_radius=self.clear_radius, marking=self.marking, clearing=self.clearing, inf_is_valid=self.inf_is_valid, track_unknown=self.track_unknown,
                    method=self.method, keep=self.keep, layer0=self.layer0, cell0=self.cell0, cost0=self.cost0, no_cost=self.cost0 is None, no_info=self.no_info)
        args.update(kw)
        return Case(name or self.name, **args)

    def take(self, b):
        one = lambda a: None if a is None else a[b:b + 1]
        return self.variant(f"{self.name} [{b}]", pose=self.pose[b], ranges=self.ranges[b], keep=one(self.keep), layer0=one(self.layer0), cell0=one(self.cell0),
                            cost0=one(self.cost0))


def host_scans(c):
    """the host build: (layer, layer_cell, cost or None, info or None)"""
    layer, cell, cost, info = c.state()
    r = harness().csh_scans(c.B, d_(c.dpar()), i_(c.ipar()), d_(c.pose), f_(c.ranges), c.n, i_(c.keep), c.W, c.H, c.res, b_(layer), i_(cell), b_(cost), i_(info))
    assert r == c.R, (c.name, r, c.R)
    return layer, cell, cost, info


def same(a, b):
    """None when the two results are the same bytes, else the first array that differs"""
    for k, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            if x is not y:
                return f"{NAMES[k]}: one is missing"
            continue
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            where = np.argwhere(x != y)[:3].tolist() if x.shape == y.shape else (x.shape, y.shape)
            return f"{NAMES[k]} differs at {where}: {x[x != y][:3].tolist() if x.shape == y.shape else ''} for {y[x != y][:3].tolist() if x.shape == y.shape else ''}"
    return None


# ---- the restatement
PI, TWO_PI = math.pi, 2.0 * math.pi


def fma(a, b, c):
    """a * b + c rounded once: exact integer ratios (every denominator a power of two), and int / int is correctly rounded"""
    (na, da), (nb, db), (nc, dc) = a.as_integer_ratio(), b.as_integer_ratio(), c.as_integer_ratio()
    return (na * nb * dc + nc * da * db) / (da * db * dc)


def sincos(x):
    """(sin, cos) of x in [-pi, pi) as rule 3 states them: reduction by pi / 2 in two fused steps, two polynomials in z = r * r"""
    k = round(x * 6.36619772367581382433e-01)          # to nearest, ties to even
    r = fma(-float(k), 1.57079632673412561417e+00, x)
    r = fma(-float(k), 6.07710050650619224932e-11, r)
    z = r * r
    ps = fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08)
    for coeff in (2.75573137070700676789e-06, -1.98412698298579493134e-04, 8.33333333332248946124e-03, -1.66666666666666324348e-01):
        ps = fma(z, ps, coeff)
    s = fma(z * r, ps, r)
    pc = fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09)
    for coeff in (-2.75573143513906633035e-07, 2.48015872894767294178e-05, -1.38888888888741095749e-03, 4.16666666666666019037e-02):
        pc = fma(z, pc, coeff)
    hz = 0.5 * z
    w = 1.0 - hz
    c = w + (((1.0 - w) - hz) + (z * z) * pc)
    q = k % 4
    s1, c1 = (c, s) if q & 1 else (s, c)
    return (-s1 if q & 2 else s1), (-c1 if (q + 1) & 2 else c1)


def wrap(th):
    """normalize_theta with a multiplication by 1 / (2 pi); NaN for what is not finite"""
    if not math.isfinite(th):
        return math.nan
    if -PI <= th < PI:
        return th
    m = float(math.floor(th * 0.15915494309189533577))
    th = th - m * TWO_PI
    if th >= PI:
        th = th - TWO_PI
    if th < -PI:
        th = th + TWO_PI
    return th


def origin_axis(pose, size, res, anchor):
    """(origin, index) of rule 1 on one axis, None for an invalid pose"""
    if not math.isfinite(pose):
        return None
    s = (float(size - 1) + 0.5) * res
    q = ((pose - s / 2) - anchor) / res
    if not math.isfinite(q) or not abs(math.floor(q)) < 2 ** 30:
        return None
    c = math.floor(q)
    return anchor + float(c) * res, c


def _cell(w, origin, res):
    """the lattice cell of a world coordinate (an int), None when it is not finite"""
    f = (w - origin) / res
    return math.floor(f) if math.isfinite(f) else None


def steps(dx, dy, R):
    da, d2 = max(abs(dx), abs(dy)), dx * dx + dy * dy
    return da if d2 <= R * R else math.isqrt(R * R * da * da // d2)


def walk(x0, y0, dx, dy, n):
    """the cells costmap_2d's bresenham2D visits: n steps, n + 1 cells"""
    adx, ady = abs(dx), abs(dy)
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    xmajor = adx >= ady
    da, db = (adx, ady) if xmajor else (ady, adx)
    err, x, y, out = da // 2, x0, y0, []
    for _ in range(n):
        out.append((x, y))
        if xmajor:
            x += sx
        else:
            y += sy
        err += db
        if err >= da:
            if xmajor:
                y += sy
            else:
                x += sx
            err -= da
    out.append((x, y))
    return out


def python_scans(c, trace=None):
    """the restatement: (layer, layer_cell, cost or None, info or None).  trace, a list, receives per instance a dict: valid, shift, cleared (the set of window cells
    the walks visited), marked (the set of cells marked), rolled (the layer after the roll), walks [(k, dx, dy, steps)]"""
    layer, cell, cost, info = c.state()
    W, H, res, R, default = c.W, c.H, c.res, c.R, c.default
    for b in range(c.B):
        px, py, yaw = (float(v) for v in c.pose[b])
        ax = origin_axis(px, W, res, c.anchor[0])
        ay = origin_axis(py, H, res, c.anchor[1])
        t = dict(valid=False, shift=None, cleared=set(), marked=set(), rolled=None, walks=[])
        if trace is not None:
            trace.append(t)
        if ax is None or ay is None or not math.isfinite(yaw):
            layer[b], cell[b] = default, (0, 0)
            if info is not None:
                info[b] = (-1, 0, 0, 0)
            continue
        t["valid"] = True
        (ox, cx), (oy, cy) = ax, ay
        # roll
        L = np.full((H, W), default, np.uint8)
        if c.keep is not None and c.keep[b] != 0:
            sx, sy = cx - int(c.cell0[b, 0]), cy - int(c.cell0[b, 1])
            t["shift"] = (sx, sy)
            if abs(sx) < W and abs(sy) < H:
                # new(x, y) = old(x + sx, y + sy)
                x_lo, x_hi, y_lo, y_hi = max(0, -sx), min(W, W - sx), max(0, -sy), min(H, H - sy)
                L[y_lo:y_hi, x_lo:x_hi] = c.layer0[b, y_lo + sy:y_hi + sy, x_lo + sx:x_hi + sx]
        t["rolled"] = L.copy()
        cell[b] = (cx, cy)
        # beams
        kept, marks = 0, []
        heading = wrap(yaw)
        if -PI <= heading < PI:
            sn, cs = sincos(heading)
            sxw = px + (cs * c.sensor[0] - sn * c.sensor[1])
            syw = py + (sn * c.sensor[0] + cs * c.sensor[1])
            scx, scy = _cell(sxw, ox, res), _cell(syw, oy, res)
            sensor_in = scx is not None and scy is not None and 0 <= scx < W and 0 <= scy < H
            for k in range(c.n):
                r = float(c.ranges[b, k])
                if c.inf_is_valid and r == math.inf:
                    r = c.range_max - 1e-4
                if math.isnan(r) or r < c.range_min or r >= c.range_max:
                    continue
                th = wrap(((yaw + c.sensor[2]) + c.angle_min) + float(k) * c.angle_inc)
                if not -PI <= th < PI:
                    continue
                kept += 1
                bs, bc = sincos(th)
                ex, ey = sxw + r * bc, syw + r * bs
                ecx, ecy = _cell(ex, ox, res), _cell(ey, oy, res)
                if c.clearing and sensor_in:
                    dx, dy = ecx - scx, ecy - scy
                    n = steps(dx, dy, R)
                    t["walks"].append((k, dx, dy, n))
                    for x, y in walk(scx, scy, dx, dy, n):
                        if 0 <= x < W and 0 <= y < H:
                            L[y, x] = 0
                            t["cleared"].add((x, y))
                ddx, ddy = ex - sxw, ey - syw
                if ecx is not None and ecy is not None and 0 <= ecx < W and 0 <= ecy < H and ddx * ddx + ddy * ddy < c.obstacle_range * c.obstacle_range:
                    marks.append((ecx, ecy))
        if c.marking:
            for x, y in marks:
                L[y, x] = LETHAL
                t["marked"].add((x, y))
        if c.clear_radius > 0:
            wx = ox + (np.arange(W, dtype=np.float64) + 0.5) * res - px
            wy = oy + (np.arange(H, dtype=np.float64) + 0.5) * res - py
            L[(wx * wx)[None, :] + (wy * wy)[:, None] <= c.clear_radius * c.clear_radius] = 0
        layer[b] = L
        changed = 0
        if cost is not None:
            s = cost[b]
            take = (L != UNKNOWN) & ((s == UNKNOWN) | (s < L)) if c.method == 1 else (L != UNKNOWN)
            out = np.where(take, L, s)
            changed = int((out != s).sum())
            cost[b] = out
        if info is not None:
            info[b] = (kept, int((L == LETHAL).sum()), int((L == 0).sum()), changed)
    return layer, cell, cost, info


# ---- the scripted cases
def lattice_index(c):
    """(B, 2) the lattice index of every instance's origin (rule 1 by the restatement), zeros for an invalid one"""
    out = np.zeros((c.B, 2), np.int64)
    for b in range(c.B):
        ax, ay = origin_axis(float(c.pose[b, 0]), c.W, c.res, c.anchor[0]), origin_axis(float(c.pose[b, 1]), c.H, c.res, c.anchor[1])
        if ax is not None and ay is not None:
            out[b] = (ax[1], ay[1])
    return out


def filled_layer(shape, seed):
    """a layer that has been lived in: free, unknown, marks and a stray value"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, UNKNOWN, LETHAL, 7], np.uint8), size=shape, p=[0.5, 0.3, 0.15, 0.05])


def byte_map():
    """16 x 16: every byte value once"""
    return np.arange(256, dtype=np.uint8).reshape(16, 16)


def room_ranges(rng, B, n, lo, hi, odd=0.05):
    """ranges between lo and hi with a share of NaN, +inf and zeros"""
    r = rng.uniform(lo, hi, (B, n)).astype(np.float32)
    u = rng.random((B, n))
    r[u < odd] = np.nan
    r[(u >= odd) & (u < 2 * odd)] = np.inf
    r[(u >= 2 * odd) & (u < 2.5 * odd)] = 0.0
    return r


def cases():
    rng = np.random.default_rng(5)
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    centre = (1.53, 1.12, 0.3)
    # the window sizes and the beam counts: rows that are and are not whole 16-byte pieces; beams around the wave (64) and the workgroup (256)
    add("1 x 1, 1 beam", centre, [[0.3]], (1, 1), 0.05)
    add("7 x 5, 63 beams", [centre, (0.2, -0.4, -2.0)], room_ranges(rng, 2, 63, 0.1, 0.5), (7, 5), 0.1)
    add("17 x 16, 64 beams", [centre, (0.2, -0.4, 2.5)], room_ranges(rng, 2, 64, 0.1, 0.6), (17, 16), 0.05, inf_is_valid=1, range_max=0.9)
    add("33 x 20, 65 beams", centre, room_ranges(rng, 1, 65, 0.1, 1.2), (33, 20), 0.05, sensor=(0.1, -0.05, 0.4))
    demo = [(1.5, 1.1, 0.0), (0.3, 0.2, 1.0), (2.9, 2.1, -2.0)]
    add("55 x 55, the demo's, 360 beams", demo, room_ranges(rng, 3, 360, 0.3, 4.5), (55, 55), 0.1, obstacle_range=3.0, raytrace_range=4.0, cost0=0)
    add("55 x 55, carlike, 360 beams", demo, room_ranges(rng, 3, 360, 0.3, 4.5), (55, 55), 0.1, obstacle_range=3.0, raytrace_range=3.5, sensor=(0.3, 0.0, 0.0), clear_radius=0.2,
        cost0=rng.choice(np.array([0, 0, 0, 254, 255], np.uint8), size=(3, 55, 55)))
    add("256 x 256, the limit, 257 beams", [(6.4, 6.4, 0.7), (-3.1, 2.2, -0.7)], room_ranges(rng, 2, 257, 0.5, 8.0), (256, 256), 0.05, obstacle_range=6.0, raytrace_range=7.0)
    add("64 x 48, 4096 beams", centre, room_ranges(rng, 1, 4096, 0.2, 2.0), (64, 48), 0.05)
    # the walk: along each axis and each diagonal from the centre of a cell, the ties |dx| = |dy|, other octants between them
    mid = (0.525 + 0.5 * 0.05 * 20, 0.525 + 0.5 * 0.05 * 20, 0.0)          # the sensor at the centre of window cell (10, 10) of 21 x 21
    add("axes and diagonals", mid, [[0.3, 0.3 * math.sqrt(2), 0.3, 0.3 * math.sqrt(2)] * 2], (21, 21), 0.05, angle_inc=math.pi / 4, range_min=0.0)
    add("sixteen octant halves", mid, [[0.4] * 16], (21, 21), 0.05, angle_inc=math.pi / 8, angle_min=-math.pi + 0.2)
    add("a zero-length ray", mid, [[0.0, 0.001]], (21, 21), 0.05, range_min=0.0)
    # truncation by raytrace_range, R = 5 cells: (20, 0) gives 5 steps by either formula; (12, 9) has hypot 15, so R da / hypot = 4 exactly: costmap_2d's doubles may give 3
    add("truncated, the formulas agree", mid, [[1.0]], (61, 61), 0.05, angle_min=0.0, angle_inc=0.1, raytrace_range=0.25)
    add("truncated, the formulas could part", mid, [[0.75, 0.5]], (61, 61), 0.05, angle_min=math.atan2(9, 12), angle_inc=math.atan2(4, 3) - math.atan2(9, 12), raytrace_range=0.25)
    # obstacle_range: beam 0 along +x from the origin of the world returns exactly at it; beam 1 one float below it
    below = np.nextafter(np.float32(2.5), np.float32(0))
    add("a return exactly at obstacle_range and one just inside", (0.0, 0.0, 0.0), [[2.5, below]], (120, 120), 0.05, angle_min=0.0, angle_inc=math.pi / 2, obstacle_range=2.5)
    add("returns outside the window", centre, rng.uniform(2.0, 2.5, (1, 40)), (20, 20), 0.05)
    # the sensor 5 m ahead of the robot, far outside a 1 m window; the beams that point back at the robot end inside it
    add("the sensor's cell outside the window", (1.0, 1.0, 0.0), np.full((1, 33), 5.0), (20, 20), 0.05, sensor=(5.0, 0.0, 0.0), angle_min=math.pi - 0.08, angle_inc=0.005,
        obstacle_range=6.0, raytrace_range=6.0)
    odd = [[math.nan, 0.05, 10.0, math.inf, -math.inf, 1.0, 0.1, np.nextafter(np.float32(10.0), np.float32(0))]]
    for iv in (0, 1):
        add(f"NaN, below range_min, at range_max, inf; inf_is_valid {iv}", mid, odd, (61, 61), 0.05, inf_is_valid=iv, obstacle_range=20.0, raytrace_range=20.0)
    # the combination: a window holding every byte value under a layer with free, marked and untouched cells
    for method in (0, 1):
        for tu in (0, 1):
            add(f"every byte value, method {method}, track_unknown {tu}", (0.4, 0.4, 0.9), room_ranges(rng, 1, 24, 0.1, 0.35, odd=0.0), (16, 16), 0.05, method=method,
                track_unknown=tu, cost0=byte_map())
    add("the disc", [(1.0, 1.0, 0.0), (1.02, 0.97, 1.0)], np.tile(np.linspace(0.1, 0.6, 36, dtype=np.float32), (2, 1)), (30, 30), 0.05, clear_radius=0.3, range_min=0.05)
    # the rolls: the layer moves by (c_new - layer_cell); eight shifts a case
    W, H = 19, 13
    poses = np.column_stack([rng.uniform(-2, 2, 8), rng.uniform(-2, 2, 8), rng.uniform(-3, 3, 8)])
    for name, shifts, scan in (("rolls of 0, +-1 and W - 1 cells", [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (W - 1, 0), (0, -(H - 1)), (-(W - 1), H - 1)], False),
                               ("rolls of a window or more, and diagonal ones", [(W, 0), (0, H), (-W, 0), (0, -H - 5), (1, 1), (-3, 2), (W + 3, 2), (2 ** 31 - 5, 0)], False),
                               ("rolls under a scan", [(0, 0), (1, 0), (-1, 1), (0, -2), (5, 5), (-(W - 1), 0), (W, H), (2, -3)], True)):
        base = Case(name, poses, room_ranges(rng, 8, 40, 0.1, 0.6), (W, H), 0.05, keep=1, layer0=filled_layer((8, H, W), 11), marking=int(scan), clearing=int(scan))
        cell0 = lattice_index(base) - np.array(shifts, np.int64)
        out.append(base.variant(cell0=np.clip(cell0, -2 ** 31, 2 ** 31 - 1)))
    add("keep 0 after a filled layer", poses[:4], room_ranges(rng, 4, 20, 0.1, 0.5), (W, H), 0.05, keep=[0, 1, 0, 1], layer0=filled_layer((4, H, W), 12),
        cell0=lattice_index(Case("", poses[:4], np.zeros((4, 1)), (W, H), 0.05)))
    add("keep NULL after a filled layer", poses[:2], room_ranges(rng, 2, 20, 0.1, 0.5), (W, H), 0.05, layer0=filled_layer((2, H, W), 13), cell0=[[3, 4], [5, 6]], track_unknown=0)
    add("a pose that is not finite", [(math.nan, 1.0, 0.0), (1.0, math.inf, 0.0), (1.0, 1.0, math.nan), (1.0, 1.0, -math.inf), (1e300, 1.0, 0.0), (1.0, -4e9, 0.0), (1.0, 1.0, 1e18),
                                     centre], room_ranges(rng, 8, 30, 0.1, 0.4), (9, 7), 0.05, keep=1, layer0=filled_layer((8, 7, 9), 14), cell0=np.zeros((8, 2)))
    add("anchor off zero, no window, no info", [(-1.6, -2.1, 3.0), (-2.9, -2.9, -3.1)], room_ranges(rng, 2, 90, 0.1, 1.0), (21, 19), 0.1, anchor=(0.013, -0.027),
        sensor=(-0.2, 0.1, -2.0), no_cost=True, no_info=True)
    add("marking off", centre, room_ranges(rng, 1, 50, 0.1, 0.5), (20, 20), 0.05, marking=0)
    add("clearing off", centre, room_ranges(rng, 1, 50, 0.1, 0.5), (20, 20), 0.05, clearing=0)
    assert {(c.W, c.H) for c in out} >= {(1, 1), (7, 5), (17, 16), (55, 55), (256, 256)} and {c.n for c in out} >= {1, 63, 64, 65, 257, 360} and max(c.B for c in out) <= 8
    return out


def random_cases(count=60, seed=27):
    """a second cycle each: a lived-in layer a few cells off, most instances keeping it"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        W, H, B, n = int(rng.integers(1, 41)), int(rng.integers(1, 41)), int(rng.integers(1, 9)), int(rng.integers(1, 131))
        res = float(rng.choice([0.05, 0.1]))
        span = max(W, H) * res
        pose = np.column_stack([rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-4, 4, B)])
        base = Case(f"random {k}", pose, room_ranges(rng, B, n, 0.05, 0.2 + 0.8 * span), (W, H), res, anchor=(float(rng.choice([0.0, 0.02])), 0.0),
                    sensor=(float(rng.choice([0.0, 0.1])), 0.0, float(rng.choice([0.0, 0.5]))), angle_min=float(rng.uniform(-3.5, 0)), angle_inc=float(rng.uniform(0.01, 0.1)),
                    range_min=0.1, range_max=float(rng.choice([1.0, 3.0])), obstacle_range=float(rng.choice([0.6, 2.5])), raytrace_range=float(rng.choice([0.5, 3.0])),
                    clear_radius=float(rng.choice([0.0, 0.0, 0.12])), marking=int(rng.random() < 0.9), clearing=int(rng.random() < 0.9), inf_is_valid=int(rng.integers(0, 2)),
                    track_unknown=int(rng.integers(0, 2)), method=int(rng.random() < 0.8), keep=(rng.random(B) < 0.8).astype(np.int32),
                    layer0=rng.choice(np.array([0, UNKNOWN, LETHAL], np.uint8), size=(B, H, W), p=[0.55, 0.35, 0.1]),
                    cost0=rng.choice(np.array([0, 0, 0, 100, 253, 254, 255], np.uint8), size=(B, H, W)))
        shift = rng.integers(-2, 3, (B, 2))
        out.append(base.variant(cell0=lattice_index(base) - shift))
    return out


# ---- the file format of the stand-alone program (tests/host_harness/costmap_scans_host.cpp, -DCSH_MAIN)
def write_cases(path, cs):
    with open(path, "wb") as f:
        for c in cs:
            np.array([c.B, c.W, c.H, c.n, c.keep is not None, c.cost0 is not None, not c.no_info], np.int32).tofile(f)
            c.ipar().tofile(f)
            np.concatenate([[c.res], c.dpar()]).tofile(f)
            c.pose.tofile(f)
            c.ranges.tofile(f)
            if c.keep is not None:
                c.keep.tofile(f)
            c.layer0.tofile(f)
            c.cell0.tofile(f)
            if c.cost0 is not None:
                c.cost0.tofile(f)


def read_outputs(path, cs):
    out = []
    with open(path, "rb") as f:
        for c in cs:
            cells = c.B * c.H * c.W
            layer = np.fromfile(f, np.uint8, cells).reshape(c.B, c.H, c.W)
            cell = np.fromfile(f, np.int32, 2 * c.B).reshape(c.B, 2)
            cost = None if c.cost0 is None else np.fromfile(f, np.uint8, cells).reshape(c.B, c.H, c.W)
            out.append((layer, cell, cost, None if c.no_info else np.fromfile(f, np.int32, 4 * c.B).reshape(c.B, 4)))
        assert f.read() == b""
    return out
