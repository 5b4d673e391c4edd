"""Shared by tests/test_costmap_window_host.py and tests/test_gpu_costmap_window.py: the host build of mpc_local_planner_amd/csrc/mpc_costmap_window.hpp
(tests/host_harness/costmap_window_host.cpp, g++ -ffp-contract=off) behind ctypes, the scripted cases, and a Python restatement of the rule written from the text of
include/mpc_costmap_window.h, not from the header's code: the nearest lethal cell by brute force in Python integers, the table with math.sqrt / math.exp, the origin
in numpy float64 scalars, one rounded operation after the other.

A CASE is one call: one map, one parameter set, B poses, one window geometry."""
import ctypes as C
import math

import numpy as np

import _harness

_harness.SHARED.setdefault("costmap_window_host", ("libmpc_costmap_window.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
d_ = lambda a: None if a is None else a.ctypes.data_as(dp)
i_ = lambda a: None if a is None else a.ctypes.data_as(ip)
b_ = lambda a: None if a is None else a.ctypes.data_as(bp)
LETHAL, INSCRIBED, UNKNOWN = 254, 253, 255
POISON, DPOISON, IPOISON = 0xA5, -7.25, -77
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("costmap_window_host"))
        lib.cwh_window.restype, lib.cwh_window.argtypes = C.c_int, [C.c_int, bp, dp, ip, dp, C.c_int, C.c_int, C.c_double, bp, dp, ip, ip]
        lib.cwh_table.restype, lib.cwh_table.argtypes = None, [C.c_double, C.c_double, C.c_double, C.c_int, bp]
        for name in ("cwh_tile_x", "cwh_tile_y", "cwh_max_r"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, []
        _lib = lib
    return _lib


def tile():
    """(kCwTileX, kCwTileY): the window cells of one workgroup of the kernel"""
    return int(harness().cwh_tile_x()), int(harness().cwh_tile_y())


class Case:
    def __init__(self, name, map_cost, pose, size, res, map_res=0.05, map_origin=(0.0, 0.0), anchor=(0.0, 0.0), inscribed=0.17, inflation=0.0, scaling=10.0, outside=0,
                 inflate_unknown=0):
        self.name = name
        self.map = np.ascontiguousarray(map_cost, dtype=np.uint8)
        self.pose = np.ascontiguousarray(np.asarray(pose, float).reshape(-1, 3))
        self.B, (self.W, self.H) = self.pose.shape[0], (int(size[0]), int(size[1]))
        self.res, self.map_res, self.map_origin, self.anchor = float(res), float(map_res), tuple(map(float, map_origin)), tuple(map(float, anchor))
        self.inscribed, self.inflation, self.scaling, self.outside, self.iu = float(inscribed), float(inflation), float(scaling), int(outside), int(inflate_unknown)

    @property
    def r(self):
        return 0 if self.inflation <= 0 else int(math.ceil(np.float64(self.inflation) / np.float64(self.res)))

    def dpar(self):
        return np.array(self.map_origin + (self.map_res,) + self.anchor + (self.inscribed, self.inflation, self.scaling))

    def ipar(self):
        return np.array([self.map.shape[1], self.map.shape[0], self.outside, self.iu], np.int32)

    def struct(self):
        """the mpc_window_params of the case"""
        from mpc_local_planner_amd._abi import MpcWindowParams
        D2 = C.c_double * 2
        return MpcWindowParams(D2(*self.map_origin), self.map_res, D2(*self.anchor), self.inscribed, self.inflation, self.scaling, self.map.shape[1], self.map.shape[0],
                               self.outside, self.iu)

    def outputs(self):
        """(cost, origin, info) as they are before a call: every word a poison"""
        return np.full((self.B, self.H, self.W), POISON, np.uint8), np.full((self.B, 2), DPOISON), np.full((self.B, 4), IPOISON, np.int32)

    def with_poses(self, pose, name=None):
        return Case(name or self.name, self.map, pose, (self.W, self.H), self.res, self.map_res, self.map_origin, self.anchor, self.inscribed, self.inflation, self.scaling,
                    self.outside, self.iu)

    def take(self, b):
        return self.with_poses(self.pose[b], f"{self.name} [{b}]")


def host_window(c, want_d2=False):
    """the host build: (cost, origin, info), with want_d2 also rule 3's d2 per window cell (-1: none)"""
    cost, origin, info = c.outputs()
    d2 = np.full((c.B, c.H, c.W), IPOISON, np.int32) if want_d2 else None
    r = harness().cwh_window(c.B, b_(c.map), d_(c.dpar()), i_(c.ipar()), d_(c.pose), c.W, c.H, c.res, b_(cost), d_(origin), i_(info), i_(d2))
    assert r == c.r, (c.name, r, c.r)
    return (cost, origin, info, d2) if want_d2 else (cost, origin, info)


def same(a, b):
    """None when the two results are the same bytes, else the first array that differs"""
    for k, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            where = np.argwhere(x != y)[:3].tolist() if x.shape == y.shape else (x.shape, y.shape)
            return f"{('cost', 'origin', 'info')[k]} differs at {where}"
    return None


# ---- the restatement
def table_of(c):
    res, r = np.float64(c.res), c.r
    out = [LETHAL]
    for d2 in range(1, r * r + 1):
        dist = float(np.float64(math.sqrt(d2)) * res)
        out.append(INSCRIBED if dist <= c.inscribed else int(252 * math.exp(-c.scaling * (dist - c.inscribed))))
    return out


def _origin_axis(pose, size, res, anchor):
    with np.errstate(all="ignore"):
        pose, res, anchor = np.float64(pose), np.float64(res), np.float64(anchor)
        s = (np.float64(size - 1) + np.float64(0.5)) * res
        half = s / np.float64(2)
        a = pose - half
        a = a - anchor
        q = a / res
        cx = np.floor(q)
        if not np.isfinite(pose) or not abs(cx) < 2.0 ** 30:
            return None
        off = cx * res
        return anchor + off


def _index_axis(origin, m, res, map_origin, map_res, map_size):
    c = (np.float64(m) + np.float64(0.5)) * np.float64(res)
    w = np.float64(origin) + c
    if w < map_origin:
        return -1
    d = w - np.float64(map_origin)
    f = d / np.float64(map_res)
    if not f < 2147483000.0:
        return -1
    k = int(f)
    return k if k < map_size else -1


def python_window(c):
    cost, origin, info = c.outputs()
    r, table = c.r, table_of(c)
    mh, mw = c.map.shape
    for b in range(c.B):
        ox, oy = _origin_axis(c.pose[b, 0], c.W, c.res, c.anchor[0]), _origin_axis(c.pose[b, 1], c.H, c.res, c.anchor[1])
        if ox is None or oy is None:
            cost[b], origin[b], info[b] = c.outside, c.anchor, (-1, 0, 0, 0)
            continue
        origin[b] = (ox, oy)
        mx = {i: _index_axis(ox, i, c.res, c.map_origin[0], c.map_res, mw) for i in range(-r, c.W + r)}
        my = {j: _index_axis(oy, j, c.res, c.map_origin[1], c.map_res, mh) for j in range(-r, c.H + r)}
        s, lethal = {}, []
        inside = n_lethal = halo = changed = 0
        for j in range(-r, c.H + r):
            for i in range(-r, c.W + r):
                isin = mx[i] >= 0 and my[j] >= 0
                v = int(c.map[my[j], mx[i]]) if isin else c.outside
                s[i, j] = v
                window = 0 <= i < c.W and 0 <= j < c.H
                inside += window and isin
                if v == LETHAL:
                    lethal.append((i, j))
                    n_lethal += window
                    halo += not window
        offsets = [(di, dj) for di in range(-r, r + 1) for dj in range(-r, r + 1) if di * di + dj * dj <= r * r]
        for j in range(c.H):
            for i in range(c.W):
                v, best = s[i, j], None
                if r > 0 and lethal:
                    if len(lethal) <= len(offsets):
                        near = [(i - a) ** 2 + (j - e) ** 2 for a, e in lethal]
                        near = [d for d in near if d <= r * r]
                    else:
                        near = [di * di + dj * dj for di, dj in offsets if s[i + di, j + dj] == LETHAL]
                    best = min(near) if near else None
                out = v
                if best is not None:
                    t = table[best]
                    if v == UNKNOWN:
                        out = t if (t > 0 if c.iu else t >= INSCRIBED) else UNKNOWN
                    else:
                        out = max(v, t)
                cost[b, j, i] = out
                changed += out != v
        info[b] = (inside, n_lethal, changed, halo)
    return cost, origin, info


# ---- the scripted cases
def scripted_map(w=60, h=44, seed=3):
    """every byte value, walls of lethal cells, a patch of unknown and a patch of inscribed cells"""
    rng = np.random.default_rng(seed)
    m = np.where(rng.random((h, w)) < 0.5, 0, rng.integers(1, 253, (h, w))).astype(np.uint8)
    m[0, :] = LETHAL; m[-1, :] = LETHAL; m[:, 0] = LETHAL; m[:, -1] = LETHAL
    m[10, 8:30] = LETHAL; m[10:30, 30] = LETHAL
    m[20:26, 40:50] = UNKNOWN
    m[30:33, 5:12] = INSCRIBED
    m[36, 20] = LETHAL; m[37, 21] = UNKNOWN; m[35, 19] = UNKNOWN; m[36, 22] = INSCRIBED; m[35, 20] = 252; m[37, 20] = 1
    return m


def byte_map():
    """16 x 16: every byte value once, 254 at (14, 15) and 255 at (15, 15)"""
    return np.arange(256, dtype=np.uint8).reshape(16, 16)


def cases():
    tx, ty = tile()
    m = scripted_map()
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    centre = (1.5, 1.1, 0.3)
    add("1 x 1", m, centre, (1, 1), 0.05)
    add("1 x 1, r 5: a window smaller than r", m, [(0.52, 0.52, 0.0), (1.52, 0.8, 0.0)], (1, 1), 0.05, inflation=0.25)
    add("7 x 5, 2 : 1, r 1", m, centre, (7, 5), 0.1, inflation=0.1)
    add("17 x 16, 0.07 over 0.05, r 5", m, [centre, (0.4, 1.9, 0.0)], (17, 16), 0.07, inflation=0.35, inflate_unknown=1)
    add("17 x 16, r 32", m, centre, (17, 16), 0.05, inflation=1.6)
    demo = [(1.5, 1.1, 0.0), (0.3, 0.2, 1.0), (2.9, 2.1, -2.0)]
    add("55 x 55, the demo's", m, demo, (55, 55), 0.1, outside=255)
    add("55 x 55, inflated", m, demo, (55, 55), 0.1, inflation=0.5, outside=255)
    add("three tiles wide", m, [(1.0, 1.0, 0.0), (3.1, 0.1, 0.0)], (2 * tx + 2, 3), 0.05, inflation=0.05)
    add("three tiles high", m, [(1.0, 1.0, 0.0), (0.1, 2.3, 0.0)], (3, 2 * ty + 2), 0.05, inflation=1.6)
    add("three tiles wide, 2 : 1, r 5", m, (1.5, 1.1, 0.0), (2 * tx + 9, 20), 0.025, map_res=0.05, inflation=0.125)
    # the four edges of the 3.0 m x 2.2 m map, a corner, wholly outside: 20 x 20 windows of 1 m
    edges = [(0.1, 1.1, 0.0), (2.95, 1.1, 0.0), (1.5, 0.05, 0.0), (1.5, 2.15, 0.0), (2.9, 2.2, 0.0), (-3.0, -3.0, 0.0), (9.0, 1.0, 0.0)]
    for outside in (0, 255):
        for iu in (0, 1):
            add(f"edges, outside {outside}, inflate_unknown {iu}", m, edges, (20, 20), 0.05, inflation=0.3, outside=outside, inflate_unknown=iu)
    add("edges, no inflation", m, edges, (20, 20), 0.05, outside=255)
    # every byte value under an inflation from (14, 15): the window is the map
    for iu in (0, 1):
        add(f"every byte value, inflate_unknown {iu}", byte_map(), (0.4, 0.4, 0.0), (16, 16), 0.05, inflation=0.4, inflate_unknown=iu, inscribed=0.12)
    add("every byte value, r 0", byte_map(), (0.4, 0.4, 0.0), (16, 16), 0.05)
    # lethal cells in the halo only: the window lies two cells inside the wall at j = 10
    add("a lethal cell in the halo only", m, (0.725, 0.325, 0.0), (8, 6), 0.05, inflation=0.2)
    # poses on a lattice line and 1e-12 m below it; 0.25 is a power of two, so the line is hit exactly: sx / 2 = 0.5625
    on = [0.5625 + 0.25 * k for k in (2, -3, 0)]
    line = [(x, x, 0.0) for x in on] + [(x - 1e-12, x - 1e-12, 0.0) for x in on]
    add("a pose on a lattice line and just below it", m, line, (5, 5), 0.25, map_res=0.05, inflation=0.25)
    add("a pose that is not finite", m, [(math.nan, 1.0, 0.0), (1.0, math.inf, 0.0), (1e300, 1.0, 0.0), (1.0, -4e9, 0.0), centre], (9, 7), 0.05, inflation=0.1, outside=255)
    add("anchor and map origin off zero", m, [(-1.6, -2.1, 0.0), (-2.9, -2.9, 0.0)], (21, 19), 0.1, map_origin=(-3.0, -3.0), anchor=(0.013, -0.027), inflation=0.3, scaling=3.0,
        inscribed=0.0)
    assert any(c.W > 2 * tx for c in out) and any(c.H > 2 * ty for c in out)
    assert {c.r for c in out} >= {0, 1, 5, 32} and any(min(c.W, c.H) < c.r for c in out) and max(c.B for c in out) <= 8
    return out


def random_cases(count=60, seed=21):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        w, h = int(rng.integers(8, 50)), int(rng.integers(8, 50))
        m = rng.integers(0, 253, (h, w)).astype(np.uint8)
        m[rng.random((h, w)) < 0.4] = 0
        m[rng.random((h, w)) < rng.choice([0.005, 0.02, 0.08])] = LETHAL
        m[rng.random((h, w)) < 0.03] = UNKNOWN
        m[rng.random((h, w)) < 0.02] = INSCRIBED
        map_res = float(rng.choice([0.05, 0.1]))
        res = float(rng.choice([0.05, 0.07, 0.1, 0.025]))
        origin = (float(rng.uniform(-2, 1)), float(rng.uniform(-2, 1)))
        B = int(rng.integers(1, 9))
        pose = np.stack([rng.uniform(origin[0] - 0.5, origin[0] + w * map_res + 0.5, B), rng.uniform(origin[1] - 0.5, origin[1] + h * map_res + 0.5, B), rng.uniform(-3, 3, B)], 1)
        r = int(rng.choice([0, 1, 2, 3, 6]))
        out.append(Case(f"random {k}", m, pose, (int(rng.integers(1, 24)), int(rng.integers(1, 24))), res, map_res=map_res, map_origin=origin,
                        anchor=(float(rng.choice([0.0, 0.02])), 0.0), inscribed=float(rng.choice([0.0, 0.1, 0.17])), inflation=r * res * 0.97, scaling=float(rng.choice([0.0, 3.0, 10.0])),
                        outside=int(rng.choice([0, 255])), inflate_unknown=int(rng.integers(0, 2))))
    return out


# ---- the file format of the stand-alone program (tests/host_harness/costmap_window_host.cpp, -DCWH_MAIN)
def write_cases(path, cs):
    with open(path, "wb") as f:
        for c in cs:
            np.array([c.B, c.W, c.H, c.map.shape[1], c.map.shape[0], c.outside, c.iu, 1], np.int32).tofile(f)
            np.concatenate([[c.res], c.dpar()]).tofile(f)
            c.map.tofile(f)
            c.pose.tofile(f)


def read_outputs(path, cs):
    out = []
    with open(path, "rb") as f:
        for c in cs:
            cost = np.fromfile(f, np.uint8, c.B * c.H * c.W).reshape(c.B, c.H, c.W)
            origin = np.fromfile(f, np.float64, 2 * c.B).reshape(c.B, 2)
            out.append((cost, origin, np.fromfile(f, np.int32, 4 * c.B).reshape(c.B, 4)))
        assert f.read() == b""
    return out
