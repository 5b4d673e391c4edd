"""Shared by tests/test_costmap_clusters_host.py and tests/test_gpu_costmap_clusters.py: the host build of mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp
(tests/host_harness/costmap_clusters_host.cpp, g++ -ffp-contract=off) behind ctypes, the scripted cases, and a Python restatement of the rule written from
include/mpc_costmap_clusters.h, not from the header's code: the clusters are scipy.spatial.cKDTree.query_pairs + scipy.sparse.csgraph.connected_components re-keyed by
their first cell, the hull is a monotone chain in Python integers, the robot test is plain Python floats.

A CASE is one call: B maps of one geometry, one parameter set, the containers as they are before the call (every word a sentinel)."""
import ctypes as C
import math

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import _harness

_harness.SHARED.setdefault("costmap_clusters_host", ("libmpc_costmap_clusters.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
SENTINEL = -7.25          # what the container holds before a call: the call must leave it in every slot and vertex it does not write
ISENTINEL = -5
LETHAL = 254
MAX_SPAN = 4096           # columns a cluster of several rows may span and still get its hull (include/mpc_costmap_clusters.h)
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("costmap_clusters_host"))
        lib.cch_polygons.restype, lib.cch_polygons.argtypes = None, [C.c_int, bp, C.c_int, C.c_int, C.c_double, dp, dp, C.c_double, C.c_int, C.c_int, C.c_int, ip, ip, dp, dp, dp, ip, ip]
        _lib = lib
    return _lib


def d_(a):
    return None if a is None else a.ctypes.data_as(dp)


def i_(a):
    return None if a is None else a.ctypes.data_as(ip)


class Case:
    """cost: uint8 [B][size_y][size_x] (or one map); origin [B][2]; pose [B][3]"""

    def __init__(self, name, cost, pose, link, V=8, O=64, res=0.0625, origin=(0.0, 0.0), behind=100.0, radius=True, velocity=True):
        cost = np.ascontiguousarray(cost, dtype=np.uint8)
        self.cost = cost[None] if cost.ndim == 2 else cost
        self.name, self.B, self.H, self.W = name, self.cost.shape[0], self.cost.shape[1], self.cost.shape[2]
        self.pose = np.broadcast_to(np.asarray(pose, dtype=np.float64), (self.B, 3)).copy()
        self.origin = np.broadcast_to(np.asarray(origin, dtype=np.float64), (self.B, 2)).copy()
        self.link, self.V, self.O, self.res, self.behind, self.radius, self.velocity = int(link), int(V), int(O), float(res), float(behind), radius, velocity

    def container(self):
        """(n_obstacles, n_vertices, vertices, radius | None, velocity | None) as they are before the call"""
        B, O, V = self.B, self.O, self.V
        return (np.full(B, ISENTINEL, np.int32), np.full((B, O), ISENTINEL, np.int32), np.full((B, O, V, 2), SENTINEL), np.full((B, O), SENTINEL) if self.radius else None,
                np.full((B, O, 2), SENTINEL) if self.velocity else None)

    def take(self, b):
        return Case(f"{self.name} [{b}]", self.cost[b], self.pose[b], self.link, self.V, self.O, self.res, self.origin[b], self.behind, self.radius, self.velocity)


def host_polygons(c):
    """the host build: (n_obstacles, n_vertices, vertices, radius, velocity, dropped, info)"""
    no, nv, vt, rd, vl = c.container()
    dr, info = np.full(c.B, -1, np.int32), np.full((c.B, 4), -1, np.int32)
    harness().cch_polygons(c.B, c.cost.ctypes.data_as(bp), c.W, c.H, c.res, d_(c.origin), d_(c.pose), c.behind, c.link, c.V, c.O, i_(no), i_(nv), d_(vt), d_(rd), d_(vl), i_(dr), i_(info))
    return no, nv, vt, rd, vl, dr, info


# ---- the restatement
def kept_cells(c, b):
    """the kept cells of instance b as an int array [K][2] of (i, j), in scan order"""
    cost, (ox, oy), (px, py, th) = c.cost[b], c.origin[b], c.pose[b]
    hx, hy = math.cos(th), math.sin(th)
    out = []
    for i in range(c.W - 1):
        wx = ox + (np.float64(i) + 0.5) * c.res
        for j in range(c.H - 1):
            if cost[j, i] != LETHAL:
                continue
            wy = oy + (np.float64(j) + 0.5) * c.res
            dx, dy = np.float64(wx - px), np.float64(wy - py)
            dot = dx * hx + dy * hy
            if dot < 0.0 and math.sqrt(dx * dx + dy * dy) > c.behind:
                continue
            out.append((i, j))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def clusters_of(cells, link):
    """lists of cell rows, one per connected component, ordered by first cell"""
    K = len(cells)
    if K == 0:
        return []
    pairs = cKDTree(cells.astype(np.float64)).query_pairs(math.sqrt(link) + 1e-6, output_type="ndarray")
    if len(pairs):
        d = cells[pairs[:, 0]] - cells[pairs[:, 1]]
        pairs = pairs[(d * d).sum(axis=1) <= link]
    g = coo_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(K, K)) if len(pairs) else coo_matrix((K, K))
    _, lab = connected_components(g, directed=False)
    groups = {}
    for k in range(K):
        groups.setdefault(int(lab[k]), []).append(k)
    return sorted(groups.values(), key=lambda g_: g_[0])


def cross(o, a, b):
    return (int(a[0]) - int(o[0])) * (int(b[1]) - int(o[1])) - (int(a[1]) - int(o[1])) * (int(b[0]) - int(o[0]))


def hull_of(pts):
    """Andrew's monotone chain on sorted integer points, collinear points dropped; counter-clockwise from the first point"""
    pts = [tuple(int(x) for x in p) for p in pts]
    if len(pts) == 1:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def python_polygons(c):
    no, nv, vt, rd, vl = c.container()
    dr, info = np.zeros(c.B, np.int32), np.zeros((c.B, 4), np.int32)
    for b in range(c.B):
        (ox, oy), (px, py, _) = c.origin[b], c.pose[b]
        world = lambda i, j: (ox + (np.float64(i) + 0.5) * c.res, oy + (np.float64(j) + 0.5) * c.res)
        u, v = float(np.float64(px - ox) / c.res - 0.5), float(np.float64(py - oy) / c.res - 0.5)
        cells = kept_cells(c, b)
        out, boxes, as_cells = [], 0, 0          # out: lists of (i, j) vertices
        groups = clusters_of(cells, c.link)
        for g in groups:
            pts = cells[g]
            h = hull_of(pts)
            imin, jmin = pts.min(axis=0)
            imax, jmax = pts.max(axis=0)
            box = len(h) > c.V or (imax - imin + 1 > MAX_SPAN and jmin < jmax)          # (a single row is a line whatever it spans, and the chain gives it)
            if box:
                boxes += 1
                h = [(imin, jmin), (imax, jmin), (imax, jmax), (imin, jmax)]
                inside = imin <= u <= imax and jmin <= v <= jmax
            else:
                inside = len(h) >= 3 and all((h[(k + 1) % len(h)][0] - h[k][0]) * (v - h[k][1]) - (h[(k + 1) % len(h)][1] - h[k][1]) * (u - h[k][0]) >= 0 for k in range(len(h)))
            if inside:
                as_cells += 1
                out.extend([[tuple(p)] for p in pts])
            else:
                out.append(h)
        for s, h in enumerate(out[:c.O]):
            nv[b, s] = len(h)
            for k, (i, j) in enumerate(h):
                vt[b, s, k] = world(i, j)
            if rd is not None:
                rd[b, s] = 0.0
            if vl is not None:
                vl[b, s] = 0.0
        no[b], dr[b] = min(len(out), c.O), len(out) - min(len(out), c.O)
        info[b] = (len(cells), len(groups), boxes, as_cells)
    return no, nv, vt, rd, vl, dr, info


def same(x, y):
    """None when the two results are the same bytes, else which array differs"""
    names = ("n_obstacles", "n_vertices", "vertices", "radius", "velocity", "dropped", "info")
    for n, a, b in zip(names, x, y):
        if (a is None) != (b is None):
            return n + ": present in one only"
        if a is not None and (a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes()):
            return n
    return None


# ---- the scripted cases
def grid(W, H, cells=()):
    m = np.zeros((H, W), np.uint8)
    for i, j in cells:
        m[j, i] = LETHAL
    return m


def pose_at(u, v, res=0.0625, th=0.0):
    """the pose whose index coordinates are exactly (u, v) on a map with origin (0, 0) and a resolution that is a power of two"""
    return ((u + 0.5) * res, (v + 0.5) * res, th)


LEFT = (-4.0, 1.0, 0.0)          # a robot to the left of every map, looking at it: nothing is behind it and no shape contains it


def disc(W, H, ci, cj, r):
    return grid(W, H, [(i, j) for i in range(ci - r, ci + r + 1) for j in range(cj - r, cj + r + 1) if (i - ci) ** 2 + (j - cj) ** 2 <= r * r])


def spiral(n):
    """a one-cell-wide square spiral that fills n x n cells (n odd) with one-cell gaps between its turns, on a map of (n + 1) x (n + 1)"""
    m = np.zeros((n + 1, n + 1), np.uint8)
    i, j, di, dj = 0, 0, 1, 0
    m[0, 0] = LETHAL
    inside = lambda a, b: 0 <= a < n and 0 <= b < n
    while True:
        steps = 0          # straight on until the border, or until the cell after the next one is wall already
        while inside(i + di, j + dj) and not m[j + dj, i + di] and not (inside(i + 2 * di, j + 2 * dj) and m[j + 2 * dj, i + 2 * di]):
            i, j = i + di, j + dj
            m[j, i] = LETHAL
            steps += 1
        if steps == 0:
            return m
        di, dj = -dj, di


def u_wall():
    """a U that opens towards +i: a back at i = 4 and two arms at j = 4 and j = 20, i = 4 .. 24; 28 x 28"""
    return grid(28, 28, [(4, j) for j in range(4, 21)] + [(i, 4) for i in range(4, 25)] + [(i, 20) for i in range(4, 25)])


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    add("1 x 1", np.full((1, 1), LETHAL), LEFT, 2)
    add("2 x 2", np.full((2, 2), LETHAL), LEFT, 2)
    blob = [(13, 2), (14, 2), (15, 3), (14, 4), (13, 4), (14, 5), (15, 6), (14, 6), (16, 4), (16, 5), (15, 8), (14, 8)]          # (16, .) and (., 8) are the last column and row
    add("17 x 9", grid(17, 9, blob), LEFT, 2)
    big = [(i, j) for i in range(13, 20) for j in range(6, 27) if (i * 7 + j * 3) % 5 != 0] + [(32, 5), (5, 32), (31, 31), (0, 0), (31, 0), (0, 31)]
    add("33 x 33", grid(33, 33, big), LEFT, 2, res=0.05, origin=(-0.7, 0.3))
    add("last row and column", grid(12, 10, [(11, j) for j in range(10)] + [(i, 9) for i in range(12)] + [(5, 5)]), LEFT, 64)
    add("lone cell", grid(9, 9, [(3, 6)]), LEFT, 64, radius=False, velocity=False)
    add("horizontal run", grid(16, 8, [(i, 3) for i in range(3, 10)]), LEFT, 1)
    add("vertical run", grid(8, 16, [(3, j) for j in range(2, 11)]), LEFT, 1)
    add("diagonal run", grid(16, 16, [(k, k) for k in range(2, 12)]), LEFT, 2)
    add("sloped run with gaps", grid(24, 16, [(2 * k, k + 1) for k in range(1, 9)]), LEFT, 5)
    add("2 x 2 block", grid(8, 8, [(3, 3), (3, 4), (4, 3), (4, 4)]), LEFT, 1)
    add("everything lethal", np.full((32, 32), LETHAL), LEFT, 1)
    checker = grid(17, 17, [(i, j) for i in range(16) for j in range(16) if (i + j) % 2 == 0])
    add("checkerboard, link 1", checker, LEFT, 1, O=160)
    add("checkerboard, link 2", checker, LEFT, 2, O=160)
    add("spiral", spiral(31), LEFT, 1)
    two = grid(16, 12, [(2, 4), (3, 4), (2, 5), (3, 5), (3, 6), (6, 4), (7, 4), (6, 5), (7, 6)])
    add("two blobs, link 8", two, LEFT, 8)
    add("two blobs, link 9", two, LEFT, 9)
    add("disc 3", disc(16, 16, 7, 7, 3), LEFT, 2)
    add("disc 4", disc(16, 16, 7, 7, 4), LEFT, 2)
    add("disc 8, V 16", disc(24, 24, 10, 10, 8), LEFT, 2, V=16)
    add("U around the robot", u_wall(), pose_at(14.0, 12.0), 2, O=160)
    add("U, capacity reached inside it", np.stack([u_wall() | grid(28, 28, [(1, 1), (2, 1), (1, 25)])] * 2), [pose_at(14.0, 12.0), pose_at(14.0, 12.25)], 2, O=7)
    add("U, pose not a number", np.stack([u_wall()] * 3), [(math.nan, 0.75, 0.0), (0.9, math.nan, 0.0), pose_at(14.0, 12.0, th=math.nan)], 2)
    sq = grid(12, 12, [(i, j) for i in range(4, 7) for j in range(4, 7)])
    add("robot on a hull vertex", sq, pose_at(4.0, 4.0), 1)
    add("robot on a hull edge", sq, pose_at(6.0, 5.25), 1)
    add("robot one cell outside", np.stack([sq] * 4), [pose_at(3.0, 4.0), pose_at(7.0, 5.0), pose_at(5.0, 7.0), pose_at(5.0, 3.0)], 1)
    d4 = disc(16, 16, 7, 7, 4)
    add("robot on the box's edge", np.stack([d4] * 3), [pose_at(3.0, 10.0), pose_at(11.0, 3.0), pose_at(4.5, 11.0)], 2)
    add("robot outside the box", np.stack([d4] * 2), [pose_at(2.0, 10.0), pose_at(3.0, 11.5)], 2)
    # the behind-robot cut: the robot stands between the arms of the U and looks out of it; the back of the U is behind it
    add("U, nothing cut", u_wall(), pose_at(16.0, 12.0), 2, behind=100.0, O=160)
    add("U, the back cut away", u_wall(), pose_at(16.0, 12.0), 2, behind=0.55, O=160)
    maps = np.stack([np.pad(disc(16, 16, 7, 7, 4), ((0, 12), (0, 12))), u_wall(), np.pad(two, ((3, 13), (5, 7)))])
    add("three maps", maps, [pose_at(14.0, 12.0), pose_at(14.0, 12.0), LEFT], 9, O=80)
    return out


def large_cases():
    """beyond the scripted sizes: a map of more than 2^18 cells (the kernel links through the labels in global memory instead of its LDS bitmap), and one on which
    clusters span more than MAX_SPAN columns (two rows and a bump: the bounding box; a single row: a line)"""
    band = [(i, 40 + i // 3 + d) for i in range(30, 660) for d in (0, 1, 2)]
    ell = [(100, j) for j in range(250, 330)] + [(i, 250) for i in range(100, 180)]
    far = grid(700, 400, band + ell + [(5, 5), (698, 398), (300, 20), (301, 27), (650, 390)])
    far |= np.pad(disc(40, 40, 20, 20, 10), ((300, 60), (400, 260)))
    wide = grid(4200, 60, [(i, j) for i in range(10, 4151) for j in (20, 21)] + [(2000, 22)] + [(i, 40) for i in range(50, 4190)] + [(7, 50), (8, 51)])
    return [Case("more than 2^18 cells", far, LEFT, 64, res=0.05, origin=(-1.0, -1.0)), Case("wider than the span", wide, LEFT, 2)]


def random_cases(count=80, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        W, H = int(rng.integers(3, 30)), int(rng.integers(3, 30))
        m = np.where(rng.random((H, W)) < rng.choice([0.05, 0.15, 0.35, 0.6]), LETHAL, rng.integers(0, 254, (H, W))).astype(np.uint8)
        pose = (float(rng.uniform(0, W)) * 0.05 - 0.3, float(rng.uniform(0, H)) * 0.05 + 0.2, float(rng.choice([0.0, math.pi / 2, 1.0, -2.5])))
        out.append(Case(f"random {k}", m, pose, int(rng.choice([1, 2, 4, 5, 64])), V=int(rng.choice([4, 6, 8])), O=int(rng.choice([6, 40, 400])), res=0.05, origin=(-0.3, 0.2),
                        behind=float(rng.choice([0.3, 1.5]))))
    return out


# ---- the file format of the stand-alone program (tests/host_harness/costmap_clusters_host.cpp, -DCCH_MAIN)
def write_cases(path, cs):
    with open(path, "wb") as f:
        for c in cs:
            np.array([c.B, c.W, c.H, c.V, c.O, c.link, int(c.radius), int(c.velocity)], np.int32).tofile(f)
            np.array([c.res, c.behind]).tofile(f)
            for a in (c.cost, c.origin, c.pose) + c.container():
                if a is not None:
                    a.tofile(f)


def read_outputs(path, cs):
    out = []
    with open(path, "rb") as f:
        for c in cs:
            B, O, V = c.B, c.O, c.V
            rdi = lambda shape: np.fromfile(f, np.int32, int(np.prod(shape))).reshape(shape)
            rdd = lambda shape: np.fromfile(f, np.float64, int(np.prod(shape))).reshape(shape)
            no, nv, vt = rdi((B,)), rdi((B, O)), rdd((B, O, V, 2))
            rd = rdd((B, O)) if c.radius else None
            vl = rdd((B, O, 2)) if c.velocity else None
            out.append((no, nv, vt, rd, vl, rdi((B,)), rdi((B, 4))))
    return out
