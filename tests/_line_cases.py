"""Shared by tests/test_costmap_lines_host.py and tests/test_gpu_costmap_lines.py: the host build of mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp
(tests/host_harness/costmap_lines_host.cpp, g++ -ffp-contract=off) behind ctypes, the scripted cases, and a Python restatement of the rule written from
include/mpc_costmap_lines.h, not from the header's code: the kept cells, the clusters (scipy) and the small clusters' shapes are those of tests/_cluster_cases.py; the
hypotheses, scores and runs are plain Python integers, which are unbounded, so that an overflow in the C++ shows as a difference.

A CASE is one call: B maps of one geometry, one parameter set, the containers as they are before the call (every word a sentinel)."""
import ctypes as C
import math

import numpy as np
from scipy.spatial import cKDTree

import _cluster_cases as K
import _harness

_harness.SHARED.setdefault("costmap_lines_host", ("libmpc_costmap_lines.so", ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]))
dp, ip, bp = K.dp, K.ip, K.bp
SENTINEL, ISENTINEL, LETHAL = K.SENTINEL, K.ISENTINEL, K.LETHAL
LEFT, grid, pose_at, same, d_, i_ = K.LEFT, K.grid, K.pose_at, K.same, K.d_, K.i_
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("costmap_lines_host"))
        lib.clh_lines.restype, lib.clh_lines.argtypes = None, [C.c_int, bp, C.c_int, C.c_int, C.c_double, dp, dp, C.c_double, ip, C.c_int, C.c_int, ip, ip, dp, dp, dp, ip, ip]
        lib.clh_list_cap.restype, lib.clh_list_cap.argtypes = C.c_int, []
        _lib = lib
    return _lib


def list_cap():
    """kClListCap: the cells of a cluster the kernel's LDS list holds"""
    return int(harness().clh_list_cap())


class Case(K.Case):
    """a case of tests/_cluster_cases.py with the line rule's parameters: inlier_dist_sq, min_inliers, n_hypotheses, remaining_outliers"""

    def __init__(self, name, cost, pose, link, inl=9, mini=10, nh=1500, rem=3, **kw):
        super().__init__(name, cost, pose, link, **kw)
        self.inl, self.mini, self.nh, self.rem = int(inl), int(mini), int(nh), int(rem)

    def prm(self):
        return np.array([self.link, self.inl, self.mini, self.nh, self.rem], np.int32)

    def take(self, b):
        return Case(f"{self.name} [{b}]", self.cost[b], self.pose[b], self.link, self.inl, self.mini, self.nh, self.rem, V=self.V, O=self.O, res=self.res,
                    origin=self.origin[b], behind=self.behind, radius=self.radius, velocity=self.velocity)

    def at(self, b, B):
        """the same map as entry b of B, among maps that have nothing to do with it"""
        rng = np.random.default_rng(5)
        cost = np.where(rng.random((B, self.H, self.W)) < 0.2, LETHAL, 0).astype(np.uint8)
        cost[b] = self.cost[0]
        pose = np.tile(np.array(LEFT), (B, 1)); pose[b] = self.pose[0]
        origin = np.tile(np.array([0.3, -0.2]), (B, 1)); origin[b] = self.origin[0]
        return Case(f"{self.name} at {b} of {B}", cost, pose, self.link, self.inl, self.mini, self.nh, self.rem, V=self.V, O=self.O, res=self.res, origin=origin,
                    behind=self.behind, radius=self.radius, velocity=self.velocity)

    def polygons(self):
        """the same call to the polygon step"""
        return K.Case(self.name, self.cost, self.pose, self.link, V=self.V, O=self.O, res=self.res, origin=self.origin, behind=self.behind, radius=self.radius, velocity=self.velocity)


def host_lines(c):
    """the host build: (n_obstacles, n_vertices, vertices, radius, velocity, dropped, info)"""
    no, nv, vt, rd, vl = c.container()
    dr, info = np.full(c.B, -1, np.int32), np.full((c.B, 4), -1, np.int32)
    prm = c.prm()
    harness().clh_lines(c.B, c.cost.ctypes.data_as(bp), c.W, c.H, c.res, d_(c.origin), d_(c.pose), c.behind, i_(prm), c.V, c.O, i_(no), i_(nv), d_(vt), d_(rd), d_(vl), i_(dr), i_(info))
    return no, nv, vt, rd, vl, dr, info


# ---- the restatement
M32 = 0xFFFFFFFF


def mix(x):
    x &= M32
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def hypotheses(r, rho, nh):
    """the pairs (a, b) of indices into R, in the order of h"""
    if r * (r - 1) // 2 <= nh:
        return [(a, b) for a in range(r) for b in range(a + 1, r)]
    salt = (rho * 0x9E3779B9) & M32
    out = []
    for h in range(nh):
        a = (mix((2 * h) ^ salt) * r) >> 32
        b = (mix((2 * h + 1) ^ salt) * (r - 1)) >> 32
        out.append((a, b + (1 if b >= a else 0)))
    return out


def inliers_of(p, q, R, inl):
    """[(t, k)] of the cells R[k] that are inliers of p -> q"""
    ex, ey = q[0] - p[0], q[1] - p[1]
    len2, out = ex * ex + ey * ey, []
    lim = inl * len2
    for k, c in enumerate(R):
        dx, dy = c[0] - p[0], c[1] - p[1]
        cr = ex * dy - ey * dx
        t = dx * ex + dy * ey
        if cr * cr <= lim and 0 <= t <= len2:
            out.append((t, k))
    return out


def count_inliers(p, q, R, inl):
    ex, ey = q[0] - p[0], q[1] - p[1]
    len2 = ex * ex + ey * ey
    lim, n = inl * len2, 0
    px, py = p
    for cx, cy in R:
        dx, dy = cx - px, cy - py
        cr = ex * dy - ey * dx
        if cr * cr <= lim and 0 <= dx * ex + dy * ey <= len2:
            n += 1
    return n


def extract(pts, c):
    """rule 3 on the cells of one cluster (tuples of Python ints, in scan order): (lines as pairs of cells, leftover cells)"""
    R, rho, lines = list(pts), 0, []
    while len(R) > c.rem:
        best, pq = 0, None
        for a, b in hypotheses(len(R), rho, c.nh):
            s = count_inliers(R[a], R[b], R, c.inl)
            if s > best:
                best, pq = s, (R[a], R[b])
        if best < c.mini:
            break
        p, q = pq
        len2 = (q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2
        seq = sorted(inliers_of(p, q, R, c.inl))
        runs, cur = [], [seq[0]]
        for prev, nxt in zip(seq, seq[1:]):
            if (nxt[0] - prev[0]) ** 2 > c.link * len2:
                runs.append(cur); cur = []
            cur.append(nxt)
        runs.append(cur)
        run = max(runs, key=len)          # the first of the longest
        if len(run) < c.mini:
            break
        lines.append((R[run[0][1]], R[run[-1][1]]))
        gone = {k for _, k in run}
        R = [x for k, x in enumerate(R) if k not in gone]
        rho += 1
    return lines, R


def python_lines(c):
    """((n_obstacles, ..., info), meta): meta[b] is one entry per obstacle of instance b, capacity aside: (kind, cluster, cells) with kind "line" (rule 3), "left" (a
    leftover point of rule 3) or "small" (rule 2)"""
    no, nv, vt, rd, vl = c.container()
    dr, info = np.zeros(c.B, np.int32), np.zeros((c.B, 4), np.int32)
    meta = []
    for b in range(c.B):
        (ox, oy), (px, py, _) = c.origin[b], c.pose[b]
        world = lambda i, j: (ox + (np.float64(i) + 0.5) * c.res, oy + (np.float64(j) + 0.5) * c.res)
        cells = K.kept_cells(c, b)
        groups = K.clusters_of(cells, c.link)
        out, tags, nlines, nleft = [], [], 0, 0
        for g, idx in enumerate(groups):
            pts = [(int(i), int(j)) for i, j in cells[idx]]
            if len(pts) < c.mini:
                one = K.Case("", K.grid(c.W, c.H, pts), c.pose[b], c.link, V=c.V, O=len(pts) + 1, res=c.res, origin=c.origin[b], behind=1e9)
                n1, v1, t1 = K.python_polygons(one)[:3]
                for s in range(int(n1[0])):
                    out.append([tuple(int(round(x)) for x in ((t1[0, s, k] - c.origin[b]) / c.res - 0.5)) for k in range(int(v1[0, s]))])
                    tags.append(("small", g, pts))
                continue
            lines, left = extract(pts, c)
            for ln in lines:
                out.append(list(ln)); tags.append(("line", g, pts))
            for p in left:
                out.append([p]); tags.append(("left", g, pts))
            nlines += len(lines); nleft += len(left)
        for s, h in enumerate(out[:c.O]):
            nv[b, s] = len(h)
            for k, (i, j) in enumerate(h):
                vt[b, s, k] = world(i, j)
            if rd is not None:
                rd[b, s] = 0.0
            if vl is not None:
                vl[b, s] = 0.0
        no[b], dr[b] = min(len(out), c.O), len(out) - min(len(out), c.O)
        info[b] = (len(cells), len(groups), nlines, nleft)
        meta.append(list(zip(tags, out)))
    return (no, nv, vt, rd, vl, dr, info), meta


# ---- what the feature is for: the two bounds, on a result's vertices (index coordinates from the world coordinates) with the restatement's meta
def _seg_dist(p, a, b):
    """distances of the points p [N][2] from the segment a -> b"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    e = b - a
    l2 = float(e @ e)
    s = np.clip(((p - a) @ e) / l2, 0.0, 1.0) if l2 > 0 else np.zeros(len(p))
    return np.linalg.norm(p - (a + s[:, None] * e), axis=1)


def _inside_convex(p, poly):
    """p [N][2] inside or on the counter-clockwise polygon"""
    ok = np.ones(len(p), bool)
    for k in range(len(poly)):
        o, a = np.asarray(poly[k], float), np.asarray(poly[(k + 1) % len(poly)], float)
        ok &= (a[0] - o[0]) * (p[:, 1] - o[1]) - (a[1] - o[1]) * (p[:, 0] - o[0]) >= -1e-9
    return ok


def bounds_miss(c, result, meta):
    """None when cover and no-overreach hold for every instance with dropped == 0, else what misses"""
    no, nv, vt = result[:3]
    for b in range(c.B):
        if result[5][b] != 0:
            continue
        shapes = [(vt[b, s, :nv[b, s]] - c.origin[b]) / c.res - 0.5 for s in range(int(no[b]))]
        assert len(shapes) == len(meta[b])
        cover, reach = 2.0 * math.sqrt(c.inl), math.sqrt(c.link / 4.0 + 4.0 * c.inl)
        by_cluster = {}
        for ((kind, g, pts), _), sh in zip(meta[b], shapes):
            by_cluster.setdefault(g, (np.array(pts, float), []))[1].append((kind, sh))
        for g, (pts, items) in by_cluster.items():
            best = np.full(len(pts), np.inf)
            for kind, sh in items:
                d = _seg_dist(pts, sh[0], sh[-1]) if len(sh) <= 2 else np.min([_seg_dist(pts, sh[k], sh[(k + 1) % len(sh)]) for k in range(len(sh))], axis=0)
                if len(sh) >= 3:
                    d = np.where(_inside_convex(pts, sh), 0.0, d)
                best = np.minimum(best, d)
                if kind == "line":          # quarter-cell samples along it, end points included
                    n = int(math.ceil(np.linalg.norm(sh[1] - sh[0]) * 4.0)) + 1
                    smp = sh[0] + np.linspace(0.0, 1.0, n)[:, None] * (sh[1] - sh[0])
                    far = cKDTree(pts).query(smp)[0].max()
                    if far > reach + 1e-9:
                        return f"instance {b}, cluster {g}: a line reaches {far} cells from the cluster's cells, above {reach}"
            if best.max() > cover + 1e-9:
                return f"instance {b}, cluster {g}: a kept cell is {best.max()} cells from every obstacle, above {cover}"
    return None


# ---- the scripted cases
def room_with_doorway():
    """48 x 48: a room of walls at i = 3 and 44, j = 3 and 44; the wall j = 3 has a doorway of 12 free cells, i = 18 .. 29, so its two pieces are joined through the far
    walls only"""
    cells = [(i, 44) for i in range(3, 45)] + [(3, j) for j in range(3, 45)] + [(44, j) for j in range(3, 45)]
    cells += [(i, 3) for i in range(3, 45) if not 18 <= i <= 29]
    return grid(48, 48, cells)


def ell():
    """an L: a wall along j = 5, i = 5 .. 29, and one along i = 5, j = 5 .. 29; the free corner is around (22, 22)"""
    return grid(40, 40, [(i, 5) for i in range(5, 30)] + [(5, j) for j in range(6, 30)])


def cases():
    out = []
    add = lambda *a, **k: out.append(Case(*a, **k))
    add("1 x 1", np.full((1, 1), LETHAL), LEFT, 2)
    add("one cell", grid(9, 9, [(3, 6)]), LEFT, 64, radius=False, velocity=False)
    add("straight wall", grid(40, 12, [(i, 4) for i in range(3, 33)]), LEFT, 2)
    add("L", ell(), LEFT, 2)
    add("L, V 4", ell(), LEFT, 2, V=4)
    add("U around the robot", K.u_wall(), pose_at(14.0, 12.0), 2)
    add("small U around the robot", grid(12, 12, [(3, 3), (4, 3), (5, 3), (3, 4), (3, 5), (4, 5), (5, 5)]), pose_at(4.25, 4.0), 2)
    add("doorway", room_with_doorway(), LEFT, 2, inl=1)
    thick = grid(40, 16, [(i, j) for i in range(4, 34) for j in (5, 6, 7)])
    add("thick wall, inlier 9", thick, LEFT, 2, inl=9)
    add("thick wall, inlier 0", thick, LEFT, 2, inl=0)
    add("diagonal wall", grid(40, 40, [(k, k) for k in range(4, 34)] + [(k + 1, k) for k in range(4, 34)]), LEFT, 2, inl=1)
    add("6 x 6 blob", grid(16, 16, [(i, j) for i in range(5, 11) for j in range(5, 11)]), LEFT, 2, inl=1)
    add("min_inliers - 1 cells", grid(16, 16, [(3, 3), (4, 3), (5, 4), (6, 4), (6, 5), (7, 6), (7, 7), (8, 7), (9, 7)]), LEFT, 2)
    # r (r - 1) / 2 = 66 hypotheses for 12 cells: all pairs at 66, sampled at 65
    bent = [(i, 4) for i in range(3, 10)] + [(9, j) for j in range(5, 10)]
    add("12 cells, 66 hypotheses", grid(16, 16, bent), LEFT, 2, inl=0, mini=4, nh=66, rem=0)
    add("12 cells, 65 hypotheses", grid(16, 16, bent), LEFT, 2, inl=0, mini=4, nh=65, rem=0)
    # r equal to remaining_outliers: nothing is extracted; one above: a line
    add("r = remaining_outliers", grid(16, 8, [(i, 3) for i in range(3, 9)]), LEFT, 2, mini=3, rem=6)
    add("r = remaining_outliers + 1", grid(16, 8, [(i, 3) for i in range(3, 10)]), LEFT, 2, mini=3, rem=6)
    # a plus sign: its two bars score the same; the lowest h -- the bar that comes first among the pairs -- wins
    plus = [(i, 8) for i in range(4, 13)] + [(8, j) for j in range(4, 13) if j != 8]
    add("two hypotheses of equal score", grid(20, 20, plus), LEFT, 2, inl=0, mini=5, nh=200, rem=0)
    # two collinear pieces joined by a detour; link 4: a gap of 2 cells along the line is no break, one of 3 is
    def gapped(gap):
        top = [(i, 4) for i in range(3, 10)] + [(i, 4) for i in range(9 + gap, 16 + gap)]
        detour = [(3, j) for j in range(5, 9)] + [(i, 8) for i in range(3, 16 + gap)] + [(15 + gap, j) for j in range(5, 8)]
        return grid(32, 16, top + detour)
    add("gap at the threshold", gapped(2), LEFT, 4, inl=0, mini=5, nh=1500, rem=0)
    add("gap one cell wider", gapped(3), LEFT, 4, inl=0, mini=5, nh=1500, rem=0)
    # pieces of 4 cells in one line, 4 cells apart, joined by a row two cells under them: once that row is a line, the score still reaches min_inliers, no run does
    comb = [(i, 4) for k in range(4) for i in range(3 + 7 * k, 7 + 7 * k)] + [(i, 6) for i in range(3, 28)]
    add("largest run of min_inliers - 1", grid(40, 12, comb), LEFT, 4, inl=0, mini=5, nh=1500, rem=0)
    add("capacity", room_with_doorway(), LEFT, 2, inl=1, O=3)
    add("pose not a number", np.stack([ell()] * 2), [(math.nan, 0.75, 0.0), (0.9, math.nan, 0.0)], 2)
    add("4096 x 2", grid(4096, 2, [(i, 0) for i in range(4096)]), LEFT, 1, nh=64)
    add("2 x 4096", grid(2, 4096, [(0, j) for j in range(4096)]), LEFT, 1, nh=64)
    add("three maps", np.stack([np.pad(ell(), ((0, 8), (0, 8))), room_with_doorway(), np.pad(thick, ((3, 29), (5, 3)))]), [LEFT, pose_at(20.0, 20.0), LEFT], 2)
    return out


def random_cases(count=80, seed=7, size=48):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        W, H = size, size
        m = np.where(rng.random((H, W)) < rng.choice([0.03, 0.08, 0.15, 0.3]), LETHAL, rng.integers(0, 254, (H, W))).astype(np.uint8)
        for _ in range(int(rng.integers(0, 4))):          # and a few walls
            i0, j0, n = int(rng.integers(0, W - 12)), int(rng.integers(0, H - 12)), int(rng.integers(6, 30))
            if rng.random() < 0.5:
                m[j0, i0:i0 + n] = LETHAL
            else:
                m[j0:j0 + n, i0] = LETHAL
        pose = (float(rng.uniform(0, W)) * 0.05 - 0.3, float(rng.uniform(0, H)) * 0.05 + 0.2, float(rng.choice([0.0, math.pi / 2, 1.0, -2.5])))
        out.append(Case(f"random {k}", m, pose, int(rng.choice([1, 2, 4])), inl=int(rng.choice([0, 1, 4, 9])), mini=int(rng.choice([3, 5, 10])), nh=int(rng.choice([6, 20, 60])),
                        rem=int(rng.choice([0, 3])), V=int(rng.choice([4, 8])), O=int(rng.choice([6, 64, 400])), res=0.05, origin=(-0.3, 0.2), behind=float(rng.choice([0.8, 3.0]))))
    return out


def capacity_cases():
    """one cluster just below the kernel's LDS list capacity and one just above it: a full block of 56 rows"""
    cap = list_cap()
    out = []
    for cells in (cap - 1, cap + 1):
        rows = 56
        cols, rest = divmod(cells, rows)
        m = grid(cols + 4, rows + 2, [(1 + i, j) for i in range(cols) for j in range(rows)] + [(1 + cols, j) for j in range(rest)])
        out.append(Case(f"{cells} cells in one cluster", m, LEFT, 1, inl=1, mini=10, nh=40, rem=3, O=400))
    return out


# ---- the file format of the stand-alone program (tests/host_harness/costmap_lines_host.cpp, -DCLH_MAIN)
def write_cases(path, cs):
    with open(path, "wb") as f:
        for c in cs:
            np.array([c.B, c.W, c.H, c.V, c.O, int(c.radius), int(c.velocity), c.link, c.inl, c.mini, c.nh, c.rem], np.int32).tofile(f)
            np.array([c.res, c.behind]).tofile(f)
            for a in (c.cost, c.origin, c.pose) + c.container():
                if a is not None:
                    a.tofile(f)


read_outputs = K.read_outputs
