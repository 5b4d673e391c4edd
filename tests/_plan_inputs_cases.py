"""Shared by tests/test_plan_inputs_host.py and tests/test_gpu_plan_inputs.py: the host build of mpc_local_planner_amd/csrc/mpc_plan_inputs.hpp (tests/host_harness/
plan_inputs_host.cpp, g++ -ffp-contract=off) behind ctypes, and the scripted plans.  mpc_plan_params belongs to a call, not to an instance, so the plans come in GROUPS:
one parameter set, one plan_stride, and the instances that run under them as one batch."""
import ctypes as C
import math
import os

import numpy as np

import _harness
from mpc_local_planner_amd._abi import MpcPlanParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = _harness.BUILD
MAX_VIA = 4          # cfg.max_via_points of the handle the GPU tests create
dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
_lib = None


def harness():
    global _lib
    if _lib is None:
        lib = C.CDLL(_harness.shared("plan_inputs_host"))
        pp = C.POINTER(MpcPlanParams)
        lib.pin_batch.argtypes = [C.c_int, pp, dp, ip, C.c_int, dp, ip, dp, ip, C.c_int, C.c_int, ip, dp, ip, ip]
        lib.pin_facade.argtypes = [pp, dp, C.c_int, dp, ip, dp, ip, C.c_int, C.c_int, ip, dp, ip, ip]
        for f in (lib.pin_goal_heading, lib.pin_facade_goal_heading):
            f.restype, f.argtypes = C.c_double, [dp, C.c_int, C.c_int, C.c_int]
        for f in (lib.pin_atan2, lib.pin_cc_atan2):
            f.restype, f.argtypes = C.c_double, [C.c_double, C.c_double]
        lib.pin_commands.argtypes = [C.c_int, dp, C.c_int, ip, ip, ip, dp, ip, ip, dp, ip]
        _lib = lib
    return _lib


def d_(a):
    return a.ctypes.data_as(dp)


def i_(a):
    return a.ctypes.data_as(ip)


def params(**kw):
    """the parameter set of the scripted plans: a 6 m x 5 m costmap (radius 0.85 * 3 m = 2.55 m), prune 1 m, look-ahead 1.5 m, via-points every 0.3 m"""
    p = MpcPlanParams(1.0, 1.5, 0.3, 0.2, 0.1, 1, 3, 120, 100, 0.05)
    for k, v in kw.items():
        assert k in dict(MpcPlanParams._fields_), k
        setattr(p, k, v)
    return p


def line(n, step, theta=0.0, x0=0.0):
    g = np.zeros((n, 3))
    g[:, 0] = x0 + step * np.arange(n)
    g[:, 2] = theta
    return g


class Group:
    def __init__(self, name, p, plan_stride):
        self.name, self.p, self.plan_stride, self.inst = name, p, plan_stride, []

    def add(self, what, plan, robot, begin=0):
        self.inst.append((what, np.ascontiguousarray(plan, dtype=np.float64).reshape(-1, 3), np.asarray(robot, dtype=np.float64), int(begin)))
        return self

    def arrays(self, order=None):
        """(global [B][gstride][3], n_global [B], robot [B][3], begin [B]) of the instances in the given order"""
        inst = self.inst if order is None else [self.inst[i] for i in order]
        gstride = max(2, max(len(q[1]) for q in inst))
        g = np.full((len(inst), gstride, 3), 777.0)          # beyond n_global: never read by a correct scan
        for b, q in enumerate(inst):
            g[b, :len(q[1])] = q[1]
        return (g, np.array([len(q[1]) for q in inst], np.int32), np.ascontiguousarray([q[2] for q in inst]), np.array([q[3] for q in inst], np.int32))


def blank_outputs(B, plan_stride, max_via=MAX_VIA):
    """(plan, n_plan, n_via, via, goal_idx, flags) pre-filled, so that entries no code writes compare equal"""
    return (np.full((B, plan_stride, 3), -7.0), np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.full((B, max_via, 3), -7.0), np.full(B, -9, np.int32),
            np.full(B, -1, np.int32))


def host_batch(p, g, ng, robot, begin, plan_stride, max_via=MAX_VIA):
    """pin_batch: (begin, plan, n_plan, n_via, via, goal_idx, flags) of the host build"""
    B = len(ng)
    bg = begin.copy()
    plan, n_plan, n_via, via, gi, fl = blank_outputs(B, plan_stride, max_via)
    harness().pin_batch(B, C.byref(p), d_(g), i_(ng), g.shape[1], d_(robot), i_(bg), d_(plan), i_(n_plan), plan_stride, max_via, i_(n_via), d_(via), i_(gi), i_(fl))
    return bg, plan, n_plan, n_via, via, gi, fl


def host_facade(p, plan_g, robot, begin, plan_stride, max_via=MAX_VIA):
    """pin_facade for ONE instance, same tuple with leading dimension 1"""
    bg = np.array([begin], np.int32)
    plan, n_plan, n_via, via, gi, fl = blank_outputs(1, plan_stride, max_via)
    g = np.ascontiguousarray(plan_g)
    harness().pin_facade(C.byref(p), d_(g), len(g), d_(np.ascontiguousarray(robot)), i_(bg), d_(plan), i_(n_plan), plan_stride, max_via, i_(n_via), d_(via), i_(gi), i_(fl))
    return bg, plan, n_plan, n_via, via, gi, fl


def goal_distance(goal, robot):
    """the distance and heading difference of the goal test exactly as :315-318 computes them"""
    dx, dy = goal[0] - robot[0], goal[1] - robot[1]
    d = math.sqrt(dx * dx + dy * dy)
    th = goal[2] - robot[2]
    pi = math.pi
    if not (-pi <= th < pi):
        th = th - math.floor(th / (2.0 * pi)) * 2.0 * pi
        if th >= pi:
            th -= 2.0 * pi
        if th < -pi:
            th += 2.0 * pi
    return d, abs(th)


def groups():
    """the scripted plans.  Chunks of 64 poses count from plan_begin (prune), from the front (nearest search) and from the nearest pose (walk): the main group places the
    pruned front, the nearest pose, the break position and the last selected pose in lanes 0, 63 and 64, with plan lengths 1, 2, 63, 64, 65, 128 and 129."""
    r0 = (0.0, 0.0, 0.0)
    main = Group("main", params(), 96)
    for n in (1, 2, 3):
        for beg in range(n):
            main.add(f"length {n}, begin {beg}", line(n, 0.5), r0, beg)
        main.add(f"length {n}, robot far", line(n, 0.5), (40.0, 40.0, 1.0))
    rep = line(40, 0.1); rep[7, :2] = rep[6, :2]
    main.add("repeated pose", rep, r0)
    back = line(200, 0.1)
    for j in range(60, 140):
        back[j, 0], back[j, 1] = 0.1 * (j if j < 100 else 199 - j), 0.5
    main.add("leaves the radius and returns", back, r0)
    main.add("nearest pose tied between two indices", line(30, 0.5), (0.75, 0.0, 0.0))
    main.add("robot beyond the prune distance of every pose", line(30, 0.1), (1.0, 1.5, 0.0))
    main.add("robot within the prune distance of the first pose", line(30, 0.1, x0=0.5), r0)
    main.add("look-ahead reached exactly at a pose", line(100, 0.25), r0)
    main.add("begin at the last pose", line(100, 0.05), r0, 99)
    # the pruned front in lanes 0, 63, 64 of the prune scan (spacing 0.5 m: the front is the pose before the robot's)
    for f, n in ((0, 2), (63, 65), (64, 128), (63, 129)):
        main.add(f"front at {f}, length {n}", line(n, 0.5), (0.5 * (f + 1), 0.0, 0.0))
    # the nearest pose in lanes 0, 63, 64 of the nearest scan (spacing 0.01 m: the front stays at 0)
    for r, n in ((0, 63), (63, 64), (64, 65), (63, 128), (64, 129)):
        main.add(f"nearest at {r}, length {n}", line(n, 0.01), (0.01 * r, 0.003, 0.2))
    # the break of the nearest scan in lanes 63 and 64 (lane 0 is "robot far" above): the first pose beyond 2.55 m
    main.add("break at 63", line(128, 0.041), r0)
    main.add("break at 64", line(129, 0.04), r0)
    # the last selected pose in lanes 0, 63, 64 of the walk: the plan ends inside the look-ahead
    for n in (1, 63, 64, 65):
        main.add(f"selection ends with the plan, length {n}", line(n, 0.02), r0)
    main.add("non-zero begin off the chunk grid", line(129, 0.05), (4.0, 0.0, 0.0), 37)
    main.add("plan ends inside the second chunk of the walk", line(70 + 37, 0.02), (0.02 * 37, 0.0, 0.0), 5)
    # neighbours of different length and shape: an arc, a prune scan that runs into its second chunk, robots at the end of their plans, one off to the side
    s = 0.05 * np.arange(129)
    main.add("arc", np.column_stack([4.0 * np.sin(s / 4.0), 4.0 * (1.0 - np.cos(s / 4.0)), s / 4.0]), (2.3, 0.8, 0.5))
    main.add("front in the second chunk of the prune scan", line(128, 0.03), (3.0, 0.0, 0.0))
    main.add("robot at the end, length 65", line(65, 0.03), (64 * 0.03, 0.0, 0.0))
    main.add("robot at the second of two poses", line(2, 0.5), (0.5, 0.0, 0.0))
    main.add("robot beside a plan of 63", line(63, 0.02), (0.5, 0.3, -0.4))
    main.add("robot on the goal of a plan of 129", line(129, 0.1), (12.8, 0.0, 0.05))
    main.add("robot beside and beyond the radius", line(64, 0.05), (0.0, 3.0, 0.0))
    out = [main]
    out.append(Group("no look-ahead limit (0)", params(max_global_plan_lookahead_dist=0.0), 96).add("line", line(100, 0.05), r0).add("short", line(3, 0.05), r0))
    out.append(Group("no look-ahead limit (< 0), truncated", params(max_global_plan_lookahead_dist=-1.0), 5).add("line", line(100, 0.05), r0).add("fits", line(5, 0.05), r0)
               .add("one more than fits", line(6, 0.05), r0))
    out.append(Group("no via-points (0)", params(global_plan_viapoint_sep=0.0), 64).add("line", line(100, 0.05), r0))
    out.append(Group("no via-points (< 0)", params(global_plan_viapoint_sep=-1.0), 64).add("line", line(100, 0.05), r0))
    out.append(Group("more via-points than fit", params(global_plan_viapoint_sep=0.05), 64).add("line", line(100, 0.05), r0).add("exactly four", line(5, 0.06), r0))
    out.append(Group("goal heading kept", params(global_plan_overwrite_orientation=0), 64).add("line", line(100, 0.05, theta=0.7), r0).add("short", line(2, 0.05, theta=-3.0), r0))
    # the goal just inside and just outside each tolerance (nextafter on the tolerance), and a heading difference of exactly +-pi
    goal_plan = line(4, 0.05)
    goal_plan[3, 2] = 0.05
    dist, dth = goal_distance(goal_plan[3], r0)
    for name, kw in (("xy tolerance, outside", dict(xy_goal_tolerance=dist)), ("xy tolerance, inside", dict(xy_goal_tolerance=math.nextafter(dist, 1.0))),
                     ("yaw tolerance, outside", dict(yaw_goal_tolerance=dth)), ("yaw tolerance, inside", dict(yaw_goal_tolerance=math.nextafter(dth, 1.0)))):
        out.append(Group(name, params(**kw), 8).add("goal", goal_plan, r0))
    turn = Group("heading difference of pi", params(yaw_goal_tolerance=math.pi), 8)
    for th in (math.pi, -math.pi):
        gp = line(4, 0.05); gp[3, 2] = th
        turn.add(f"goal heading {th}", gp, r0)
    out.append(turn)
    out.append(Group("heading difference of pi, wide", params(yaw_goal_tolerance=math.nextafter(math.pi, 4.0)), 8).add("goal heading pi", turn.inst[0][1], r0))
    return out


def random_plans(count=300, seed=31):
    """(params, plan, robot, begin, plan_stride, max_via): smooth random plans of 1..150 poses, robots near them, both orientation modes, every look-ahead / separation mode"""
    rng = np.random.default_rng(seed)
    for rep in range(count):
        n = int(rng.integers(1, 151))
        th = np.cumsum(np.concatenate([[rng.uniform(-math.pi, math.pi)], 0.6 * (rng.uniform(size=n - 1) - 0.5)]))
        step = 0.02 + 0.1 * rng.uniform(size=n)
        g = np.column_stack([np.concatenate([[0.0], np.cumsum(step[1:] * np.cos(th[1:]))]), np.concatenate([[0.0], np.cumsum(step[1:] * np.sin(th[1:]))]), th])
        at = int(rng.integers(0, n))
        robot = np.array([g[at, 0] + 0.6 * (rng.uniform() - 0.5), g[at, 1] + 0.6 * (rng.uniform() - 0.5), rng.uniform(-math.pi, math.pi)])
        p = params(global_plan_overwrite_orientation=rep % 2, max_global_plan_lookahead_dist=0.0 if rep % 5 == 0 else float(rng.uniform(0.5, 3.0)),
                   global_plan_viapoint_sep=-1.0 if rep % 3 == 0 else float(rng.uniform(0.05, 0.55)))
        yield p, np.ascontiguousarray(g), robot, (int(rng.integers(0, n)) if rep % 4 == 0 else 0), int(rng.integers(4, 64)), 1 + rep % 6
