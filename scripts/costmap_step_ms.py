"""Device time of the three costmap steps (lines, polygons, points) on the scene of profiles/r23_costmap_lines.md, for the library given on the command line:

    python scripts/costmap_step_ms.py mpc_local_planner_amd/csrc/libmpc_hip.so

B = 1024 maps of 128 x 128 at 0.05 m, robot at cell (10, 64) looking along +x, behind_robot_dist 1.5, link_dist_sq 64, the shipped line parameters: a corridor of two walls
two cells thick and 112 long, four 5 x 5 pillars whose places vary with the instance, a 30-cell wall stub ahead, twelve scattered cells, pillars and scattered cells at
least ten cells from the walls.  Each step on device pointers with max_obstacles = the largest count of the batch; mpc_last_costmap_ms of 10 launches after 3 warm ones."""
import ctypes as C
import os
import sys

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
os.environ["MPC_HIP_LIB"] = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mpc_local_planner_amd as m

B, S, RES = 1024, 128, 0.05
rng = np.random.default_rng(23)
cost = np.zeros((B, S, S), np.uint8)          # [b][j][i]
cost[:, 44:46, 8:120] = 254
cost[:, 83:85, 8:120] = 254
cost[:, 64, 90:120] = 254
for b in range(B):
    for i, j in zip(rng.integers(20, 100, 4), rng.integers(56, 69, 4)):
        cost[b, j:j + 5, i:i + 5] = 254
    cost[b, rng.integers(56, 73, 12), rng.integers(14, 108, 12)] = 254
origin = np.zeros((B, 2))
pose = np.tile([10.5 * RES, 64.5 * RES, 0.0], (B, 1))

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
p = lambda t: C.c_void_p(t.data_ptr())


def solver(O, V):
    return m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=int(O), max_vertices=V), max_batch=B)


# the containers' sizes, from the host-pointer calls on a small container: n_obstacles + dropped is what a step would emit
s = solver(16, 16)
lines, polys, points = s.costmap_to_lines(cost, RES, origin, pose), s.costmap_to_polygons(cost, RES, origin, pose), s.costmap_to_obstacles(cost, RES, origin, pose)
s.close()
for name, a in (("kept cells", lines[6][:, 0]), ("clusters", lines[6][:, 1]), ("lines", lines[6][:, 2]), ("cells left as points", lines[6][:, 3])):
    print(f"{name} per instance: {a.min()} .. {a.max()} (mean {a.mean():.1f})")

d_cost, d_origin, d_pose = dev(cost), dev(origin), dev(pose)
for name, O, V in (("lines", (lines[0] + lines[5]).max(), 4), ("polygons", (polys[0] + polys[5]).max(), 16), ("points", (points[0] + points[3]).max(), 1)):
    s = solver(O, V)
    no, nv, vt = dev(np.zeros(B, np.int32)), dev(np.zeros((B, O), np.int32)), dev(np.zeros((B, O, V, 2)))
    rd, vl, dr, info = dev(np.zeros((B, O))), dev(np.zeros((B, O, 2))), dev(np.zeros(B, np.int32)), dev(np.zeros((B, 4), np.int32))
    args = (B, d_cost.data_ptr(), S, S, RES, d_origin.data_ptr(), d_pose.data_ptr())
    outs = tuple(t.data_ptr() for t in (no, nv, vt, rd, vl, dr, info))
    ms = []
    for it in range(13):
        if name == "lines":
            s.costmap_to_lines_device(*args, s.line_params(RES), *outs)
        elif name == "polygons":
            s.costmap_to_polygons_device(*args, s.cluster_params(RES), *outs)
        else:
            s._check(s._lib.mpc_costmap_to_obstacles_device(s._h, B, p(d_cost), S, S, RES, p(d_origin), p(d_pose), 1.5, p(no), p(nv), p(vt), p(dr)))
        ms.append(s.last_costmap_ms())
    ms = ms[3:]
    assert int(no.max()) == O and not bool(dr.any())
    print(f"{name} (O = {O}, V = {V}): {np.median(ms):.4f} ms ({min(ms):.4f} .. {max(ms):.4f})")
    s.close()
