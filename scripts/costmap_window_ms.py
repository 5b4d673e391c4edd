"""Device time of mpc_costmap_window_device beside the two costmap steps it feeds, for the library given on the command line:

    python scripts/costmap_window_ms.py mpc_local_planner_amd/csrc/libmpc_hip.so

B = 1024 windows of 128 x 128 at 0.05 m cut from one 1024 x 1024 map at 0.05 m (51.2 m square): walls two cells thick every 96 cells in both directions, each with a
door of 24 cells per room, and 400 pillars of 4 x 4 cells; robots at random poses at least 4 m inside the map.  The window step without inflation (r = 0) and with
inflation_radius 0.5 m (r = 10, inscribed_radius 0.17, cost_scaling_factor 10); then mpc_costmap_to_obstacles_device and mpc_costmap_to_lines_device on the uninflated
windows.  Each on device pointers: mpc_last_costmap_ms (HIP events on the handle's stream) of seven launches after three warm ones, median (min .. max)."""
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

B, S, M, RES = 1024, 128, 1024, 0.05
rng = np.random.default_rng(26)
grid = np.zeros((M, M), np.uint8)
for k in range(0, M, 96):
    grid[k:k + 2, :] = 254
    grid[:, k:k + 2] = 254
for a in range(0, M, 96):          # a door per room in the wall below it and in the wall left of it
    for b in range(0, M, 96):
        grid[a:a + 2, b + 36:b + 60] = 0
        grid[b + 36:b + 60, a:a + 2] = 0
for i, j in zip(rng.integers(0, M - 4, 400), rng.integers(0, M - 4, 400)):
    grid[j:j + 4, i:i + 4] = 254
pose = np.column_stack([rng.uniform(4.0, M * RES - 4.0, B), rng.uniform(4.0, M * RES - 4.0, B), rng.uniform(-3.0, 3.0, B)])

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
p = lambda t: C.c_void_p(t.data_ptr())


def timed(s, launch):
    ms = []
    for _ in range(10):
        launch()
        ms.append(s.last_costmap_ms())
    ms = ms[3:]
    return f"{np.median(ms):.4f} ms ({min(ms):.4f} .. {max(ms):.4f})"


s = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=64, max_vertices=4), max_batch=B)
d_map, d_pose = dev(grid), dev(pose)
d_cost, d_origin, d_info = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2))), dev(np.zeros((B, 4), np.int32))
for name, inflation in (("r = 10", 0.5), ("r = 0", 0.0)):          # the uninflated windows last: the steps below read them
    prm = s.window_params(RES, grid.shape, inscribed_radius=0.17, inflation_radius=inflation)
    t = timed(s, lambda: s.costmap_window_device(B, d_map.data_ptr(), prm, d_pose.data_ptr(), S, S, RES, d_cost.data_ptr(), d_origin.data_ptr(), d_info.data_ptr()))
    s.synchronize()
    info = d_info.cpu().numpy()
    print(f"window, {name}: {t}; per instance: lethal cells {info[:, 1].min()} .. {info[:, 1].max()} (mean {info[:, 1].mean():.1f}), cells changed by inflation "
          f"{info[:, 2].min()} .. {info[:, 2].max()} (mean {info[:, 2].mean():.1f}), lethal cells in the halo only {info[:, 3].min()} .. {info[:, 3].max()}")
    assert (info[:, 0] == S * S).all()
lethal = int(d_info.cpu().numpy()[:, 1].max())
print(f"bytes: {B * S * S} written, {B * S * S} (r = 0) and {B * (S + 20) * (S + 20)} (r = 10, tiles of 64 x 64 with their halo: {B * 4 * 84 * 84}) map bytes gathered, "
      f"from a map of {M * M} bytes")

no, nv, vt = dev(np.zeros(B, np.int32)), dev(np.zeros((B, 64), np.int32)), dev(np.zeros((B, 64, 4, 2)))
rd, vl, dr, linfo = dev(np.zeros((B, 64))), dev(np.zeros((B, 64, 2))), dev(np.zeros(B, np.int32)), dev(np.zeros((B, 4), np.int32))
args = (B, d_cost.data_ptr(), S, S, RES, d_origin.data_ptr(), d_pose.data_ptr())
t = timed(s, lambda: s.costmap_to_lines_device(*args, s.line_params(RES), *(x.data_ptr() for x in (no, nv, vt, rd, vl, dr, linfo))))
s.synchronize()
li = linfo.cpu().numpy()
print(f"lines (O = 64, V = 4): {t}; per instance: kept cells mean {li[:, 0].mean():.1f}, lines mean {li[:, 2].mean():.1f}, dropped max {int(dr.max())}")
s.close()

s = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=lethal, max_vertices=1), max_batch=B)
no, nv, vt, dr = dev(np.zeros(B, np.int32)), dev(np.zeros((B, lethal), np.int32)), dev(np.zeros((B, lethal, 1, 2))), dev(np.zeros(B, np.int32))
t = timed(s, lambda: s._check(s._lib.mpc_costmap_to_obstacles_device(s._h, B, p(d_cost), S, S, RES, p(d_origin), p(d_pose), 1.5, p(no), p(nv), p(vt), p(dr))))
s.synchronize()
print(f"points (O = {lethal}, V = 1): {t}; obstacles per instance mean {no.float().mean().item():.1f}")
s.close()
