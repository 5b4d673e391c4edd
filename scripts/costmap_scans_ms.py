"""Device time of mpc_costmap_scans_device beside mpc_costmap_window_device on the same windows, for the library given on the command line:

    python scripts/costmap_scans_ms.py mpc_local_planner_amd/csrc/libmpc_hip.so

The windows of scripts/costmap_window_ms.py: B = 1024 windows of 128 x 128 at 0.05 m cut from one 1024 x 1024 map at 0.05 m (walls two cells thick every 96 cells with a
door of 24 cells per room, 400 pillars of 4 x 4 cells), robots at random poses at least 4 m inside the map.  A scan of 360 beams per robot by marching every ray through
that map in numpy (5 cm steps, range_max 10 m, +inf where nothing is hit), so the layer marks what the static map holds; obstacle_range 3.0, raytrace_range 4.0,
track_unknown 1, combination_method 1 (the shipped diff-drive files).  The scans step on device pointers: a first cycle (keep NULL), then cycles that keep the layer
while every robot moves on by (0.07, 0.03) m and turns by 0.05 rad per cycle, with and without the window to combine into; the window step (r = 0) between them on the
same poses.  mpc_last_costmap_ms (HIP events on the handle's stream) of seven launches after three warm ones, median (min .. max)."""
import math
import os
import sys

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
os.environ["MPC_HIP_LIB"] = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mpc_local_planner_amd as m

B, S, M, RES, BEAMS = 1024, 128, 1024, 0.05, 360
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
pose0 = np.column_stack([rng.uniform(4.0, M * RES - 4.0, B), rng.uniform(4.0, M * RES - 4.0, B), rng.uniform(-3.0, 3.0, B)])
DRIFT = np.array([0.07, 0.03, 0.05])


def scan(pose):
    """ranges float32 (B, BEAMS): the first lethal map cell along every ray, marched in 5 cm steps up to 10 m"""
    th = pose[:, 2:3] - math.pi + 2 * math.pi / BEAMS * np.arange(BEAMS)[None, :]
    cs, sn = np.cos(th), np.sin(th)
    out = np.full((B, BEAMS), np.inf, np.float32)
    for step in range(1, 200):
        r = step * RES
        ix = np.clip(((pose[:, 0:1] + r * cs) / RES).astype(np.int64), 0, M - 1)
        iy = np.clip(((pose[:, 1:2] + r * sn) / RES).astype(np.int64), 0, M - 1)
        hit = (grid[iy, ix] == 254) & np.isinf(out)
        out[hit] = r
    return out


dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
s = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=64, max_vertices=4), max_batch=B)
wp = s.window_params(RES, grid.shape)
sp = s.scan_params(angle_min=-math.pi, angle_increment=2 * math.pi / BEAMS, range_min=0.05, range_max=10.0, obstacle_range=3.0, raytrace_range=4.0, track_unknown=1)
d_map = dev(grid)
d_cost, d_origin = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2)))
d_layer, d_cell, d_info = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2), np.int32)), dev(np.zeros((B, 4), np.int32))
d_keep = dev(np.ones(B, np.int32))
cycles = [(dev(pose0 + k * DRIFT), dev(scan(pose0 + k * DRIFT))) for k in range(10)]


def timed(what, launch, counts=True):
    ms = []
    for k in range(10):
        launch(k)
        ms.append(s.last_costmap_ms())
    s.synchronize()
    ms = ms[3:]
    info = d_info.cpu().numpy()
    print(f"{what}: {np.median(ms):.4f} ms ({min(ms):.4f} .. {max(ms):.4f})" + (f"; per instance after the last launch: beams kept mean {info[:, 0].mean():.1f}, marked cells mean "
          f"{info[:, 1].mean():.1f}, free cells mean {info[:, 2].mean():.1f}, window cells changed mean {info[:, 3].mean():.1f}" if counts else ""))


def window(k):
    s.costmap_window_device(B, d_map.data_ptr(), wp, cycles[k][0].data_ptr(), S, S, RES, d_cost.data_ptr(), d_origin.data_ptr())


def scans(k, keep, cost):
    s.costmap_scans_device(B, sp, cycles[k][0].data_ptr(), cycles[k][1].data_ptr(), BEAMS, d_keep.data_ptr() if keep else None, S, S, RES, d_layer.data_ptr(), d_cell.data_ptr(),
                           d_cost.data_ptr() if cost else None, d_info.data_ptr())


timed("window, r = 0", window, counts=False)
window(0)
timed("scans, first cycle (keep NULL), into the window", lambda k: scans(0, False, True))
timed("scans, keeping the layer, robots moving, into the window", lambda k: (window(k), scans(k, True, True)))
timed("scans, keeping the layer, robots moving, no window", lambda k: scans(k, True, False))
timed("window, r = 0, again", window, counts=False)
print(f"bytes per launch: layer {B * S * S} read and {B * S * S} written, window {B * S * S} read and {B * S * S} written, ranges {B * BEAMS * 4}; LDS per workgroup {S * S + 16}")
s.close()
