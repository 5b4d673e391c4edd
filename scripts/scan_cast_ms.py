"""Device time of mpc_scan_cast_device beside mpc_costmap_window_device and mpc_costmap_scans_device on the same robots, for the library given on the command line:

    python scripts/scan_cast_ms.py mpc_local_planner_amd/csrc/libmpc_hip.so

The map and the robots of scripts/costmap_scans_ms.py: one 1024 x 1024 map at 0.05 m (walls two cells thick every 96 cells with a door of 24 cells per room, 400
pillars of 4 x 4 cells), B = 1024 robots at random poses at least 4 m inside the map.  Two lasers: 360 beams around the robot at range_max 10 m, and the demo's
(ex/stage/robots/*.inc: 640 samples over 58 degrees at 6.5 m, 0.1 m behind the robot's centre); each without a pool and with the 1024 robots themselves as discs of
0.2 m, self_index = the robot's own entry.  The cast ranges of the first laser then feed the scans step, which is timed with the window step for scale, as is the numpy
march of scripts/costmap_scans_ms.py (1024 x 360 rays in 5 cm steps) on this machine's cores.  mpc_last_costmap_ms (HIP events on the handle's stream) of seven launches
after three warm ones, median (min .. max)."""
import math
import os
import sys
import time

import numpy as np

if len(sys.argv) != 2:
    sys.exit(__doc__)
os.environ["MPC_HIP_LIB"] = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mpc_local_planner_amd as m
from mpc_local_planner_amd import params as P

B, S, M, RES, V = 1024, 128, 1024, 0.05, 4
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


def march(beams=360):
    """the host march of scripts/costmap_scans_ms.py"""
    th = pose[:, 2:3] - math.pi + 2 * math.pi / beams * np.arange(beams)[None, :]
    cs, sn = np.cos(th), np.sin(th)
    out = np.full((B, beams), np.inf, np.float32)
    for step in range(1, 200):
        r = step * RES
        ix = np.clip(((pose[:, 0:1] + r * cs) / RES).astype(np.int64), 0, M - 1)
        iy = np.clip(((pose[:, 1:2] + r * sn) / RES).astype(np.int64), 0, M - 1)
        hit = (grid[iy, ix] == 254) & np.isinf(out)
        out[hit] = r
    return out


dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
s = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=64, max_vertices=V), max_batch=B)
d_map, d_pose = dev(grid), dev(pose)
pv = np.zeros((B, V, 2))
pv[:, 0] = pose[:, :2]
d_nv, d_pv, d_rad, d_self = dev(np.ones(B, np.int32)), dev(pv), dev(np.full(B, 0.2)), dev(np.arange(B, dtype=np.int32))
pool = (B, d_nv.data_ptr(), d_pv.data_ptr(), d_rad.data_ptr())
d_info = dev(np.zeros((B, 4), np.int32))


def timed(what, launch, counts=None):
    ms = []
    for _ in range(10):
        launch()
        ms.append(s.last_costmap_ms())
    s.synchronize()
    ms = ms[3:]
    print(f"{what}: {np.median(ms):.4f} ms ({min(ms):.4f} .. {max(ms):.4f})" + (counts() if counts else ""), flush=True)


def cast_counts():
    info = d_info.cpu().numpy()
    return f"; per robot: by the map {info[:, 0].mean():.1f}, by the pool {info[:, 1].mean():.1f}, no return {info[:, 2].mean():.1f}, blocking cells in the square {info[:, 3].mean():.0f}"


lasers = (("360 beams, 10 m", s.cast_params(RES, grid.shape, angle_min=-math.pi, angle_increment=2 * math.pi / 360, range_max=10.0), 360),
          ("640 beams, 6.5 m, 58 degrees", P.cast_params_from_ranger(58.0, 640, 6.5, (-0.1, 0.0, 0.0), RES, grid.shape), 640))
kept = {}
for name, cp, beams in lasers:
    d_ranges, d_hit = dev(np.zeros((B, beams), np.float32)), dev(np.zeros((B, beams), np.int32))
    kept[name] = d_ranges
    Rc = int(math.ceil(cp.range_max / RES)) + 1
    side = 2 * Rc + 1
    print(f"{name}: Rc {Rc}, LDS per workgroup {side * ((side + 63) // 64) * 8 + 4 * 512 + 64} bytes; map bytes read per robot at most {side * side}; written per launch: ranges "
          f"{B * beams * 4}, hit {B * beams * 4}, info {B * 16}")
    for label, pl, si in (("no pool", None, None), ("the 1024 robots as discs", pool, d_self.data_ptr())):
        timed(f"cast, {name}, {label}", lambda: s.scan_cast_device(B, d_map.data_ptr(), cp, d_pose.data_ptr(), beams, d_ranges.data_ptr(), pool=pl, self_index=si, hit=d_hit.data_ptr(),
                                                                   info=d_info.data_ptr()), cast_counts)
    timed(f"cast, {name}, no pool, hit and info NULL", lambda: s.scan_cast_device(B, d_map.data_ptr(), cp, d_pose.data_ptr(), beams, d_ranges.data_ptr()))
    s.scan_cast_device(B, d_map.data_ptr(), cp, d_pose.data_ptr(), beams, d_ranges.data_ptr())          # the ranges kept for the scans step: the map alone

# for scale: the window and the scans step on the same robots, the scans fed with the cast ranges of the first laser
wp = s.window_params(RES, grid.shape)
sp = s.scan_params(angle_min=-math.pi, angle_increment=2 * math.pi / 360, range_min=0.05, range_max=10.0, obstacle_range=3.0, raytrace_range=4.0, track_unknown=1)
d_cost, d_origin = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2)))
d_layer, d_cell = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2), np.int32))
timed("window, r = 0", lambda: s.costmap_window_device(B, d_map.data_ptr(), wp, d_pose.data_ptr(), S, S, RES, d_cost.data_ptr(), d_origin.data_ptr()))
timed("scans, first cycle, into the window, from the cast ranges", lambda: s.costmap_scans_device(B, sp, d_pose.data_ptr(), kept["360 beams, 10 m"].data_ptr(), 360, None, S, S, RES,
                                                                                                  d_layer.data_ptr(), d_cell.data_ptr(), d_cost.data_ptr(), d_info.data_ptr()))
s.synchronize()
t0 = time.perf_counter()
marched = march()
t1 = time.perf_counter()
cast = kept["360 beams, 10 m"].cpu().numpy()
both = np.isfinite(marched) & np.isfinite(cast)
print(f"host march, 1024 x 360 rays in 5 cm steps with numpy: {1e3 * (t1 - t0):.0f} ms; beams both return {both.mean():.3f}, median |march - cast| over them "
      f"{np.median(np.abs(marched[both] - cast[both])):.3f} m")
s.close()
