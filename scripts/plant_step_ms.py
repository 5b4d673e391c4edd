"""Device time of mpc_plant_step_device beside mpc_scan_cast_device, mpc_costmap_window_device and mpc_costmap_scans_device on the same robots, for the library given
on the command line:

    python scripts/plant_step_ms.py mpc_local_planner_amd/csrc/libmpc_hip.so

The map and the robots of scripts/scan_cast_ms.py: one 1024 x 1024 map at 0.05 m (walls two cells thick every 96 cells with a door of 24 cells per room, 400 pillars of
4 x 4 cells), B = 1024 robots at random poses at least 4 m inside the map.  The plant: the car-like robot of the demos (ex/stage/robots/carlike_robot.inc through
params.plant_params_from_position: drive "car", wheelbase 0.4, the footprint of its line 16, interval_sim 100), every robot commanded 0.5 m/s at a steering angle of
0.2 rad; 1 and 10 sub-steps per call; without a pool and with the 1024 robots themselves as discs of 0.2 m, self_index = the robot's own entry.  Every launch starts
from the same poses (they are copied back on the device in front of it, outside the timed events).  For scale the cast (360 beams at 10 m, no pool), the window and
the scans step of the same cycle.  mpc_last_costmap_ms (HIP events on the handle's stream) of seven launches after three warm ones, median (min .. max)."""
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

dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
s = m.BatchSolver(m.config_unicycle_quadratic(20, max_obstacles=64, max_vertices=V), max_batch=B)
d_map, d_start, d_pose = dev(grid), dev(pose), dev(pose)
pv = np.zeros((B, V, 2))
pv[:, 0] = pose[:, :2]
d_nv, d_pv, d_rad, d_self = dev(np.ones(B, np.int32)), dev(pv), dev(np.full(B, 0.2)), dev(np.arange(B, dtype=np.int32))
pool = (B, d_nv.data_ptr(), d_pv.data_ptr(), d_rad.data_ptr())
d_cmd, d_vel = dev(np.tile([0.5, 0.0, 0.2], (B, 1))), dev(np.zeros((B, 3)))
d_stall, d_info = dev(np.zeros(B, np.int32)), dev(np.zeros((B, 4), np.int32))


def timed(what, launch, counts=None, before=None):
    ms = []
    for _ in range(10):
        if before:
            before()
            torch.cuda.synchronize()          # the copy runs on torch's stream, the launch on the handle's
        launch()
        ms.append(s.last_costmap_ms())
    s.synchronize()
    ms = ms[3:]
    print(f"{what}: {np.median(ms):.4f} ms ({min(ms):.4f} .. {max(ms):.4f})" + (counts() if counts else ""), flush=True)


def plant_counts():
    info, stall = d_info.cpu().numpy(), d_stall.cpu().numpy()
    why = info[info[:, 1] >= 0, 2]
    return (f"; per robot: sub-steps moved {info[:, 0].mean():.2f}, stalled {stall.mean():.2f}; robots blocked {len(why)}: by the map {(why == -2).sum()}, off the map "
            f"{(why == -3).sum()}, by a robot {(why >= 0).sum()}")


def reset():
    d_pose.copy_(d_start)
    d_vel.zero_()


car = dict(drive="car", wheelbase=0.4, size=(0.6, 0.25, 0.40), origin=(0.2, 0.0, 0.0, 0.0))          # ex/stage/robots/carlike_robot.inc
print(f"B {B}, map {M} x {M} at {RES} m; read per robot: pose, cmd, vel 72 B, with the pool its 1024 entries of {V * 16 + 12} B once for the culling; written per robot: pose, vel "
      f"48 B, stall 4 B, info 16 B")
for n_sub in (1, 10):
    pp = P.plant_params_from_position(car["drive"], car["wheelbase"], car["size"], car["origin"], 100, RES, grid.shape)
    pp.n_substeps = n_sub
    for label, pl, si in (("no pool", None, None), ("the 1024 robots as discs", pool, d_self.data_ptr())):
        timed(f"plant step, {n_sub} sub-step(s), {label}",
              lambda: s.plant_step_device(B, pp, d_cmd.data_ptr(), d_pose.data_ptr(), map_cost=d_map.data_ptr(), pool=pl, self_index=si, vel=d_vel.data_ptr(), stall=d_stall.data_ptr(),
                                          info=d_info.data_ptr()), plant_counts, reset)
    timed(f"plant step, {n_sub} sub-step(s), no pool, no map", lambda: s.plant_step_device(B, pp, d_cmd.data_ptr(), d_pose.data_ptr(), vel=d_vel.data_ptr(), stall=d_stall.data_ptr(),
                                                                                              info=d_info.data_ptr()), plant_counts, reset)
    timed(f"plant step, {n_sub} sub-step(s), no pool, vel, stall and info NULL", lambda: s.plant_step_device(B, pp, d_cmd.data_ptr(), d_pose.data_ptr(), map_cost=d_map.data_ptr()), None, reset)

# for scale: the cast, the window and the scans step of the same cycle on the same robots
reset()
torch.cuda.synchronize()
cp = s.cast_params(RES, grid.shape, angle_min=-math.pi, angle_increment=2 * math.pi / 360, range_max=10.0)
wp = s.window_params(RES, grid.shape)
sp = s.scan_params(angle_min=-math.pi, angle_increment=2 * math.pi / 360, range_min=0.05, range_max=10.0, obstacle_range=3.0, raytrace_range=4.0, track_unknown=1)
d_ranges = dev(np.zeros((B, 360), np.float32))
d_cost, d_origin = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2)))
d_layer, d_cell = dev(np.zeros((B, S, S), np.uint8)), dev(np.zeros((B, 2), np.int32))
timed("cast, 360 beams, 10 m, no pool", lambda: s.scan_cast_device(B, d_map.data_ptr(), cp, d_pose.data_ptr(), 360, d_ranges.data_ptr()))
timed("cast, 360 beams, 10 m, the 1024 robots as discs", lambda: s.scan_cast_device(B, d_map.data_ptr(), cp, d_pose.data_ptr(), 360, d_ranges.data_ptr(), pool=pool, self_index=d_self.data_ptr()))
timed("window, r = 0", lambda: s.costmap_window_device(B, d_map.data_ptr(), wp, d_pose.data_ptr(), S, S, RES, d_cost.data_ptr(), d_origin.data_ptr()))
timed("scans, first cycle, into the window, from the cast ranges", lambda: s.costmap_scans_device(B, sp, d_pose.data_ptr(), d_ranges.data_ptr(), 360, None, S, S, RES, d_layer.data_ptr(),
                                                                                                  d_cell.data_ptr(), d_cost.data_ptr(), d_info.data_ptr()))
s.close()
