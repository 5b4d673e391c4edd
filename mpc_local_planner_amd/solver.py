"""BatchSolver -- thin Python host wrapper over the C ABI (include/mpc_hip.h).

Mirrors the lifecycle of the reference's Controller (configure -> step ... -> reset,
include/mpc_local_planner/controller.h:61-104) for B independent planner instances.
All arithmetic happens in the HIP library; this file only marshals pointers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._abi import (MpcCastParams, MpcClusterParams, MpcConfig, MpcLineParams, MpcCycleParams, MpcEvalOut, MpcObstacles, MpcPlanParams, MpcPlantParams, MpcPool, MpcPoolParams, MpcScanParams,
                   MpcWindowParams, MPC_OK)


class MpcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mpc_hip error {code}: {msg}")
        self.code = code


@dataclass
class BatchResult:
    x: np.ndarray        # (B, n, 3)
    u: np.ndarray        # (B, n, 2)  last row duplicates u_{n-2}
    dt: np.ndarray       # (B,)
    status: np.ndarray   # (B,) int32, 0 = converged
    iters: np.ndarray    # (B,) int32


@dataclass
class TrajectoryEval:
    """what mpc_evaluate_batch reports for B trajectories (include/mpc_hip.h, struct mpc_eval_out)"""
    objective: np.ndarray       # (B,)
    eq_violation: np.ndarray    # (B,)
    ineq_violation: np.ndarray  # (B,)
    clearance: np.ndarray       # (B,)  +inf without obstacles
    closest: np.ndarray         # (B, 2) int32: (grid point, obstacle) of the clearance, (-1, -1) without obstacles


@dataclass
class PlanInputs:
    """what mpc_plan_inputs_batch prepares for B robots (include/mpc_hip.h)"""
    plan: np.ndarray            # (B, plan_stride, 3) the local plan, first pose = the robot pose
    n_plan: np.ndarray          # (B,) int32 poses of it
    plan_begin: np.ndarray      # (B,) int32 the pruned fronts: plan_begin of the next cycle
    goal_idx: np.ndarray        # (B,) int32 index of the local goal counted from the front (-1: plan empty)
    flags: np.ndarray           # (B,) int32 PLAN_* bits
    n_via: Optional[np.ndarray]     # (B,) int32, with via_points
    via: Optional[np.ndarray]       # (B, max_via_points, 3)


@dataclass
class Commands:
    """what mpc_commands_batch makes of a step's result for B robots (include/mpc_hip.h)"""
    cmd: np.ndarray             # (B, 3) linear.x, linear.y, angular.z
    result: np.ndarray          # (B,) int32 CMD_*
    reset_next: np.ndarray      # (B,) int32: reset of the next controller_step
    u_prev_next: np.ndarray     # (B, 2): u_prev of the next controller_step
    infeasible_count: np.ndarray    # (B,) int32 failures in a row


# ---- how each kind of argument reaches the C ABI ---------------------------------------------------------------------------------------------------------------------
def _addr(a):
    """address of a host array, None -> NULL"""
    return None if a is None else C.c_void_p(a.ctypes.data)


def _dev(p):
    """a device address (int), 0 / None -> NULL"""
    return C.c_void_p(p) if p else None


def _floats(p):
    """a float array at an address (int; host or device), as the tables bind `const float*`; 0 / None -> NULL"""
    return C.cast(C.c_void_p(p), C.POINTER(C.c_float)) if p else None


def _as_f64(a, shape):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _as_i32(a, B, name=None):
    """contiguous int32 of shape (B,), None -> None; a wrong shape raises under `name`, without a name whatever has B elements is taken as (B,)"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.int32)
    if name is None:
        return a.reshape(B)
    if a.shape != (B,):
        raise ValueError(f"{name} must have shape (B,)")
    return a


def _dev_obstacles(obstacles):
    """const mpc_obstacles* of up to five device addresses, None -> NULL"""
    if obstacles is None:
        return None
    return C.byref(MpcObstacles(*(tuple(obstacles) + (None,) * (5 - len(obstacles)))))


def _params(name, struct, defaults, fields):
    """a parameter struct `name` with the library's defaults (defaults(byref(p)): the caller's <name>_defaults call, whose other arguments differ), then the given fields"""
    p = struct()
    defaults(C.byref(p))
    for k, v in fields.items():
        if k not in dict(struct._fields_):
            raise ValueError(f"{name} has no field {k}")
        setattr(p, k, v)
    return p


class BatchSolver:
    def __init__(self, cfg: MpcConfig, max_batch: int, device: int = 0):
        self._lib = _lib.load()
        self.cfg = cfg
        self.n = int(cfg.n)
        self.max_batch = int(max_batch)
        self.device = int(device)
        h = C.c_void_p()
        rc = self._lib.mpc_create(C.byref(cfg), self.max_batch, self.device, C.byref(h))
        if rc != MPC_OK:
            raise MpcError(rc, self._lib.mpc_last_error().decode())
        self._h = h

    @classmethod
    def from_yaml(cls, path: str, max_batch: int, device: int = 0, namespace="MpcLocalPlannerROS", costmap_footprint=None, **sizing):
        """A solver configured from a parameter file of the reference (its keys, its defaults: mpc_local_planner_amd/params.py).  The grid
        is sized for the largest size the reference's grid adaptation may reach.  The facade options and the notes of the reader are kept
        as `controller_options` / `param_notes`."""
        from . import params
        cfg, ctrl, notes = params.config_from_yaml(path, namespace=namespace, costmap_footprint=costmap_footprint, **sizing)
        n_ref = int(cfg.n)
        cfg.n = max(n_ref, int(ctrl.get("n_max", n_ref)))          # capacity: grid/variable_grid/grid_adaptation/max_grid_size
        s = cls(cfg, max_batch, device)
        if cfg.n > n_ref:
            s.set_grid_sizes([n_ref] * max_batch)                   # every instance starts at grid/grid_size_ref, as the reference's grid does
        s.controller_options, s.param_notes, s.n_ref = ctrl, notes, n_ref
        return s

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mpc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != MPC_OK:
            raise MpcError(rc, self._lib.mpc_last_error().decode())

    def reset(self):
        self._check(self._lib.mpc_reset(self._h))

    # ---- host buffers (numpy) ------------------------------------------------
    def _pack_obstacles(self, obstacles, B):
        """(const mpc_obstacles* of host arrays or NULL, the arrays: they have to outlive the call)"""
        if obstacles is None:
            return None, None
        O, V = int(self.cfg.max_obstacles), int(self.cfg.max_vertices)
        no = np.ascontiguousarray(obstacles[0], dtype=np.int32)
        nv = np.ascontiguousarray(obstacles[1], dtype=np.int32)
        vv = _as_f64(obstacles[2], (B, O, V, 2))
        rr = _as_f64(obstacles[3], (B, O)) if len(obstacles) > 3 and obstacles[3] is not None else None
        vel = _as_f64(obstacles[4], (B, O, 2)) if len(obstacles) > 4 and obstacles[4] is not None else None
        if no.shape != (B,) or nv.shape != (B, O):
            raise ValueError("obstacle arrays have the wrong shape")
        keep = (no, nv, vv, rr, vel)
        return C.byref(MpcObstacles(*(a.ctypes.data if a is not None else None for a in keep))), keep

    def _solve_inputs(self, x0, xf, u_prev, dt_prev, init):
        """B and the seven input arrays solve() and step() share, checked: x0, xf, u_prev, dt_prev, x_init, u_init, dt_init"""
        x0 = np.ascontiguousarray(x0, dtype=np.float64)
        B, n = int(x0.shape[0]), self.n
        cycle = (_as_f64(x0, (B, 3)), _as_f64(xf, (B, 3)), _as_f64(u_prev, (B, 2)), _as_f64(dt_prev, (B,)))
        if init is None:
            return B, cycle + (None, None, None)
        return B, cycle + (_as_f64(init[0], (B, n, 3)), _as_f64(init[1], (B, n, 2)), _as_f64(init[2], (B,)))

    def _outputs(self, B, alloc=np.zeros):
        """(BatchResult of fresh arrays, their addresses in the order of the C ABI: x_out, u_out, dt_out, status, iters)"""
        r = BatchResult(alloc((B, self.n, 3)), alloc((B, self.n, 2)), alloc(B), alloc(B, np.int32), alloc(B, np.int32))
        return r, [_addr(r.x), _addr(r.u), _addr(r.dt), _addr(r.status), _addr(r.iters)]

    def solve(self, x0, xf, u_prev=None, dt_prev=None, init=None, obstacles=None) -> BatchResult:
        """One control cycle for B instances (Controller::step, src/controller.cpp:111-179).
        init = (x_init (B,n,3), u_init (B,n,2), dt_init (B,)) or None for the reference cold start.
        obstacles = (n_obstacles (B,), n_vertices (B,O), vertices (B,O,V,2)[, radius (B,O)[, velocity (B,O,2)]]) when the solver was
        created with max_obstacles > 0."""
        B, inputs = self._solve_inputs(x0, xf, u_prev, dt_prev, init)
        ob, keep = self._pack_obstacles(obstacles, B)
        r, outs = self._outputs(B, np.empty)
        self._check(self._lib.mpc_solve_batch(self._h, B, *map(_addr, inputs), ob, *outs))
        return r

    def step(self, x0, xf, u_prev=None, dt_prev=None, init=None, obstacles=None, outer_iterations=1, adapt=False, n_min=3, n_max=0, dt_hyst_ratio=0.1):
        """One control cycle = `outer_iterations` x (grid update -> solve) in ONE call (mpc_step_batch: PredictiveController::step's outer OCP iterations,
        src/controller.cpp:70-72,172, without a host round trip between them).  Returns (BatchResult of the last solve, grid sizes after the call)."""
        B, inputs = self._solve_inputs(x0, xf, u_prev, dt_prev, init)
        ob, keep = self._pack_obstacles(obstacles, B)
        (r, outs), ng = self._outputs(B), np.zeros(B, np.int32)
        self._check(self._lib.mpc_step_batch(self._h, B, *map(_addr, inputs), ob, int(outer_iterations), int(bool(adapt)), int(n_min), int(n_max if n_max > 0 else self.n),
                                             float(dt_hyst_ratio), *outs, _addr(ng)))
        return r, ng

    def cycle_params(self, **fields) -> MpcCycleParams:
        """mpc_cycle_params with the reference's in-code defaults (mpc_cycle_params_defaults), then the given fields"""
        return _params("mpc_cycle_params", MpcCycleParams, self._lib.mpc_cycle_params_defaults, fields)

    def controller_step(self, params: MpcCycleParams, plan, n_plan, x_feedback=None, feedback_age=None, reset=None, u_prev=None, dt_prev=None, obstacles=None):
        """One whole Controller::step cycle for B robots (mpc_controller_step_batch; src/controller.cpp:111-179): state estimate, re-initialisation decision, initial
        trajectory from the plan or grid update of the slot's previous solution, the solves.  plan (B, plan_stride, 3) with n_plan (B,) poses each (first = the
        odometry pose, last = the goal); x_feedback (B, 3) with feedback_age (B,) seconds, both or neither; reset (B,) non-zero where Controller::reset() was called.
        Returns (BatchResult, reinit (B,) MPC_REINIT_* bits, grid sizes (B,))."""
        plan = np.ascontiguousarray(plan, dtype=np.float64)
        B, stride = int(plan.shape[0]), int(plan.shape[1])
        plan = _as_f64(plan, (B, stride, 3))
        npl = _as_i32(n_plan, B, "n_plan")
        cycle = (_as_f64(x_feedback, (B, 3)), _as_f64(feedback_age, (B,)), _as_i32(reset, B), _as_f64(u_prev, (B, 2)), _as_f64(dt_prev, (B,)))
        ob, keep = self._pack_obstacles(obstacles, B)
        (r, outs), ri, ng = self._outputs(B), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._check(self._lib.mpc_controller_step_batch(self._h, B, C.byref(params), _addr(plan), _addr(npl), stride, *map(_addr, cycle), ob, *outs, _addr(ri), _addr(ng)))
        return r, ri, ng

    def controller_step_device(self, B: int, params: MpcCycleParams, plan: int, n_plan: int, plan_stride: int, x_feedback: Optional[int], feedback_age: Optional[int],
                               reset: Optional[int], u_prev: Optional[int], dt_prev: Optional[int], x_out: int, u_out: int, dt_out: int, status: Optional[int],
                               iters: Optional[int], reinit_out: Optional[int] = None, obstacles=None) -> None:
        """mpc_controller_step_batch_device: the same cycle with device addresses (ints), asynchronous on the solver's stream, no host round trip"""
        cycle, outs = (x_feedback, feedback_age, reset, u_prev, dt_prev), (x_out, u_out, dt_out, status, iters, reinit_out)
        self._check(self._lib.mpc_controller_step_batch_device(self._h, int(B), C.byref(params), _dev(plan), _dev(n_plan), int(plan_stride), *map(_dev, cycle),
                                                               _dev_obstacles(obstacles), *map(_dev, outs)))

    def controller_state(self, B: int):
        """(seq (B,), empty (B,), last_goal (B, 3)) of the controller slots (mpc_controller_state)"""
        seq = np.zeros(B, np.int32); empty = np.zeros(B, np.int32); goal = np.zeros((B, 3))
        self._check(self._lib.mpc_controller_state(self._h, int(B), _addr(seq), _addr(empty), _addr(goal)))
        return seq, empty, goal

    # ---- device buffers (raw HBM addresses, e.g. torch tensors' data_ptr()) -----
    def solve_device(self, B: int, x0: int, xf: int, u_prev: Optional[int], dt_prev: Optional[int], x_init: Optional[int],
                     u_init: Optional[int], dt_init: Optional[int], x_out: int, u_out: int, dt_out: int,
                     status: Optional[int], iters: Optional[int], obstacles=None) -> None:
        """Asynchronous solve on the solver's stream; all arguments are device addresses (ints)."""
        self._check(self._lib.mpc_solve_batch_device(self._h, B, *map(_dev, (x0, xf, u_prev, dt_prev, x_init, u_init, dt_init)), _dev_obstacles(obstacles),
                                                     *map(_dev, (x_out, u_out, dt_out, status, iters))))

    def evaluate(self, x0, xf, x, u, dt, u_prev=None, dt_prev=None, obstacles=None) -> TrajectoryEval:
        """Objective, largest equality / inequality violation and clearance to every obstacle of B trajectories under this solver's NLP (mpc_evaluate_batch), in
        fp64 whatever the solver's precision is.  x (B, n, 3), u (B, n, 2), dt (B,) in the layout of BatchResult; x0 / xf (B, 3) or None (= the trajectory's own first /
        last grid point); obstacles as for solve()."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        B, n = int(x.shape[0]), self.n
        x, u, dt = _as_f64(x, (B, n, 3)), _as_f64(u, (B, n, 2)), _as_f64(dt, (B,))
        x0, xf, u_prev, dt_prev = _as_f64(x0, (B, 3)), _as_f64(xf, (B, 3)), _as_f64(u_prev, (B, 2)), _as_f64(dt_prev, (B,))
        ob, keep = self._pack_obstacles(obstacles, B)
        r = TrajectoryEval(np.empty(B), np.empty(B), np.empty(B), np.empty(B), np.empty((B, 2), np.int32))
        out = MpcEvalOut(r.objective.ctypes.data, r.eq_violation.ctypes.data, r.ineq_violation.ctypes.data, r.clearance.ctypes.data, r.closest.ctypes.data)
        self._check(self._lib.mpc_evaluate_batch(self._h, B, *map(_addr, (x0, xf, u_prev, dt_prev, x, u, dt)), ob, C.byref(out)))
        return r

    def evaluate_device(self, B: int, x0: Optional[int], xf: Optional[int], x: int, u: int, dt: Optional[int], objective: Optional[int] = None, eq_violation: Optional[int] = None,
                        ineq_violation: Optional[int] = None, clearance: Optional[int] = None, closest: Optional[int] = None, u_prev: Optional[int] = None,
                        dt_prev: Optional[int] = None, obstacles=None) -> None:
        """mpc_evaluate_batch_device: the same with device addresses (ints), asynchronous on the solver's stream -- e.g. right behind solve_device on its outputs"""
        out = MpcEvalOut(objective or None, eq_violation or None, ineq_violation or None, clearance or None, closest or None)
        self._check(self._lib.mpc_evaluate_batch_device(self._h, int(B), *map(_dev, (x0, xf, u_prev, dt_prev, x, u, dt)), _dev_obstacles(obstacles), C.byref(out)))

    def plan_params(self, **fields) -> MpcPlanParams:
        """mpc_plan_params with the reference's in-code defaults (mpc_plan_params_defaults), then the given fields"""
        return _params("mpc_plan_params", MpcPlanParams, self._lib.mpc_plan_params_defaults, fields)

    def plan_inputs(self, params: MpcPlanParams, global_plan, n_global, robot_pose, plan_stride: int, plan_begin=None, via_points: bool = False) -> PlanInputs:
        """What the plugin prepares before Controller::step, for B robots (mpc_plan_inputs_batch; src/mpc_local_planner_ros.cpp:294-354): prune, select, via-points,
        goal-reached test, local goal heading, start / goal overwrite.  global_plan (B, gstride, 3) in the planning frame with n_global (B,) poses each; robot_pose (B, 3);
        plan_begin (B,) the persistent fronts of the cycle before (None = 0).  via_points: also fill n_via / via (needs cfg.max_via_points > 0)."""
        gp = np.ascontiguousarray(global_plan, dtype=np.float64)
        B, gstride = int(gp.shape[0]), int(gp.shape[1])
        gp = _as_f64(gp, (B, gstride, 3))
        ng = _as_i32(n_global, B, "n_global")
        rp = _as_f64(robot_pose, (B, 3))
        r = PlanInputs(np.zeros((B, int(plan_stride), 3)), np.zeros(B, np.int32),
                       np.zeros(B, np.int32) if plan_begin is None else np.array(plan_begin, dtype=np.int32).reshape(B),
                       np.zeros(B, np.int32), np.zeros(B, np.int32),
                       np.zeros(B, np.int32) if via_points else None, np.zeros((B, max(int(self.cfg.max_via_points), 0), 3)) if via_points else None)
        self._check(self._lib.mpc_plan_inputs_batch(self._h, B, C.byref(params), _addr(gp), _addr(ng), gstride, _addr(rp), _addr(r.plan_begin), _addr(r.plan), _addr(r.n_plan),
                                                    int(plan_stride), _addr(r.n_via), _addr(r.via), _addr(r.goal_idx), _addr(r.flags)))
        return r

    def plan_inputs_device(self, B: int, params: MpcPlanParams, global_plan: int, n_global: int, gstride: int, robot_pose: int, plan_begin: Optional[int], plan: int,
                           n_plan: int, plan_stride: int, n_via: Optional[int] = None, via: Optional[int] = None, goal_idx: Optional[int] = None,
                           flags: Optional[int] = None) -> None:
        """mpc_plan_inputs_batch_device: the same with device addresses (ints), asynchronous on the solver's stream; plan / n_plan feed controller_step_device, n_via / via
        mpc_set_via_points_device"""
        self._check(self._lib.mpc_plan_inputs_batch_device(self._h, int(B), C.byref(params), _dev(global_plan), _dev(n_global), int(gstride), _dev(robot_pose), _dev(plan_begin),
                                                           _dev(plan), _dev(n_plan), int(plan_stride), _dev(n_via), _dev(via), _dev(goal_idx), _dev(flags)))

    def commands(self, u, status, feasible=None, plan_flags=None, infeasible_count=None) -> Commands:
        """What the plugin does with the step's result, for B robots (mpc_commands_batch; src/mpc_local_planner_ros.cpp:394-452): the velocity command, the result code,
        the reset flag and the previous control of the next cycle.  u (B, n, 2) = BatchResult.u; status (B,); feasible (B,) of check_feasibility (None = feasible);
        plan_flags (B,) of plan_inputs (None = none); infeasible_count (B,): the counts so far (None = 0)."""
        u = np.ascontiguousarray(u, dtype=np.float64)
        B = int(u.shape[0])
        u = _as_f64(u, (B, self.n, 2))
        st, fe, fl = _as_i32(status, B), _as_i32(feasible, B), _as_i32(plan_flags, B)
        r = Commands(np.zeros((B, 3)), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros((B, 2)),
                     np.zeros(B, np.int32) if infeasible_count is None else np.array(infeasible_count, dtype=np.int32).reshape(B))
        self._check(self._lib.mpc_commands_batch(self._h, B, *map(_addr, (u, st, fe, fl, r.cmd, r.result, r.reset_next, r.u_prev_next, r.infeasible_count))))
        return r

    def commands_device(self, B: int, u: int, status: int, feasible: Optional[int], plan_flags: Optional[int], cmd: int, result: int, reset_next: Optional[int] = None,
                        u_prev_next: Optional[int] = None, infeasible_count: Optional[int] = None) -> None:
        """mpc_commands_batch_device: the same with device addresses (ints), asynchronous on the solver's stream; reset_next / u_prev_next are the reset / u_prev of the
        next controller_step_device"""
        self._check(self._lib.mpc_commands_batch_device(self._h, int(B), *map(_dev, (u, status, feasible, plan_flags, cmd, result, reset_next, u_prev_next, infeasible_count))))

    def pool_params(self, **fields) -> MpcPoolParams:
        """mpc_pool_params with the library's defaults (mpc_pool_params_defaults: reach = cfg.cutoff_dist, min_speed = 0.001, append = 1), then the given fields"""
        return _params("mpc_pool_params", MpcPoolParams, lambda p: self._lib.mpc_pool_params_defaults(self._h, p), fields)

    def obstacles_from_pool(self, pool, robot_pose, self_index=None, params=None, obstacles=None):
        """Obstacles that are not in the costmap, for B robots (mpc_obstacles_from_pool, include/mpc_fleet.h): the entries of a shared pool within params.reach of each
        robot, the nearest ones when they do not all fit, behind what the robot's container holds.  pool = (n_vertices (P,), vertices (P, V, 2)[, radius (P,)[, velocity
        (P, 2)]]) in the planning frame; robot_pose (B, 3); self_index (B,): the pool entry that is the robot itself (-1 / None: none); obstacles: an existing container
        (n_obstacles, n_vertices, vertices[, radius[, velocity]]) to append to -- it is copied, not written -- or None for an empty one.
        Returns (n_obstacles (B,), n_vertices (B, O), vertices (B, O, V, 2), radius (B, O), velocity (B, O, 2), dropped (B,), n_taken (B,)): the first five are `obstacles`
        of solve() / step() / controller_step()."""
        rp = np.ascontiguousarray(robot_pose, dtype=np.float64)
        B, O, V = int(rp.shape[0]), int(self.cfg.max_obstacles), max(1, int(self.cfg.max_vertices))
        rp = _as_f64(rp, (B, 3))
        pnv = np.ascontiguousarray(pool[0], dtype=np.int32).reshape(-1)
        P = int(pnv.shape[0])
        pv = _as_f64(pool[1], (P, V, 2))
        pr = _as_f64(pool[2], (P,)) if len(pool) > 2 and pool[2] is not None else None
        pvel = _as_f64(pool[3], (P, 2)) if len(pool) > 3 and pool[3] is not None else None
        si = _as_i32(self_index, B, "self_index")
        params = self.pool_params() if params is None else params
        given = tuple(obstacles) + (None,) * 5 if obstacles is not None else (None,) * 5
        held = lambda a, shape, dtype: np.zeros(shape, dtype) if a is None else np.array(a, dtype=dtype).reshape(shape)
        no, nv, vt = held(given[0], (B,), np.int32), held(given[1], (B, O), np.int32), held(given[2], (B, O, V, 2), np.float64)
        rd, vl = held(given[3], (B, O), np.float64), held(given[4], (B, O, 2), np.float64)
        dr, tk = np.zeros(B, np.int32), np.zeros(B, np.int32)
        cp = MpcPool(P, *(a.ctypes.data if a is not None and P > 0 else None for a in (pnv, pv, pr, pvel)))
        self._check(self._lib.mpc_obstacles_from_pool(self._h, B, C.byref(cp), _addr(rp), _addr(si), C.byref(params), *map(_addr, (no, nv, vt, rd, vl, dr, tk))))
        return no, nv, vt, rd, vl, dr, tk

    def obstacles_from_pool_device(self, B: int, pool, robot_pose: int, self_index: Optional[int], params: MpcPoolParams, n_obstacles: int, n_vertices: int, vertices: int,
                                   radius: Optional[int] = None, velocity: Optional[int] = None, dropped: Optional[int] = None, n_taken: Optional[int] = None) -> None:
        """mpc_obstacles_from_pool_device: the same with device addresses (ints), asynchronous on the solver's stream; pool = (P, n_vertices, vertices[, radius[, velocity]])
        with device addresses; n_obstacles is read and written, e.g. right behind mpc_costmap_to_obstacles_device on the same arrays"""
        cp = MpcPool(int(pool[0]), *((tuple(a or None for a in pool[1:]) + (None,) * 4)[:4]))
        self._check(self._lib.mpc_obstacles_from_pool_device(self._h, int(B), C.byref(cp), _dev(robot_pose), _dev(self_index), C.byref(params),
                                                             *map(_dev, (n_obstacles, n_vertices, vertices, radius, velocity, dropped, n_taken))))

    def fleet_pool(self, robot_pose, x=None, dt=None, status=None, radius=0.0, pool=None, pool_offset: int = 0):
        """A pool made of the fleet itself (mpc_fleet_pool, include/mpc_fleet.h): robot b becomes entry pool_offset + b -- a circle of its radius at its pose, with the
        velocity of the first interval of its own plan.  robot_pose (B, 3); x (B, n, 3), dt (B,), status (B,): BatchResult.x / .dt / .status of the robots' solves (None:
        velocity 0); radius: one number or (B,).  pool: existing arrays (n_vertices, vertices, radius, velocity) to write into -- copied -- or None for one of
        pool_offset + B entries.  Returns (n_vertices (P,), vertices (P, V, 2), radius (P,), velocity (P, 2)): `pool` of obstacles_from_pool, with self_index =
        pool_offset + arange(B)."""
        rp = np.ascontiguousarray(robot_pose, dtype=np.float64)
        B, V, off = int(rp.shape[0]), max(1, int(self.cfg.max_vertices)), int(pool_offset)
        rp = _as_f64(rp, (B, 3))
        xs, dts, st = _as_f64(x, (B, self.n, 3)), _as_f64(dt, (B,)), _as_i32(status, B, "status")
        per_robot = None if np.ndim(radius) == 0 else _as_f64(radius, (B,))
        P = max(off, 0) + B if pool is None else int(np.shape(pool[0])[0])
        if off < 0 or off + B > P:
            raise ValueError("the pool has no room for pool_offset + B entries")
        held = lambda a, shape, dtype: np.zeros(shape, dtype) if a is None else np.array(a, dtype=dtype).reshape(shape)
        given = (None,) * 4 if pool is None else tuple(pool)
        nv, vt, rd, vl = held(given[0], (P,), np.int32), held(given[1], (P, V, 2), np.float64), held(given[2], (P,), np.float64), held(given[3], (P, 2), np.float64)
        self._check(self._lib.mpc_fleet_pool(self._h, B, _addr(rp), _addr(xs), _addr(dts), _addr(st), 0.0 if per_robot is not None else float(radius), _addr(per_robot), off,
                                             *map(_addr, (nv, vt, rd, vl))))
        return nv, vt, rd, vl

    def fleet_pool_device(self, B: int, robot_pose: int, x: Optional[int], dt: Optional[int], status: Optional[int], radius: float, pool_n_vertices: int, pool_vertices: int,
                          pool_radius: Optional[int] = None, pool_velocity: Optional[int] = None, pool_offset: int = 0, radius_per_robot: Optional[int] = None) -> None:
        """mpc_fleet_pool_device: the same with device addresses (ints), asynchronous on the solver's stream -- e.g. right behind solve_device on its outputs; the pool
        arrays feed obstacles_from_pool_device"""
        self._check(self._lib.mpc_fleet_pool_device(self._h, int(B), _dev(robot_pose), _dev(x), _dev(dt), _dev(status), float(radius), _dev(radius_per_robot), int(pool_offset),
                                                    *map(_dev, (pool_n_vertices, pool_vertices, pool_radius, pool_velocity))))

    def set_grid_sizes(self, n_grid=None):
        """Per-instance grid sizes n_i <= cfg.n for the following solves (grid adaptation); None = uniform cfg.n."""
        a = None if n_grid is None else np.ascontiguousarray(n_grid, dtype=np.int32)
        self._check(self._lib.mpc_set_grid_sizes(self._h, _addr(a), 0 if a is None else int(a.shape[0])))

    def set_parameter_sets(self, sets=None, set_of=None):
        """Per-instance parameter sets for the following solves (mpc_set_parameter_sets): instance b solves with sets[set_of[b]], a complete MpcConfig
        that differs from the handle's configuration in double fields only.  set_of=None: one set per instance (instance b uses sets[b]); sets=None
        gives every instance the handle's own configuration again."""
        if sets is None:
            self._check(self._lib.mpc_set_parameter_sets(self._h, 0, None, 0, None))
            return
        sets = list(sets)
        arr = (MpcConfig * len(sets))(*sets)
        so = np.ascontiguousarray(np.arange(len(sets)) if set_of is None else set_of, dtype=np.int32)
        self._check(self._lib.mpc_set_parameter_sets(self._h, len(sets), C.cast(arr, C.c_void_p), int(so.shape[0]), _addr(so)))

    def set_via_points(self, n_via=None, via=None):
        """Via-points of the minimum_time_via_points objective for the following solves: n_via[B], via[B][cfg.max_via_points][3]
        (x, y, theta); None clears them."""
        if n_via is None:
            self._check(self._lib.mpc_set_via_points(self._h, 0, None, None))
            return
        nv = np.ascontiguousarray(n_via, dtype=np.int32)
        vp = np.ascontiguousarray(via, dtype=np.float64)
        assert vp.shape == (nv.shape[0], self.cfg.max_via_points, 3), vp.shape
        self._check(self._lib.mpc_set_via_points(self._h, int(nv.shape[0]), _addr(nv), _addr(vp)))

    @staticmethod
    def _costmap_inputs(cost, origin, robot_pose):
        """(cost uint8 (B, size_y, size_x), origin (B, 2), robot_pose (B, 3), B, size_x, size_y), contiguous, of a costmap step's inputs"""
        cost = np.ascontiguousarray(cost, dtype=np.uint8)
        B, sy, sx = cost.shape
        return cost, np.ascontiguousarray(origin, dtype=np.float64).reshape(B, 2), np.ascontiguousarray(robot_pose, dtype=np.float64).reshape(B, 3), B, sx, sy

    def _shape_outputs(self, B):
        """the zeroed outputs of costmap_to_polygons / costmap_to_lines, in the order of their return tuple"""
        O, V, z = int(self.cfg.max_obstacles), max(1, int(self.cfg.max_vertices)), np.zeros
        return z(B, np.int32), z((B, O), np.int32), z((B, O, V, 2)), z((B, O)), z((B, O, 2)), z(B, np.int32), z((B, 4), np.int32)

    def costmap_to_obstacles(self, cost, resolution, origin, robot_pose, behind_robot_dist=1.5):
        """Lethal costmap cells -> point obstacles in this solver's obstacle layout (mpc_costmap_to_obstacles).
        cost: uint8 [B][size_y][size_x]; origin [B][2]; robot_pose [B][3].  Returns (n_obstacles[B], n_vertices[B][O], vertices[B][O][V][2], dropped[B])."""
        cost, org, pose, B, sx, sy = self._costmap_inputs(cost, origin, robot_pose)
        O, V = self.cfg.max_obstacles, max(1, self.cfg.max_vertices)
        no = np.zeros(B, np.int32); nv = np.zeros((B, O), np.int32); vt = np.zeros((B, O, V, 2)); dr = np.zeros(B, np.int32)
        self._check(self._lib.mpc_costmap_to_obstacles(self._h, B, _addr(cost), sx, sy, float(resolution), _addr(org), _addr(pose), float(behind_robot_dist),
                                                       _addr(no), _addr(nv), _addr(vt), _addr(dr)))
        return no, nv, vt, dr

    def cluster_params(self, resolution, cluster_max_distance=0.4, behind_robot_dist=1.5) -> MpcClusterParams:
        """mpc_cluster_params with the library's rule (mpc_cluster_params_defaults): link_dist_sq = clamp(floor((cluster_max_distance / resolution)^2 + 1e-9), 1, 64)"""
        p = MpcClusterParams()
        self._lib.mpc_cluster_params_defaults(C.byref(p), float(resolution), float(cluster_max_distance))
        p.behind_robot_dist = float(behind_robot_dist)
        return p

    def costmap_to_polygons(self, cost, resolution, origin, robot_pose, cluster_max_distance=0.4, behind_robot_dist=1.5):
        """Lethal costmap cells -> one point, line or convex polygon per cluster of cells (mpc_costmap_to_polygons, include/mpc_costmap_clusters.h): the kept cells of
        costmap_to_obstacles, clustered within cluster_max_distance, each cluster as its convex hull (its bounding box when the hull has more than cfg.max_vertices
        vertices, its cells when the shape contains the robot).  Convex hulls overreach concave clusters: an L-shaped wall becomes a triangle.
        cost: uint8 [B][size_y][size_x]; origin [B][2]; robot_pose [B][3].  Returns (n_obstacles (B,), n_vertices (B, O), vertices (B, O, V, 2), radius (B, O),
        velocity (B, O, 2), dropped (B,), info (B, 4) = kept cells, clusters, hulls replaced by their box, clusters emitted as cells): the first five are `obstacles` of
        solve() / step() / controller_step()."""
        cost, org, pose, B, sx, sy = self._costmap_inputs(cost, origin, robot_pose)
        out = self._shape_outputs(B)
        p = self.cluster_params(resolution, cluster_max_distance, behind_robot_dist)
        self._check(self._lib.mpc_costmap_to_polygons(self._h, B, _addr(cost), sx, sy, float(resolution), _addr(org), _addr(pose), C.byref(p),
                                                      *map(_addr, out)))
        return out

    def costmap_to_polygons_device(self, B: int, cost: int, size_x: int, size_y: int, resolution: float, origin: int, robot_pose: int, params: MpcClusterParams,
                                   n_obstacles: int, n_vertices: int, vertices: int, radius: Optional[int] = None, velocity: Optional[int] = None,
                                   dropped: Optional[int] = None, info: Optional[int] = None) -> None:
        """mpc_costmap_to_polygons_device: the same with device addresses (ints), asynchronous on the solver's stream, in the slot of the fleet cycle where
        mpc_costmap_to_obstacles_device stands; slots at or above the new n_obstacles keep their bytes"""
        self._check(self._lib.mpc_costmap_to_polygons_device(self._h, int(B), _dev(cost), int(size_x), int(size_y), float(resolution), _dev(origin), _dev(robot_pose),
                                                             C.byref(params), *map(_dev, (n_obstacles, n_vertices, vertices, radius, velocity, dropped, info))))

    def line_params(self, resolution, cluster_max_distance=0.4, ransac_inlier_distance=0.15, behind_robot_dist=1.5, min_inliers=10, n_hypotheses=1500,
                    remaining_outliers=3) -> MpcLineParams:
        """mpc_line_params with the library's rules (mpc_line_params_defaults): link_dist_sq as cluster_params has it, inlier_dist_sq =
        clamp(floor((ransac_inlier_distance / resolution)^2 + 1e-9), 0, 64); the other fields as given (the shipped block's 10, 1500, 3)"""
        p = MpcLineParams()
        self._lib.mpc_line_params_defaults(C.byref(p), float(resolution), float(cluster_max_distance), float(ransac_inlier_distance))
        p.behind_robot_dist = float(behind_robot_dist)
        p.min_inliers, p.n_hypotheses, p.remaining_outliers = int(min_inliers), int(n_hypotheses), int(remaining_outliers)
        return p

    def costmap_to_lines(self, cost, resolution, origin, robot_pose, params: Optional[MpcLineParams] = None):
        """Lethal costmap cells -> line segments along the walls (mpc_costmap_to_lines, include/mpc_costmap_lines.h): the clusters of costmap_to_polygons; a cluster of
        at least min_inliers cells is cut into lines by a deterministic consensus rule in integers (an L-shaped wall becomes two segments and the free corner stays
        free), what is left of it comes out as points; smaller clusters come out as costmap_to_polygons emits them.  params: line_params(resolution) by default.
        cost: uint8 [B][size_y][size_x]; origin [B][2]; robot_pose [B][3].  Returns (n_obstacles (B,), n_vertices (B, O), vertices (B, O, V, 2), radius (B, O),
        velocity (B, O, 2), dropped (B,), info (B, 4) = kept cells, clusters, lines, cells emitted as points by the line rule): the first five are `obstacles` of
        solve() / step() / controller_step()."""
        cost, org, pose, B, sx, sy = self._costmap_inputs(cost, origin, robot_pose)
        out = self._shape_outputs(B)
        p = params if params is not None else self.line_params(resolution)
        self._check(self._lib.mpc_costmap_to_lines(self._h, B, _addr(cost), sx, sy, float(resolution), _addr(org), _addr(pose), C.byref(p),
                                                   *map(_addr, out)))
        return out

    def costmap_to_lines_device(self, B: int, cost: int, size_x: int, size_y: int, resolution: float, origin: int, robot_pose: int, params: MpcLineParams,
                                n_obstacles: int, n_vertices: int, vertices: int, radius: Optional[int] = None, velocity: Optional[int] = None,
                                dropped: Optional[int] = None, info: Optional[int] = None) -> None:
        """mpc_costmap_to_lines_device: the same with device addresses (ints), asynchronous on the solver's stream, in the slot of the fleet cycle where
        mpc_costmap_to_obstacles_device and mpc_costmap_to_polygons_device stand; slots at or above the new n_obstacles keep their bytes"""
        self._check(self._lib.mpc_costmap_to_lines_device(self._h, int(B), _dev(cost), int(size_x), int(size_y), float(resolution), _dev(origin), _dev(robot_pose),
                                                          C.byref(params), *map(_dev, (n_obstacles, n_vertices, vertices, radius, velocity, dropped, info))))

    def window_params(self, map_resolution, map_shape, **fields) -> MpcWindowParams:
        """mpc_window_params with the library's defaults (mpc_window_params_defaults) for a map of map_shape = (map_size_y, map_size_x) cells, then the given fields
        (map_origin and lattice_anchor as pairs)"""
        fields = {k: (C.c_double * 2)(*map(float, v)) if k in ("map_origin", "lattice_anchor") else v for k, v in fields.items()}
        return _params("mpc_window_params", MpcWindowParams,
                       lambda p: self._lib.mpc_window_params_defaults(p, float(map_resolution), int(map_shape[1]), int(map_shape[0])), fields)

    def costmap_window(self, map_cost, params: MpcWindowParams, robot_pose, size, resolution):
        """One shared map -> the local costmap window of every robot (mpc_costmap_window, include/mpc_costmap_window.h): the window's origin from the pose alone, on the
        lattice of the window's resolution; every cell the map byte under its centre (outside_value off the map); optionally inflated from the exact nearest lethal
        cell, the r cells around the window included.  map_cost: uint8 (map_size_y, map_size_x) in costmap values; robot_pose (B, 3); size = (size_x, size_y) in cells.
        Returns (cost uint8 (B, size_y, size_x), origin (B, 2), info (B, 4) = window cells inside the map, lethal cells, cells inflation changed, lethal cells in the
        halo only): cost and origin are what the costmap converters, controller_step and check_feasibility take."""
        m = np.ascontiguousarray(map_cost, dtype=np.uint8)
        if m.shape != (params.map_size_y, params.map_size_x):
            raise ValueError(f"map_cost has shape {m.shape}, params say {(params.map_size_y, params.map_size_x)}")
        pose = np.ascontiguousarray(robot_pose, dtype=np.float64).reshape(-1, 3)
        B, (sx, sy) = pose.shape[0], (int(size[0]), int(size[1]))
        cost, origin, info = np.zeros((B, max(sy, 0), max(sx, 0)), np.uint8), np.zeros((B, 2)), np.zeros((B, 4), np.int32)
        self._check(self._lib.mpc_costmap_window(self._h, B, _addr(m), C.byref(params), _addr(pose), sx, sy, float(resolution), _addr(cost), _addr(origin), _addr(info)))
        return cost, origin, info

    def costmap_window_device(self, B: int, map_cost: int, params: MpcWindowParams, robot_pose: int, size_x: int, size_y: int, resolution: float, cost: int, origin: int,
                              info: Optional[int] = None) -> None:
        """mpc_costmap_window_device: the same with device addresses (ints), asynchronous on the solver's stream, in front of the costmap converters of the fleet
        cycle; cost and origin are written in full"""
        self._check(self._lib.mpc_costmap_window_device(self._h, int(B), _dev(map_cost), C.byref(params), _dev(robot_pose), int(size_x), int(size_y), float(resolution),
                                                        _dev(cost), _dev(origin), _dev(info)))

    def scan_params(self, **fields) -> MpcScanParams:
        """mpc_scan_params with the library's defaults (mpc_scan_params_defaults), then the given fields (lattice_anchor as a pair, sensor_pose as a triple)"""
        sized = {"lattice_anchor": 2, "sensor_pose": 3}
        fields = {k: (C.c_double * sized[k])(*map(float, v)) if k in sized else v for k, v in fields.items()}
        return _params("mpc_scan_params", MpcScanParams, self._lib.mpc_scan_params_defaults, fields)

    def costmap_scans(self, params: MpcScanParams, robot_pose, ranges, size, resolution, layer=None, layer_cell=None, keep=None, cost=None, want_info=True):
        """One cycle of every robot's laser-scan obstacle layer (mpc_costmap_scans, include/mpc_costmap_scans.h): the layer rolled with the window, cleared along the
        rays, marked at the returns, and combined into the windows costmap_window made.  robot_pose (B, 3); ranges float32 (B, n_beams); size = (size_x, size_y) in
        cells; layer uint8 (B, size_y, size_x) and layer_cell int32 (B, 2) are the state of the previous cycle (None: a first cycle, which needs no keep); keep (B,)
        says which instances keep theirs (None: none does); cost uint8 (B, size_y, size_x) or None.  Nothing passed in is changed.
        Returns (layer, layer_cell, cost or None, info (B, 4) = beams kept, marked cells, free cells, window cells changed; None without want_info)."""
        pose = np.ascontiguousarray(robot_pose, dtype=np.float64).reshape(-1, 3)
        B, (sx, sy) = pose.shape[0], (int(size[0]), int(size[1]))
        rng = np.ascontiguousarray(ranges, dtype=np.float32).reshape(B, -1)
        shape = (B, max(sy, 0), max(sx, 0))
        if (layer is None) != (layer_cell is None) or (layer is None and keep is not None):
            raise ValueError("layer and layer_cell come together, and keep needs them")
        layer = np.zeros(shape, np.uint8) if layer is None else np.array(layer, dtype=np.uint8).reshape(shape)
        layer_cell = np.zeros((B, 2), np.int32) if layer_cell is None else np.array(layer_cell, dtype=np.int32).reshape(B, 2)
        cost = None if cost is None else np.array(cost, dtype=np.uint8).reshape(shape)
        info = np.zeros((B, 4), np.int32) if want_info else None
        self._check(self._lib.mpc_costmap_scans(self._h, B, C.byref(params), _addr(pose), _floats(rng.ctypes.data), int(rng.shape[1]), _addr(_as_i32(keep, B, "keep")), sx, sy,
                                                float(resolution), _addr(layer), _addr(layer_cell), _addr(cost), _addr(info)))
        return layer, layer_cell, cost, info

    def costmap_scans_device(self, B: int, params: MpcScanParams, robot_pose: int, ranges: int, n_beams: int, keep: Optional[int], size_x: int, size_y: int,
                             resolution: float, layer: int, layer_cell: int, cost: Optional[int] = None, info: Optional[int] = None) -> None:
        """mpc_costmap_scans_device: the same with device addresses (ints), asynchronous on the solver's stream, between costmap_window_device and the costmap
        converters of the fleet cycle; layer and layer_cell are the caller's and are rolled in place, cost is combined in place"""
        self._check(self._lib.mpc_costmap_scans_device(self._h, int(B), C.byref(params), _dev(robot_pose), _floats(ranges), int(n_beams), _dev(keep), int(size_x), int(size_y),
                                                       float(resolution), _dev(layer), _dev(layer_cell), _dev(cost), _dev(info)))

    def cast_params(self, map_resolution, map_shape, **fields) -> MpcCastParams:
        """mpc_cast_params with the library's defaults (mpc_cast_params_defaults) for a map of map_shape = (map_size_y, map_size_x) cells, then the given fields
        (map_origin as a pair, sensor_pose as a triple)"""
        sized = {"map_origin": 2, "sensor_pose": 3}
        fields = {k: (C.c_double * sized[k])(*map(float, v)) if k in sized else v for k, v in fields.items()}
        return _params("mpc_cast_params", MpcCastParams,
                       lambda p: self._lib.mpc_cast_params_defaults(p, float(map_resolution), int(map_shape[1]), int(map_shape[0])), fields)

    def scan_cast(self, map_cost, params: MpcCastParams, robot_pose, n_beams, pool=None, self_index=None):
        """The laser scan of every robot, cast through one shared map and a pool of other bodies (mpc_scan_cast, include/mpc_scan_cast.h): the ranges costmap_scans
        takes.  map_cost: uint8 (map_size_y, map_size_x) in costmap values; robot_pose (B, 3); pool = (n_vertices (P,), vertices (P, V, 2)[, radius (P,)]) as
        obstacles_from_pool and fleet_pool have it (a velocity behind them is not read), or None; self_index (B,): the pool entry that is the robot itself (None: none).
        Returns (ranges float32 (B, n_beams), hit int32 (B, n_beams): -2 the map, p a pool entry, -1 no return, info (B, 4) = beams returned by the map, by the pool,
        without a return, blocking map cells around the sensor)."""
        m = np.ascontiguousarray(map_cost, dtype=np.uint8)
        if m.shape != (params.map_size_y, params.map_size_x):
            raise ValueError(f"map_cost has shape {m.shape}, params say {(params.map_size_y, params.map_size_x)}")
        pose = np.ascontiguousarray(robot_pose, dtype=np.float64).reshape(-1, 3)
        B, n, V = pose.shape[0], int(n_beams), max(1, int(self.cfg.max_vertices))
        cp = None
        if pool is not None:
            pnv = np.ascontiguousarray(pool[0], dtype=np.int32).reshape(-1)
            P = int(pnv.shape[0])
            pv = _as_f64(pool[1], (P, V, 2))
            pr = _as_f64(pool[2], (P,)) if len(pool) > 2 and pool[2] is not None else None
            cp = MpcPool(P, *(a.ctypes.data if a is not None and P > 0 else None for a in (pnv, pv, pr)), None)
        si = _as_i32(self_index, B, "self_index")
        ranges, hit, info = np.zeros((B, max(n, 0)), np.float32), np.zeros((B, max(n, 0)), np.int32), np.zeros((B, 4), np.int32)
        self._check(self._lib.mpc_scan_cast(self._h, B, _addr(m), C.byref(params), _addr(pose), None if cp is None else C.byref(cp), _addr(si), n, _floats(ranges.ctypes.data),
                                            _addr(hit), _addr(info)))
        return ranges, hit, info

    def scan_cast_device(self, B: int, map_cost: int, params: MpcCastParams, robot_pose: int, n_beams: int, ranges: int, pool=None, self_index: Optional[int] = None,
                         hit: Optional[int] = None, info: Optional[int] = None) -> None:
        """mpc_scan_cast_device: the same with device addresses (ints), asynchronous on the solver's stream, in front of costmap_window_device and
        costmap_scans_device, which takes `ranges` as it is; pool = (P, n_vertices, vertices[, radius]) with device addresses, or None"""
        cp = None if pool is None else MpcPool(int(pool[0]), *((tuple(a or None for a in pool[1:4]) + (None,) * 4)[:4]))
        self._check(self._lib.mpc_scan_cast_device(self._h, int(B), _dev(map_cost), C.byref(params), _dev(robot_pose), None if cp is None else C.byref(cp), _dev(self_index),
                                                   int(n_beams), _floats(ranges), _dev(hit), _dev(info)))

    def plant_params(self, map_resolution, map_shape, **fields) -> MpcPlantParams:
        """mpc_plant_params with the library's defaults (mpc_plant_params_defaults) for a map of map_shape = (map_size_y, map_size_x) cells, then the given fields
        (map_origin as a pair, v_min / v_max / a_max as triples; footprint as up to 16 (x, y) pairs in the robot frame, which sets n_footprint too unless it is given)"""
        fields = dict(fields)
        if "footprint" in fields:
            pts = [(float(x), float(y)) for x, y in fields["footprint"]]
            if len(pts) > 16:
                raise ValueError("mpc_plant_params holds a footprint of at most 16 vertices")
            fields.setdefault("n_footprint", len(pts))
            fields["footprint"] = ((C.c_double * 2) * 16)(*((C.c_double * 2)(*q) for q in pts))
        sized = {"map_origin": 2, "v_min": 3, "v_max": 3, "a_max": 3}
        fields = {k: (C.c_double * sized[k])(*map(float, v)) if k in sized else v for k, v in fields.items()}
        return _params("mpc_plant_params", MpcPlantParams,
                       lambda p: self._lib.mpc_plant_params_defaults(p, float(map_resolution), int(map_shape[1]), int(map_shape[0])), fields)

    def plant_step(self, params: MpcPlantParams, cmd, pose, map_cost=None, pool=None, self_index=None, vel=None):
        """Every robot moved by its command for params.n_substeps sub-steps of params.interval seconds, stalled where its footprint's outline would meet the map or a
        body of the pool (mpc_plant_step, include/mpc_plant.h).  cmd (B, 3) = Commands.cmd; pose (B, 3); map_cost: uint8 (map_size_y, map_size_x) in costmap values, or
        None for no map test; pool = (n_vertices (P,), vertices (P, V, 2)[, radius (P,)]) as scan_cast takes it, or None; self_index (B,): the pool entry that is the
        robot itself (None: none); vel (B, 3): the body velocity kept between calls, or None to start every call at the commanded velocity.  Nothing given is written.
        Returns (pose (B, 3), vel (B, 3) or None, stall (B,) = blocked sub-steps, info (B, 4) = sub-steps moved, first blocked sub-step, its reason (-4 heading, -3 off
        the map, -2 the map, p a pool entry), the lowest edge that shows it)."""
        pose = np.array(pose, dtype=np.float64).reshape(-1, 3)
        B, V = pose.shape[0], max(1, int(self.cfg.max_vertices))
        cmd = _as_f64(cmd, (B, 3))
        vel = None if vel is None else np.array(_as_f64(vel, (B, 3)))
        m = None
        if map_cost is not None:
            m = np.ascontiguousarray(map_cost, dtype=np.uint8)
            if m.shape != (params.map_size_y, params.map_size_x):
                raise ValueError(f"map_cost has shape {m.shape}, params say {(params.map_size_y, params.map_size_x)}")
        cp = None
        if pool is not None:
            pnv = np.ascontiguousarray(pool[0], dtype=np.int32).reshape(-1)
            P = int(pnv.shape[0])
            pv = _as_f64(pool[1], (P, V, 2))
            pr = _as_f64(pool[2], (P,)) if len(pool) > 2 and pool[2] is not None else None
            cp = MpcPool(P, *(a.ctypes.data if a is not None and P > 0 else None for a in (pnv, pv, pr)), None)
        si = _as_i32(self_index, B, "self_index")
        stall, info = np.zeros(B, np.int32), np.zeros((B, 4), np.int32)
        self._check(self._lib.mpc_plant_step(self._h, B, _addr(m), C.byref(params), _addr(cmd), None if cp is None else C.byref(cp), _addr(si), _addr(pose), _addr(vel),
                                             _addr(stall), _addr(info)))
        return pose, vel, stall, info

    def plant_step_device(self, B: int, params: MpcPlantParams, cmd: int, pose: int, map_cost: Optional[int] = None, pool=None, self_index: Optional[int] = None,
                          vel: Optional[int] = None, stall: Optional[int] = None, info: Optional[int] = None) -> None:
        """mpc_plant_step_device: the same with device addresses (ints), asynchronous on the solver's stream, behind commands_device, whose `cmd` it takes as it is, and
        in front of fleet_pool_device, which takes `pose`; pose and vel are advanced in place; pool = (P, n_vertices, vertices[, radius]) with device addresses, or None"""
        cp = None if pool is None else MpcPool(int(pool[0]), *((tuple(a or None for a in pool[1:4]) + (None,) * 4)[:4]))
        self._check(self._lib.mpc_plant_step_device(self._h, int(B), _dev(map_cost), C.byref(params), _dev(cmd), None if cp is None else C.byref(cp), _dev(self_index),
                                                    _dev(pose), _dev(vel), _dev(stall), _dev(info)))

    def last_costmap_ms(self) -> float:
        """device milliseconds of the most recent costmap step (mpc_last_costmap_ms), 0 when there has been none"""
        ms = C.c_float(0.0)
        self._check(self._lib.mpc_last_costmap_ms(self._h, C.byref(ms)))
        return float(ms.value)

    def last_candidates(self, B: int):
        """(winner[B], iters_total[B]) of the most recent solve (mpc_last_candidates): index of the candidate initial trajectory that
        supplied each instance's result (-1: none converged) and the iterations spent over all candidates of the instance."""
        win = np.empty(B, np.int32); tot = np.empty(B, np.int32)
        self._check(self._lib.mpc_last_candidates(self._h, int(B), _addr(win), _addr(tot)))
        return win, tot

    def check_feasibility(self, x, cost, resolution, origin, footprint_spec, inscribed_radius, min_resolution_collision_check_angular=0.3, look_ahead_idx=-1):
        """Controller::isPoseTrajectoryFeasible for B planned trajectories (mpc_check_feasibility): x (B, n, 3), cost uint8 (B, size_y, size_x),
        origin (B, 2), footprint_spec (F, 2) in the robot frame.  Returns int32 (B,): 1 feasible, 0 not."""
        x = _as_f64(x, (np.asarray(x).shape[0], self.n, 3))
        B = x.shape[0]
        cost = np.ascontiguousarray(cost, dtype=np.uint8)
        _, sy, sx = cost.shape
        org = np.ascontiguousarray(origin, dtype=np.float64).reshape(B, 2)
        spec = np.ascontiguousarray(footprint_spec, dtype=np.float64).reshape(-1, 2)
        out = np.zeros(B, np.int32)
        self._check(self._lib.mpc_check_feasibility(self._h, B, _addr(x), _addr(cost), sx, sy, float(resolution), _addr(org), _addr(spec), int(spec.shape[0]),
                                                    float(inscribed_radius), float(min_resolution_collision_check_angular), int(look_ahead_idx), _addr(out)))
        return out

    def grid_update_device(self, B: int, x0_new: Optional[int], x: int, u: int, dt: int, adapt: bool = False, n_min: int = 3, n_max: int = 0, dt_hyst_ratio: float = 0.1):
        """mpc_grid_update_device: warm-start shift (fixed grid) / single-step grid adaptation + resampling (variable grid) of a whole batch, in place
        on device arrays (addresses)."""
        self._check(self._lib.mpc_grid_update_device(self._h, int(B), _dev(x0_new), _dev(x), _dev(u), _dev(dt), int(bool(adapt)), int(n_min), int(n_max or self.n), float(dt_hyst_ratio)))

    def grid_sizes(self, B: int):
        out = np.zeros(B, np.int32)
        self._check(self._lib.mpc_get_grid_sizes(self._h, int(B), _addr(out)))
        return out

    def last_rows_dropped(self, B: int):
        """per instance: clearance rows that did not fit into max_obstacle_rows in the most recent solve (mpc_last_rows_dropped)"""
        out = np.zeros(B, np.int32)
        self._check(self._lib.mpc_last_rows_dropped(self._h, int(B), _addr(out)))
        return out

    def synchronize(self):
        self._check(self._lib.mpc_synchronize(self._h))

    def lds_bytes(self) -> int:
        """dynamic LDS of one workgroup of the solve kernel = the working set of one instance; 163840 // lds_bytes() workgroups are resident per compute unit"""
        b = C.c_int64(0)
        self._check(self._lib.mpc_lds_bytes(self._h, C.byref(b)))
        return int(b.value)

    def occupancy(self, B: int):
        """(resident workgroups per compute unit, dynamic LDS bytes of one) of the kernel a launch of B instances selects, from the runtime's occupancy calculation"""
        w, b = C.c_int32(0), C.c_int64(0)
        self._check(self._lib.mpc_occupancy(self._h, int(B), C.byref(w), C.byref(b)))
        return int(w.value), int(b.value)

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        self._check(self._lib.mpc_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)
