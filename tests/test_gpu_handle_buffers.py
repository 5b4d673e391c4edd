"""GPU test (-m gpu) of the handle's buffers (the table of mpc_capi.hip that mpc_create allocates and fills from, mpc_reset refills from and mpc_destroy frees
from): a handle that is created, used, reset and destroyed over and over gives every device buffer back.  Per kind of handle (n = 8, max_batch = 16384) one
create / use / mpc_reset / destroy cycle, the free device memory, 64 more cycles, the free device memory again: the second reading is not lower than the first
by as much as 64 times the smallest buffer of such a handle ([max_batch] int32 = 64 KiB, so 4 MiB) -- what a leak of that one buffer would cost.  The kinds
cover the buffers a configuration may or may not get (MPC_MIXED's iteration counts, candidate records and kept multipliers, the block pool of the clearance
rows, the via-point copies) and the ones that are allocated or grown after mpc_create (the table of parameter sets: 2 sets, then 5; the helpers' staging:
an 8 x 8 costmap, then 64 x 64; the shared staging pair of the other host-pointer calls: mpc_evaluate_batch, mpc_plan_inputs_batch with
mpc_commands_batch and mpc_controller_step_batch at B = 3, then 70, mpc_costmap_to_obstacles on 8 x 8, then 64 x 64).  After the cycles a fresh handle of the kind returns, bit for bit, what the first one returned: x, u, dt, status and iters of
the solve, and per kind the winner of the hedged candidates, the dropped clearance rows, the trajectory under two parameter sets, the feasibility answers on
both maps.  The iterations summed over all hedged candidates (mpc_last_candidates) are not among them: how much of a losing hedge runs depends on when it sees
the winner, so that sum differs from launch to launch (83 against 84 here, before any change to the handle).

Observed drift (first reading minus second, the library before the table existed / with it): profiles/r10_capi_refactor.md; with the
shared staging pair and its four kinds: profiles/r15_capi_staging.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, MAX_BATCH, B, CYCLES = 8, 16384, 4, 64
SMALLEST = MAX_BATCH * 4          # bytes of the smallest buffer of a handle: one int32 per instance
SMALL, BIG = 3, 70                # batches of the kinds whose staging grows between two calls


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as pkg
    return pkg


def _result(r, **more):
    return dict(x=r.x, u=r.u, dt=r.dt, status=r.status, iters=r.iters, **more)


def _plain(m, s):
    return _result(s.solve(*m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0))))


def _candidates(m, s):
    r = s.solve(*m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0)))
    winner, _iters_total = s.last_candidates(B)      # iters_total is not compared: how much of a losing hedge runs depends on when it sees the winner (mpc_solve_kernel.hpp)
    return _result(r, winner=winner)


def _obstacles(m, s):
    x0, xf, up, dtp, ob = m.workloads.carlike_moving_obstacle_inputs(B, goal_range=(1.0, 2.0))
    return _result(s.solve(x0, xf, up, dtp, obstacles=ob[:4]), rows_dropped=s.last_rows_dropped(B))


def _via_points(m, s):
    x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0))
    via = np.zeros((B, 2, 3))
    via[:, 0, :2] = 0.5 * xf[:, :2] + 0.1
    s.set_via_points(np.full(B, 1, np.int32), via)
    return _result(s.solve(x0, xf, up, dtp))


def _parameter_sets(m, s):
    def robot(k):
        c = m.config_carlike_min_time(N)
        c.u_ub[0] = 0.4 - 0.03 * k
        return c
    inputs = m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0))
    s.set_parameter_sets([robot(k) for k in range(2)], np.arange(B) % 2)
    r2 = s.solve(*inputs)
    s.set_parameter_sets([robot(k) for k in range(5)], np.arange(B) % 5)          # more entries than the table has room for: it is replaced
    return _result(s.solve(*inputs), x_two_sets=r2.x)


def _feasibility(m, s):
    r = s.solve(*m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0)))
    feas = []
    for cells in (8, 64):                                                         # the second map does not fit the staging of the first
        cost = np.zeros((B, cells, cells), np.uint8)
        cost[:, cells // 2, :] = 254
        feas.append(s.check_feasibility(r.x, cost, 6.4 / cells, np.full((B, 2), -3.2), np.zeros((0, 2)), 0.2))
    return _result(r, feasible_8=feas[0], feasible_64=feas[1])


def _line_plans(x0, xf, stride):
    """(B, stride, 3) poses on the straight line from x0 to xf"""
    return np.ascontiguousarray(x0[:, None, :] + np.linspace(0.0, 1.0, stride)[None, :, None] * (xf - x0)[:, None, :])


def _evaluate(m, s):
    x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(BIG, goal_range=(1.0, 2.0))
    r = s.solve(x0, xf, up, dtp)
    more = {}
    for b in (SMALL, BIG):                                                        # the second batch does not fit the staging of the first
        e = s.evaluate(x0[:b], xf[:b], r.x[:b], r.u[:b], r.dt[:b], up[:b], dtp[:b])
        more.update({f"objective_{b}": e.objective, f"eq_{b}": e.eq_violation, f"ineq_{b}": e.ineq_violation, f"clearance_{b}": e.clearance, f"closest_{b}": e.closest})
    return _result(r, **more)


def _plan_inputs_commands(m, s):
    x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(BIG, goal_range=(1.0, 2.0))
    r = s.solve(x0, xf, up, dtp)
    more = {}
    for b in (SMALL, BIG):                                                        # 70: more than one 64-lane workgroup of the commands kernel, with a ragged tail
        q = s.plan_inputs(s.plan_params(), _line_plans(x0[:b], xf[:b], 16), np.full(b, 16, np.int32), x0[:b], 8)
        c = s.commands(r.u[:b], r.status[:b], plan_flags=q.flags, infeasible_count=np.arange(b) % 3)
        more.update({f"plan_{b}": q.plan, f"n_plan_{b}": q.n_plan, f"begin_{b}": q.plan_begin, f"goal_idx_{b}": q.goal_idx, f"flags_{b}": q.flags, f"cmd_{b}": c.cmd,
                     f"result_{b}": c.result, f"reset_next_{b}": c.reset_next, f"u_prev_next_{b}": c.u_prev_next, f"infeasible_{b}": c.infeasible_count})
    return _result(r, **more)


def _controller_step(m, s):
    x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(BIG, goal_range=(1.0, 2.0))
    more = {}
    for b in (SMALL, BIG):
        r, reinit, n_grid = s.controller_step(s.cycle_params(), _line_plans(x0[:b], xf[:b], 2), np.full(b, 2, np.int32), u_prev=up[:b], dt_prev=dtp[:b])
        more.update({f"x_{b}": r.x, f"u_{b}": r.u, f"dt_{b}": r.dt, f"status_{b}": r.status, f"iters_{b}": r.iters, f"reinit_{b}": reinit, f"n_grid_{b}": n_grid})
    return more


def _costmap(m, s):
    x0 = m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 2.0))[0]
    more = {}
    for cells in (8, 64):                                                         # the second map does not fit the staging of the first
        cost = np.zeros((B, cells, cells), np.uint8)
        cost[:, cells // 2, ::3] = 254
        no, nv, vt, dr = s.costmap_to_obstacles(cost, 6.4 / cells, np.full((B, 2), -3.2), x0)
        more.update({f"n_obstacles_{cells}": no, f"n_vertices_{cells}": nv, f"vertices_{cells}": vt, f"dropped_{cells}": dr})
    return more


def _kinds(m):
    from mpc_local_planner_amd import _abi as A
    cands = dict(candidates=(A.CAND_REFERENCE, A.CAND_HERMITE_FF, A.CAND_HERMITE_FR), candidate_max_iter=(40, 40, 40), candidate_param=(0.0, 2.0, 1.5))
    return {
        "fp64": (lambda: m.config_carlike_min_time(N), _plain),
        "mixed": (lambda: m.config_carlike_min_time(N, precision=A.MIXED), _plain),
        "candidates_dual_warm_start": (lambda: m.config_carlike_min_time(N, dual_warm_start=True, **cands), _candidates),
        "point_obstacles": (lambda: m.config_carlike_min_time(N, max_obstacles=3, max_vertices=1, max_obstacle_rows=4), _obstacles),
        "via_points": (lambda: m.config_carlike_min_time(N, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=2), _via_points),
        "parameter_sets_2_then_5": (lambda: m.config_carlike_min_time(N), _parameter_sets),
        "feasibility_8x8_then_64x64": (lambda: m.config_carlike_min_time(N), _feasibility),
        "evaluate_3_then_70": (lambda: m.config_carlike_min_time(N), _evaluate),
        "plan_inputs_commands_3_then_70": (lambda: m.config_carlike_min_time(N), _plan_inputs_commands),
        "controller_step_3_then_70": (lambda: m.config_carlike_min_time(N), _controller_step),
        "costmap_to_obstacles_8x8_then_64x64": (lambda: m.config_carlike_min_time(N, max_obstacles=3, max_vertices=1, max_obstacle_rows=4), _costmap),
    }


KINDS = ("fp64", "mixed", "candidates_dual_warm_start", "point_obstacles", "via_points", "parameter_sets_2_then_5", "feasibility_8x8_then_64x64", "evaluate_3_then_70",
         "plan_inputs_commands_3_then_70", "controller_step_3_then_70", "costmap_to_obstacles_8x8_then_64x64")


def test_the_kinds_are_the_listed_ones(m):
    assert tuple(_kinds(m)) == KINDS


@pytest.mark.parametrize("kind", KINDS)
def test_cycles_of_create_use_reset_destroy_give_every_buffer_back(m, kind):
    import torch
    make, use = _kinds(m)[kind]

    def cycle():
        s = m.BatchSolver(make(), max_batch=MAX_BATCH)
        out = use(m, s)
        s.reset()
        s.close()
        return out

    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    first = cycle()
    free1 = free_bytes()
    for _ in range(CYCLES):
        cycle()
    free2 = free_bytes()
    print(f"handle_buffers {kind}: free memory after 1 cycle {free1}, after {1 + CYCLES} cycles {free2}, drift {free1 - free2} bytes (bound {CYCLES * SMALLEST})")
    assert free1 - free2 < CYCLES * SMALLEST
    again = cycle()                                  # a fresh handle, after all of them
    assert sorted(again) == sorted(first)
    for key, v in first.items():
        assert again[key].tobytes() == v.tobytes(), key


def _same(a, b, what):
    assert len(a) == len(b), what
    for i, (u, v) in enumerate(zip(a, b)):
        assert np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes(), (what, i)


@pytest.mark.parametrize("kind", ("hedged_candidates", "one_candidate_point_obstacles"))
def test_other_host_calls_between_a_solve_and_last_candidates_leave_the_solve_alone(m, kind):
    """One handle: solve (host pointers), then evaluate, check_feasibility (64 x 64), plan_inputs, commands and -- on the handle with obstacles -- costmap_to_obstacles, each
    staging more than every call before it (so each grows the shared pair and writes over all of it), then last_candidates: the winners are those a second handle reports
    straight after the same solve, and every call returned, byte for byte, what it returns as the first call on a fresh handle.  Without hedged candidates the winners are
    read from the status array the solve left in its own device block (mpc_solver::d_out): they would not survive if the solve's outputs shared the other calls' staging."""
    from mpc_local_planner_amd import _abi as A
    obst = kind == "one_candidate_point_obstacles"
    if obst:
        make = lambda: m.BatchSolver(m.config_carlike_min_time(N, max_obstacles=3, max_vertices=1, max_obstacle_rows=4), max_batch=MAX_BATCH)
        x0, xf, up, dtp, ob = m.workloads.carlike_moving_obstacle_inputs(BIG, goal_range=(1.0, 2.0))
        ob = ob[:4]
    else:
        make = lambda: m.BatchSolver(m.config_carlike_min_time(N, candidates=(A.CAND_REFERENCE, A.CAND_HERMITE_FF, A.CAND_HERMITE_FR), candidate_max_iter=(40, 40, 40),
                                                               candidate_param=(0.0, 2.0, 1.5)), max_batch=MAX_BATCH)
        x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(BIG, goal_range=(1.0, 2.0))
        ob = None
    ref = make()
    want = ref.solve(x0, xf, up, dtp, obstacles=ob)
    want_winner = ref.last_candidates(BIG)[0]
    ref.close()
    rng = np.random.default_rng(5)
    cost = np.zeros((BIG, 64, 64), np.uint8)
    cost[:, 32, ::3] = 254
    org = np.full((BIG, 2), -3.2)
    wide = MAX_BATCH // 32                                     # batches that make the later calls' staging the larger one: 512 maps of 64 x 64 are 2 MiB
    gplan = _line_plans(x0, xf, 256)                           # 70 plans of 256 poses: 420 KiB, more than the 280 KiB of the 70 maps before them
    u_all = rng.uniform(-0.3, 0.3, (MAX_BATCH, N, 2))          # commands for max_batch robots: 1.2 MiB
    st_all = (np.arange(MAX_BATCH) % 5 == 0).astype(np.int32)
    calls = [
        ("evaluate", lambda s, r: (lambda e: (e.objective, e.eq_violation, e.ineq_violation, e.clearance, e.closest))(s.evaluate(x0, xf, r.x, r.u, r.dt, up, dtp, obstacles=ob))),
        ("check_feasibility", lambda s, r: (s.check_feasibility(r.x, cost, 0.1, org, np.zeros((0, 2)), 0.2),)),
        ("plan_inputs", lambda s, r: (lambda q: (q.plan, q.n_plan, q.plan_begin, q.goal_idx, q.flags))(s.plan_inputs(s.plan_params(), gplan, np.full(BIG, 256, np.int32), x0, 8))),
        ("commands", lambda s, r: (lambda c: (c.cmd, c.result, c.reset_next, c.u_prev_next, c.infeasible_count))(s.commands(u_all, st_all, infeasible_count=np.arange(MAX_BATCH) % 3))),
    ]
    if obst:
        wide_cost = np.zeros((wide, 64, 64), np.uint8)
        wide_cost[:, 20, ::5] = 254
        calls.append(("costmap_to_obstacles", lambda s, r: s.costmap_to_obstacles(wide_cost, 0.1, np.full((wide, 2), -3.2), np.zeros((wide, 3)))))
    s = make()
    r = s.solve(x0, xf, up, dtp, obstacles=ob)
    _same((r.x, r.u, r.dt, r.status, r.iters), (want.x, want.u, want.dt, want.status, want.iters), "solve")
    got = [(name, call(s, r)) for name, call in calls]
    winner = s.last_candidates(BIG)[0]
    s.close()
    assert winner.tobytes() == want_winner.tobytes()
    for (name, outputs), (_, call) in zip(got, calls):
        fresh = make()
        _same(outputs, call(fresh, want), name)
        fresh.close()
