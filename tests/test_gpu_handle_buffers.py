"""GPU test (-m gpu) of the handle's buffers (the table of mpc_capi.hip that mpc_create allocates and fills from, mpc_reset refills from and mpc_destroy frees
from): a handle that is created, used, reset and destroyed over and over gives every device buffer back.  Per kind of handle (n = 8, max_batch = 16384) one
create / use / mpc_reset / destroy cycle, the free device memory, 64 more cycles, the free device memory again: the second reading is not lower than the first
by as much as 64 times the smallest buffer of such a handle ([max_batch] int32 = 64 KiB, so 4 MiB) -- what a leak of that one buffer would cost.  The kinds
cover the buffers a configuration may or may not get (MPC_MIXED's iteration counts, candidate records and kept multipliers, the block pool of the clearance
rows, the via-point copies) and the ones that are allocated or grown after mpc_create (the table of parameter sets: 2 sets, then 5; the helpers' staging:
an 8 x 8 costmap, then 64 x 64).  After the cycles a fresh handle of the kind returns, bit for bit, what the first one returned: x, u, dt, status and iters of
the solve, and per kind the winner of the hedged candidates, the dropped clearance rows, the trajectory under two parameter sets, the feasibility answers on
both maps.  The iterations summed over all hedged candidates (mpc_last_candidates) are not among them: how much of a losing hedge runs depends on when it sees
the winner, so that sum differs from launch to launch (83 against 84 here, before any change to the handle).

Observed drift (first reading minus second, the library before the table existed / with it): profiles/r10_capi_refactor.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, MAX_BATCH, B, CYCLES = 8, 16384, 4, 64
SMALLEST = MAX_BATCH * 4          # bytes of the smallest buffer of a handle: one int32 per instance


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
    }


KINDS = ("fp64", "mixed", "candidates_dual_warm_start", "point_obstacles", "via_points", "parameter_sets_2_then_5", "feasibility_8x8_then_64x64")


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
