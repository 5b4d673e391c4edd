"""GPU tests (-m gpu) of the fixed-layout kernel's per-solve lane constants (mpc_wave_pit.inc::PitLaneConsts): the fp64 headline kernel for records of 50 grid points
takes the places and steps of the partitioned sweeps' streams, its combine records and the forward half's pointer table from a packed per-lane table that is built once
per solve.  Only that instantiation does; the generic kernel (a handle created for n = 51 with every grid size set to 50) and the global form (STAGE_GLOBAL) work the same
values out per factorisation as before.  Same arithmetic on the same operands, so the three must agree BIT FOR BIT in x, u, dt, status and iteration count: after 1, 2 and
4 iterations (the iterate is written whatever the status) and after the full solve, with one candidate and with the headline's four, with dt_prev = 0 (no first rate rows)
and from a warm start (the forward half then runs from a non-trivial point).  Below 40 grid points the partitioned sweeps do not run and 50 is the only fixed layout, so
the grid stays at 50 and the batch is what is small: 64 instances of the bench's seed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N = 64, 50
FOUR = dict(candidates=(0, 5, 5, 7), candidate_param=(0.0, 2.0, 3.0, 1.5))
CAPS = (100, 45, 40, 35)


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")          # torch's HIP runtime before the library's
    import mpc_local_planner_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def inputs(m):
    return m.workloads.carlike_min_time_inputs(B, seed=20260924)


def _kw(four, max_iter):
    kw = {}
    if four: kw.update(FOUR, candidate_max_iter=CAPS if max_iter is None else (max_iter,) * 4)
    if max_iter is not None: kw["max_iter"] = max_iter
    return kw


def _pad(a):
    """an initial guess of 50 grid points for the handle created with 51: the last point once more (never read: every grid size is 50)"""
    return np.concatenate([a, a[:, -1:]], axis=1)


def _three(m, kw, inp, init=None):
    """the same batch through the fixed-layout kernel, the generic kernel and the global form"""
    from mpc_local_planner_amd import _abi as A
    fixed = m.BatchSolver(m.config_carlike_min_time(N, **kw), max_batch=B)
    rf = fixed.solve(*inp, init=init)
    fixed.close()
    generic = m.BatchSolver(m.config_carlike_min_time(N + 1, **kw), max_batch=B)
    generic.set_grid_sizes(np.full(B, N, dtype=np.int32))
    rg = generic.solve(*inp, init=None if init is None else (_pad(init[0]), _pad(init[1]), init[2]))
    generic.close()
    glob = m.BatchSolver(m.config_carlike_min_time(N, stage_data=A.STAGE_GLOBAL, **kw), max_batch=B)
    rs = glob.solve(*inp, init=init)
    glob.close()
    return rf, rg, rs


def _assert_equal(rf, rg, rs):
    assert np.array_equal(rf.x, rg.x[:, :N], equal_nan=True) and np.array_equal(rf.u[:, :N - 1], rg.u[:, :N - 1], equal_nan=True), "x / u: fixed layout against the generic kernel"
    assert np.array_equal(rf.x, rs.x, equal_nan=True) and np.array_equal(rf.u[:, :N - 1], rs.u[:, :N - 1], equal_nan=True), "x / u: fixed layout against the global form"
    for f in ("dt", "status", "iters"):
        assert np.array_equal(getattr(rf, f), getattr(rg, f), equal_nan=True), f + ": fixed layout against the generic kernel"
        assert np.array_equal(getattr(rf, f), getattr(rs, f), equal_nan=True), f + ": fixed layout against the global form"


@pytest.mark.parametrize("max_iter", [1, 2, 4, None])
@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_fixed_layout_iterates_equal_generic_and_global_form(m, inputs, four, max_iter):
    rf, rg, rs = _three(m, _kw(four, max_iter), inputs)
    print(f"four {four} max_iter {max_iter}: converged {np.mean(rf.status == 0):.3f}, iterations {rf.iters.min()} .. {rf.iters.max()}")
    _assert_equal(rf, rg, rs)
    if max_iter is None:
        assert np.mean(rf.status == 0) > 0.9      # (two equal failures must not pass)
    else:
        assert np.isfinite(rf.x).all() and not np.array_equal(rf.x[:, 1:-1], np.zeros_like(rf.x[:, 1:-1]))      # an iterate was written


@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_fixed_layout_without_first_rate_rows(m, inputs, four):
    """dt_prev = 0: the rate rows of the first control are off"""
    x0, xf, up, dtp = inputs
    rf, rg, rs = _three(m, _kw(four, None), (x0, xf, up, np.zeros_like(dtp)))
    print(f"dt_prev = 0, four {four}: converged {np.mean(rf.status == 0):.3f}, iterations {rf.iters.min()} .. {rf.iters.max()}")
    _assert_equal(rf, rg, rs)
    assert np.mean(rf.status == 0) > 0.9


@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_fixed_layout_warm_start_from_the_previous_solution(m, inputs, four):
    """the same problems again with the previous solution as the initial guess (an instance without one starts from the straight line)"""
    x0, xf, up, dtp = inputs
    cold = m.BatchSolver(m.config_carlike_min_time(N), max_batch=B)
    prev = cold.solve(x0, xf, up, dtp)
    cold.close()
    ok = prev.status == 0
    assert ok.mean() > 0.9
    x_init = np.where(ok[:, None, None], prev.x, np.linspace(x0, xf, N, axis=1))
    u_init = np.where(ok[:, None, None], prev.u, 0.0)
    dt_init = np.where(ok, prev.dt, 0.3)
    rf, rg, rs = _three(m, _kw(four, None), inputs, init=(x_init, u_init, dt_init))
    print(f"warm start, four {four}: converged {np.mean(rf.status == 0):.3f}, iterations {rf.iters.min()} .. {rf.iters.max()}")
    _assert_equal(rf, rg, rs)
    assert np.mean(rf.status == 0) > 0.9
