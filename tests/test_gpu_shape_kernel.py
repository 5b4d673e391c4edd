"""GPU tests (-m gpu) of the shape-known fixed-layout kernel (IpmWave's SHAPE, mpc_core.hpp::kHeadlineShape): for a handle whose shape word -- fixed goal components,
dt free, objective, terminal cost, rate rows -- is the headline's, the fp64 kernel for records of 50 grid points has that word compiled in, and the (dt, nu) root system
in its shape-known form (riccati_root_shape).  It removes tests and selects, no floating-point operation, so it must agree BIT FOR BIT in x, u, dt, status and iteration
count with the fixed-layout kernel that reads the word at run time (the same handle behind the developer switch mpc_debug_use_shape_kernel) and with the generic-layout
kernel (a handle created for n = 51 with every grid size set to 50): after 1, 2 and 4 iterations and after the full solve, with one candidate and the headline's four,
with dt_prev = 0 (the first rate rows are off at run time), from a warm start, and on a ragged launch (grid sizes 40, 43 and 50: the smallest grid the partitioned sweeps
run on, their leftovers, the full record).  Handles one bit away from the shape must NOT get the kernel and must equal the generic-layout kernel bit for bit.  Which
kernel a launch runs is read from the launch plan (mpc_debug_kernel_shape, which asks plan_launch as the launch and mpc_occupancy do).  64 instances of the bench's seed."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N = 64, 50
SHAPE = 0x103cf      # mpc_core.hpp::kHeadlineShape: bits 0..2 goal fixed, 3 dt free, 6..9 rate rows, 16 minimum time
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
    """an initial guess of 50 grid points for the handle created with 51: the last point once more (never read: no grid size is above 50)"""
    return np.concatenate([a, a[:, -1:]], axis=1)


def _plan(s, batch=B):
    """(the handle's shape word, the shape word compiled into the kernel a launch of `batch` instances runs; 0 = read at run time)"""
    fn = s._lib.mpc_debug_kernel_shape
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    f, k = C.c_int32(-1), C.c_int32(-1)
    assert fn(s._h, batch, C.byref(f), C.byref(k)) == 0
    return f.value, k.value


def _use_shape_kernel(s, on):
    fn = s._lib.mpc_debug_use_shape_kernel
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert fn(s._h, int(on)) == 0


def _three(m, kw, inp, init=None, grid=None):
    """the same batch through the shape-known kernel, the run-time-flags fixed-layout kernel and the generic-layout kernel, each asserted to be the one the plan runs"""
    ng = np.full(B, N, dtype=np.int32) if grid is None else grid
    s = m.BatchSolver(m.config_carlike_min_time(N, **kw), max_batch=B)
    if grid is not None: s.set_grid_sizes(ng)
    assert _plan(s) == (SHAPE, SHAPE) and s.occupancy(B) == (4, 40128)      # one wave per SIMD, four workgroups per CU, the record as it was
    rk = s.solve(*inp, init=init)
    _use_shape_kernel(s, False)
    assert _plan(s) == (SHAPE, 0) and s.occupancy(B) == (4, 40128)
    rf = s.solve(*inp, init=init)
    _use_shape_kernel(s, True)
    assert _plan(s) == (SHAPE, SHAPE)
    s.close()
    g = m.BatchSolver(m.config_carlike_min_time(N + 1, **kw), max_batch=B)
    g.set_grid_sizes(ng)
    assert _plan(g) == (SHAPE, 0)
    rg = g.solve(*inp, init=None if init is None else (_pad(init[0]), _pad(init[1]), init[2]))
    g.close()
    return rk, rf, rg


def _assert_equal(rk, rf, rg, what=("run-time-flags fixed-layout kernel", "generic-layout kernel")):
    for r, name in ((rf, what[0]), (rg, what[1])):
        if r is None: continue
        assert np.array_equal(rk.x[:, :N], r.x[:, :N], equal_nan=True) and np.array_equal(rk.u[:, :N - 1], r.u[:, :N - 1], equal_nan=True), "x / u against the " + name
        for f in ("dt", "status", "iters"):
            assert np.array_equal(getattr(rk, f), getattr(r, f), equal_nan=True), f + " against the " + name


@pytest.mark.parametrize("max_iter", [1, 2, 4, None])
@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_shape_kernel_iterates_equal_run_time_flags_and_generic_layout(m, inputs, four, max_iter):
    rk, rf, rg = _three(m, _kw(four, max_iter), inputs)
    print(f"four {four} max_iter {max_iter}: converged {np.mean(rk.status == 0):.3f}, iterations {rk.iters.min()} .. {rk.iters.max()}")
    _assert_equal(rk, rf, rg)
    if max_iter is None:
        assert np.mean(rk.status == 0) > 0.9      # (two equal failures must not pass)
    else:
        assert np.isfinite(rk.x).all() and not np.array_equal(rk.x[:, 1:-1], np.zeros_like(rk.x[:, 1:-1]))      # an iterate was written


@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_shape_kernel_without_first_rate_rows(m, inputs, four):
    """dt_prev = 0: the rate rows of the first control are off at run time (row0_on), whatever the shape says about the slots"""
    x0, xf, up, dtp = inputs
    rk, rf, rg = _three(m, _kw(four, None), (x0, xf, up, np.zeros_like(dtp)))
    print(f"dt_prev = 0, four {four}: converged {np.mean(rk.status == 0):.3f}, iterations {rk.iters.min()} .. {rk.iters.max()}")
    _assert_equal(rk, rf, rg)
    assert np.mean(rk.status == 0) > 0.9


@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_shape_kernel_warm_start_from_the_previous_solution(m, inputs, four):
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
    rk, rf, rg = _three(m, _kw(four, None), inputs, init=(x_init, u_init, dt_init))
    print(f"warm start, four {four}: converged {np.mean(rk.status == 0):.3f}, iterations {rk.iters.min()} .. {rk.iters.max()}")
    _assert_equal(rk, rf, rg)
    assert np.mean(rk.status == 0) > 0.9


@pytest.mark.parametrize("four", [False, True], ids=["one_candidate", "four_candidates"])
def test_shape_kernel_ragged_launch(m, inputs, four):
    """grid sizes 40, 43 and 50 in one launch.  (The outputs behind an instance's last grid point repeat that point in every kernel: compared as well.)"""
    grid = np.array([40, 43, 50], dtype=np.int32)[np.arange(B) % 3]
    rk, rf, rg = _three(m, _kw(four, None), inputs, grid=grid)
    print(f"ragged, four {four}: converged {np.mean(rk.status == 0):.3f}, iterations {rk.iters.min()} .. {rk.iters.max()}")
    _assert_equal(rk, rf, rg)
    assert np.mean(rk.status == 0) > 0.9


def _one_bit_away():
    from mpc_local_planner_amd import _abi as A
    return {
        "goal_heading_free": (dict(xf_fixed=(True, True, False)), SHAPE & ~4),
        "quadratic_objective": (dict(objective=A.OBJ_QUADRATIC, Q=(2.0, 2.0, 0.25), R=(0.1, 0.05)), (SHAPE | 16) & ~0x10000),      # (the objective is two bits of the word)
        "has_Qf": (dict(Qf=(10.0, 10.0, 0.5)), SHAPE | 32),
        "rate_row_off": (dict(du_lb=(-1e30, -0.5)), SHAPE & ~64),
    }


@pytest.mark.parametrize("case", ["goal_heading_free", "quadratic_objective", "has_Qf", "rate_row_off"])
def test_other_shapes_keep_the_run_time_flags_kernel(m, inputs, case):
    """a handle at n = 50 whose word differs from the shape: the plan keeps it on the run-time-flags fixed-layout kernel, and it equals the generic-layout kernel"""
    kw, word = _one_bit_away()[case]
    s = m.BatchSolver(m.config_carlike_min_time(N, **kw), max_batch=B)
    assert _plan(s) == (word, 0) and word != SHAPE
    _use_shape_kernel(s, True)                     # (the switch gives back the plan's own decision, nothing more)
    assert _plan(s) == (word, 0)
    rf = s.solve(*inputs)
    s.close()
    g = m.BatchSolver(m.config_carlike_min_time(N + 1, **kw), max_batch=B)
    g.set_grid_sizes(np.full(B, N, dtype=np.int32))
    assert _plan(g) == (word, 0)
    rg = g.solve(*inputs)
    g.close()
    print(f"{case}: converged {np.mean(rf.status == 0):.3f}, iterations {rf.iters.min()} .. {rf.iters.max()}")
    _assert_equal(rf, None, rg)
    assert np.isfinite(rf.x).all() and rf.iters.max() > 1      # it ran


def test_plan_gives_the_shape_kernel_to_the_fixed_layout_alone(m):
    """the headline shape on any other record (n = 49, n = 51, the global form, fp32) runs a kernel that reads the word at run time"""
    from mpc_local_planner_amd import _abi as A
    for kw in (dict(n=49), dict(n=51), dict(n=N, stage_data=A.STAGE_GLOBAL), dict(n=N, precision=A.FP32, tol=1e-4)):
        s = m.BatchSolver(m.config_carlike_min_time(**kw), max_batch=B)
        assert _plan(s) == (SHAPE, 0), kw
        s.close()
    s = m.BatchSolver(m.config_bicycle_min_time(N), max_batch=B)      # another model with the same word: its own shape-known kernel
    assert _plan(s) == (SHAPE, SHAPE)
    s.close()
