"""GPU tests (-m gpu) of parameter sets (mpc_set_parameter_sets): one handle solves instances with different double parameters of mpc_config in one launch,
and instance b returns, bit for bit, what a handle created with its set returns for the same inputs.  Every case gives K = 4 sets to B = 256 instances
interleaved (set_of[b] = b % 4) and solves each set's instances again on a handle of their own; at least one set has to change the answers of the
handle's own configuration, so that a table the kernel ignores cannot pass."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K, B = 4, 256
OFFDIAG_Q = ((2.0, 0.3, 0.1), (0.3, 2.0, 0.0), (0.0, 0.0, 0.25))
RECT = ((0.35, 0.2), (-0.25, 0.2), (-0.25, -0.2), (0.35, -0.2))


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as pkg
    return pkg


def _sliced(inputs, idx):
    return tuple(None if a is None else (_sliced(a, idx) if isinstance(a, tuple) else np.ascontiguousarray(a[idx])) for a in inputs)


def _solve(inputs, candidates=False):
    """run(solver, idx): one cold solve of the instances idx"""
    def run(s, idx):
        x0, xf, up, dtp = _sliced(inputs[:4], idx)
        ob = _sliced(inputs[4], idx) if len(inputs) > 4 else None
        r = s.solve(x0, xf, up, dtp, obstacles=ob)
        out = dict(x=r.x, u=r.u, dt=r.dt, status=r.status, iters=r.iters)
        if candidates:
            out["winner"] = s.last_candidates(len(idx))[0]
        return out
    return run


def _carlike_sets(c, k):
    """speed limit, wheelbase and rate limits of robot k"""
    c.model_params[0] = 0.3 + 0.07 * k
    c.u_ub[0] = 0.45 - 0.05 * k
    for j in range(2):
        c.du_lb[j], c.du_ub[j] = -(0.6 - 0.1 * k), 0.6 - 0.1 * k
    return c


def _check(m, make, vary, run, K=K, B=B):
    cfg = make()
    sets = [vary(make(), k) for k in range(K)]
    set_of = (np.arange(B) % K).astype(np.int32)
    own = m.BatchSolver(cfg, max_batch=B)
    uni = run(own, np.arange(B))                 # the handle's own configuration for every instance
    own.close()
    big = m.BatchSolver(cfg, max_batch=B)
    big.set_parameter_sets(sets, set_of)
    got = run(big, np.arange(B))
    big.close()
    differs = 0
    for k in range(K):
        idx = np.nonzero(set_of == k)[0]
        sep = m.BatchSolver(sets[k], max_batch=len(idx))
        ref = run(sep, idx)
        sep.close()
        for key, v in ref.items():
            assert np.array_equal(got[key][idx], v), (k, key, np.nonzero(~np.all((got[key][idx] == v).reshape(len(idx), -1), 1))[0][:8])
        differs += int(not (np.array_equal(uni["x"][idx], got["x"][idx]) and np.array_equal(uni["dt"][idx], got["dt"][idx])))
    assert differs > 0, "no set changed the answers of the handle's own configuration"
    return got


def test_config2_fixed_layout(m):
    _check(m, lambda: m.config_carlike_min_time(50), _carlike_sets, _solve(m.workloads.carlike_min_time_inputs(B)))


def test_two_waves_per_simd(m):
    got = _check(m, lambda: m.config_carlike_min_time(20, two_wave_min_batch=64), _carlike_sets, _solve(m.workloads.carlike_min_time_inputs(B, goal_range=(1.0, 3.0))))
    assert (got["status"] == 0).mean() > 0.5


def test_global_form(m):
    from mpc_local_planner_amd import _abi as A
    _check(m, lambda: m.config_carlike_min_time(50, stage_data=A.STAGE_GLOBAL), _carlike_sets, _solve(m.workloads.carlike_min_time_inputs(B)))


def test_circle_footprint_with_point_obstacles(m):
    x0, xf, up, dtp, ob = m.workloads.carlike_moving_obstacle_inputs(B)

    def vary(c, k):
        c.footprint_radius = 0.1 + 0.06 * k
        c.min_obstacle_dist = 0.25 + 0.1 * k
        return _carlike_sets(c, k)
    _check(m, lambda: m.config_carlike_min_time(30, footprint_kind=1, footprint_radius=0.2, max_obstacles=3, max_vertices=1, max_obstacle_rows=4), vary,
           _solve((x0, xf, up, dtp, ob[:4])))


def test_polygon_footprint_level_1(m):
    x0, xf, up, dtp, ob = m.workloads.carlike_moving_obstacle_inputs(B, seed=953)

    def vary(c, k):
        for i in range(8):
            c.footprint_vertices[i] *= 0.7 + 0.2 * k
        c.min_obstacle_dist = 0.2 + 0.05 * k
        return c
    _check(m, lambda: m.config_carlike_min_time(30, footprint_kind=4, footprint_vertices=RECT, max_obstacles=3, max_vertices=1, max_obstacle_rows=4), vary,
           _solve((x0, xf, up, dtp, ob[:4])))


def test_offdiagonal_weights_and_terminal_ball_level_2(m):
    def vary(c, k):
        c.Q_offdiag[0] = 0.1 + 0.25 * k
        c.R_offdiag = 0.01 * (k + 1)
        c.terminal_ball_gamma = 0.05 + 0.3 * k
        return c
    _check(m, lambda: m.config_unicycle_quadratic(20, Q=OFFDIAG_Q, terminal_ball_S=(1.0, 1.0, 0.1), terminal_ball_gamma=0.5), vary,
           _solve(m.workloads.unicycle_quadratic_inputs(B)))


def test_fp32(m):
    from mpc_local_planner_amd import _abi as A
    _check(m, lambda: m.config_carlike_min_time(50, precision=A.FP32, tol=1e-4), _carlike_sets, _solve(m.workloads.carlike_min_time_inputs(B)))


def test_mixed_precision(m):
    from mpc_local_planner_amd import _abi as A

    def vary(c, k):
        c.tol = 1e-8 * (1 + k)
        return _carlike_sets(c, k)
    _check(m, lambda: m.config_carlike_min_time(50, precision=A.MIXED), vary, _solve(m.workloads.carlike_min_time_inputs(B)))


def test_hedged_candidates(m):
    from mpc_local_planner_amd import _abi as A
    cands = dict(candidates=(A.CAND_REFERENCE, A.CAND_HERMITE_FF, A.CAND_HERMITE_FR), candidate_max_iter=(40, 40, 40), candidate_param=(0.0, 2.0, 1.5))

    def vary(c, k):
        c.candidate_param[1] = 1.0 + 0.5 * k
        c.candidate_param[2] = 1.5 + 0.25 * k
        return _carlike_sets(c, k)
    got = _check(m, lambda: m.config_carlike_min_time(30, **cands), vary, _solve(m.workloads.carlike_min_time_inputs(B), candidates=True))
    assert (got["winner"] > 0).any()


def test_two_cycles_with_kept_multipliers_and_the_fixed_grid_shift(m):
    import torch
    dev = torch.device("cuda", 0)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x0, xf, up, dtp = m.workloads.unicycle_quadratic_inputs(B, seed=962)

    def run(s, idx):
        a0, af, au, ad = _sliced((x0, xf, up, dtp), idx)
        r1 = s.solve(a0, af, au, ad)
        x0n = r1.x[:, 2].copy()                                  # the robot advanced two grid intervals along its plan
        dx, du, dd, d0 = T(r1.x), T(r1.u), T(r1.dt), T(x0n)
        s.grid_update_device(len(idx), d0.data_ptr(), dx.data_ptr(), du.data_ptr(), dd.data_ptr())
        s.synchronize()
        r2 = s.solve(x0n, af, r1.u[:, 0], ad, init=(dx.cpu().numpy(), du.cpu().numpy(), dd.cpu().numpy()))
        return dict(x1=r1.x, dt1=r1.dt, st1=r1.status, it1=r1.iters, x=r2.x, u=r2.u, dt=r2.dt, status=r2.status, iters=r2.iters)

    def vary(c, k):
        c.Q[0] = c.Q[1] = 1.0 + 0.5 * k
        c.u_ub[0] = 0.3 + 0.05 * k
        c.mu_init_dual = 1e-3 * (1 + k)
        return c
    _check(m, lambda: m.config_unicycle_quadratic(20, dual_warm_start=True, mu_init_dual=1e-3, mu_init_warm=1e-2), vary, run)


def test_step_batch_with_grid_adaptation_against_each_dt_ref(m):
    x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(B)

    def run(s, idx):
        s.set_grid_sizes([40] * len(idx))
        r, ng = s.step(*_sliced((x0, xf, up, dtp), idx), outer_iterations=3, adapt=True, n_min=3, n_max=50, dt_hyst_ratio=0.1)
        return dict(x=r.x, u=r.u, dt=r.dt, status=r.status, iters=r.iters, n_grid=ng)

    def vary(c, k):
        c.dt_ref = 0.15 + 0.1 * k
        return _carlike_sets(c, k)
    got = _check(m, lambda: m.config_carlike_min_time(50), vary, run)
    assert len(np.unique(got["n_grid"])) > 1


def test_sets_equal_to_the_handle_change_nothing_and_clearing_restores_the_handle(m):
    inputs = m.workloads.carlike_min_time_inputs(B)
    cfg = m.config_carlike_min_time(50)
    s = m.BatchSolver(cfg, max_batch=B)
    r0 = s.solve(*inputs)
    s.set_parameter_sets([m.config_carlike_min_time(50) for _ in range(16)], np.random.default_rng(5).integers(0, 16, B))
    r1 = s.solve(*inputs)
    s.set_parameter_sets([_carlike_sets(m.config_carlike_min_time(50), k) for k in range(K)], np.arange(B) % K)
    r2 = s.solve(*inputs)
    s.set_parameter_sets(None)
    r3 = s.solve(*inputs)
    s.close()
    for key in ("x", "u", "dt", "status", "iters"):
        assert getattr(r0, key).tobytes() == getattr(r1, key).tobytes(), key
        assert getattr(r0, key).tobytes() == getattr(r3, key).tobytes(), key
    assert not np.array_equal(r0.x, r2.x)


def test_refusals_through_the_abi_keep_the_sets_in_force(m):
    from mpc_local_planner_amd import _abi as A
    Bs = 64
    inputs = m.workloads.carlike_min_time_inputs(Bs)
    s = m.BatchSolver(m.config_carlike_min_time(50), max_batch=Bs)
    sets = [_carlike_sets(m.config_carlike_min_time(50), k) for k in range(2)]
    s.set_parameter_sets(sets, np.arange(Bs) % 2)
    r0 = s.solve(*inputs)
    lib, h = s._lib, s._h

    def call(cfgs, set_of, n_sets=None, B_=None):
        arr = (A.MpcConfig * max(1, len(cfgs)))(*cfgs)
        so = np.ascontiguousarray(set_of, dtype=np.int32)
        rc = lib.mpc_set_parameter_sets(h, len(cfgs) if n_sets is None else n_sets, C.cast(arr, C.c_void_p), len(so) if B_ is None else B_, C.c_void_p(so.ctypes.data))
        return rc, lib.mpc_last_error().decode()

    bad_n = m.config_carlike_min_time(60)
    rc, msg = call([sets[0], bad_n], np.zeros(Bs))
    assert rc == A.MPC_EINVAL and msg == "mpc_set_parameter_sets: set 1: n is 60 here and 50 in the handle's configuration", msg
    inf_rate = m.config_carlike_min_time(50, du_ub=(0.5, A.INF))
    rc, msg = call([inf_rate], np.zeros(Bs))
    assert rc == A.MPC_EINVAL and msg == "mpc_set_parameter_sets: set 0: du_ub[1] is infinite here and finite in the handle's configuration", msg
    rc, msg = call(sets, np.arange(Bs) % 3)
    assert rc == A.MPC_EINVAL and "set_of[2] = 2" in msg, msg
    rc, _ = call(sets, np.zeros(Bs + 1))
    assert rc == A.MPC_EBATCH
    rc, _ = call(sets, np.zeros(Bs), n_sets=Bs + 1)
    assert rc == A.MPC_EBATCH
    rc, _ = call(sets, np.zeros(Bs), B_=0)
    assert rc == A.MPC_EBATCH
    r1 = s.solve(*inputs)                        # the sets of the accepted call are still in force
    for key in ("x", "u", "dt", "status", "iters"):
        assert getattr(r0, key).tobytes() == getattr(r1, key).tobytes(), key
    # a solve or grid update of more instances than the last accepted call gave sets for
    s.set_parameter_sets(sets, np.arange(Bs // 2) % 2)
    with pytest.raises(m.MpcError) as e:
        s.solve(*inputs)
    assert e.value.code == A.MPC_EBATCH
    rh = s.solve(*_sliced(inputs, np.arange(Bs // 2)))
    assert np.array_equal(rh.x, r0.x[:Bs // 2])
    s.reset()                                    # mpc_reset keeps the sets
    assert np.array_equal(s.solve(*_sliced(inputs, np.arange(Bs // 2))).x, r0.x[:Bs // 2])
    s.close()
