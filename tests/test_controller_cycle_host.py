"""CPU tests of the per-instance logic of mpc_controller_step_batch* (mpc_local_planner_amd/csrc/mpc_controller_cycle.hpp), compiled for the host with g++ by a
tests-only harness (tests/host_harness/controller_cycle_host.cpp): the guess a re-initialised slot builds from its plan equals, bit for bit, two independent codes --
oracle.se2_nlp (generate_initial_state_trajectory + initialize_sequences_xinit) and the facade's initial_state_trajectory (include/mpc_controller.hpp) --; the
re-initialisation decision equals a numpy restatement of src/controller.cpp:152-158 on a scripted sequence that hits every cause just above and just below its
threshold; and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs its own cases clean."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from oracle import se2_nlp as R
import _harness

FIRST, NUM_STEPS, GOAL_DIST, GOAL_ANGULAR, RESET = 1, 2, 4, 8, 16      # MPC_REINIT_* of include/mpc_hip.h
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(_harness.shared("controller_cycle_host"))
    lib.cyc_atan2.restype = C.c_double
    lib.cyc_atan2.argtypes = [C.c_double, C.c_double]
    lib.cyc_dt_sample.restype = C.c_double
    lib.cyc_dt_sample.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]
    sig = [C.c_int, dp, dp, dp, C.c_int, C.c_double, C.c_int, C.c_double, dp]
    lib.cyc_plan_guess.argtypes = sig
    lib.cyc_facade_guess.argtypes = sig
    lib.cyc_plan_guess_device_yaw.argtypes = sig
    lib.cyc_decide_sequence.argtypes = [C.c_int, dp, C.POINTER(C.c_int), C.c_int, C.c_double, C.c_double, C.POINTER(C.c_int)]
    lib.cyc_state_estimate.argtypes = [dp, dp, dp, C.c_int, C.c_int, C.c_double, dp]
    return lib


def _ptr(a):
    return a.ctypes.data_as(dp)


def _guess(fn, plan, x0, xf, n_ref, dt_ref, est, dt_sample):
    out = np.full((n_ref, 3), np.nan)
    fn(len(plan), _ptr(plan), _ptr(x0), _ptr(xf), n_ref, dt_ref, int(est), dt_sample, _ptr(out))
    return out


def _plans():
    """random plans of 2..9 poses; every fifth with all headings at +-pi; some with a segment along -x (estimated yaw = pi) or a repeated pose (atan2(0, 0))"""
    rng = np.random.default_rng(20)
    for rep in range(240):
        npo = 2 + rep % 8
        plan = np.ascontiguousarray(np.column_stack([rng.uniform(-2, 2, npo), rng.uniform(-2, 2, npo), rng.uniform(-math.pi, math.pi, npo)]))
        if rep % 5 == 0:
            plan[:, 2] = np.where(np.arange(npo) % 2 == 0, -math.pi, math.pi)
        if rep % 7 == 0 and npo > 3:
            plan[2, :2] = plan[1, :2] + (-0.5, 0.0)
        if rep % 11 == 0 and npo > 4:
            plan[3, :2] = plan[2, :2]
        yield rep, plan


def test_plan_guess_equals_the_oracle_and_the_facade_bit_for_bit(h):
    rng = np.random.default_rng(21)
    checked = 0
    for rep, plan in _plans():
        x0 = plan[0].copy() + (rng.uniform(-0.1, 0.1, 3) if rep % 2 else 0.0)      # the state estimate need not be the plan's first pose (state feedback)
        xf = plan[-1].copy()
        dt_ref = float(rng.uniform(0.1, 0.5))
        for n_ref in (3, 8, 12):
            for dt_sample in (dt_ref, dt_ref * float(rng.uniform(0.4, 1.6))):
                for est in (True, False):
                    mine = _guess(h.cyc_plan_guess, plan, x0, xf, n_ref, dt_ref, est, dt_sample)
                    facade = _guess(h.cyc_facade_guess, plan, x0, xf, n_ref, dt_ref, est, dt_sample)
                    t, v = R.generate_initial_state_trajectory(plan, x0, xf, n_ref, dt_ref, estimate_orientation=est)
                    ocfg = R.config_carlike_min_time(n_ref)
                    ocfg.dt_ref = dt_sample           # initialize_sequences_xinit samples at k * cfg.dt_ref: the spacing of the SAMPLING here
                    oracle = R.initialize_sequences_xinit(ocfg, x0, xf, t, v).x
                    assert mine.tobytes() == facade.tobytes(), (rep, n_ref, dt_sample, est)
                    assert mine.tobytes() == np.ascontiguousarray(oracle, dtype=np.float64).tobytes(), (rep, n_ref, dt_sample, est)
                    checked += 1
    assert checked == 240 * 3 * 2 * 2


def _atan2_exact(y, x):
    import mpmath as mp
    with mp.workprec(200):
        return float(mp.atan2(mp.mpf(y), mp.mpf(x)))


def test_the_devices_atan2_is_correctly_rounded_and_the_hosts_is_the_one_that_is_not(h):
    """The yaw estimate of an intermediate plan pose.  The device build computes it with cc_atan2 (double-double, rounded once); the facade and the oracle call
    the host's libm.  cc_atan2 must be the correctly rounded value (200-bit evaluation) on every argument; where math.atan2 differs from it, math.atan2 is the one
    that is off -- by one ulp, and rarely (glibc 2.35: 0.08 % of such arguments)."""
    rng = np.random.default_rng(22)
    ys = np.concatenate([rng.uniform(-3, 3, 20000), rng.normal(0, 1e-3, 5000), rng.uniform(-3, 3, 5000)])
    xs = np.concatenate([rng.uniform(-3, 3, 20000), rng.uniform(-3, 3, 5000), rng.normal(0, 1e-3, 5000)])
    edge = [(0.0, 0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, 1.0), (0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (1.0, -0.0), (1.0, 1.0), (-1.0, 1.0), (1.0, -1.0),
            (-1.0, -1.0), (0.5, 0.5), (1e-300, 1.0), (1.0, 1e-300), (0.125, 1.0), (0.0625, 1.0), (0.1875, 1.0), (1.0, 0.9375)]
    pairs = list(zip(ys.tolist(), xs.tolist())) + edge
    bits = lambda v: np.float64(v).tobytes()
    wrong, host_off = [], 0
    for y, x in pairs:
        mine, host = h.cyc_atan2(y, x), math.atan2(y, x)
        if bits(mine) == bits(host):
            continue                                   # two independent routines agree (every signed-zero case among them)
        exact = _atan2_exact(y, x)
        if bits(mine) != bits(exact):
            wrong.append((y, x, mine, exact))
        else:
            host_off += 1
            assert abs(host - exact) <= np.spacing(abs(exact)), (y, x)
    print(f"cc_atan2: {len(pairs)} arguments, correctly rounded on all; the host's atan2 is 1 ulp off on {host_off}")
    assert not wrong, wrong[:5]
    assert host_off < len(pairs) // 100
    sample = rng.choice(len(pairs) - len(edge), 3000, replace=False)      # and directly against the 200-bit value where the two agree
    assert all(bits(h.cyc_atan2(*pairs[i])) == bits(_atan2_exact(*pairs[i])) for i in sample)


def test_plan_guess_with_the_devices_yaw_differs_from_the_facade_only_where_the_hosts_atan2_is_off(h):
    rng = np.random.default_rng(24)
    differ = 0
    for rep, plan in _plans():
        x0, xf, dt_ref = plan[0].copy(), plan[-1].copy(), float(rng.uniform(0.1, 0.5))
        dev = _guess(h.cyc_plan_guess_device_yaw, plan, x0, xf, 12, dt_ref, True, dt_ref)
        facade = _guess(h.cyc_facade_guess, plan, x0, xf, 12, dt_ref, True, dt_ref)
        if dev.tobytes() != facade.tobytes():
            differ += 1
            seg = [(plan[i + 1, 1] - plan[i, 1], plan[i + 1, 0] - plan[i, 0]) for i in range(1, len(plan) - 1)]
            assert any(h.cyc_atan2(y, x) != math.atan2(y, x) for y, x in seg), rep
            assert dev[:, :2].tobytes() == facade[:, :2].tobytes() and np.abs(dev[:, 2] - facade[:, 2]).max() < 1e-15, rep
    print(f"plan guess with the device's yaw estimate: {differ} of 240 plans differ from the facade (in a heading, by the host's atan2)")
    assert differ <= 4


def _decide_numpy(goals, reset, num_steps, dist, ang):
    """src/controller.cpp:152-158 with the slot's bookkeeping (:176-177), written from the source: 1 where the grid is cleared"""
    empty, seq, last = True, 0, np.zeros(3)
    out = []
    for g, r in zip(goals, reset):
        if r:
            empty = True                                                      # Controller::reset() -> _grid->clear()
        if num_steps > 0 and seq % num_steps == 0:
            empty = True
        if not empty and (np.sqrt((g[0] - last[0]) * (g[0] - last[0]) + (g[1] - last[1]) * (g[1] - last[1])) > dist
                          or abs(R.normalize_theta(g[2] - last[2])) > ang):
            empty = True
        out.append(int(empty))
        empty, seq, last = False, seq + 1, np.array(g, float)
    return out


def test_reinit_decision_on_a_scripted_sequence_hits_every_cause_at_its_threshold(h):
    up1, q = math.nextafter(1.0, 2.0), 1.5707963267948966
    qup = math.nextafter(q, 2.0)
    # step:   0 first     1 1.0 m      2 back 1.0 m  3 1 m + 1 ulp  4 turn 90 deg  5 back 90 deg  6 90 deg + 1 ulp  7 7th step     8 reset        9 nothing
    goals = [(0, 0, 0), (1.0, 0, 0), (0, 0, 0), (up1, 0, 0), (up1, 0, q), (up1, 0, 0), (up1, 0, qup), (up1, 0, qup), (up1, 0, qup), (up1, 0, qup), (up1, 3.0, qup)]
    reset = [0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    expect = [FIRST | NUM_STEPS, 0, 0, GOAL_DIST, 0, 0, GOAL_ANGULAR, NUM_STEPS, RESET, 0, GOAL_DIST]
    g = np.ascontiguousarray(goals, dtype=np.float64)
    r = (C.c_int * len(reset))(*reset)
    causes = (C.c_int * len(reset))()
    h.cyc_decide_sequence(len(reset), _ptr(g), r, 7, 1.0, q, causes)
    assert list(causes) == expect
    assert [int(c != 0) for c in causes] == _decide_numpy(goals, reset, 7, 1.0, q)
    # a random walk of goals around both thresholds, with resets: the same decisions as the restatement, step by step
    rng = np.random.default_rng(23)
    T = 400
    g = np.cumsum(np.column_stack([rng.choice([0.0, 0.6, 1.0, up1, 1.4], T), rng.choice([0.0, 0.0, 0.3], T), rng.choice([0.0, q, -q, qup, 3.0, 0.2], T)]), axis=0)
    rs = (rng.uniform(size=T) < 0.05).astype(np.int32)
    for num_steps in (0, 7):
        causes = (C.c_int * T)()
        h.cyc_decide_sequence(T, _ptr(np.ascontiguousarray(g)), (C.c_int * T)(*rs.tolist()), num_steps, 1.0, q, causes)
        assert [int(c != 0) for c in causes] == _decide_numpy(g.tolist(), rs.tolist(), num_steps, 1.0, q)
        assert all(bool(c & RESET) == bool(r) for c, r in zip(causes, rs))


def test_state_estimate_and_sampling_spacing(h):
    plan0 = np.array([1.0, 2.0, 0.5])
    fb = np.array([[9.0, 9.0, 9.0], [1.5, 2.5, 0.25]])
    x0 = np.zeros(3)
    for age, prefer, use in ((0.19, 1, True), (0.2, 1, False), (0.05, 0, False), (0.3, 1, False)):      # fresh means younger than 2 periods (src/controller.cpp:137)
        h.cyc_state_estimate(_ptr(plan0), _ptr(fb), _ptr(np.array([7.0, age])), 1, prefer, 0.1, _ptr(x0))
        assert x0.tolist() == (fb[1] if use else plan0).tolist(), (age, prefer)
    h.cyc_state_estimate(_ptr(plan0), None, None, 0, 1, 0.1, _ptr(x0))
    assert x0.tolist() == plan0.tolist()
    # the last optimised dt only with reference sampling, a solution, the variable grid and dt > 0 (include/mpc_controller.hpp, Controller::step)
    assert h.cyc_dt_sample(1, 1, 1, 0.21, 0.3) == 0.21
    for args in ((0, 1, 1, 0.21), (1, 0, 1, 0.21), (1, 1, 0, 0.21), (1, 1, 1, 0.0), (1, 1, 1, -1.0)):
        assert h.cyc_dt_sample(*args, 0.3) == 0.3, args


def test_cycle_params_reader_fills_the_struct_from_the_reference_keys():
    from mpc_local_planner_amd import params
    p = params.cycle_params_from_dict({"controller": {"outer_ocp_iterations": 2, "force_reinit_num_steps": 7, "force_reinit_new_goal_dist": 0.8, "prefer_x_feedback": True},
                                       "grid": {"grid_size_ref": 8, "warm_start": False,
                                                "variable_grid": {"enable": True, "grid_adaptation": {"enable": True, "max_grid_size": 12, "min_grid_size": 4, "dt_hyst_ratio": 0.2}}}},
                                      period=0.2)
    assert (p.n_ref, p.outer_iterations, p.adapt, p.n_min, p.n_max, p.dt_hyst_ratio) == (8, 2, 1, 4, 12, 0.2)
    assert (p.warm_start, p.force_reinit_num_steps, p.force_reinit_new_goal_dist, p.prefer_x_feedback, p.period) == (0, 7, 0.8, 1, 0.2)
    d = params.cycle_params_from_dict({})
    assert (d.n_ref, d.outer_iterations, d.adapt, d.n_min, d.n_max, d.dt_hyst_ratio, d.warm_start, d.force_reinit_num_steps) == (20, 1, 1, 2, 50, 0.1, 1, 0)
    assert params.cycle_params_from_dict({"grid": {"variable_grid": {"enable": False}}}).adapt == 0
    assert (d.force_reinit_new_goal_dist, d.force_reinit_new_goal_angular, d.initial_plan_estimate_orientation, d.prefer_x_feedback, d.reference_reinit_sampling, d.period) == \
        (1.0, 0.5 * math.pi, 1, 0, 1, 0.1)


def test_harness_runs_clean_under_address_and_undefined_sanitizers():
    """the stand-alone program (own main, own sampling and decision cases) built with -fsanitize=address,undefined; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("controller_cycle_host", ("CYC_MAIN",))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "410 cases, 0 differ" in r.stdout and "runtime error" not in r.stderr
