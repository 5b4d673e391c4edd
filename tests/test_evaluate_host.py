"""CPU tests of the trajectory evaluation (mpc_evaluate_batch*, mpc_local_planner_amd/csrc/mpc_evaluate.hpp): its __host__ __device__ arithmetic, compiled for the host
with g++ by a tests-only harness (tests/host_harness/evaluate_host.cpp) and driven one lane at a time, is held to the untouched oracle (oracle/se2_nlp.py:
ReferenceNlp and footprint_distance) on random, non-optimal trajectories -- tests/_evaluate_cases.py has the case list, the reference and the measured bounds --; per-instance
parameter sets and the scope of a NaN behave as the header says; the harness, built as a stand-alone program with -fsanitize=address,undefined, runs clean; and the two
new entry points are declared, exported and bound."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _evaluate_cases as E
import _harness
from mpc_local_planner_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "mpc_local_planner_amd", "csrc")


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(_harness.shared("evaluate_host"))
    lib.evh_evaluate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.POINTER(A.MpcObstacles), C.c_void_p, C.c_void_p, C.POINTER(A.MpcEvalOut)]
    lib.evh_evaluate.restype = C.c_int
    return lib


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host_evaluate(h, case, sets=None, set_of=None, x0_given=True):
    B = case.B
    out = {k: np.full(B, -7.0) for k in E.OUTPUTS}
    out["closest"] = np.full((B, 2), -7, np.int32)
    eo = A.MpcEvalOut(*(out[k].ctypes.data for k in E.OUTPUTS + ("closest",)))
    ob = None
    if case.obstacles is not None:
        arrs = [np.ascontiguousarray(a) if a is not None else None for a in case.obstacles]
        ob = A.MpcObstacles(*(a.ctypes.data if a is not None else None for a in arrs))
    cfgs = (A.MpcConfig * len(sets))(*sets) if sets else (A.MpcConfig * 1)(case.cfg)
    so = np.ascontiguousarray(set_of, np.int32) if set_of is not None else None
    nvia, via = (np.ascontiguousarray(case.via[0]), np.ascontiguousarray(case.via[1])) if case.via is not None else (None, None)
    rc = h.evh_evaluate(C.cast(cfgs, C.c_void_p), len(cfgs), _p(so), B, _p(case.n_grid), _p(case.x0) if x0_given else None, _p(case.xf) if x0_given else None, _p(case.u_prev),
                        _p(case.dt_prev), _p(case.x), _p(case.u), _p(case.dt), C.byref(ob) if ob is not None else None, _p(nvia), _p(via), C.byref(eo))
    assert rc == 0
    return out


@pytest.fixture(scope="module")
def measured(h):
    """every case of the list once: (case, host result, reference)"""
    return [(c, host_evaluate(h, c), E.reference(c)) for c in E.host_cases()]


def _has_empty_slot(c):
    """an obstacle slot below n_obstacles[b] with n_vertices = 0 (and NaN data behind it)"""
    no, nv = c.obstacles[0], c.obstacles[1]
    return any(nv[b, o] == 0 and np.isnan(c.obstacles[2][b, o]).all() for b in range(c.B) for o in range(int(no[b])))


def test_case_list_covers_what_it_claims():
    cases = E.host_cases()
    cf = [c.cfg for c in cases]
    assert {(c.model, c.collocation) for c in cf} >= {(m, k) for m in range(4) for k in range(3)}
    assert {(c.objective, c.integral_form, c.cost_integration, c.dt_free) for c in cf} >= {(0, 0, 0, 1), (2, 0, 0, 1), (1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 0, 0, 1), (1, 1, 0, 1), (1, 1, 1, 1)}
    assert any(c.hybrid_cost_minimum_time for c in cf) and any(c.Q_offdiag[0] != 0 and c.R_offdiag != 0 and c.Qf_offdiag[0] != 0 for c in cf)
    assert any(c.terminal_ball and all(c.xf_fixed) for c in cf) and any(c.has_Qf and all(c.xf_fixed) for c in cf)      # edges that a completely fixed goal drops
    assert any(c.terminal_ball and c.terminal_ball_gamma > 100 for c in cf) and any(c.terminal_ball and c.terminal_ball_gamma < 1 and c.terminal_ball_S_offdiag[0] != 0 for c in cf)
    assert {tuple(c.xf_fixed) for c in cf} >= {(1, 1, 1), (0, 0, 0), (1, 0, 1), (1, 1, 0), (0, 0, 1)}
    assert {(c.via_points_ordered, c.vp_orientation_weight > 0) for c in cf if c.objective == 2} == {(0, False), (0, True), (1, False), (1, True)}
    assert {(c.footprint_kind, c.enable_dynamic_obstacles) for c in cf if c.max_obstacles} == {(k, d) for k in range(5) for d in (0, 1)}
    for c in cases:
        assert {3, 4, int(c.cfg.n)} <= set(int(v) for v in c.n_grid)
        assert (c.dt_prev == 0).any() and (c.dt_prev != 0).any()
        if c.obstacles is not None:
            no, nv, _, rad, _ = c.obstacles
            kinds = {(int(nv[b, o]), bool(rad[b, o] > 0)) for b in range(c.B) for o in range(int(no[b]))}
            assert kinds >= {(1, False), (1, True), (2, False)} and any(k[0] >= 3 for k in kinds) and (no == 0).any()
            assert _has_empty_slot(c)


def test_device_case_list_covers_the_shapes():
    """(no GPU needed: the list tests/test_gpu_evaluate.py runs on the device)"""
    CASES = E.device_cases()
    assert {int(c.cfg.n) for c in CASES} >= {3, 4, 63, 64, 65, 129} and {c.B for c in CASES} == {1, 37}
    ob = [c for c in CASES if c.obstacles is not None]
    assert {(int(c.cfg.max_obstacles), int(c.cfg.max_vertices)) for c in ob} >= {(1, 1), (16, 1), (16, 2), (16, 8), (1, 8)}
    assert {(c.obstacles[3] is None, c.obstacles[4] is None) for c in ob} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {(int(c.cfg.footprint_kind), int(c.cfg.enable_dynamic_obstacles)) for c in ob} >= {(k, d) for k in range(5) for d in (0, 1) if (k, d) != (1, 0)} | {(1, 0)}
    assert any((c.obstacles[0] == 0).any() for c in ob)
    for c in CASES:
        if c.B > 1:
            assert {3, int(c.cfg.n)} <= set(int(v) for v in c.n_grid)
            assert np.isnan(c.x[c.n_grid < c.cfg.n]).any() or int(c.cfg.n) == 3
    assert any(_has_empty_slot(c) for c in ob)


def test_host_build_equals_the_oracle_on_random_trajectories(measured):
    """every instance of every case, all four numbers within the measured bound, the arg-min of the clearance equal; the residuals are far from zero (non-optimal
    trajectories), so nothing passes by being small"""
    worst = {k: 0.0 for k in E.OUTPUTS}
    for case, got, ref in measured:
        assert np.isfinite(got["objective"]).all() and np.isfinite(got["eq_violation"]).all() and np.isfinite(got["ineq_violation"]).all(), case.name      # NaN rows beyond n_b: never read
        assert (ref["eq_violation"] > 1e-2).all(), case.name
        for k in E.OUTPUTS:
            d = E.deviation(got[k], ref[k])
            worst[k] = max(worst[k], d)
            assert d <= E.TOL_HOST[k], (case.name, k, d)
        assert np.array_equal(got["closest"], ref["closest"]), case.name
        if case.obstacles is not None:
            none = case.obstacles[0] == 0
            assert np.isposinf(got["clearance"][none]).all() and (got["closest"][none] == -1).all() and np.isfinite(got["clearance"][~none | (case.n_grid < 3)]).all()
        else:
            assert np.isposinf(got["clearance"]).all() and (got["closest"] == -1).all()
    print("[evaluate, host build against the oracle] worst deviation per output: " + ", ".join(f"{k} {v:.3e} (bound {E.measured_bound(v):.3e})" for k, v in worst.items()))
    for k in E.OUTPUTS:
        assert E.TOL_HOST[k] <= 1e-10 and E.TOL_HOST[k] <= 4.0 * max(E.measured_bound(worst[k]), 2.0 ** -52), (k, worst[k])      # the constants are the measured ones, not looser


def test_violations_and_objective_are_exact_where_nothing_rounds(measured):
    by = {c.name: (c, g, r) for c, g, r in measured}
    c, g, r = by["ball_inside"]
    assert (g["ineq_violation"] == 0.0).all() and (r["ineq_violation"] == 0.0).all()
    c, g, r = by["ball_outside"]
    assert (g["ineq_violation"] > 0.1).all()
    c, g, r = by["model1_colloc0"]
    assert np.array_equal(g["objective"], (c.n_grid - 1) * c.dt)      # minimum time: (n_b - 1) dt, one multiplication


def test_null_x0_and_xf_take_the_trajectory_s_own_ends(h):
    case = E.host_cases()[1]
    own = E.Case(**{**case.__dict__, "x0": np.ascontiguousarray(case.x[:, 0]), "xf": np.ascontiguousarray(case.x[np.arange(case.B), case.n_grid - 1])})
    a, b = host_evaluate(h, own), host_evaluate(h, case, x0_given=False)
    for k in E.OUTPUTS + ("closest",):
        assert np.array_equal(a[k], b[k]), k


def test_parameter_sets_apply_per_instance(h):
    """instance b evaluated with sets[set_of[b]] equals, bit for bit, the evaluation under that set alone"""
    case = next(c for c in E.host_cases() if c.name == "quad_offdiag")
    other = A.MpcConfig.from_buffer_copy(case.cfg)
    other.Q[0] = 3.5; other.R[1] = 0.4; other.Qf_offdiag[0] = -0.5; other.u_ub[0] = 0.1; other.du_ub[0] = 0.2; other.du_ub[1] = 0.1; other.du_lb[0] = -0.3; other.du_lb[1] = -0.2; other.dt_ub = 0.3; other.model_params[0] = 0.7
    set_of = np.arange(case.B) % 2
    mixed = host_evaluate(h, case, sets=[case.cfg, other], set_of=set_of)
    alone = [host_evaluate(h, case), host_evaluate(h, case, sets=[other])]
    for k in E.OUTPUTS:
        want = np.where(set_of == 0, alone[0][k], alone[1][k])
        assert np.array_equal(mixed[k], want), k
        if k in ("objective", "ineq_violation"):
            assert (alone[0][k] != alone[1][k]).all()
    ref = E.reference(case, cfg_of=lambda b: (case.cfg, other)[set_of[b]])
    for k in E.OUTPUTS:
        assert E.deviation(mixed[k], ref[k]) <= E.TOL_HOST[k], k


def test_a_nan_gives_nan_outputs_for_its_instance_only(h):
    case = next(c for c in E.host_cases() if c.name == "footprint_line_dyn1")
    clean = host_evaluate(h, case)
    bad = E.Case(**{**case.__dict__, "x": case.x.copy(), "u": case.u.copy(), "dt": case.dt.copy()})
    bad.x[0, 5, 1] = np.nan; bad.u[3, 2, 0] = np.inf; bad.dt[4] = np.nan
    got = host_evaluate(h, bad)
    hit = np.array([True, False, False, True, True])
    for k in E.OUTPUTS:
        assert np.isnan(got[k][hit]).all() and np.array_equal(got[k][~hit], clean[k][~hit]), k
    assert (got["closest"][hit] == -1).all() and np.array_equal(got["closest"][~hit], clean["closest"][~hit])


def test_stand_alone_harness_runs_clean_under_the_sanitizers():
    exe = _harness.sanitized("evaluate_host", ("EVALUATE_HOST_MAIN",), recover="all")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    rows = [l.split() for l in r.stdout.splitlines()]
    assert len(rows) == 9 and all(row[5] == "inf" and row[6:] == ["-1", "-1"] for row in rows if row[1] == "1")      # the instance without obstacles


def test_entry_points_are_declared_exported_and_bound():
    """include/mpc_hip.h declares the two calls and struct mpc_eval_out, _lib.EXPORTS names them (test_abi compares the two lists and the built library), the ctypes
    mirror has the C layout, and the version is 0.9.0"""
    from mpc_local_planner_amd import _lib, BatchSolver, TrajectoryEval      # noqa: F401
    txt = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("mpc_evaluate_batch", "mpc_evaluate_batch_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code) and name in _lib.EXPORTS
    fields = re.search(r"typedef struct mpc_eval_out \{(.*?)\} mpc_eval_out;", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)\s*;", fields) == [f[0] for f in A.MpcEvalOut._fields_]
    assert C.sizeof(A.MpcEvalOut) == 5 * C.sizeof(C.c_void_p)
    assert hasattr(BatchSolver, "evaluate") and hasattr(BatchSolver, "evaluate_device")
    assert "return 900;" in open(os.path.join(CSRC, "mpc_capi.hip")).read()
