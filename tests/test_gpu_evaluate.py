"""-m gpu: the trajectory evaluation on the device (mpc_evaluate_batch*, csrc/mpc_evaluate.hpp; BatchSolver.evaluate / evaluate_device).

  1. device against the oracle on the case list of tests/_evaluate_cases.py at the shapes that can break the kernel (the reference is oracle/se2_nlp.py, untouched; the
     bounds TOL_DEV are measured on the MI355X over this list, profiles/r12_evaluate.md section 4);
  2. consistency with the solver on converged answers of BASELINE configs[1] and configs[2] (32 instances each): the violations are within tol in the solver's own
     scaling, the objective is the oracle's; an iterate stopped after one iteration evaluates too;
  3. the same instance gives the same bits wherever it sits in whichever batch, run after run;
  4. parameter sets: each instance equals what a handle created with its set returns, bit for bit;
  5. a NaN spoils its own instance only;
  6. the host-pointer call equals the device call; the refusals return their codes and set mpc_last_error;
  7. composition: behind mpc_step_batch_device on the solver's stream, without a synchronisation in between, the clearance reproduces the plain geometry of
     tests/test_gpu_clearance.py (clearance_to_polygons, copied here)."""
import ctypes as C

import numpy as np
import pytest

import _evaluate_cases as E

pytestmark = pytest.mark.gpu

KEYS = E.OUTPUTS + ("closest",)


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as pkg
    return pkg


def _solver(m, case, max_batch=None, cfg=None):
    s = m.BatchSolver(cfg if cfg is not None else case.cfg, max_batch=max_batch or case.B)
    if not (case.n_grid == case.cfg.n).all():
        s.set_grid_sizes(case.n_grid)
    if case.via is not None:
        s.set_via_points(case.via[0], case.via[1])
    return s


def _result(r):
    return {"objective": r.objective, "eq_violation": r.eq_violation, "ineq_violation": r.ineq_violation, "clearance": r.clearance, "closest": r.closest}


def host_call(s, case, x0_given=True):
    return _result(s.evaluate(case.x0 if x0_given else None, case.xf if x0_given else None, case.x, case.u, case.dt, u_prev=case.u_prev, dt_prev=case.dt_prev,
                              obstacles=case.obstacles))


def device_call(s, case, sync=True):
    """the device-pointer call on torch tensors; outputs pre-filled with a pattern the kernel has to overwrite"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None
    B = case.B
    d = {k: t(getattr(case, k)) for k in ("x0", "xf", "u_prev", "dt_prev", "x", "u", "dt")}
    ob = [t(a) for a in case.obstacles] if case.obstacles is not None else None
    out = {k: torch.full((B,), -7.0, dtype=torch.float64, device="cuda") for k in E.OUTPUTS}
    out["closest"] = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()      # the solver's stream is not ordered against torch's
    p = lambda v: v.data_ptr() if v is not None else None
    s.evaluate_device(B, p(d["x0"]), p(d["xf"]), p(d["x"]), p(d["u"]), p(d["dt"]), **{k: p(v) for k, v in out.items()}, u_prev=p(d["u_prev"]), dt_prev=p(d["dt_prev"]),
                      obstacles=tuple(p(a) for a in ob) if ob is not None else None)
    if sync:
        s.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def clearance_to_polygons(x, no, nv, verts):
    """min over grid points 1..n-2 and ALL polygons of the instance of the distance point -> closed edge loop (teb's PolygonObstacle::getMinimumDistance for a
    point: no inside test); plain numpy, nothing of the solver.  (Copy of the helper of tests/test_gpu_clearance.py.)"""
    B = x.shape[0]
    out = np.full(B, np.inf)
    for b in range(B):
        p = x[b, 1:-1, :2]
        for o in range(int(no[b])):
            k = int(nv[b, o]); a = verts[b, o, :k]; c = np.roll(a, -1, axis=0); ab = c - a
            t = np.clip(((p[:, None, :] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1)[None], 0.0, 1.0)
            q = a[None] + t[..., None] * ab[None]
            out[b] = min(out[b], float(np.sqrt(((p[:, None, :] - q) ** 2).sum(-1)).min()))
    return out


# ---- 1. device against the oracle

CASES = E.device_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_equals_the_oracle(m, case):
    ref = E.reference(case)
    s = _solver(m, case)
    got = device_call(s, case)
    s.close()
    for k in ("objective", "eq_violation", "ineq_violation"):
        assert np.isfinite(got[k]).all(), k      # the NaN rows beyond n_b are never read
    dev = {k: E.deviation(got[k], ref[k]) for k in E.OUTPUTS}
    print(f"[evaluate, device against the oracle] {case.name}: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    for k in E.OUTPUTS:
        assert dev[k] <= E.TOL_DEV[k] <= 1e-10, (k, dev[k])
    assert np.array_equal(got["closest"], ref["closest"])
    if case.obstacles is None:
        assert np.isposinf(got["clearance"]).all() and (got["closest"] == -1).all()
    else:
        none = (case.obstacles[0] == 0) | (case.n_grid < 3)
        assert np.isposinf(got["clearance"][none]).all() and (got["closest"][none] == -1).all() and np.isfinite(got["clearance"][~none]).all()


# ---- 2. consistency with the solver

def _as_case(cfg, x0, xf, up, dtp, r, obstacles=None):
    B = x0.shape[0]
    return E.Case("solved", cfg, x0, xf, up, dtp, r.x, r.u, r.dt, np.full(B, cfg.n, np.int32), obstacles)


def _solver_scale(case, b):
    """the solve stops when its primal infeasibility is at most tol in SOLVER form (err_value: e.rp carries no multiplier scaling): collocation rows dt x the reference's,
    rate rows dt (first row: dt_prev) x the reference's; the boxes hold strictly (interior point); + the rounding of either form at states of order 10"""
    dt = float(case.dt[b]) if case.cfg.dt_free else case.cfg.dt_ref
    dtp = float(case.dt_prev[b])
    return 1.0 / dt, 1.0 / min(dt, dtp if dtp > 0 else dt)


@pytest.mark.parametrize("config", ["config2", "config3"])
def test_converged_answers_are_feasible_to_tol_and_cost_what_the_oracle_says(m, config):
    B, tol = 32, 1e-8
    if config == "config2":
        x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(B)
        cfg, obstacles = m.config_carlike_min_time(50, tol=tol, acceptable_tol=-1.0), None
    else:
        x0, xf, up, dtp, (no, nv, verts) = m.workloads.unicycle_obstacle_inputs(B, n_obst=16, max_vertices=6)
        cfg, obstacles = m.config_unicycle_quadratic(80, max_obstacles=16, max_vertices=6, max_obstacle_rows=4, tol=tol, acceptable_tol=-1.0), (no, nv, verts)
    s = m.BatchSolver(cfg, max_batch=B)
    r = s.solve(x0, xf, up, dtp, obstacles=obstacles)
    case = _as_case(cfg, x0, xf, up, dtp, r, obstacles + (None, None) if obstacles else None)
    got = host_call(s, case)
    s.close()
    ok = r.status == 0
    assert ok.mean() >= 0.8
    ref = E.reference(E.Case(**{**case.__dict__, "obstacles": None}))      # (the clearance has its own test below: plain Python over 16 polygons x 78 poses x 32 is slow)
    for b in np.flatnonzero(ok):
        se, si = _solver_scale(case, b)
        assert got["eq_violation"][b] <= tol * se + 1e-13 and got["ineq_violation"][b] <= tol * si + 1e-13, (b, got["eq_violation"][b], got["ineq_violation"][b])
    print(f"[evaluate, solver outputs against the oracle] {config}: objective {E.deviation(got['objective'], ref['objective']):.3e}, worst eq_violation of a converged answer x dt / tol "
          f"{max(got['eq_violation'][b] / (tol * _solver_scale(case, b)[0]) for b in np.flatnonzero(ok)):.3f}")
    assert E.deviation(got["objective"], ref["objective"]) <= E.TOL_DEV["objective"]
    if config == "config2":
        assert E.deviation(got["objective"], (cfg.n - 1) * r.dt) <= E.TOL_DEV["objective"]      # minimum time: (n_b - 1) dt
    else:
        c = clearance_to_polygons(r.x, no, nv, verts)
        assert E.deviation(got["clearance"], c) <= E.TOL_DEV["clearance"]
    # an iterate stopped after one iteration evaluates too, far from feasible
    cfg1 = m.config_carlike_min_time(50, tol=tol, max_iter=1) if config == "config2" else m.config_unicycle_quadratic(80, max_obstacles=16, max_vertices=6, max_obstacle_rows=4, tol=tol, max_iter=1)
    s1 = m.BatchSolver(cfg1, max_batch=B)
    r1 = s1.solve(x0, xf, up, dtp, obstacles=obstacles)
    c1 = _as_case(cfg1, x0, xf, up, dtp, r1, obstacles + (None, None) if obstacles else None)
    g1 = host_call(s1, c1)
    s1.close()
    assert (r1.status == 1).mean() >= 0.9 and (g1["eq_violation"][r1.status == 1] > 1e4 * tol).all() and np.isfinite(g1["objective"]).all()
    ref1 = E.reference(E.Case(**{**c1.__dict__, "obstacles": None}))
    for k in ("objective", "eq_violation", "ineq_violation"):
        assert E.deviation(g1[k], ref1[k]) <= E.TOL_DEV[k], k


# ---- 3. independence from the batch and the run

def _take(case, idx):
    idx = np.asarray(idx)
    f = lambda a: np.ascontiguousarray(a[idx]) if a is not None else None
    return E.Case(case.name, case.cfg, f(case.x0), f(case.xf), f(case.u_prev), f(case.dt_prev), f(case.x), f(case.u), f(case.dt), f(case.n_grid),
                  tuple(f(a) for a in case.obstacles) if case.obstacles is not None else None, tuple(f(a) for a in case.via) if case.via is not None else None)


@pytest.mark.parametrize("name", ["footprint_line_dyn0_n4_B37_O16_V8", "via_ordered1_wo0.3_n129_B37", "quad_trapz_free_n129_B37"])
def test_same_bits_in_every_batch_position_and_run(m, name):
    case = next(c for c in CASES if c.name == name)
    B = case.B
    src = int(np.argmax(case.n_grid == case.cfg.n))      # a full-size instance
    order = np.arange(B)
    order[[0, 17, B - 1]] = src
    batch = _take(case, order)
    s = _solver(m, batch)
    a, b = device_call(s, batch), device_call(s, batch)
    s.close()
    one = _take(case, [src])
    s1 = _solver(m, one, max_batch=4)
    c = device_call(s1, one)
    s1.close()
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k                                   # two runs
        for pos in (0, 17, B - 1):
            assert a[k][pos].tobytes() == c[k][0].tobytes(), (k, pos)                # positions 0, 17, B-1 of 37 and the batch of 1


# ---- 4. parameter sets

def test_parameter_sets_equal_handles_created_with_the_sets(m):
    case = next(c for c in CASES if c.name == "footprint_circle_dyn1_n65_B1_O16_V2")
    case = _take(case, [0] * 6)
    case.x = case.x + np.random.default_rng(5).uniform(-0.05, 0.05, case.x.shape)
    other = type(case.cfg).from_buffer_copy(case.cfg)
    other.u_ub[0] = 0.1; other.du_ub[1] = 0.1; other.dt_lb = 0.3; other.min_obstacle_dist = 0.9; other.footprint_radius = 0.4; other.model_params[0] = 0.7
    sets = [case.cfg, other]
    set_of = np.array([0, 1, 1, 0, 1, 0], np.int32)
    s = _solver(m, case)
    s.set_parameter_sets(sets, set_of)
    mixed = device_call(s, case)
    s.set_parameter_sets(None)
    plain = device_call(s, case)
    s.close()
    alone = []
    for c in sets:
        h = _solver(m, case, cfg=c)
        alone.append(device_call(h, case))
        h.close()
    for k in KEYS:
        want = np.where(set_of.reshape((-1,) + (1,) * (alone[0][k].ndim - 1)) == 0, alone[0][k], alone[1][k])
        assert mixed[k].tobytes() == want.tobytes(), k
        assert plain[k].tobytes() == alone[0][k].tobytes(), k
    assert (alone[0]["clearance"] != alone[1]["clearance"]).all() and (alone[0]["ineq_violation"] != alone[1]["ineq_violation"]).all()


# ---- 5. scope of a NaN

def test_a_nan_spoils_its_own_instance_only(m):
    case = next(c for c in CASES if c.name == "footprint_point_dyn1_n64_B37_O1_V1")
    s = _solver(m, case)
    clean = device_call(s, case)
    bad = _take(case, np.arange(case.B))
    full = np.flatnonzero(case.n_grid >= 10)
    hit = full[:4]
    bad.x[hit[0], 5, 1] = np.nan; bad.u[hit[1], 2, 0] = np.inf; bad.dt[hit[2]] = np.nan; bad.xf[hit[3], 0] = -np.inf
    got = device_call(s, bad)
    s.close()
    keep = np.setdiff1d(np.arange(case.B), hit)
    for k in E.OUTPUTS:
        assert np.isnan(got[k][hit]).all(), k
        assert got[k][keep].tobytes() == clean[k][keep].tobytes(), k
    assert (got["closest"][hit] == -1).all() and np.array_equal(got["closest"][keep], clean["closest"][keep])


# ---- 6. host variant and refusals

def test_host_call_equals_device_call_and_refusals_name_their_reason(m):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MPC_EBATCH, MpcEvalOut
    case = next(c for c in CASES if c.name == "footprint_polygon_dyn1_n3_B37_O16_V8")
    s = _solver(m, case)
    a, b = device_call(s, case), host_call(s, case)
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    own = _take(case, np.arange(case.B))
    own.x0 = np.ascontiguousarray(case.x[:, 0]); own.xf = np.ascontiguousarray(case.x[np.arange(case.B), case.n_grid - 1])
    c, d = host_call(s, own), host_call(s, case, x0_given=False)      # NULL x0 / xf: the trajectory's own ends
    for k in KEYS:
        assert c[k].tobytes() == d[k].tobytes(), k
    lib, h = s._lib, s._h
    buf = np.zeros(case.B)
    out = MpcEvalOut(buf.ctypes.data, None, None, None, None)
    p = lambda arr: C.c_void_p(arr.ctypes.data)
    for fn in (lib.mpc_evaluate_batch, lib.mpc_evaluate_batch_device):
        assert fn(h, case.B, None, None, None, None, None, p(case.u), p(case.dt), None, C.byref(out)) == MPC_EINVAL and lib.mpc_last_error() != b""
        assert fn(h, case.B, None, None, None, None, p(case.x), p(case.u), None, None, C.byref(out)) == MPC_EINVAL      # dt on the variable grid
        assert fn(h, case.B, None, None, None, None, p(case.x), p(case.u), p(case.dt), None, None) == MPC_EINVAL and b"null" in lib.mpc_last_error()
        assert fn(h, case.B + 1, None, None, None, None, p(case.x), p(case.u), p(case.dt), None, C.byref(out)) == MPC_EBATCH and b"max_batch" in lib.mpc_last_error()
    s.close()
    big = m.BatchSolver(case.cfg, max_batch=case.B)
    big.set_parameter_sets([case.cfg], np.zeros(4, np.int32))
    assert lib.mpc_evaluate_batch(big._h, 5, None, None, None, None, p(case.x), p(case.u), p(case.dt), None, C.byref(out)) == MPC_EBATCH and b"parameter sets" in lib.mpc_last_error()
    big.set_parameter_sets(None)
    assert lib.mpc_evaluate_batch(big._h, 5, None, None, None, None, p(case.x), p(case.u), p(case.dt), None, C.byref(out)) == 0      # optional outputs: only the objective is written
    big.close()
    vc = next(c for c in CASES if c.name.startswith("via_ordered0_wo0.3"))
    v = m.BatchSolver(vc.cfg, max_batch=max(vc.B, 4))
    v.set_via_points(vc.via[0][:1], vc.via[1][:1])
    xx, uu, dd = np.zeros((2, vc.cfg.n, 3)), np.zeros((2, vc.cfg.n, 2)), np.ones(2)
    assert lib.mpc_evaluate_batch(v._h, 2, None, None, None, None, p(xx), p(uu), p(dd), None, C.byref(out)) == MPC_EBATCH and b"via-points" in lib.mpc_last_error()
    v.close()


# ---- 7. composition behind the control cycle on the solver's stream

def test_clearance_behind_step_batch_device_reproduces_the_plain_geometry(m):
    import torch
    B, n, O, V, dmin = 32, 80, 16, 6, 0.2
    x0, xf, up, dtp, (no, nv, verts) = m.workloads.unicycle_obstacle_inputs(B, n_obst=O, max_vertices=V, lateral=(0.15, 0.8))
    s = m.BatchSolver(m.config_unicycle_quadratic(n, max_obstacles=O, max_vertices=V, max_obstacle_rows=4, acceptable_tol=-1.0), max_batch=B)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [t(a) for a in (x0, xf, up, dtp)]
    ob = [t(no), t(nv), t(verts)]
    xo, uo, do = torch.zeros((B, n, 3), dtype=torch.float64, device="cuda"), torch.zeros((B, n, 2), dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda")
    st, it = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    cl, cs = torch.full((B,), -7.0, dtype=torch.float64, device="cuda"), torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
    ev = torch.full((3, B), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = lambda v: C.c_void_p(v.data_ptr())
    from mpc_local_planner_amd._abi import MpcObstacles
    mo = MpcObstacles(ob[0].data_ptr(), ob[1].data_ptr(), ob[2].data_ptr(), None, None)
    rc = s._lib.mpc_step_batch_device(s._h, B, p(d[0]), p(d[1]), p(d[2]), p(d[3]), None, None, None, C.byref(mo), 3, 0, 3, n, 0.1, p(xo), p(uo), p(do), p(st), p(it))
    assert rc == 0
    # no synchronisation: the evaluation is ordered behind the three solves by the solver's stream
    s.evaluate_device(B, d[0].data_ptr(), d[1].data_ptr(), xo.data_ptr(), uo.data_ptr(), do.data_ptr(), objective=ev[0].data_ptr(), eq_violation=ev[1].data_ptr(),
                      ineq_violation=ev[2].data_ptr(), clearance=cl.data_ptr(), closest=cs.data_ptr(), u_prev=d[2].data_ptr(), dt_prev=d[3].data_ptr(),
                      obstacles=(ob[0].data_ptr(), ob[1].data_ptr(), ob[2].data_ptr()))
    s.synchronize()
    s.close()
    x, status, clr, closest = xo.cpu().numpy(), st.cpu().numpy(), cl.cpu().numpy(), cs.cpu().numpy()
    want = clearance_to_polygons(x, no, nv, verts)
    print(f"[evaluate, clearance behind the control cycle against plain numpy] {E.deviation(clr, want):.3e}")
    assert E.deviation(clr, want) <= E.TOL_DEV["clearance"]
    ok = status == 0
    assert ok.mean() >= 0.9 and (clr[ok] >= dmin - 1e-6).all()      # what tests/test_gpu_clearance.py asserts with the host-side geometry, now read off the device
    assert ((closest[:, 0] >= 1) & (closest[:, 0] <= n - 2) & (closest[:, 1] >= 0) & (closest[:, 1] < no)).all()
    assert (ev.cpu().numpy()[1][ok] <= 1e-8 / 0.3 + 1e-13).all()
