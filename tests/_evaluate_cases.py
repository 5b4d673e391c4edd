"""Cases and reference of the trajectory evaluation (mpc_evaluate_batch*), shared by tests/test_evaluate_host.py (CPU: the host build of csrc/mpc_evaluate.hpp) and
tests/test_gpu_evaluate.py (-m gpu: the kernel).

A case is an ABI configuration plus a batch of RANDOM, non-optimal trajectories (every residual far from zero) with ragged grid sizes, rows beyond n_b filled with
NaN, optional obstacles of mixed kinds and optional via-points.  The reference of every number is oracle/se2_nlp.py, untouched: ReferenceNlp (objective, equalities,
inequalities, bounds) built from the same CycleInputs and via-point association, and footprint_distance minimised over ALL obstacles and k = 1..n_b-2.

Deviation of an output from the reference: |got - ref| / max(|ref|, FLOOR) -- relative, with an absolute floor for values at zero.  The bounds are MEASURED (the
rule of tests/_truncated.py and tests/test_gpu_truncated_solves.py): per output the next power of two at or above 4 x the worst deviation seen over the case list,
on the host build (TOL_HOST) and on the MI355X (TOL_DEV); profiles/r12_evaluate.md has the measured figures.  Both sides are plain fp64, so a bound above 1e-10
would mean an error, not a loose constant (asserted)."""
import dataclasses
import math
from typing import Optional

import numpy as np

from oracle import se2_nlp as R
from mpc_local_planner_amd import _abi as A

FLOOR = 1e-2
OUTPUTS = ("objective", "eq_violation", "ineq_violation", "clearance")
# measured: profiles/r12_evaluate.md (worst deviation x 4, rounded up to a power of two)
TOL_HOST = {"objective": 2.0 ** -49, "eq_violation": 2.0 ** -49, "ineq_violation": 2.0 ** -50, "clearance": 2.0 ** -46}
# measured on the MI355X (tests/test_gpu_evaluate.py prints every figure): worst over device_cases() 7.051e-16 / 1.774e-16 / 2.498e-16 / 6.575e-15; the objective of the solver's
# own outputs (config 3, n = 80: a sum of 79 stage costs) deviates by 2.863e-15 from the oracle's and sets that bound
TOL_DEV = {"objective": 2.0 ** -46, "eq_violation": 2.0 ** -50, "ineq_violation": 2.0 ** -49, "clearance": 2.0 ** -45}

FQ = [[2.0, 0.3, -0.1], [0.3, 1.5, 0.2], [-0.1, 0.2, 0.4]]
FR = [[0.1, 0.02], [0.02, 0.05]]
FQF = [[8.0, 1.0, 0.0], [1.0, 9.0, 0.5], [0.0, 0.5, 0.6]]
FS = [[1.0, 0.2, 0.0], [0.2, 1.0, 0.1], [0.0, 0.1, 0.5]]
FOOTPRINTS = {
    "point": dict(footprint_kind=0),
    "circle": dict(footprint_kind=1, footprint_radius=0.25),
    "line": dict(footprint_kind=2, footprint_params=(-0.1, 0.05, 0.4, 0.0)),
    "two_circles": dict(footprint_kind=3, footprint_params=(0.3, 0.2, 0.15, 0.25)),
    "polygon": dict(footprint_kind=4, footprint_vertices=((0.35, 0.0), (0.1, 0.2), (-0.2, 0.15), (-0.2, -0.15))),
}
MODELS = {0: (0.0, 0.0), 1: (0.4, 0.0), 2: (0.45, 0.0), 3: (0.9, 1.1)}
BOX = dict(u_lb=(-0.2, -0.6), u_ub=(0.4, 0.6), du_lb=(-0.5, -0.5), du_ub=(0.5, 0.5), dt_lb=0.15, dt_ub=0.5)


@dataclasses.dataclass
class Case:
    name: str
    cfg: A.MpcConfig
    x0: np.ndarray
    xf: np.ndarray
    u_prev: np.ndarray
    dt_prev: np.ndarray
    x: np.ndarray
    u: np.ndarray
    dt: np.ndarray
    n_grid: np.ndarray
    obstacles: Optional[tuple] = None      # (n_obstacles, n_vertices, vertices, radius or None, velocity or None)
    via: Optional[tuple] = None            # (n_via, via)

    @property
    def B(self):
        return self.x.shape[0]


def ocfg_from_abi(c: A.MpcConfig, n: int) -> R.OcpConfig:
    """the oracle's description of the same parameter set (grid size n)"""
    def sym(d, o):
        m = np.diag([float(v) for v in d])
        if len(d) == 3:
            m[0, 1] = m[1, 0] = o[0]; m[0, 2] = m[2, 0] = o[1]; m[1, 2] = m[2, 1] = o[2]
        else:
            m[0, 1] = m[1, 0] = o[0]
        return m
    fk = int(c.footprint_kind)
    fpar = {0: (), 1: (c.footprint_radius,), 2: tuple(c.footprint_params), 3: tuple(c.footprint_params), 4: tuple(c.footprint_vertices[:2 * c.footprint_n_vertices])}[fk]
    return R.OcpConfig(model=int(c.model), model_params=(c.model_params[0], c.model_params[1]), n=n, dt_ref=c.dt_ref, dt_free=bool(c.dt_free), dt_lb=c.dt_lb, dt_ub=c.dt_ub,
                       xf_fixed=tuple(bool(v) for v in c.xf_fixed), collocation=int(c.collocation), objective=int(c.objective), Q=sym(c.Q, c.Q_offdiag), R=sym(c.R, [c.R_offdiag]),
                       integral_form=bool(c.integral_form), cost_integration="trapezoidal_rule" if c.cost_integration == A.COST_TRAPEZOIDAL else "left_sum",
                       hybrid_min_time=bool(c.hybrid_cost_minimum_time), Qf=sym(c.Qf, c.Qf_offdiag) if c.has_Qf else None, vp_position_weight=c.vp_position_weight,
                       vp_orientation_weight=c.vp_orientation_weight, via_points_ordered=bool(c.via_points_ordered),
                       terminal_ball_S=sym(c.terminal_ball_S, c.terminal_ball_S_offdiag) if c.terminal_ball else None, terminal_ball_gamma=c.terminal_ball_gamma,
                       u_lb=np.array(c.u_lb[:]), u_ub=np.array(c.u_ub[:]), du_lb=np.array(c.du_lb[:]), du_ub=np.array(c.du_ub[:]), min_obstacle_dist=c.min_obstacle_dist,
                       enable_dynamic_obstacles=bool(c.enable_dynamic_obstacles), footprint_kind=fk, footprint_params=fpar)


def make_case(name, abi, n, B, seed, O=0, V=1, kinds="pclg", radius=True, velocity=True, via=0, n_grid=None):
    """abi: keywords of _abi.make_config.  kinds: obstacle kinds drawn in turn from p(oint) c(ircle) l(ine) (poly)g(on), as far as V allows."""
    rng = np.random.default_rng(seed)
    kw = dict(BOX); kw.update(abi)
    cfg = A.make_config(n=n, max_obstacles=O, max_vertices=V, max_via_points=via, **kw)
    if n_grid is None:
        n_grid = [(3, 4, n, max(3, n // 3), max(3, n - 1))[b % 5] if b < 5 else int(rng.integers(3, n + 1)) for b in range(B)]
    n_grid = np.minimum(np.asarray(n_grid, np.int32), n)
    x = np.concatenate([rng.uniform(-2.0, 2.0, (B, n, 2)), rng.uniform(-math.pi, math.pi, (B, n, 1))], -1)
    u = rng.uniform(-0.7, 0.7, (B, n, 2))
    dt = rng.uniform(0.1, 0.6, B)
    for b in range(B):
        u[b, n_grid[b] - 1] = u[b, n_grid[b] - 2]      # the duplicate of the last control (never read)
        x[b, n_grid[b]:] = np.nan; u[b, n_grid[b]:] = np.nan      # rows at and beyond n_b are never read
    x0 = np.concatenate([rng.uniform(-2.0, 2.0, (B, 2)), rng.uniform(-2 * math.pi, 2 * math.pi, (B, 1))], -1)      # headings beyond [-pi, pi): normalised by the call
    xf = np.concatenate([rng.uniform(-2.0, 2.0, (B, 2)), rng.uniform(-2 * math.pi, 2 * math.pi, (B, 1))], -1)
    u_prev = rng.uniform(-0.5, 0.5, (B, 2))
    dt_prev = np.where(np.arange(B) % 2 == 0, 0.0, rng.uniform(0.1, 0.4, B))      # with and without the first control-rate row
    obstacles = None
    if O > 0:
        no = np.array([(O, 0, max(1, O // 2))[b % 3] if b < 3 else int(rng.integers(0, O + 1)) for b in range(B)], np.int32)      # full, none, some
        if B == 1:
            no[0] = O
        nv = np.ones((B, O), np.int32)
        verts = rng.uniform(-2.5, 2.5, (B, O, V, 2))
        rad = np.zeros((B, O))
        allowed = [k for k in kinds if (k in "pc") or (k == "l" and V >= 2) or (k == "g" and V >= 3)]
        for b in range(B):
            for o in range(O):
                k = allowed[(b + o) % len(allowed)]
                if k == "c":
                    rad[b, o] = rng.uniform(0.05, 0.3)
                elif k == "l":
                    nv[b, o] = 2
                elif k == "g":
                    nv[b, o] = int(rng.integers(3, V + 1))
                    c = rng.uniform(-2.0, 2.0, 2)      # a compact polygon (any orientation, not necessarily convex)
                    verts[b, o] = c + rng.uniform(-0.6, 0.6, (V, 2))
        vel = rng.uniform(-0.3, 0.3, (B, O, 2))
        for b in range(0, B, 2):      # an EMPTY slot below n_obstacles[b] (n_vertices = 0, as the solve accepts and skips): no obstacle, its data (NaN here) never read
            if no[b] >= 2:
                nv[b, 1] = 0; verts[b, 1] = np.nan; rad[b, 1] = np.nan; vel[b, 1] = np.nan
        obstacles = (no, nv, verts, rad if radius else None, vel if velocity else None)
    vp = None
    if via > 0:
        nvia = np.array([(via, 0, 1)[b % 3] if b < 3 else int(rng.integers(0, via + 1)) for b in range(B)], np.int32)
        pts = np.concatenate([rng.uniform(-2.0, 2.0, (B, via, 2)), rng.uniform(-math.pi, math.pi, (B, via, 1))], -1)
        for b in range(B):
            if nvia[b] > 0:
                pts[b, 0, :2] = x0[b, :2] + 1e-3      # closest to x_0: skipped (unordered) or attached to grid point 1 (ordered)
        vp = (nvia, pts)
    return Case(name, cfg, x0, xf, u_prev, dt_prev, x, u, dt, n_grid, obstacles, vp)


def _obstacle(case, b, o):
    no, nv, verts, rad, vel = case.obstacles
    k = int(nv[b, o])
    r = float(rad[b, o]) if rad is not None else 0.0
    kind = (R.OBST_CIRCLE if rad is not None else R.OBST_POINT) if k == 1 else (R.OBST_LINE if k == 2 else R.OBST_POLYGON)
    return R.Obstacle(kind, verts[b, o, :k].copy(), r, vel[b, o].copy() if vel is not None else None)


def reference(case: Case, cfg_of=None):
    """dict of (B,) arrays objective / eq_violation / ineq_violation / clearance and closest (B, 2), from the oracle.  cfg_of(b): the ABI configuration of instance b
    (parameter sets); default the case's."""
    B = case.B
    out = {k: np.zeros(B) for k in OUTPUTS}
    out["closest"] = np.full((B, 2), -1, np.int32)
    for b in range(B):
        c = cfg_of(b) if cfg_of else case.cfg
        n = int(case.n_grid[b])
        oc = ocfg_from_abi(c, n)
        x0 = case.x0[b].copy(); xf = case.xf[b].copy()
        x0[2] = R.normalize_theta(x0[2]); xf[2] = R.normalize_theta(xf[2])
        x = case.x[b, :n].copy()
        x[0] = x0
        for i in range(3):
            if oc.xf_fixed[i]:
                x[n - 1, i] = xf[i]
        dt = float(case.dt[b]) if oc.dt_free else oc.dt_ref
        via = None
        if case.via is not None and oc.objective == R.OBJ_MIN_TIME_VIA_POINTS:
            via = case.via[1][b, :int(case.via[0][b])]
        inp = R.CycleInputs(x0=x0, xf=xf, u_prev=case.u_prev[b].copy(), dt_prev=float(case.dt_prev[b]), via_points=via)
        nlp = R.ReferenceNlp(oc, inp, via_idx=R.associate_via_points(oc, x, via))
        z = nlp.pack(R.Trajectory(x, case.u[b, :n - 1].copy(), dt))
        lb, ub = nlp.bounds()
        rows = nlp.inequalities(z)
        out["objective"][b] = nlp.objective(z)
        out["eq_violation"][b] = np.abs(nlp.equalities(z)).max()
        out["ineq_violation"][b] = max(0.0, float(rows.max()) if rows.size else 0.0, float((lb - z).max()), float((z - ub).max()))
        best, arg = math.inf, (-1, -1)
        if case.obstacles is not None:
            for k in range(1, n - 1):
                for o in range(int(case.obstacles[0][b])):
                    if case.obstacles[1][b, o] <= 0:
                        continue
                    d = R.footprint_distance(oc.footprint_kind, oc.footprint_params, x[k], _obstacle(case, b, o), k * dt if oc.enable_dynamic_obstacles else 0.0)
                    if d < best:
                        best, arg = d, (k, o)
        out["clearance"][b] = best
        out["closest"][b] = arg
    return out


def deviation(got, ref):
    """worst |got - ref| / max(|ref|, FLOOR) over the batch; equal infinities (no obstacles) deviate by 0; a NaN anywhere gives inf"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    same_inf = np.isinf(ref) & (got == ref)
    with np.errstate(invalid="ignore"):
        d = np.where(same_inf, 0.0, np.abs(got - ref) / np.maximum(np.abs(ref), FLOOR))
    return float(np.where(np.isnan(d), np.inf, d).max())


def measured_bound(worst):
    """the project's rule: 4 x the worst deviation, rounded up to a power of two"""
    return 2.0 ** math.ceil(math.log2(4.0 * worst)) if worst > 0 else 0.0


def _nlp_specs():
    """(name, keywords of _abi.make_config, via-points) of the cases without obstacles: 4 models x 3 collocation rules; every objective variant; one-sided rate rows;
    terminal ball inside and outside; free and fixed goal components; via-points ordered and unordered"""
    out = []
    mt = dict(objective=A.OBJ_MIN_TIME, dt_free=True)
    for model in range(4):
        for coll in range(3):
            out.append((f"model{model}_colloc{coll}", dict(mt, model=model, model_params=MODELS[model], collocation=coll), 0))
    quad = dict(objective=A.OBJ_QUADRATIC, Q=(2.0, 2.0, 0.25), R=(0.1, 0.05), xf_fixed=(False, False, False))
    wide = dict(u_lb=(-2.0, -2.0), u_ub=(2.0, 2.0), du_lb=(-A.INF, -A.INF), du_ub=(A.INF, A.INF), dt_lb=0.0, dt_ub=10.0)
    variants = {
        "quad_sum_fixed": dict(quad, dt_free=False, Qf=(10.0, 10.0, 0.5)),
        "quad_left_fixed": dict(quad, dt_free=False, integral_form=True),
        "quad_trapz_fixed": dict(quad, dt_free=False, integral_form=True, cost_integration=A.COST_TRAPEZOIDAL, Qf=(10.0, 10.0, 0.5)),
        "quad_sum_free": dict(quad, dt_free=True),
        "quad_left_free": dict(quad, dt_free=True, integral_form=True, Qf=(10.0, 10.0, 0.5)),
        "quad_trapz_free": dict(quad, dt_free=True, integral_form=True, cost_integration=A.COST_TRAPEZOIDAL),
        "quad_hybrid": dict(quad, dt_free=True, Q=(0.0, 0.0, 0.0), hybrid_cost_minimum_time=True, xf_fixed=(True, True, True)),
        "quad_offdiag": dict(quad, dt_free=True, Q=FQ, R=FR, Qf=FQF, integral_form=True, cost_integration=A.COST_TRAPEZOIDAL),
        "quad_offdiag_fixed_goal_xy": dict(quad, dt_free=False, Q=FQ, R=FR, Qf=FQF, xf_fixed=(True, True, False)),
        "min_time_terminal_cost_free_y": dict(mt, Qf=(10.0, 10.0, 0.5), xf_fixed=(True, False, True)),
        "min_time_terminal_cost_fixed_goal": dict(mt, Qf=(10.0, 10.0, 0.5), xf_fixed=(True, True, True)),      # no edge: the goal is completely fixed
        "ball_inside": dict(mt, xf_fixed=(False, False, False), terminal_ball_S=(1.0, 1.0, 0.5), terminal_ball_gamma=1e3, **wide),      # nothing violated: ineq_violation = 0 exactly
        "ball_outside": dict(mt, xf_fixed=(False, False, True), terminal_ball_S=FS, terminal_ball_gamma=0.01, **wide),      # the ball row is the only violated one
        "rate_one_sided": dict(mt, du_lb=(-A.INF, -0.3), du_ub=(0.4, A.INF)),
    }
    for name, kw in variants.items():
        out.append((name, dict(kw, model=0, model_params=MODELS[0]), 0))
    for ordered in (False, True):
        for wo in (0.0, 0.3):
            out.append((f"via_ordered{int(ordered)}_wo{wo}", dict(mt, objective=A.OBJ_MIN_TIME_VIA_POINTS, model=1, model_params=MODELS[1], via_points_ordered=ordered,
                                                                vp_position_weight=0.7, vp_orientation_weight=wo), 6))
    # (appended last: the device shapes of the specs above stay as they are)
    out.append(("ball_fixed_goal", dict(mt, model=0, model_params=MODELS[0], xf_fixed=(True, True, True), terminal_ball_S=FS, terminal_ball_gamma=0.01, **wide), 0))      # no edge: the goal is completely fixed
    return out


def host_cases():
    """the CPU list: _nlp_specs at cfg.n = 50 with grid sizes 3, 4, 50 (and others) in every batch, then 5 footprints x point / circle / line / polygon obstacles, static and
    moving"""
    out = [make_case(name, abi, 50, 7, 1001 + i, via=via) for i, (name, abi, via) in enumerate(_nlp_specs())]
    mt = dict(objective=A.OBJ_MIN_TIME, dt_free=True, model=0, model_params=MODELS[0])
    seed = 1500
    for fp, fkw in FOOTPRINTS.items():
        for dyn in (False, True):
            seed += 1
            out.append(make_case(f"footprint_{fp}_dyn{int(dyn)}", dict(mt, enable_dynamic_obstacles=dyn, **fkw), 12, 5, seed, O=8, V=5, n_grid=(12, 3, 4, 7, 12)))
    return out


def device_cases():
    """the same list at the shapes that can break the kernel: cfg.n = 3 (one interior point), 4, 63, 64, 65, 129 (the lane loop exactly full, one over, twice plus a
    remainder), B = 1 and 37, ragged n_b from 3 to cfg.n, instances without obstacles, O = 1 and 16 with V = 1, 2, 8, radius / velocity NULL and given, dynamic obstacles
    on and off.  The expensive geometry (polygon x polygon) runs on the short grids, the long grids carry cheap obstacles: the reference is plain Python."""
    shapes = [(3, 37), (4, 37), (63, 1), (64, 37), (65, 1), (129, 37), (64, 1), (129, 1), (3, 1), (65, 37), (4, 1), (63, 37)]
    out = []
    for i, (name, abi, via) in enumerate(_nlp_specs()):
        n, B = shapes[i % len(shapes)]
        out.append(make_case(f"{name}_n{n}_B{B}", abi, n, B, 2001 + i, via=via, n_grid=[n] if B == 1 else None))
    mt = dict(objective=A.OBJ_MIN_TIME, dt_free=True, model=0, model_params=MODELS[0])
    obst = [  # footprint, dyn, n, B, O, V, kinds, radius, velocity
        ("point", False, 129, 37, 1, 1, "p", False, False), ("point", True, 64, 37, 1, 1, "pc", True, True), ("circle", True, 65, 1, 16, 2, "pcl", True, True),
        ("circle", False, 63, 1, 16, 1, "pc", True, False), ("line", False, 4, 37, 16, 8, "pclg", True, True), ("line", True, 64, 1, 16, 2, "pcl", False, True),
        ("two_circles", True, 3, 37, 16, 8, "pclg", True, True), ("two_circles", False, 129, 1, 1, 2, "l", False, False), ("polygon", False, 4, 37, 16, 8, "pclg", True, False),
        ("polygon", True, 3, 37, 16, 8, "pclg", True, True), ("polygon", True, 65, 1, 1, 8, "g", False, True), ("point", True, 63, 37, 1, 8, "g", True, True),
    ]
    for j, (fp, dyn, n, B, O, V, kinds, rad, vel) in enumerate(obst):
        out.append(make_case(f"footprint_{fp}_dyn{int(dyn)}_n{n}_B{B}_O{O}_V{V}", dict(mt, enable_dynamic_obstacles=dyn, **FOOTPRINTS[fp]), n, B, 2501 + j, O=O, V=V, kinds=kinds,
                             radius=rad, velocity=vel, n_grid=[n] if B == 1 else None))
    return out
