"""CPU test of the parameter-set policy (mpc_problem.hpp::parameter_set_error) and of the records a set gives (mpc_problem.hpp::fill_records, what
mpc_create keeps for the handle and mpc_set_parameter_sets uploads for every set), compiled for the host with g++ by a tests-only harness
(tests/host_harness/parameter_sets_host.cpp).  A set may change the double fields of mpc_config and nothing that selects the kernel."""
import ctypes as C
import os
import shutil

import pytest

from mpc_local_planner_amd import _abi as A
import _harness

CANDS = dict(candidates=(A.CAND_REFERENCE, A.CAND_HERMITE_FF, A.CAND_HERMITE_FR), candidate_max_iter=(40, 40, 40), candidate_param=(0.0, 2.0, 1.5))
CIRCLE = dict(footprint_kind=1, footprint_radius=0.3, max_obstacles=6, max_vertices=1, max_obstacle_rows=4)
POLYGON = dict(footprint_kind=4, footprint_vertices=((0.3, 0.2), (-0.3, 0.2), (-0.3, -0.2), (0.3, -0.2)), max_obstacles=4, max_vertices=1, max_obstacle_rows=4)
OFFDIAG_Q = ((2.0, 0.3, 0.1), (0.3, 2.0, 0.0), (0.0, 0.0, 0.25))
CASES = {
    "config2_carlike_n50": lambda: A.config_carlike_min_time(50),
    "carlike_n20_two_waves": lambda: A.config_carlike_min_time(20, two_wave_min_batch=64),
    "carlike_n50_global": lambda: A.config_carlike_min_time(50, stage_data=A.STAGE_GLOBAL),
    "carlike_n50_fp32": lambda: A.config_carlike_min_time(50, precision=A.FP32),
    "carlike_n50_mixed": lambda: A.config_carlike_min_time(50, precision=A.MIXED),
    "carlike_n50_mixed_candidates": lambda: A.config_carlike_min_time(50, precision=A.MIXED, **CANDS),
    "carlike_n50_candidates": lambda: A.config_carlike_min_time(50, **CANDS),
    "carlike_n30_circle_rows": lambda: A.config_carlike_min_time(30, **CIRCLE),
    "carlike_n30_polygon_rows": lambda: A.config_carlike_min_time(30, **POLYGON),
    "carlike_n20_dual_warm_start": lambda: A.config_carlike_min_time(20, dual_warm_start=True),
    "unicycle_quadratic_n20": lambda: A.config_unicycle_quadratic(20),
    "unicycle_quadratic_n20_offdiag_ball": lambda: A.config_unicycle_quadratic(20, Q=OFFDIAG_Q, terminal_ball_S=(1.0, 1.0, 0.1)),
    "unicycle_quadratic_n20_trapezoid": lambda: A.config_unicycle_quadratic(20, integral_form=True, cost_integration=A.COST_TRAPEZOIDAL),
    "carlike_n50_via_points": lambda: A.config_carlike_min_time(50, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=8),
}

# record fields (mpc_core.hpp::Problem) a double field of mpc_config may move
ALLOWED = {
    "model_params": {"p0", "p1"}, "dt_ref": {"dt_ref", "Q", "R", "Qf", "Qo", "Ro", "Qfo"}, "dt_lb": {"dt_lb"}, "dt_ub": {"dt_ub"},
    "Q": {"Q", "Qf"}, "R": {"R"}, "Qf": {"Qf"}, "u_lb": {"u_lb"}, "u_ub": {"u_ub"}, "du_lb": {"rate_lim"}, "du_ub": {"rate_lim"},
    "tol": {"tol", "pit_mu_min"}, "mu_init": {"mu_init", "mu_init_warm"}, "min_obstacle_dist": {"d_min"}, "force_inclusion_dist": {"force_incl"},
    "cutoff_dist": {"cutoff"}, "footprint_radius": {"fp_radius"}, "mu_init_warm": {"mu_init_warm"}, "terminal_ball_S": {"ball_S"},
    "terminal_ball_gamma": {"ball_gamma"}, "vp_position_weight": {"vp_wp"}, "vp_orientation_weight": {"vp_wo"}, "footprint_vertices": {"fp_poly"},
    "footprint_params": {"fp_line"}, "mu_init_dual": {"mu_init_dual"}, "candidate_param": {"cand_param"}, "Q_offdiag": {"Qo", "Qfo"}, "R_offdiag": {"Ro"},
    "Qf_offdiag": {"Qfo"}, "terminal_ball_S_offdiag": {"So"}, "acceptable_tol": {"acc_tol"},
}
# configurations the double fields are walked on, and the fields whose change every one of them must see in its fp64 record
WALK = {
    "unicycle_quadratic_circle_offdiag_ball_candidates": (
        lambda: A.config_unicycle_quadratic(20, Q=OFFDIAG_Q, R=((0.1, 0.02), (0.02, 0.05)), Qf=(10.0, 10.0, 0.5), terminal_ball_S=((1.0, 0.1, 0.0), (0.1, 1.0, 0.0), (0.0, 0.0, 0.1)),
                                            **CIRCLE, **CANDS),
        {"model_params[0]", "dt_ref", "Q[0]", "R[1]", "Qf[2]", "u_lb[0]", "u_ub[1]", "du_lb[0]", "du_ub[1]", "tol", "mu_init", "min_obstacle_dist",
         "force_inclusion_dist", "cutoff_dist", "footprint_radius", "terminal_ball_S[1]", "terminal_ball_gamma", "candidate_param[1]", "Q_offdiag[0]",
         "R_offdiag", "Qf_offdiag[1]", "terminal_ball_S_offdiag[2]", "acceptable_tol"}),
    "carlike_mixed_candidates": (lambda: A.config_carlike_min_time(30, precision=A.MIXED, **CANDS),
                                 {"model_params[0]", "dt_ref", "dt_lb", "dt_ub", "u_lb[1]", "du_ub[0]", "tol", "mu_init_dual", "candidate_param[2]"}),
    "bicycle_polygon_via_points": (lambda: A.make_config(model=A.MODEL_KINEMATIC_BICYCLE, model_params=(1.0, 1.0), n=30, objective=A.OBJ_MIN_TIME_VIA_POINTS, max_via_points=4, **POLYGON),
                                   {"model_params[1]", "footprint_vertices[5]", "vp_position_weight", "vp_orientation_weight", "mu_init_warm"}),
    "carlike_line_footprint": (lambda: A.config_carlike_min_time(30, footprint_kind=2, footprint_params=(0.0, 0.0, 0.4, 0.0), max_obstacles=4, max_vertices=1),
                               {"footprint_params[2]"}),
}


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(_harness.shared("parameter_sets_host"))
    lib.named_bytes.restype = C.c_int64
    lib.record_bytes.restype = C.c_int64
    return lib


def _error(h, handle, s):
    err = C.create_string_buffer(512)
    rc = h.set_error(C.byref(handle), C.byref(s), err, 512)
    return err.value.decode() if rc else None


def _diff(h, handle, s):
    out = C.create_string_buffer(2048)
    h.record_diff(C.byref(handle), C.byref(s), out, 2048)
    d64, d32 = out.value.decode().split(";")
    return set(filter(None, d64.split(","))), set(filter(None, d32.split(",")))


def _copy(cfg):
    c = A.MpcConfig()
    C.memmove(C.byref(c), C.byref(cfg), C.sizeof(cfg))
    return c


def _elements(ctype):
    """(field name, element index or None, element type) of every scalar of mpc_config"""
    for name, t in A.MpcConfig._fields_:
        if hasattr(t, "_length_"):
            for i in range(t._length_):
                yield name, i, t._type_
        else:
            yield name, None, t


def _get(c, name, i):
    v = getattr(c, name)
    return v[i] if i is not None else v


def _set(c, name, i, value):
    if i is None:
        setattr(c, name, value)
    else:
        getattr(c, name)[i] = value


def _label(name, i):
    return f"{name}[{i}]" if i is not None else name


def test_the_record_field_list_covers_the_records(h):
    """the harness names every field of Problem<T> (what it does not name is padding)"""
    for f32 in (0, 1):
        assert 0 <= h.record_bytes(f32) - h.named_bytes(f32) < 8 * 16
        assert h.record_bytes(f32) % 16 == 0          # the kernel copies the record in 16-byte pieces


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_set_equal_to_the_handle_gives_the_handle_records(h, name):
    cfg = CASES[name]()
    s = _copy(cfg)
    assert _error(h, cfg, s) is None
    assert _diff(h, cfg, s) == (set(), set())          # both records, MPC_MIXED's two phases included
    assert h.same_plan(C.byref(cfg), C.byref(s)) == 1


def _valid_alternatives(v):
    return [v + 1, v - 1, 1 - v, 0, 1, 2, 4, 8, 64, -1, v + 2]


@pytest.mark.parametrize("field", sorted({_label(n, i) for n, i, t in _elements(A.MpcConfig) if t is C.c_int32}))
def test_every_integer_field_is_refused(h, field):
    """every int32_t field of mpc_config set to another value that mpc_create accepts: the set is refused and the message names the field"""
    name, _, idx = field.partition("[")
    i = int(idx[:-1]) if idx else None
    seen = 0
    for base in (CASES["config2_carlike_n50"](), CASES["unicycle_quadratic_n20"](), CASES["carlike_n50_candidates"](), CASES["carlike_n30_polygon_rows"]()):
        v = _get(base, name, i)
        for alt in _valid_alternatives(v):
            if alt == v:
                continue
            s = _copy(base)
            _set(s, name, i, alt)
            if h.set_error(C.byref(s), C.byref(s), C.create_string_buffer(512), 512):
                continue                                # not a configuration mpc_create takes
            why = _error(h, base, s)
            assert why is not None and why.startswith(f"{field} is {alt} here and {v} in the handle's configuration"), why
            seen += 1
            break
    assert seen > 0, f"no valid other value of {field} found"


@pytest.mark.parametrize("walk", sorted(WALK))
def test_every_double_field_is_accepted_and_moves_only_its_record_fields(h, walk):
    make, must_move = WALK[walk]
    base = make()
    assert _error(h, base, _copy(base)) is None
    moved = set()
    for name, i, t in _elements(A.MpcConfig):
        if t is not C.c_double:
            continue
        v = _get(base, name, i)
        s = _copy(base)
        _set(s, name, i, v * 1.1 if v != 0 else 0.01)        # within its range: bounds move apart, infinite rate bounds stay infinite
        label = _label(name, i)
        assert _error(h, base, s) is None, label
        d64, d32 = _diff(h, base, s)
        assert d64 <= ALLOWED[name] and d32 <= ALLOWED[name], (label, d64, d32)
        assert h.same_plan(C.byref(base), C.byref(s)) == 1, label
        if d64:
            moved.add(label)
    assert must_move <= moved, sorted(must_move - moved)


def test_a_double_field_out_of_its_range_is_refused_as_mpc_create_refuses_it(h):
    base = A.config_carlike_min_time(50)
    s = _copy(base)
    s.dt_ref = 20.0
    assert _error(h, base, s) == "dt_ref must lie in [dt_lb, dt_ub] on the variable grid"
    s = _copy(base)
    s.u_ub[0] = -0.5
    assert _error(h, base, s) == "control box must be finite and non-empty"


def test_the_finiteness_of_the_rate_bounds_is_refused_with_its_own_message(h):
    base = A.config_carlike_min_time(50)          # every rate bound finite
    s = _copy(base)
    s.du_ub[1] = A.INF
    assert _error(h, base, s) == "du_ub[1] is infinite here and finite in the handle's configuration"
    free = A.config_carlike_min_time(50, du_lb=(-A.INF, -A.INF), du_ub=(A.INF, A.INF))
    s = _copy(free)
    s.du_lb[0] = -0.5
    assert _error(h, free, s) == "du_lb[0] is finite here and infinite in the handle's configuration"


def test_zero_off_diagonal_terms_are_refused_with_their_own_message(h):
    diag = A.config_unicycle_quadratic(20)
    s = _copy(diag)
    s.Q_offdiag[1] = 0.2
    assert _error(h, diag, s) == "Q_offdiag[1] is non-zero here and every off-diagonal cost term is zero in the handle's configuration"
    s = _copy(diag)
    s.R_offdiag = -0.01
    assert _error(h, diag, s).startswith("R_offdiag is non-zero here")
    full = A.config_unicycle_quadratic(20, Q=OFFDIAG_Q)
    s = _copy(full)
    for j in range(3):
        s.Q_offdiag[j] = 0.0
    assert _error(h, full, s) == "the off-diagonal cost terms are all zero here and not in the handle's configuration (they select the kernel level)"
    s.R_offdiag = 0.05                              # another non-zero term keeps the kernel level: accepted
    assert _error(h, full, s) is None
    # the minimum-time objective has no quadratic form: its off-diagonal weights select nothing
    mt = A.config_carlike_min_time(50)
    s = _copy(mt)
    s.Q_offdiag[0] = 0.3
    assert _error(h, mt, s) is None and _diff(h, mt, s) == (set(), set())


def test_the_entry_point_refuses_a_null_handle_without_a_gpu():
    from mpc_local_planner_amd import _lib
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    lib = _lib.load()
    cfg = A.config_carlike_min_time(50)
    set_of = (C.c_int32 * 1)(0)
    assert lib.mpc_set_parameter_sets(None, 1, C.byref(cfg), 1, set_of) == A.MPC_EINVAL
    assert lib.mpc_set_parameter_sets(None, 0, None, 0, None) == A.MPC_EINVAL
