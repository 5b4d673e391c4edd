"""CPU tests of the drop-in boundary, for every header of _abi.HEADERS: the C-ABI library builds for gfx950, loads, exports and binds every function a header declares;
every prototype table matches its header's declarations, parameter by parameter; every ctypes mirror has the C layout; and -- without a GPU -- mpc_create fails loudly
instead of falling back to a CPU path.  No compute calls here.  What is particular to one side header (the values of its defaults, its refusals without a handle) is in
tests/test_fleet_abi.py and tests/test_costmap_{clusters,lines,window}_abi.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _abi_check as K
from _abi_check import ROOT, lib      # noqa: F401 (lib: the fixture)
from mpc_local_planner_amd import _abi, _lib
from mpc_local_planner_amd._abi import CLUSTER_PROTOTYPES, FLEET_PROTOTYPES, HEADERS, LINE_PROTOTYPES, PROTOTYPES, WINDOW_PROTOTYPES

STRUCTS = [(header, struct) for header, (_, mirrors) in HEADERS.items() for struct in mirrors]


def _declared_functions():
    txt = re.sub(r"/\*.*?\*/", "", K.header_text(K.MAIN), flags=re.S)
    return sorted(set(re.findall(r"\b(mpc_[a-z_0-9]+)\s*\(", txt)))


# header -> (the name of its table in _abi, the sorted names it declares)
PINNED = {
    "mpc_hip.h": ("PROTOTYPES", _declared_functions()),
    "mpc_fleet.h": ("FLEET_PROTOTYPES", ["mpc_fleet_pool", "mpc_fleet_pool_device", "mpc_obstacles_from_pool", "mpc_obstacles_from_pool_device", "mpc_pool_params_defaults"]),
    "mpc_costmap_clusters.h": ("CLUSTER_PROTOTYPES", ["mpc_cluster_params_defaults", "mpc_costmap_to_polygons", "mpc_costmap_to_polygons_device", "mpc_last_costmap_ms"]),
    "mpc_costmap_lines.h": ("LINE_PROTOTYPES", ["mpc_costmap_to_lines", "mpc_costmap_to_lines_device", "mpc_line_params_defaults"]),
    "mpc_costmap_window.h": ("WINDOW_PROTOTYPES", ["mpc_costmap_window", "mpc_costmap_window_device", "mpc_window_params_defaults"]),
}


def test_header_functions_all_exported(lib):
    names = _declared_functions()
    assert set(names) == set(_lib.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n


def test_the_registry_is_the_five_tables_and_they_are_disjoint():
    assert list(HEADERS) == list(PINNED) and all(HEADERS[h][0] is getattr(_abi, t) for h, (t, _) in PINNED.items())
    assert len(PINNED[K.MAIN][1]) == len(PROTOTYPES) == 37 and _lib.EXPORTS == list(PROTOTYPES)
    assert sum(len(t) for t, _ in HEADERS.values()) == len(set().union(*(t for t, _ in HEADERS.values()))) == 52


# ---- every prototype of every table against its declaration --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", list(HEADERS))
def test_every_prototype_matches_its_declaration(header):
    table, mirrors = HEADERS[header]
    text = K.header_text(header)
    assert sorted(K.declarations(text)) == sorted(table) == PINNED[header][1]
    assert K.mismatches(header, table) == []
    assert sorted(re.findall(r"typedef struct (\w+) \{", text)) == sorted(mirrors)      # no struct of the header without its mirror


def test_spot_pins():
    """single rows, by hand: the comparator's rule and the tables agree with what callers pass"""
    from mpc_local_planner_amd._abi import MpcClusterParams, MpcEvalOut, MpcLineParams, MpcPool, MpcWindowParams
    assert C.c_int is C.c_int32 and PROTOTYPES["mpc_evaluate_batch"][1][10] is C.POINTER(MpcEvalOut) and PROTOTYPES["mpc_grid_update_device"][1][9] is C.c_double
    assert len(FLEET_PROTOTYPES["mpc_fleet_pool_device"][1]) == 13 and FLEET_PROTOTYPES["mpc_obstacles_from_pool"][1][2] is C.POINTER(MpcPool)
    poly, lines, window = (t[n][1] for t, n in ((CLUSTER_PROTOTYPES, "mpc_costmap_to_polygons_device"), (LINE_PROTOTYPES, "mpc_costmap_to_lines_device"),
                                                (WINDOW_PROTOTYPES, "mpc_costmap_window_device")))
    assert poly[8] is C.POINTER(MpcClusterParams) and len(poly) == 16
    assert lines[8] is C.POINTER(MpcLineParams) and len(lines) == 16
    assert window[3] is C.POINTER(MpcWindowParams) and len(window) == 11
    assert lines[:8] == poly[:8] and lines[9:] == poly[9:]      # the argument lists of the line step mirror the polygon step's, the params struct aside


# the comparator reports each of these, and nothing else: it cannot pass by seeing nothing, and it accepts one object per parameter.
# (header, function, parameter, bound as, the report); parameter None: the last one dropped; MISSING: the function taken out of the table
MISSING = "missing"
_OBSTACLES, _I32P = C.POINTER(_abi.MpcObstacles), C.POINTER(C.c_int32)
CORRUPTED = [
    ("mpc_hip.h", "mpc_step_batch", None, None, "mpc_step_batch: 21 parameters declared, 20 bound"),
    ("mpc_hip.h", "mpc_grid_update_device", 9, C.c_int32, f"mpc_grid_update_device: parameter 9 is double dt_hyst_ratio, bound as {C.c_int32}"),
    ("mpc_hip.h", "mpc_synchronize", MISSING, None, "mpc_synchronize: declared, not in the table"),
    ("mpc_hip.h", "mpc_evaluate_batch", 10, C.c_void_p, f"mpc_evaluate_batch: parameter 10 is mpc_eval_out* out, bound as {C.c_void_p}"),      # callers pass byref(MpcEvalOut)
    ("mpc_hip.h", "mpc_create", 0, C.c_void_p, f"mpc_create: parameter 0 is mpc_config* cfg, bound as {C.c_void_p}"),
    ("mpc_hip.h", "mpc_occupancy", 2, C.c_void_p, f"mpc_occupancy: parameter 2 is int32_t* workgroups_per_cu, bound as {C.c_void_p}"),
    ("mpc_hip.h", "mpc_get_grid_sizes", 2, _I32P, f"mpc_get_grid_sizes: parameter 2 is int32_t* n_grid, bound as {_I32P}"),
    ("mpc_hip.h", "mpc_solve_batch", 9, _OBSTACLES, f"mpc_solve_batch: parameter 9 is mpc_obstacles* obstacles, bound as {_OBSTACLES}"),
    ("mpc_fleet.h", "mpc_fleet_pool_device", 6, C.c_int32, f"mpc_fleet_pool_device: parameter 6 is double robot_radius, bound as {C.c_int32}"),
    ("mpc_fleet.h", "mpc_obstacles_from_pool", 2, C.c_void_p, f"mpc_obstacles_from_pool: parameter 2 is mpc_pool* pool, bound as {C.c_void_p}"),
    ("mpc_fleet.h", "mpc_fleet_pool", MISSING, None, "mpc_fleet_pool: declared, not in the table"),
    ("mpc_costmap_clusters.h", "mpc_costmap_to_polygons_device", 5, C.c_int32, f"mpc_costmap_to_polygons_device: parameter 5 is double resolution, bound as {C.c_int32}"),
    ("mpc_costmap_clusters.h", "mpc_costmap_to_polygons", 8, C.c_void_p, f"mpc_costmap_to_polygons: parameter 8 is mpc_cluster_params* params, bound as {C.c_void_p}"),
    ("mpc_costmap_clusters.h", "mpc_last_costmap_ms", MISSING, None, "mpc_last_costmap_ms: declared, not in the table"),
    ("mpc_costmap_lines.h", "mpc_costmap_to_lines", 8, C.c_void_p, f"mpc_costmap_to_lines: parameter 8 is mpc_line_params* params, bound as {C.c_void_p}"),
    ("mpc_costmap_window.h", "mpc_costmap_window_device", 7, C.c_int32, f"mpc_costmap_window_device: parameter 7 is double resolution, bound as {C.c_int32}"),
    ("mpc_costmap_window.h", "mpc_costmap_window", 3, C.c_void_p, f"mpc_costmap_window: parameter 3 is mpc_window_params* params, bound as {C.c_void_p}"),
    ("mpc_costmap_window.h", "mpc_window_params_defaults", MISSING, None, "mpc_window_params_defaults: declared, not in the table"),
]


@pytest.mark.parametrize("header,function,index,bound,report", CORRUPTED, ids=[f"{r[1]}-{r[2]}" for r in CORRUPTED])
def test_the_comparator_reports_a_corrupted_table(header, function, index, bound, report):
    table = dict(HEADERS[header][0])
    restype, argtypes = table.pop(function)
    if index != MISSING:
        table[function] = (restype, argtypes[:-1] if index is None else argtypes[:index] + [bound] + argtypes[index + 1:])
    assert K.mismatches(header, table) == [report]


@pytest.mark.parametrize("header", K.SIDE)
def test_mpc_hip_h_declares_nothing_of_a_side_header(header):
    """a side header's functions and structs are declared there alone; include/mpc_hip.h keeps its 37 declarations and does not know the side header"""
    table, mirrors = HEADERS[header]
    hip_text = K.header_text(K.MAIN)
    hip = K.header_code(hip_text)
    for name in list(table) + list(mirrors):
        assert not re.search(r"\b%s\b" % name, hip), name
    assert len(K.declarations(hip_text)) == 37
    assert '#include "mpc_hip.h"' in K.header_text(header) and header[:-len(".h")] not in hip_text


# ---- every mirrored struct against the C compiler's layout ----------------------------------------------------------------------------------------------------------------
# struct -> (the field names or their number, sizeof, the enumerators that ride with it: C name -> the Python constant of _abi); None: not pinned here
LAYOUTS = {
    "mpc_config": (None, None, {}),
    "mpc_obstacles": (5, None, {}),
    "mpc_eval_out": (5, None, {}),
    "mpc_cycle_params": (14, None, {f"MPC_REINIT_{k}": f"REINIT_{k}" for k in ("FIRST", "NUM_STEPS", "GOAL_DIST", "GOAL_ANGULAR", "RESET", "PLAN_GUESS")}),
    "mpc_plan_params": (10, None, {**{f"MPC_PLAN_{k}": f"PLAN_{k}" for k in ("GOAL_REACHED", "EMPTY", "TRUNCATED", "VIA_DROPPED", "GOAL_INJECTED")},
                                   **{f"MPC_CMD_{k}": f"CMD_{k}" for k in ("SUCCESS", "GOAL_REACHED", "PLAN_EMPTY", "SOLVE_FAILED", "INFEASIBLE", "NOT_FINITE")}}),
    "mpc_pool": (5, None, {}),
    "mpc_pool_params": (3, None, {}),
    "mpc_cluster_params": (["behind_robot_dist", "link_dist_sq"], None, {}),
    "mpc_line_params": (["behind_robot_dist", "link_dist_sq", "inlier_dist_sq", "min_inliers", "n_hypotheses", "remaining_outliers"], 32, {}),
    "mpc_window_params": (["map_origin", "map_resolution", "lattice_anchor", "inscribed_radius", "inflation_radius", "cost_scaling_factor", "map_size_x", "map_size_y",
                           "outside_value", "inflate_unknown"], 80, {}),
}


def test_every_struct_of_the_registry_has_its_pins():
    assert sorted(s for _, s in STRUCTS) == sorted(LAYOUTS) and len(LAYOUTS) == 10


@pytest.mark.parametrize("header,struct", STRUCTS, ids=[s for _, s in STRUCTS])
def test_struct_layout_matches_c(header, struct, tmp_path):
    """sizeof, every offsetof and the field names in header order of the ctypes mirror, against the C compiler (every header compiles as C); and the enumerators that
    belong to the struct's calls"""
    mirror = HEADERS[header][1][struct]
    pinned, size, enums = LAYOUTS[struct]
    fields = [f[0] for f in mirror._fields_]
    assert fields == K.struct_fields(header, struct) and pinned in (None, len(fields), fields)
    out = K.c_layout(header, struct, fields, enums, tmp_path)
    assert len(out) == 1 + len(fields) + len(enums) and out[0] == C.sizeof(mirror) and size in (None, out[0])
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f
    assert out[1 + len(fields):] == [getattr(_abi, v) for v in enums.values()]


@pytest.mark.parametrize("header", list(HEADERS))
def test_library_exports_and_binds_every_prototype(header, lib):
    table = HEADERS[header][0]
    assert len(_lib.EXPORTS) == 37 and (header == K.MAIN or not set(table) & set(_lib.EXPORTS))
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert lib.mpc_version() == 900


def test_defaults_match_reference_in_code_defaults(lib):
    from mpc_local_planner_amd._abi import MpcConfig
    c = MpcConfig()
    lib.mpc_config_defaults(C.byref(c))
    # src/controller.cpp:274,278,236,282,391,346
    assert c.n == 20 and c.dt_ref == pytest.approx(0.3) and c.dt_free == 1
    assert list(c.xf_fixed) == [1, 1, 1] and c.max_iter == 100 and c.model == 0
    assert c.du_lb[0] < -1e29 and c.du_ub[1] > 1e29
    assert lib.mpc_version() >= 100


def test_invalid_config_rejected(lib):
    from mpc_local_planner_amd._abi import config_carlike_min_time, MPC_EINVAL
    h = C.c_void_p()
    bad = config_carlike_min_time(n=2)
    assert lib.mpc_create(C.byref(bad), 4, 0, C.byref(h)) == MPC_EINVAL
    assert b"n out of range" in lib.mpc_last_error()
    bad = config_carlike_min_time(n=20)
    bad.collocation = 7          # unknown method (0 forward, 1 midpoint, 2 Crank-Nicolson exist)
    assert lib.mpc_create(C.byref(bad), 4, 0, C.byref(h)) == MPC_EINVAL
    bad = config_carlike_min_time(n=20)
    bad.dt_free = 0
    assert lib.mpc_create(C.byref(bad), 4, 0, C.byref(h)) == MPC_EINVAL


def test_per_instance_int32_arrays_are_checked():
    """what controller_step's n_plan / reset, plan_inputs' n_global and commands' arrays go through: a wrong size raises, it is not read out of bounds"""
    from mpc_local_planner_amd.solver import _as_i32
    assert _as_i32(None, 4) is None and _as_i32([1, 2, 3, 4], 4).dtype == np.int32 and _as_i32(np.ones((4, 1)), 4).shape == (4,)
    with pytest.raises(ValueError, match=r"n_plan must have shape \(B,\)"):
        _as_i32(np.zeros(3), 4, "n_plan")
    with pytest.raises(ValueError):      # reset of controller_step: numpy's own message
        _as_i32(np.zeros(3, np.int32), 4)


def test_parameter_structs_are_the_defaults_then_the_given_fields(lib):
    """what cycle_params, plan_params, pool_params and window_params go through: the caller's defaults call, then the fields; an unknown field raises by the struct's name"""
    from mpc_local_planner_amd._abi import MpcCycleParams, MpcPoolParams
    from mpc_local_planner_amd.solver import _params
    ref, p = MpcCycleParams(), _params("mpc_cycle_params", MpcCycleParams, lib.mpc_cycle_params_defaults, {"n_min": 7})
    lib.mpc_cycle_params_defaults(C.byref(ref))
    assert p.n_min == 7 and [getattr(p, f) for f, _ in p._fields_ if f != "n_min"] == [getattr(ref, f) for f, _ in p._fields_ if f != "n_min"]
    q = _params("mpc_pool_params", MpcPoolParams, lambda p: lib.mpc_pool_params_defaults(None, p), {"append": 0})
    assert (q.reach, q.min_speed, q.append) == (0.0, 0.001, 0)
    with pytest.raises(ValueError, match="^mpc_pool_params has no field bogus$"):
        _params("mpc_pool_params", MpcPoolParams, lambda p: lib.mpc_pool_params_defaults(None, p), {"bogus": 1})


def test_no_gpu_means_loud_failure_not_cpu_fallback(lib):
    """In the CPU-only container mpc_create must return MPC_ENODEV (the product has no CPU path)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the -m gpu tests")
    from mpc_local_planner_amd import BatchSolver, MpcError, config_carlike_min_time
    from mpc_local_planner_amd._abi import MPC_ENODEV
    with pytest.raises(MpcError) as ei:
        BatchSolver(config_carlike_min_time(20), max_batch=4)
    assert ei.value.code == MPC_ENODEV
    assert "no CPU fallback" in str(ei.value)


def test_product_package_does_not_import_the_oracle():
    code = ("import sys; import mpc_local_planner_amd; "
            "bad=[m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; print(bad); sys.exit(1 if bad else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for dirpath, _, files in os.walk(os.path.join(ROOT, "mpc_local_planner_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "oracle/" not in txt.replace("oracle/se2_nlp.py)", ""), f


def test_workloads_are_deterministic_and_in_range():
    from mpc_local_planner_amd import workloads as W
    a = W.carlike_min_time_inputs(64)
    b = W.carlike_min_time_inputs(64)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(p, q)
    x0, xf, up, dtp = a
    r = np.hypot(xf[:, 0], xf[:, 1])
    assert r.min() >= 1.0 and r.max() <= 6.0
    assert up[:, 0].min() >= -0.2 and up[:, 0].max() <= 0.4 and np.abs(up[:, 1]).max() <= 0.5
    assert (dtp == 0.2).all()
    c = W.carlike_min_time_inputs(64, seed=W.SEED_CONFIG2 + 1)
    assert not np.array_equal(c[0], a[0])
