"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every symbol that
include/mpc_hip.h declares, the ctypes mirror of mpc_config has the C layout, and -- without a GPU --
mpc_create fails loudly instead of falling back to a CPU path.  No compute calls here."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mpc_hip.h")


@pytest.fixture(scope="module")
def lib():
    from mpc_local_planner_amd import _lib
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    return _lib.load()


def _declared_functions():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mpc_[a-z_0-9]+)\s*\(", txt)))


def test_header_functions_all_exported(lib):
    from mpc_local_planner_amd import _lib
    names = _declared_functions()
    assert set(names) == set(_lib.EXPORTS)
    for n in names:
        assert hasattr(lib, n), n


# ---- every prototype of _abi.PROTOTYPES against its declaration -----------------------------------------------------------------------------------------------------
STRUCT_MIRRORS = {"mpc_config": "MpcConfig", "mpc_obstacles": "MpcObstacles", "mpc_eval_out": "MpcEvalOut", "mpc_cycle_params": "MpcCycleParams", "mpc_plan_params": "MpcPlanParams"}


def _header_code(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _declarations(text):
    """{name: (return type, [(parameter type, parameter name), ...])} of every `ret name(params);` of the header, types without const"""
    def ctype(words):
        return " ".join(w for w in words if w != "const").replace(" *", "*")
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(mpc_\w+)\s*\(([^)]*)\)\s*;", _header_code(text)):
        params = [p.replace("*", " * ").split() for p in params.split(",")]
        out[name] = (ctype(ret.replace("*", " * ").split()), [] if params == [["void"]] else [(ctype(p[:-1]), p[-1]) for p in params])
    return out


# where the binding deviates from the rule of _bound (found by the comparator when the table or the header changes; kept as the parent's load() had them)
VOID_STRUCTS = ("mpc_obstacles",)                                            # const mpc_obstacles* is bound as c_void_p everywhere: callers pass byref() or NULL
EXCEPTIONS = {("mpc_set_parameter_sets", "sets"): C.c_void_p,                # an array of mpc_config, passed as a cast address
              ("mpc_occupancy", "workgroups_per_cu"): C.POINTER(C.c_int32)}  # the one int32_t* that is a byref() scalar and not an array


def _bound(function, ctype, name=None):
    """THE ctypes object a return value (name None) or a parameter of this C type is bound as: exactly one"""
    from mpc_local_planner_amd import _abi
    if (function, name) in EXCEPTIONS:
        return EXCEPTIONS[function, name]
    if ctype in ("double", "int32_t", "int"):
        return C.c_double if ctype == "double" else C.c_int32      # (c_int32 is c_int here: one object)
    if name is None:
        return {"void": None, "char*": C.c_char_p}[ctype]
    assert ctype.endswith("*"), ctype
    base = ctype[:-1]
    if base in STRUCT_MIRRORS and base not in VOID_STRUCTS:
        return C.POINTER(getattr(_abi, STRUCT_MIRRORS[base]))
    return {"mpc_solver*": C.POINTER(C.c_void_p), "float": C.POINTER(C.c_float), "int64_t": C.POINTER(C.c_int64)}.get(base, C.c_void_p)


def abi_mismatches(header_text, table):
    """what differs between the header's declarations and a prototype table: a function of the two alone"""
    decl = _declarations(header_text)
    bad = [f"{n}: declared, not in the table" for n in sorted(set(decl) - set(table))] + [f"{n}: in the table, not declared" for n in sorted(set(table) - set(decl))]
    for name in sorted(set(decl) & set(table)):
        (ret, params), (restype, argtypes) = decl[name], table[name]
        if restype is not _bound(name, ret):
            bad.append(f"{name}: returns {ret}, bound as {restype}")
        if len(params) != len(argtypes):
            bad.append(f"{name}: {len(params)} parameters declared, {len(argtypes)} bound")
            continue
        bad += [f"{name}: parameter {i} is {t} {p}, bound as {a}" for i, ((t, p), a) in enumerate(zip(params, argtypes)) if a is not _bound(name, t, p)]
    return bad


def _with(table, function, index, bound):
    """a copy of the table with one parameter of one function bound differently (index None: the parameter dropped)"""
    restype, argtypes = table[function]
    return {**table, function: (restype, argtypes[:-1] if index is None else argtypes[:index] + [bound] + argtypes[index + 1:])}


def test_every_prototype_matches_its_declaration():
    from mpc_local_planner_amd._abi import PROTOTYPES, MpcEvalOut, MpcObstacles
    header = open(HEADER).read()
    assert len(_declarations(header)) == len(PROTOTYPES) == 37 and set(_declarations(header)) == set(_declared_functions())
    assert abi_mismatches(header, PROTOTYPES) == []
    assert C.c_int is C.c_int32 and PROTOTYPES["mpc_evaluate_batch"][1][10] is C.POINTER(MpcEvalOut) and PROTOTYPES["mpc_grid_update_device"][1][9] is C.c_double
    # the comparator reports each of these, and nothing else: it cannot pass by seeing nothing, and it accepts one object per parameter
    corrupted = [
        (_with(PROTOTYPES, "mpc_step_batch", None, None), "mpc_step_batch: 21 parameters declared, 20 bound"),
        (_with(PROTOTYPES, "mpc_grid_update_device", 9, C.c_int32), f"mpc_grid_update_device: parameter 9 is double dt_hyst_ratio, bound as {C.c_int32}"),
        ({k: v for k, v in PROTOTYPES.items() if k != "mpc_synchronize"}, "mpc_synchronize: declared, not in the table"),
        (_with(PROTOTYPES, "mpc_evaluate_batch", 10, C.c_void_p), f"mpc_evaluate_batch: parameter 10 is mpc_eval_out* out, bound as {C.c_void_p}"),      # callers pass byref(MpcEvalOut)
        (_with(PROTOTYPES, "mpc_create", 0, C.c_void_p), f"mpc_create: parameter 0 is mpc_config* cfg, bound as {C.c_void_p}"),
        (_with(PROTOTYPES, "mpc_occupancy", 2, C.c_void_p), f"mpc_occupancy: parameter 2 is int32_t* workgroups_per_cu, bound as {C.c_void_p}"),
        (_with(PROTOTYPES, "mpc_get_grid_sizes", 2, C.POINTER(C.c_int32)), f"mpc_get_grid_sizes: parameter 2 is int32_t* n_grid, bound as {C.POINTER(C.c_int32)}"),
        (_with(PROTOTYPES, "mpc_solve_batch", 9, C.POINTER(MpcObstacles)), f"mpc_solve_batch: parameter 9 is mpc_obstacles* obstacles, bound as {C.POINTER(MpcObstacles)}"),
    ]
    for table, report in corrupted:
        assert abi_mismatches(header, table) == [report]


# ---- every mirrored struct against the C compiler's layout ----------------------------------------------------------------------------------------------------------------
# struct -> (number of fields, the enumerators that ride with it: C name -> the Python constant of _abi)
LAYOUTS = {
    "mpc_config": (None, {}),
    "mpc_obstacles": (5, {}),
    "mpc_eval_out": (5, {}),
    "mpc_cycle_params": (14, {f"MPC_REINIT_{k}": f"REINIT_{k}" for k in ("FIRST", "NUM_STEPS", "GOAL_DIST", "GOAL_ANGULAR", "RESET", "PLAN_GUESS")}),
    "mpc_plan_params": (10, {**{f"MPC_PLAN_{k}": f"PLAN_{k}" for k in ("GOAL_REACHED", "EMPTY", "TRUNCATED", "VIA_DROPPED", "GOAL_INJECTED")},
                             **{f"MPC_CMD_{k}": f"CMD_{k}" for k in ("SUCCESS", "GOAL_REACHED", "PLAN_EMPTY", "SOLVE_FAILED", "INFEASIBLE", "NOT_FINITE")}}),
}


def _header_fields(struct):
    """the field names of `typedef struct <struct> {...} <struct>;` in header order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header_code(open(HEADER).read()), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]      # `double Q[3], R[2]` -> Q, R


@pytest.mark.parametrize("struct", sorted(LAYOUTS))
def test_struct_layout_matches_c(struct, tmp_path):
    """sizeof, every offsetof and the field names in header order of the ctypes mirror, against the C compiler; and the enumerators that belong to the struct's calls"""
    from mpc_local_planner_amd import _abi
    mirror = getattr(_abi, STRUCT_MIRRORS[struct])
    count, enums = LAYOUTS[struct]
    fields = [f[0] for f in mirror._fields_]
    assert fields == _header_fields(struct) and (count is None or len(fields) == count)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_hip.h"\nint main(){\nprintf("%%zu\\n", sizeof(%s));\n' % struct +
                   "".join('printf("%%zu\\n", offsetof(%s,%s));\n' % (struct, f) for f in fields) + "".join('printf("%%d\\n", %s);\n' % e for e in enums) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(out) == 1 + len(fields) + len(enums) and out[0] == C.sizeof(mirror)
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f
    assert out[1 + len(fields):] == [getattr(_abi, v) for v in enums.values()]


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
