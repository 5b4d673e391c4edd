"""CPU tests of the boundary of include/mpc_fleet.h: every declaration against _abi.FLEET_PROTOTYPES, parameter by parameter (the comparator of tests/test_abi.py with the
two structs of this header added); the ctypes mirrors of mpc_pool and mpc_pool_params against the C compiler's sizeof / offsetof; the library exports and binds every name;
and include/mpc_hip.h, whose declarations and prototype table tests/test_abi.py pins, declares none of them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

import test_abi as A

ROOT = A.ROOT
HEADER = os.path.join(ROOT, "include", "mpc_fleet.h")
NAMES = ["mpc_fleet_pool", "mpc_fleet_pool_device", "mpc_obstacles_from_pool", "mpc_obstacles_from_pool_device", "mpc_pool_params_defaults"]
MIRRORS = {"mpc_pool": "MpcPool", "mpc_pool_params": "MpcPoolParams"}


def _bound(function, ctype, name=None):
    """the rule of tests/test_abi.py, with this header's structs bound as pointers to their mirrors"""
    from mpc_local_planner_amd import _abi
    if name is not None and ctype.endswith("*") and ctype[:-1] in MIRRORS:
        return C.POINTER(getattr(_abi, MIRRORS[ctype[:-1]]))
    return A._bound(function, ctype, name)


def _mismatches(header_text, table):
    decl = A._declarations(header_text)
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


def test_every_fleet_prototype_matches_its_declaration():
    from mpc_local_planner_amd._abi import FLEET_PROTOTYPES, PROTOTYPES, MpcPool
    header = open(HEADER).read()
    assert sorted(A._declarations(header)) == sorted(FLEET_PROTOTYPES) == NAMES
    assert _mismatches(header, FLEET_PROTOTYPES) == []
    assert not set(FLEET_PROTOTYPES) & set(PROTOTYPES) and len(PROTOTYPES) == 37
    # the comparator sees what it is there to see
    restype, argtypes = FLEET_PROTOTYPES["mpc_fleet_pool_device"]
    assert _mismatches(header, {**FLEET_PROTOTYPES, "mpc_fleet_pool_device": (restype, argtypes[:6] + [C.c_int32] + argtypes[7:])}) == \
        [f"mpc_fleet_pool_device: parameter 6 is double robot_radius, bound as {C.c_int32}"]
    restype, argtypes = FLEET_PROTOTYPES["mpc_obstacles_from_pool"]
    assert _mismatches(header, {**FLEET_PROTOTYPES, "mpc_obstacles_from_pool": (restype, argtypes[:2] + [C.c_void_p] + argtypes[3:])}) == \
        [f"mpc_obstacles_from_pool: parameter 2 is mpc_pool* pool, bound as {C.c_void_p}"]
    assert _mismatches(header, {k: v for k, v in FLEET_PROTOTYPES.items() if k != "mpc_fleet_pool"}) == ["mpc_fleet_pool: declared, not in the table"]
    assert argtypes[2] is C.POINTER(MpcPool) and len(argtypes) == 13


def test_mpc_hip_h_declares_none_of_the_fleet_names():
    hip = A._header_code(open(A.HEADER).read())
    for name in NAMES + list(MIRRORS):
        assert not re.search(r"\b%s\b" % name, hip), name
    assert len(A._declarations(open(A.HEADER).read())) == 37
    assert '#include "mpc_hip.h"' in open(HEADER).read()


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), A._header_code(open(HEADER).read()), flags=re.S).group(1)
    return [re.search(r"(\w+)\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")]


@pytest.mark.parametrize("struct,count", [("mpc_pool", 5), ("mpc_pool_params", 3)])
def test_fleet_struct_layout_matches_c(struct, count, tmp_path):
    """sizeof, every offsetof and the field names in header order of the ctypes mirror, against the C compiler (the header compiles as C)"""
    from mpc_local_planner_amd import _abi
    mirror = getattr(_abi, MIRRORS[struct])
    fields = [f[0] for f in mirror._fields_]
    assert fields == _fields(struct) and len(fields) == count
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_fleet.h"\nint main(){\nprintf("%%zu\\n", sizeof(%s));\n' % struct +
                   "".join('printf("%%zu\\n", offsetof(%s,%s));\n' % (struct, f) for f in fields) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(out) == 1 + len(fields) and out[0] == C.sizeof(mirror)
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f


def test_library_exports_and_binds_the_fleet_functions():
    from mpc_local_planner_amd import _lib
    from mpc_local_planner_amd._abi import FLEET_PROTOTYPES, MPC_EINVAL, MpcPoolParams
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    lib = _lib.load()
    assert len(_lib.EXPORTS) == 37 and not set(NAMES) & set(_lib.EXPORTS)
    for name, (restype, argtypes) in FLEET_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    # without a handle: the defaults that do not depend on one, and a refusal instead of a crash
    p = MpcPoolParams(-1.0, -1.0, -1)
    lib.mpc_pool_params_defaults(None, C.byref(p))
    assert (p.reach, p.min_speed, p.append) == (0.0, 0.001, 1)
    assert lib.mpc_obstacles_from_pool_device(None, 1, None, None, None, None, None, None, None, None, None, None, None) == MPC_EINVAL
    assert lib.mpc_fleet_pool(None, 1, None, None, None, None, 0.2, None, 0, None, None, None, None) == MPC_EINVAL
    assert b"mpc_fleet_pool: null argument" in lib.mpc_last_error()
    assert lib.mpc_version() == 900
