"""CPU tests of the boundary of include/mpc_costmap_clusters.h: every declaration against _abi.CLUSTER_PROTOTYPES, parameter by parameter (the comparator of
tests/test_abi.py with the struct of this header added); the ctypes mirror of mpc_cluster_params against the C compiler's sizeof / offsetof; the library exports and binds
every name and refuses without a GPU what it can refuse without one; and include/mpc_hip.h, whose declarations tests/test_abi.py pins at 37, declares none of them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import test_abi as A

ROOT = A.ROOT
HEADER = os.path.join(ROOT, "include", "mpc_costmap_clusters.h")
NAMES = ["mpc_cluster_params_defaults", "mpc_costmap_to_polygons", "mpc_costmap_to_polygons_device", "mpc_last_costmap_ms"]
MIRRORS = {"mpc_cluster_params": "MpcClusterParams"}


def _bound(function, ctype, name=None):
    """the rule of tests/test_abi.py, with this header's struct bound as a pointer to its mirror"""
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


def test_every_cluster_prototype_matches_its_declaration():
    from mpc_local_planner_amd._abi import CLUSTER_PROTOTYPES, FLEET_PROTOTYPES, PROTOTYPES, MpcClusterParams
    header = open(HEADER).read()
    assert sorted(A._declarations(header)) == sorted(CLUSTER_PROTOTYPES) == NAMES
    assert _mismatches(header, CLUSTER_PROTOTYPES) == []
    assert not set(CLUSTER_PROTOTYPES) & (set(PROTOTYPES) | set(FLEET_PROTOTYPES)) and len(PROTOTYPES) == 37
    # the comparator sees what it is there to see
    restype, argtypes = CLUSTER_PROTOTYPES["mpc_costmap_to_polygons_device"]
    assert _mismatches(header, {**CLUSTER_PROTOTYPES, "mpc_costmap_to_polygons_device": (restype, argtypes[:5] + [C.c_int32] + argtypes[6:])}) == \
        [f"mpc_costmap_to_polygons_device: parameter 5 is double resolution, bound as {C.c_int32}"]
    assert _mismatches(header, {**CLUSTER_PROTOTYPES, "mpc_costmap_to_polygons": (restype, argtypes[:8] + [C.c_void_p] + argtypes[9:])}) == \
        [f"mpc_costmap_to_polygons: parameter 8 is mpc_cluster_params* params, bound as {C.c_void_p}"]
    assert _mismatches(header, {k: v for k, v in CLUSTER_PROTOTYPES.items() if k != "mpc_last_costmap_ms"}) == ["mpc_last_costmap_ms: declared, not in the table"]
    assert argtypes[8] is C.POINTER(MpcClusterParams) and len(argtypes) == 16


def test_mpc_hip_h_declares_none_of_the_cluster_names():
    hip = A._header_code(open(A.HEADER).read())
    for name in NAMES + list(MIRRORS):
        assert not re.search(r"\b%s\b" % name, hip), name
    assert len(A._declarations(open(A.HEADER).read())) == 37
    assert '#include "mpc_hip.h"' in open(HEADER).read()


def test_cluster_struct_layout_matches_c(tmp_path):
    """sizeof, every offsetof and the field names in header order of the ctypes mirror, against the C compiler (the header compiles as C)"""
    from mpc_local_planner_amd._abi import MpcClusterParams as mirror
    struct = "mpc_cluster_params"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), A._header_code(open(HEADER).read()), flags=re.S).group(1)
    fields = [f[0] for f in mirror._fields_]
    assert fields == [re.search(r"(\w+)\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")] == ["behind_robot_dist", "link_dist_sq"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_costmap_clusters.h"\nint main(){\nprintf("%%zu\\n", sizeof(%s));\n' % struct +
                   "".join('printf("%%zu\\n", offsetof(%s,%s));\n' % (struct, f) for f in fields) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(out) == 1 + len(fields) and out[0] == C.sizeof(mirror)
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f


def test_library_exports_binds_and_refuses_without_a_gpu():
    from mpc_local_planner_amd import _lib
    from mpc_local_planner_amd._abi import CLUSTER_PROTOTYPES, MPC_EINVAL, MpcClusterParams
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    lib = _lib.load()
    assert len(_lib.EXPORTS) == 37 and not set(NAMES) & set(_lib.EXPORTS)
    for name, (restype, argtypes) in CLUSTER_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    # the defaults need no handle: the shipped 0.4 m at 0.05 m per cell, the clamp at both ends, the floor in between, a quotient that is not a number
    p = MpcClusterParams(-1.0, -1)
    for res, d, want in ((0.05, 0.4, 64), (0.025, 0.4, 64), (0.05, 0.01, 1), (0.05, 0.1, 4), (0.05, 0.12, 5), (0.1, 0.3, 9), (0.0, 0.0, 1)):
        lib.mpc_cluster_params_defaults(C.byref(p), res, d)
        assert (p.behind_robot_dist, p.link_dist_sq) == (1.5, want), (res, d)
    lib.mpc_cluster_params_defaults(None, 0.05, 0.4)
    # without a handle: a refusal instead of a crash
    assert lib.mpc_costmap_to_polygons_device(None, 1, None, 8, 8, 0.05, None, None, None, None, None, None, None, None, None, None) == MPC_EINVAL
    assert lib.mpc_costmap_to_polygons(None, 1, None, 8, 8, 0.05, None, None, C.byref(p), None, None, None, None, None, None, None) == MPC_EINVAL
    assert b"mpc_costmap_to_polygons: null argument" in lib.mpc_last_error()
    assert lib.mpc_last_costmap_ms(None, None) == MPC_EINVAL
    assert lib.mpc_version() == 900
