"""CPU tests of the boundary of include/mpc_costmap_lines.h: every declaration against _abi.LINE_PROTOTYPES, parameter by parameter (the comparator of
tests/test_costmap_clusters_abi.py with this header's struct); the ctypes mirror of mpc_line_params against the C compiler's sizeof / offsetof; the library exports and
binds every name, gives the stated defaults and refuses without a GPU what it can refuse without one; and include/mpc_hip.h, whose declarations tests/test_abi.py pins at
37, declares none of them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import test_abi as A
import test_costmap_clusters_abi as CA

ROOT = A.ROOT
HEADER = os.path.join(ROOT, "include", "mpc_costmap_lines.h")
NAMES = ["mpc_costmap_to_lines", "mpc_costmap_to_lines_device", "mpc_line_params_defaults"]
FIELDS = ["behind_robot_dist", "link_dist_sq", "inlier_dist_sq", "min_inliers", "n_hypotheses", "remaining_outliers"]


def test_every_line_prototype_matches_its_declaration(monkeypatch):
    from mpc_local_planner_amd._abi import CLUSTER_PROTOTYPES, FLEET_PROTOTYPES, LINE_PROTOTYPES, PROTOTYPES, MpcLineParams
    monkeypatch.setitem(CA.MIRRORS, "mpc_line_params", "MpcLineParams")
    header = open(HEADER).read()
    assert sorted(A._declarations(header)) == sorted(LINE_PROTOTYPES) == NAMES
    assert CA._mismatches(header, LINE_PROTOTYPES) == []
    assert not set(LINE_PROTOTYPES) & (set(PROTOTYPES) | set(FLEET_PROTOTYPES) | set(CLUSTER_PROTOTYPES)) and len(PROTOTYPES) == 37
    # the comparator sees what it is there to see
    restype, argtypes = LINE_PROTOTYPES["mpc_costmap_to_lines_device"]
    assert CA._mismatches(header, {**LINE_PROTOTYPES, "mpc_costmap_to_lines": (restype, argtypes[:8] + [C.c_void_p] + argtypes[9:])}) == \
        [f"mpc_costmap_to_lines: parameter 8 is mpc_line_params* params, bound as {C.c_void_p}"]
    assert argtypes[8] is C.POINTER(MpcLineParams) and len(argtypes) == 16
    # the argument lists mirror the polygon step's, the params struct aside
    poly = CLUSTER_PROTOTYPES["mpc_costmap_to_polygons_device"][1]
    assert argtypes[:8] == poly[:8] and argtypes[9:] == poly[9:]


def test_mpc_hip_h_declares_none_of_the_line_names():
    hip_text = open(A.HEADER).read()
    hip = A._header_code(hip_text)
    for name in NAMES + ["mpc_line_params"]:
        assert not re.search(r"\b%s\b" % name, hip), name
    assert len(A._declarations(hip_text)) == 37
    assert '#include "mpc_hip.h"' in open(HEADER).read() and "mpc_costmap_lines" not in hip_text


def test_line_struct_layout_matches_c(tmp_path):
    """sizeof, every offsetof and the field names in header order of the ctypes mirror, against the C compiler (the header compiles as C)"""
    from mpc_local_planner_amd._abi import MpcLineParams as mirror
    struct = "mpc_line_params"
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), A._header_code(open(HEADER).read()), flags=re.S).group(1)
    fields = [f[0] for f in mirror._fields_]
    assert fields == [re.search(r"(\w+)\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")] == FIELDS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_costmap_lines.h"\nint main(){\nprintf("%%zu\\n", sizeof(%s));\n' % struct +
                   "".join('printf("%%zu\\n", offsetof(%s,%s));\n' % (struct, f) for f in fields) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(out) == 1 + len(fields) and out[0] == C.sizeof(mirror) == 32
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f


def test_library_exports_binds_and_refuses_without_a_gpu():
    from mpc_local_planner_amd import _lib
    from mpc_local_planner_amd._abi import LINE_PROTOTYPES, MPC_EINVAL, MpcLineParams
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    lib = _lib.load()
    assert len(_lib.EXPORTS) == 37 and not set(NAMES) & set(_lib.EXPORTS)
    for name, (restype, argtypes) in LINE_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    # the defaults need no handle: the shipped block at 0.05 m per cell, the clamps at both ends, the floor in between, quotients that are not numbers
    p = MpcLineParams(-1.0, -1, -1, -1, -1, -1)
    for res, d, inl, want in ((0.05, 0.4, 0.15, (64, 9)), (0.025, 0.4, 0.4, (64, 64)), (0.05, 0.01, 0.01, (1, 0)), (0.05, 0.1, 0.1, (4, 4)), (0.05, 0.12, 0.12, (5, 5)),
                              (0.1, 0.3, 0.15, (9, 2)), (0.05, 0.4, 0.0, (64, 0)), (0.05, 0.4, 0.05, (64, 1)), (0.0, 0.0, 0.0, (1, 0))):
        lib.mpc_line_params_defaults(C.byref(p), res, d, inl)
        assert (p.behind_robot_dist, p.link_dist_sq, p.inlier_dist_sq, p.min_inliers, p.n_hypotheses, p.remaining_outliers) == (1.5,) + want + (10, 1500, 3), (res, d, inl)
    lib.mpc_line_params_defaults(None, 0.05, 0.4, 0.15)
    # without a handle: a refusal instead of a crash
    assert lib.mpc_costmap_to_lines_device(None, 1, None, 8, 8, 0.05, None, None, None, None, None, None, None, None, None, None) == MPC_EINVAL
    assert lib.mpc_costmap_to_lines(None, 1, None, 8, 8, 0.05, None, None, C.byref(p), None, None, None, None, None, None, None) == MPC_EINVAL
    assert b"mpc_costmap_to_lines: null argument" in lib.mpc_last_error()
    assert lib.mpc_version() == 900
