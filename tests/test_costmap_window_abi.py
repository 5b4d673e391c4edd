"""CPU tests of the boundary of include/mpc_costmap_window.h: every declaration against _abi.WINDOW_PROTOTYPES, parameter by parameter (the comparator of
tests/test_costmap_clusters_abi.py with this header's struct); the ctypes mirror of mpc_window_params against the C compiler's sizeof / offsetof; the library exports
and binds every name, gives the stated defaults and refuses without a GPU what it can refuse without one; and include/mpc_hip.h, whose declarations tests/test_abi.py
pins at 37, declares none of them."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import test_abi as A
import test_costmap_clusters_abi as K

ROOT = A.ROOT
HEADER = os.path.join(ROOT, "include", "mpc_costmap_window.h")
NAMES = ["mpc_costmap_window", "mpc_costmap_window_device", "mpc_window_params_defaults"]
STRUCT, MIRROR = "mpc_window_params", "MpcWindowParams"
FIELDS = ["map_origin", "map_resolution", "lattice_anchor", "inscribed_radius", "inflation_radius", "cost_scaling_factor", "map_size_x", "map_size_y", "outside_value",
          "inflate_unknown"]


def _mismatches(header_text, table):
    """the comparator of tests/test_costmap_clusters_abi.py with this header's struct among its mirrors"""
    before = dict(K.MIRRORS)
    K.MIRRORS[STRUCT] = MIRROR
    try:
        return K._mismatches(header_text, table)
    finally:
        K.MIRRORS.clear()
        K.MIRRORS.update(before)


def test_every_window_prototype_matches_its_declaration():
    from mpc_local_planner_amd._abi import CLUSTER_PROTOTYPES, FLEET_PROTOTYPES, LINE_PROTOTYPES, PROTOTYPES, WINDOW_PROTOTYPES, MpcWindowParams
    header = open(HEADER).read()
    assert sorted(A._declarations(header)) == sorted(WINDOW_PROTOTYPES) == NAMES
    assert _mismatches(header, WINDOW_PROTOTYPES) == []
    assert not set(WINDOW_PROTOTYPES) & (set(PROTOTYPES) | set(FLEET_PROTOTYPES) | set(CLUSTER_PROTOTYPES) | set(LINE_PROTOTYPES)) and len(PROTOTYPES) == 37
    # the comparator sees what it is there to see
    restype, argtypes = WINDOW_PROTOTYPES["mpc_costmap_window_device"]
    assert _mismatches(header, {**WINDOW_PROTOTYPES, "mpc_costmap_window_device": (restype, argtypes[:7] + [C.c_int32] + argtypes[8:])}) == \
        [f"mpc_costmap_window_device: parameter 7 is double resolution, bound as {C.c_int32}"]
    assert _mismatches(header, {**WINDOW_PROTOTYPES, "mpc_costmap_window": (restype, argtypes[:3] + [C.c_void_p] + argtypes[4:])}) == \
        [f"mpc_costmap_window: parameter 3 is mpc_window_params* params, bound as {C.c_void_p}"]
    assert _mismatches(header, {k: v for k, v in WINDOW_PROTOTYPES.items() if k != "mpc_window_params_defaults"}) == ["mpc_window_params_defaults: declared, not in the table"]
    assert argtypes[3] is C.POINTER(MpcWindowParams) and len(argtypes) == 11
    # the chain comment is led by this step
    chain = header[:header.index("#ifndef")]
    assert 0 < chain.index("mpc_costmap_window_device") < chain.index("mpc_costmap_to_obstacles_device") < chain.index("mpc_controller_step_batch_device")


def test_mpc_hip_h_declares_none_of_the_window_names():
    hip = A._header_code(open(A.HEADER).read())
    for name in NAMES + [STRUCT]:
        assert not re.search(r"\b%s\b" % name, hip), name
    assert len(A._declarations(open(A.HEADER).read())) == 37
    assert '#include "mpc_hip.h"' in open(HEADER).read()


def test_window_struct_layout_matches_c(tmp_path):
    """sizeof, every offsetof and the field names in header order of the ctypes mirror, against the C compiler (the header compiles as C)"""
    from mpc_local_planner_amd._abi import MpcWindowParams as mirror
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (STRUCT, STRUCT), A._header_code(open(HEADER).read()), flags=re.S).group(1)
    fields = [f[0] for f in mirror._fields_]
    assert fields == [re.search(r"(\w+)\s*(\[\d+\])?\s*$", d).group(1) for decl in body.split(";") if decl.strip() for d in decl.split(",")] == FIELDS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpc_costmap_window.h"\nint main(){\nprintf("%%zu\\n", sizeof(%s));\n' % STRUCT +
                   "".join('printf("%%zu\\n", offsetof(%s,%s));\n' % (STRUCT, f) for f in fields) + 'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert len(out) == 1 + len(fields) and out[0] == C.sizeof(mirror) == 80
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f


def test_library_exports_binds_gives_the_defaults_and_refuses_without_a_gpu():
    from mpc_local_planner_amd import _lib
    from mpc_local_planner_amd._abi import MPC_EINVAL, WINDOW_PROTOTYPES, MpcWindowParams
    if shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc"):
        _lib.build()
    lib = _lib.load()
    assert len(_lib.EXPORTS) == 37 and not set(NAMES) & set(_lib.EXPORTS)
    for name, (restype, argtypes) in WINDOW_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    # the defaults as the header states them
    p = MpcWindowParams((C.c_double * 2)(7.0, 7.0), -1.0, (C.c_double * 2)(7.0, 7.0), -1.0, -1.0, -1.0, -1, -1, -1, -1)
    lib.mpc_window_params_defaults(C.byref(p), 0.05, 1200, 400)
    assert (tuple(p.map_origin), p.map_resolution, tuple(p.lattice_anchor), p.inscribed_radius, p.inflation_radius, p.cost_scaling_factor, p.map_size_x, p.map_size_y,
            p.outside_value, p.inflate_unknown) == ((0.0, 0.0), 0.05, (0.0, 0.0), 0.0, 0.0, 10.0, 1200, 400, 0, 0)
    lib.mpc_window_params_defaults(None, 0.05, 1, 1)
    # without a handle: a refusal instead of a crash, with its text
    for fn in (lib.mpc_costmap_window, lib.mpc_costmap_window_device):
        assert fn(None, 1, None, C.byref(p), None, 8, 8, 0.05, None, None, None) == MPC_EINVAL
        assert b"mpc_costmap_window: null argument" in lib.mpc_last_error()
        assert fn(None, 1, None, None, None, 8, 8, math.nan, None, None, None) == MPC_EINVAL
    assert lib.mpc_version() == 900
