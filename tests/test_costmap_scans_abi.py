"""CPU tests of include/mpc_costmap_scans.h at the drop-in boundary.  tests/test_abi.py pins _abi.HEADERS to the five headers and 52 functions it was written for, so
this header's row lives in _abi.LATER_HEADERS and is held here by the same means (tests/_abi_check.py): its declarations against _abi.SCAN_PROTOTYPES, the layout of
mpc_scan_params against the C compiler, the library's exports and the binding.  Then what is particular to it: its place in the fleet cycle's comment, the values of its
defaults, and what the library can refuse without a GPU."""
import ctypes as C
import math
import re

import pytest

import _abi_check as K
from _abi_check import lib      # noqa: F401 (the fixture)
from mpc_local_planner_amd import _abi, _lib

HEADER = "mpc_costmap_scans.h"
FIELDS = ["lattice_anchor", "sensor_pose", "angle_min", "angle_increment", "range_min", "range_max", "obstacle_range", "raytrace_range", "footprint_clear_radius", "marking",
          "clearing", "inf_is_valid", "track_unknown", "combination_method"]


@pytest.fixture
def registered(monkeypatch):
    """the comparator looks a header's mirrors up in _abi.HEADERS: the row is there for the length of a test"""
    monkeypatch.setitem(_abi.HEADERS, HEADER, _abi.LATER_HEADERS[HEADER])
    return _abi.LATER_HEADERS[HEADER]


def test_the_later_registry_is_this_header_and_shares_nothing_with_the_pinned_five():
    assert list(_abi.LATER_HEADERS) == [HEADER] and _abi.LATER_HEADERS[HEADER][0] is _abi.SCAN_PROTOTYPES and HEADER not in _abi.HEADERS
    assert sorted(_abi.SCAN_PROTOTYPES) == ["mpc_costmap_scans", "mpc_costmap_scans_device", "mpc_scan_params_defaults"]
    assert not set(_abi.SCAN_PROTOTYPES) & set().union(*(t for t, _ in _abi.HEADERS.values()))


def test_every_prototype_matches_its_declaration(registered):
    table, mirrors = registered
    text = K.header_text(HEADER)
    assert sorted(K.declarations(text)) == sorted(table)
    assert K.mismatches(HEADER, table) == []
    assert sorted(re.findall(r"typedef struct (\w+) \{", text)) == sorted(mirrors)
    scans = table["mpc_costmap_scans_device"][1]
    assert len(scans) == 14 and scans[2] is C.POINTER(_abi.MpcScanParams) and scans[4] is C.POINTER(C.c_float) and scans[9] is C.c_double
    assert table["mpc_costmap_scans"] is table["mpc_costmap_scans_device"]


@pytest.mark.parametrize("function,index,bound,report", [
    ("mpc_costmap_scans_device", 9, C.c_int32, f"mpc_costmap_scans_device: parameter 9 is double resolution, bound as {C.c_int32}"),
    ("mpc_costmap_scans", 2, C.c_void_p, f"mpc_costmap_scans: parameter 2 is mpc_scan_params* params, bound as {C.c_void_p}"),
    ("mpc_costmap_scans", 4, C.c_void_p, f"mpc_costmap_scans: parameter 4 is float* ranges, bound as {C.c_void_p}"),
    ("mpc_scan_params_defaults", None, None, "mpc_scan_params_defaults: declared, not in the table")])
def test_the_comparator_reports_a_corrupted_table(registered, function, index, bound, report):
    table = dict(registered[0])
    restype, argtypes = table.pop(function)
    if index is not None:
        table[function] = (restype, argtypes[:index] + [bound] + argtypes[index + 1:])
    assert K.mismatches(HEADER, table) == [report]


def test_mpc_hip_h_declares_nothing_of_this_header(registered):
    table, mirrors = registered
    hip_text = K.header_text(K.MAIN)
    for name in list(table) + list(mirrors):
        assert not re.search(r"\b%s\b" % name, K.header_code(hip_text)), name
    assert len(K.declarations(hip_text)) == 37 and '#include "mpc_hip.h"' in K.header_text(HEADER) and HEADER[:-len(".h")] not in hip_text


def test_struct_layout_matches_c(registered, tmp_path):
    mirror = registered[1]["mpc_scan_params"]
    fields = [f[0] for f in mirror._fields_]
    assert fields == K.struct_fields(HEADER, "mpc_scan_params") == FIELDS
    out = K.c_layout(HEADER, "mpc_scan_params", fields, {}, tmp_path)
    assert len(out) == 1 + len(fields) and out[0] == C.sizeof(mirror) == 120
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f


def test_the_chain_comments_put_the_step_between_the_window_and_the_converters():
    for header in (HEADER, "mpc_costmap_window.h"):
        text = K.header_text(header)
        chain = text[:text.index("#ifndef")]
        assert 0 < chain.index("mpc_costmap_window_device") < chain.index("mpc_costmap_scans_device") < chain.index("mpc_costmap_to_obstacles_device"), header
    text = K.header_text(HEADER)
    assert "cannot be verified here" in text and "OF OURS" in text and "NOT inflated" in text


def test_library_exports_binds_gives_the_defaults_and_refuses_without_a_gpu(lib):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MpcScanParams
    for name, (restype, argtypes) in _abi.SCAN_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes and name not in _lib.EXPORTS, name
    # the defaults as the header states them
    p = MpcScanParams((C.c_double * 2)(7.0, 7.0), (C.c_double * 3)(7.0, 7.0, 7.0), *([-1.0] * 7), *([-1] * 5))
    lib.mpc_scan_params_defaults(C.byref(p))
    assert (tuple(p.lattice_anchor), tuple(p.sensor_pose), p.angle_min, p.angle_increment, p.range_min, p.range_max, p.obstacle_range, p.raytrace_range, p.footprint_clear_radius,
            p.marking, p.clearing, p.inf_is_valid, p.track_unknown, p.combination_method) == ((0.0, 0.0), (0.0, 0.0, 0.0), -math.pi, 2 * math.pi / 360, 0.0, 30.0, 2.5, 3.0, 0.0,
                                                                                              1, 1, 0, 0, 1)
    lib.mpc_scan_params_defaults(None)
    # without a handle: a refusal instead of a crash, with its text; the null test comes first, whatever else is wrong
    for fn in (lib.mpc_costmap_scans, lib.mpc_costmap_scans_device):
        assert fn(None, 1, C.byref(p), None, None, 360, None, 8, 8, 0.05, None, None, None, None) == MPC_EINVAL
        assert b"mpc_costmap_scans: null argument" in lib.mpc_last_error()
        assert fn(None, 1, None, None, None, 0, None, 0, 8, math.nan, None, None, None, None) == MPC_EINVAL
        assert b"mpc_costmap_scans: null argument" in lib.mpc_last_error()
    assert lib.mpc_version() == 900
