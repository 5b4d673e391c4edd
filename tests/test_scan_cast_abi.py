"""CPU tests of include/mpc_scan_cast.h at the drop-in boundary.  tests/test_abi.py pins _abi.HEADERS and tests/test_costmap_scans_abi.py pins _abi.LATER_HEADERS to
the rows they were written for, so this header's row lives in _abi.OPEN_HEADERS and is held here by the same means (tests/_abi_check.py): its declarations against
_abi.CAST_PROTOTYPES, the layout of mpc_cast_params against the C compiler, the library's exports and the binding.  This module asserts that its own row is there, not
that the registry holds nothing else: the next header is a row, not a fourth registry.  Then what is particular to the header: its place in the cycle's comment, the
values of its defaults, and what the library can refuse without a GPU."""
import ctypes as C
import math
import re

import pytest

import _abi_check as K
from _abi_check import lib      # noqa: F401 (the fixture)
from mpc_local_planner_amd import _abi, _lib

HEADER = "mpc_scan_cast.h"
FIELDS = ["map_origin", "map_resolution", "sensor_pose", "angle_min", "angle_increment", "range_max", "map_size_x", "map_size_y", "block_threshold", "unknown_blocks",
          "hit_point", "miss_is_inf"]


@pytest.fixture
def registered(monkeypatch):
    """the comparator looks a header's mirrors up in _abi.HEADERS: the row is there for the length of a test"""
    monkeypatch.setitem(_abi.HEADERS, HEADER, _abi.OPEN_HEADERS[HEADER])
    return _abi.OPEN_HEADERS[HEADER]


def test_the_open_registry_has_this_row_and_shares_no_function_with_the_pinned_ones():
    assert HEADER in _abi.OPEN_HEADERS and _abi.OPEN_HEADERS[HEADER][0] is _abi.CAST_PROTOTYPES and HEADER not in _abi.HEADERS and HEADER not in _abi.LATER_HEADERS
    assert sorted(_abi.CAST_PROTOTYPES) == ["mpc_cast_params_defaults", "mpc_scan_cast", "mpc_scan_cast_device"]
    pinned = set().union(*(t for t, _ in list(_abi.HEADERS.values()) + list(_abi.LATER_HEADERS.values())))
    assert not set(_abi.CAST_PROTOTYPES) & pinned
    # the pool is mpc_fleet.h's, mirrored once
    assert _abi.OPEN_HEADERS[HEADER][1]["mpc_pool"] is _abi.HEADERS["mpc_fleet.h"][1]["mpc_pool"]


def test_every_prototype_matches_its_declaration(registered):
    table, mirrors = registered
    text = K.header_text(HEADER)
    assert sorted(K.declarations(text)) == sorted(table)
    assert K.mismatches(HEADER, table) == []
    assert re.findall(r"typedef struct (\w+) \{", text) == ["mpc_cast_params"] and set(mirrors) == {"mpc_cast_params", "mpc_pool"} and '#include "mpc_fleet.h"' in text
    cast = table["mpc_scan_cast_device"][1]
    assert len(cast) == 11 and cast[3] is C.POINTER(_abi.MpcCastParams) and cast[5] is C.POINTER(_abi.MpcPool) and cast[8] is C.POINTER(C.c_float)
    assert table["mpc_scan_cast"] is table["mpc_scan_cast_device"]


@pytest.mark.parametrize("function,index,bound,report", [
    ("mpc_scan_cast_device", 7, C.c_double, f"mpc_scan_cast_device: parameter 7 is int32_t n_beams, bound as {C.c_double}"),
    ("mpc_scan_cast", 3, C.c_void_p, f"mpc_scan_cast: parameter 3 is mpc_cast_params* params, bound as {C.c_void_p}"),
    ("mpc_scan_cast", 8, C.c_void_p, f"mpc_scan_cast: parameter 8 is float* ranges, bound as {C.c_void_p}"),
    ("mpc_cast_params_defaults", None, None, "mpc_cast_params_defaults: declared, not in the table")])
def test_the_comparator_reports_a_corrupted_table(registered, function, index, bound, report):
    table = dict(registered[0])
    restype, argtypes = table.pop(function)
    if index is not None:
        table[function] = (restype, argtypes[:index] + [bound] + argtypes[index + 1:])
    assert K.mismatches(HEADER, table) == [report]


def test_mpc_hip_h_declares_nothing_of_this_header(registered):
    table, _ = registered
    hip_text = K.header_text(K.MAIN)
    for name in list(table) + ["mpc_cast_params"]:
        assert not re.search(r"\b%s\b" % name, K.header_code(hip_text)), name
    assert len(K.declarations(hip_text)) == 37 and HEADER[:-len(".h")] not in hip_text


def test_struct_layout_matches_c(registered, tmp_path):
    mirror = registered[1]["mpc_cast_params"]
    fields = [f[0] for f in mirror._fields_]
    assert fields == K.struct_fields(HEADER, "mpc_cast_params") == FIELDS
    out = K.c_layout(HEADER, "mpc_cast_params", fields, {}, tmp_path)
    assert len(out) == 1 + len(fields) and out[0] == C.sizeof(mirror) == 96
    for f, o in zip(fields, out[1:]):
        assert getattr(mirror, f).offset == o, f


def test_the_chain_comment_puts_the_step_in_front_of_the_scans_step():
    text = K.header_text(HEADER)
    chain = text[:text.index("#ifndef")]
    chain = chain[chain.index("\n *     mpc_scan_cast_device"):]          # the drawing of the cycle, behind the opening sentence
    assert 0 < chain.index("mpc_scan_cast_device") < chain.index("mpc_costmap_window_device") < chain.index("mpc_costmap_scans_device") < chain.index("mpc_costmap_to_obstacles_device")
    assert "cannot be verified here" in text and "OF OURS" in text and "OUT OF SCOPE" in text and "sensor noise" in text and "0.02 m" in text


def test_library_exports_binds_gives_the_defaults_and_refuses_without_a_gpu(lib):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MpcCastParams, MpcPool
    for name, (restype, argtypes) in _abi.CAST_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes and name not in _lib.EXPORTS, name
    # the defaults as the header states them
    p = MpcCastParams((C.c_double * 2)(7.0, 7.0), -1.0, (C.c_double * 3)(7.0, 7.0, 7.0), *([-1.0] * 3), *([-1] * 6))
    lib.mpc_cast_params_defaults(C.byref(p), 0.05, 600, 400)
    assert (tuple(p.map_origin), p.map_resolution, tuple(p.sensor_pose), p.angle_min, p.angle_increment, p.range_max, p.map_size_x, p.map_size_y, p.block_threshold, p.unknown_blocks,
            p.hit_point, p.miss_is_inf) == ((0.0, 0.0), 0.05, (0.0, 0.0, 0.0), -math.pi, 2 * math.pi / 360, 6.5, 600, 400, 254, 0, 1, 1)
    lib.mpc_cast_params_defaults(None, 0.05, 1, 1)
    # without a handle: a refusal instead of a crash, with its text; the null test comes first, whatever else is wrong
    bad_pool = MpcPool(-3, None, None, None, None)
    for fn in (lib.mpc_scan_cast, lib.mpc_scan_cast_device):
        assert fn(None, 1, None, C.byref(p), None, None, None, 360, None, None, None) == MPC_EINVAL
        assert b"mpc_scan_cast: null argument" in lib.mpc_last_error()
        p.block_threshold = 0
        assert fn(None, 1, None, None, None, C.byref(bad_pool), None, 0, None, None, None) == MPC_EINVAL
        assert b"mpc_scan_cast: null argument" in lib.mpc_last_error()
        p.block_threshold = 254
    assert lib.mpc_version() == 900
