"""CPU tests of the per-instance rule of mpc_costmap_scans* (mpc_local_planner_amd/csrc/mpc_costmap_scans.hpp), compiled for the host with g++ by a tests-only
harness (tests/host_harness/costmap_scans_host.cpp): on every scripted case (tests/_scan_cases.py) and on 60 random second cycles every byte of the layer and of the
window, every lattice index and every count equals a Python restatement written independently from the text of include/mpc_costmap_scans.h; the pieces of the rule
(sine and cosine, the wrap, the step count, the origin) are held on their own; a layer persists over cycles as a fleet needs it to; and the harness, built
as a stand-alone program with -fsanitize=address,undefined, runs the scripted cases clean and to the same bytes.  The parameter reader is tested here too, on the shipped
costmap files recorded as data under tests/golden/."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _harness
import _scan_cases as Sc
from mpc_local_planner_amd import params as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_costmap_params.json")


@pytest.fixture(scope="module")
def all_cases():
    return Sc.cases()


@pytest.fixture(scope="module")
def seen(all_cases):
    return {c.name: Sc.host_scans(c) for c in all_cases}


@pytest.fixture(scope="module")
def restated(all_cases):
    """name -> (the restatement's result, its trace per instance)"""
    out = {}
    for c in all_cases:
        trace = []
        out[c.name] = (Sc.python_scans(c, trace), trace)
    return out


def test_scripted_cases_equal_the_python_restatement(all_cases, seen, restated):
    for c in all_cases:
        assert Sc.same(seen[c.name], restated[c.name][0]) is None, (c.name, Sc.same(seen[c.name], restated[c.name][0]))
    assert len(seen) == len(all_cases) >= 30


def test_random_second_cycles_equal_the_python_restatement():
    cs = Sc.random_cases()
    cleared = marked = rolled_with_survivors = 0
    for c in cs:
        trace = []
        mine, ref = Sc.host_scans(c), Sc.python_scans(c, trace)
        assert Sc.same(mine, ref) is None, (c.name, Sc.same(mine, ref))
        cleared += sum(len(t["cleared"]) for t in trace)
        marked += sum(len(t["marked"]) for t in trace)
        survives = False
        for b, t in enumerate(trace):
            if t["valid"] and t["shift"] not in (None, (0, 0)):
                old = {(int(x), int(y)) for y, x in np.argwhere((t["rolled"] == Sc.LETHAL) & (ref[0][b] == Sc.LETHAL))}
                survives |= bool(old - t["marked"])
        rolled_with_survivors += survives
    # the generator gives the step something to do
    assert len(cs) == 60 and max(c.B for c in cs) <= 8
    assert cleared > 2000 and marked > 500 and rolled_with_survivors >= 10, (cleared, marked, rolled_with_survivors)


def test_the_cases_do_what_they_are_there_for(all_cases, seen, restated):
    by = {c.name: c for c in all_cases}
    tr = lambda name: restated[name][1]
    info = lambda name: seen[name][3].tolist()
    assert {(c.W, c.H) for c in all_cases} >= {(1, 1), (7, 5), (17, 16), (55, 55), (256, 256)} and {c.n for c in all_cases} >= {1, 63, 64, 65, 257, 360}
    assert {c.W % 16 for c in all_cases} >= {0, 1, 7} and max(c.W * c.H for c in all_cases) == 65536
    # the walk: every direction of the eight, ties on the four diagonals, every octant; a ray of no length visits its own cell
    dirs = {(np.sign(dx), np.sign(dy)) for _, dx, dy, _ in tr("axes and diagonals")[0]["walks"]}
    assert len(dirs) == 8 and sum(abs(dx) == abs(dy) != 0 for _, dx, dy, _ in tr("axes and diagonals")[0]["walks"]) == 4
    assert len({(dx > 0, dy > 0, abs(dx) > abs(dy)) for _, dx, dy, _ in tr("sixteen octant halves")[0]["walks"]}) == 8
    assert tr("a zero-length ray")[0]["walks"][0][1:] == (0, 0, 0) and (10, 10) in tr("a zero-length ray")[0]["cleared"]
    layer = seen["axes and diagonals"][0][0]
    assert (layer[10, 4:17] != Sc.UNKNOWN).all() and (layer[4:17, 10] != Sc.UNKNOWN).all() and all(layer[10 + d, 10 + d] != Sc.UNKNOWN for d in range(-6, 7)) and layer[0, 0] == Sc.UNKNOWN
    # truncation: R = 5 cells.  (20, 0): 5 steps by both formulas.  (12, 9) and (6, 8): R da / hypot = 4 exactly, where costmap_2d's doubles may land on 3
    assert tr("truncated, the formulas agree")[0]["walks"] == [(0, 20, 0, 5)] and int(min(1.0, 5 / math.hypot(20, 0)) * 20) == 5
    assert tr("truncated, the formulas could part")[0]["walks"] == [(0, 12, 9, 4), (1, 6, 8, 4)]
    assert len(tr("truncated, the formulas agree")[0]["cleared"]) == 6 and info("truncated, the formulas agree")[0][1] == 1          # the mark beyond the cleared stretch stays
    # obstacle_range: exactly at it is not marked, one float inside it is
    assert info("a return exactly at obstacle_range and one just inside")[0][:2] == [2, 1]
    assert len(tr("a return exactly at obstacle_range and one just inside")[0]["walks"]) == 2
    # returns outside the window: cleared up to the border, nothing marked
    assert info("returns outside the window")[0][0] == 40 and info("returns outside the window")[0][1] == 0 and info("returns outside the window")[0][2] > 50
    # the sensor's cell outside the window: nothing is cleared but marks are made
    t = tr("the sensor's cell outside the window")[0]
    assert not t["walks"] and not t["cleared"] and len(t["marked"]) >= 3 and info("the sensor's cell outside the window")[0][1:3] == [len(t["marked"]), 0]
    # the odd ranges: 1.0, 0.1 and the float below range_max are kept; +inf only when inf_is_valid
    assert info("NaN, below range_min, at range_max, inf; inf_is_valid 0")[0][0] == 3 and info("NaN, below range_min, at range_max, inf; inf_is_valid 1")[0][0] == 4
    # the combination over every byte value
    for tu in (0, 1):
        over, most = seen[f"every byte value, method 0, track_unknown {tu}"], seen[f"every byte value, method 1, track_unknown {tu}"]
        s = Sc.byte_map()
        known = over[0][0] != Sc.UNKNOWN
        assert known.any() and (over[0][0] == Sc.LETHAL).any() and (over[0][0] == 0).any() and known.all() == (tu == 0)
        assert (over[2][0][known] == over[0][0][known]).all() and (over[2][0][~known] == s[~known]).all()
        l = most[0][0]
        want = np.where((l != Sc.UNKNOWN) & ((s == Sc.UNKNOWN) | (s < l)), l, s)
        assert (most[2][0] == want).all() and (most[2][0] != over[2][0]).any()
    # the disc clears the marks made inside it, and the robot's own surroundings
    for b in range(2):
        marked, layer = tr("the disc")[b]["marked"], seen["the disc"][0][b]
        gone = [m for m in marked if layer[m[1], m[0]] == 0]
        assert gone and len(gone) < len(marked)
    # the rolls
    shifts = [t["shift"] for name in ("rolls of 0, +-1 and W - 1 cells", "rolls of a window or more, and diagonal ones") for t in tr(name)]
    assert {(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (18, 0), (0, -12), (-18, 12), (19, 0), (0, 13), (-19, 0), (1, 1), (-3, 2)} <= set(shifts)
    c = by["rolls of 0, +-1 and W - 1 cells"]
    got = seen[c.name][0]
    assert (got[0] == c.layer0[0]).all() and (got[1][:, :-1] == c.layer0[1][:, 1:]).all() and (got[1][:, -1] == Sc.UNKNOWN).all()
    assert (got[5][:, 0] == c.layer0[5][:, -1]).all() and (got[5][:, 1:] == Sc.UNKNOWN).all()
    wide = seen["rolls of a window or more, and diagonal ones"][0]
    assert all((wide[b] == Sc.UNKNOWN).all() for b in (0, 1, 2, 3, 6, 7)) and (wide[4][:-1, :-1] == by["rolls of a window or more, and diagonal ones"].layer0[4][1:, 1:]).all()
    # keep 0, or no keep at all: no trace of the layer that was there
    c = by["keep 0 after a filled layer"]
    for b in range(4):
        fresh = Sc.host_scans(c.take(b).variant(layer0=None, cell0=None, keep=[0]))
        assert (seen[c.name][0][b].tobytes() == fresh[0][0].tobytes()) == (c.keep[b] == 0)
    assert set(np.unique(seen["keep NULL after a filled layer"][0])) <= {0, Sc.LETHAL}
    # not finite, or too far for the lattice: the default throughout, {0, 0}, the window untouched, -1; a heading beyond every turn keeps no beam
    layer, cell, cost, inf = seen["a pose that is not finite"]
    assert (layer[:6] == Sc.UNKNOWN).all() and (cell[:6] == 0).all() and (cost[:6] == Sc.POISON).all() and inf[:6].tolist() == [[-1, 0, 0, 0]] * 6
    assert inf[6].tolist()[:2] == [0, 0] and inf[6, 2] == 0 and (layer[6] == Sc.UNKNOWN).all() and inf[7, 0] > 20
    assert seen["anchor off zero, no window, no info"][2] is None and seen["anchor off zero, no window, no info"][3] is None
    assert info("marking off")[0][1] == 0 and info("marking off")[0][2] > 0 and info("clearing off")[0][2] == 0 and info("clearing off")[0][1] > 0


def test_sine_and_cosine_round_as_the_restatement_and_stay_within_an_ulp_of_libm():
    lib = Sc.harness()
    rng = np.random.default_rng(8)
    xs = np.concatenate([rng.uniform(-math.pi, math.pi, 4000), [-math.pi, 0.0, -0.0, math.pi / 4, -math.pi / 4, math.pi / 2, np.nextafter(math.pi, 0), 1e-300, 3 * math.pi / 4]])
    s, c = C_double(), C_double()
    for x in xs:
        lib.csh_sincos(float(x), s, c)
        assert (s.value, c.value) == Sc.sincos(float(x)), x
        assert abs(s.value - math.sin(x)) <= 2.3e-16 and abs(c.value - math.cos(x)) <= 2.3e-16, x


def C_double():
    import ctypes
    return ctypes.c_double()


def test_wrap_step_count_and_origin_on_their_own():
    lib = Sc.harness()
    rng = np.random.default_rng(9)
    for th in np.concatenate([rng.uniform(-50, 50, 2000), [math.pi, -math.pi, 3 * math.pi, -3 * math.pi, 2 * math.pi, 1e9, -1e9, 1e18, 1e300, -1e300]]):
        got, want = lib.csh_wrap(float(th)), Sc.wrap(float(th))
        assert got == want, th
        assert abs(th) > 1e6 or (-math.pi <= got < math.pi and abs(math.remainder(got - th, 2 * math.pi)) < 1e-13), th
    assert math.isnan(lib.csh_wrap(math.inf)) and math.isnan(lib.csh_wrap(math.nan)) and not -math.pi <= lib.csh_wrap(1e18) < math.pi
    # the step count: the largest m with m^2 (dx^2 + dy^2) <= R^2 da^2, by brute force
    for dx, dy, R in [(20, 0, 5), (12, 9, 5), (6, 8, 5), (-12, 9, 5), (3, -4, 5), (3, 4, 4), (0, 0, 0), (0, 7, 0), (1, 1, 1), (32769, 32769, 4096), (-32769, 5, 4096), (100, 99, 70)] + \
            [tuple(int(v) for v in rng.integers(-300, 300, 2)) + (int(rng.integers(0, 200)),) for _ in range(2000)]:
        da, d2 = max(abs(dx), abs(dy)), dx * dx + dy * dy
        want = da if d2 <= R * R else max(m for m in range(da + 1) if m * m * d2 <= R * R * da * da) if da < 1000 else Sc.steps(dx, dy, R)
        assert lib.csh_steps(dx, dy, R) == want == Sc.steps(dx, dy, R), (dx, dy, R)
    # rule 1 is the window's rule 1: the same origin, the same refusals; the index times the resolution is the origin
    import ctypes
    org, cell = ctypes.c_double(), ctypes.c_int32()
    for pose, size, res, anchor in [(1.5, 55, 0.1, 0.0), (-2.9, 19, 0.1, -0.027), (0.5625, 5, 0.25, 0.0), (0.5625 - 1e-12, 5, 0.25, 0.0), (math.nan, 5, 0.1, 0.0), (1e300, 5, 0.1, 0.0),
                                    (5e7, 5, 0.05, 0.0), (6e7, 5, 0.05, 0.0)] + [(float(rng.uniform(-9, 9)), int(rng.integers(1, 99)), 0.05, 0.013) for _ in range(500)]:
        assert lib.csh_origin_agrees(pose, size, res, anchor, org, cell) == 1, (pose, size)
        want = Sc.origin_axis(pose, size, res, anchor)
        assert want is None or (org.value, cell.value) == want, (pose, size)


def test_a_layer_persists_over_cycles():
    """cycle 1 marks a wall ahead.  Cycle 2: the robot has moved three cells and turned its back, the wall is out of the scanner's field of view: the marks are still
    there, at the shifted cells.  Cycle 3: it looks that way again, with a wider fan, and the rays pass through where the wall stood: the marks are gone."""
    res, size = 0.05, (40, 40)
    fan = dict(angle_min=-0.3, angle_inc=0.02, obstacle_range=2.5, raytrace_range=3.0, track_unknown=1)
    first = Sc.Case("cycle 1", (1.0, 1.0, 0.0), np.full((1, 31), 0.6), size, res, **fan)
    l1, c1, _, i1 = Sc.host_scans(first)
    marks1 = {(int(x), int(y)) for y, x in np.argwhere(l1[0] == Sc.LETHAL)}
    assert i1[0, 1] == len(marks1) >= 5
    second = Sc.Case("cycle 2", (1.15, 1.0, math.pi), np.full((1, 31), 0.5), size, res, keep=1, layer0=l1, cell0=c1, **fan)
    l2, c2, _, i2 = Sc.host_scans(second)
    assert (c2 - c1).tolist() == [[3, 0]]
    assert all(l2[0][y, x - 3] == Sc.LETHAL for x, y in marks1) and i2[0, 1] > len(marks1)
    third = Sc.Case("cycle 3", (1.15, 1.0, 0.0), np.full((1, 61), 1.2), size, res, keep=1, layer0=l2, cell0=c2, **{**fan, "angle_min": -0.6})
    l3, c3, _, i3 = Sc.host_scans(third)
    assert (c3 == c2).all() and all(l3[0][y, x - 3] == 0 for x, y in marks1)
    for c, got in ((first, (l1, c1, None, i1)), (second, (l2, c2, None, i2)), (third, (l3, c3, None, i3))):
        ref = Sc.python_scans(c)
        assert Sc.same((got[0], got[1], ref[2], got[3]), ref) is None, c.name


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, restated, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as the restatement gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("costmap_scans_host", ("CSH_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    Sc.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, Sc.read_outputs(dst, all_cases)):
        assert Sc.same(got, restated[c.name][0]) is None, c.name


def test_scan_params_from_the_shipped_costmap_files():
    """the obstacle_layer blocks of the shipped costmap files, recorded as data"""
    shipped = json.load(open(GOLDEN))
    scan = dict(angle_min=-2.0, angle_increment=0.01, range_min=0.05, range_max=12.0, sensor_pose=(0.1, 0.0, 0.2))
    values = lambda p: (p.obstacle_range, p.raytrace_range, p.track_unknown, p.combination_method, p.marking, p.clearing, p.inf_is_valid)
    diff, car = shipped["cfg"]["diff_drive"], shipped["cfg"]["carlike"]
    p = P.scan_params_from_costmap_yaml(diff["local_costmap"], diff["costmap_common"], scan)
    assert values(p) == (3.0, 4.0, 1, 1, 1, 1, 0)
    assert (p.angle_min, p.angle_increment, p.range_min, p.range_max, tuple(p.sensor_pose), tuple(p.lattice_anchor)) == (-2.0, 0.01, 0.05, 12.0, (0.1, 0.0, 0.2), (0.0, 0.0))
    assert p.footprint_clear_radius == 0.17          # footprint clearing is costmap_2d's default, and the diff-drive file has a robot_radius
    p = P.scan_params_from_costmap_yaml(car["local_costmap"], car["costmap_common"], scan)
    # the carlike file sets track_unknown_space false; a polygon footprint: no radius is known
    assert values(p) == (3.0, 3.5, 0, 1, 1, 1, 0) and p.footprint_clear_radius == 0.0
    # what the reader reads, on a block of our own; the local file's keys win
    local = dict(diff["local_costmap"]["local_costmap"])
    name = [pl["name"] for pl in local["plugins"] if pl["type"] == "costmap_2d::ObstacleLayer"][0]
    block = {"observation_sources": "scan", "scan": {"data_type": "LaserScan", "marking": False, "clearing": True, "inf_is_valid": True}, "track_unknown_space": False,
             "combination_method": 0, "footprint_clearing_enabled": False}
    p = P.scan_params_from_costmap_yaml({**local, name: block}, diff["costmap_common"], scan)
    assert values(p) == (2.5, 3.0, 0, 0, 0, 1, 1) and p.footprint_clear_radius == 0.0
    p = P.scan_params_from_costmap_yaml({**local, name: {**block, "footprint_clearing_enabled": True, "obstacle_range": 1.5}, "robot_radius": 0.3}, None, {})
    assert (p.obstacle_range, p.footprint_clear_radius, p.range_max) == (1.5, 0.3, 30.0)
    # the refusals
    common = diff["costmap_common"]
    layer = common[name]
    source = layer[layer["observation_sources"].split()[0]]
    swap = lambda **kw: {**common, name: {**layer, **kw}}
    for bad_local, bad_common in (({**local, "plugins": [{"name": name, "type": "costmap_2d::VoxelLayer"}]}, common),
                                  ({**local, "plugins": [pl for pl in local["plugins"] if pl["type"] != "costmap_2d::ObstacleLayer"]}, common),
                                  ({k: v for k, v in local.items() if k != "plugins"}, common),
                                  (local, swap(**{layer["observation_sources"].split()[0]: {**source, "data_type": "PointCloud2"}})),
                                  (local, swap(**{layer["observation_sources"].split()[0]: {**source, "data_type": "PointCloud"}})),
                                  (local, swap(observation_sources="scan_a scan_b", scan_a=source, scan_b=source)),
                                  (local, swap(observation_sources="")),
                                  (local, swap(observation_sources="nothing_by_that_name")),
                                  (local, swap(combination_method=2))):
        with pytest.raises(P.ParamNotImplemented):
            P.scan_params_from_costmap_yaml(bad_local, bad_common, scan)
    with pytest.raises(P.ParamNotImplemented):
        P.scan_params_from_costmap_yaml(local, common, {**scan, "beams": 3})
