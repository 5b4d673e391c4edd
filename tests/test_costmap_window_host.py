"""CPU tests of the per-instance rule of mpc_costmap_window* (mpc_local_planner_amd/csrc/mpc_costmap_window.hpp), compiled for the host with g++ by a tests-only
harness (tests/host_harness/costmap_window_host.cpp): on every scripted case (tests/_window_cases.py) and on random maps every byte of the windows, every origin and
every count equals a Python restatement of include/mpc_costmap_window.h written independently; the separable distance passes agree with scipy's Euclidean distance
transform; the table follows from the rule; and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs the scripted cases clean and to the
same bytes.  The two parameter readers are tested here too, on the shipped costmap files recorded as data under tests/golden/."""
import json
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import _harness
import _window_cases as Wn
from mpc_local_planner_amd import params as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_costmap_params.json")


@pytest.fixture(scope="module")
def all_cases():
    return Wn.cases()


@pytest.fixture(scope="module")
def seen(all_cases):
    return {c.name: Wn.host_window(c, want_d2=True) for c in all_cases}


@pytest.fixture(scope="module")
def restated(all_cases):
    return {c.name: Wn.python_window(c) for c in all_cases}


def test_scripted_cases_equal_the_python_restatement(all_cases, seen, restated):
    for c in all_cases:
        assert Wn.same(seen[c.name][:3], restated[c.name]) is None, (c.name, Wn.same(seen[c.name][:3], restated[c.name]))
    assert len(seen) == len(all_cases) >= 20


def test_random_maps_equal_the_python_restatement():
    cs = Wn.random_cases()
    inflated = 0
    for c in cs:
        mine, ref = Wn.host_window(c), Wn.python_window(c)
        assert Wn.same(mine, ref) is None, (c.name, Wn.same(mine, ref))
        inflated += int(mine[2][:, 2].clip(0).sum())
    assert len(cs) == 60 and max(c.B for c in cs) <= 8 and inflated > 2000          # the generator does make something to inflate


def test_the_cases_do_what_they_are_there_for(all_cases, seen):
    by = {c.name: c for c in all_cases}
    info = lambda name: seen[name][2].tolist()
    tx, ty = Wn.tile()
    assert {(c.W, c.H) for c in all_cases} >= {(1, 1), (7, 5), (17, 16), (55, 55)}
    assert by["three tiles wide"].W > 2 * tx and by["three tiles high"].H > 2 * ty
    assert {round(c.res / c.map_res, 6) for c in all_cases} >= {1.0, 2.0, 1.4}
    # the demo's window: origin on the lattice of 0.1 m, every cell of the first robot inside the map or off it as counted
    c = by["55 x 55, the demo's"]
    cost, origin, inf, _ = seen[c.name]
    assert np.allclose(origin / 0.1, np.round(origin / 0.1), atol=1e-9) and (inf[:, 2] == 0).all() and (inf[:, 0] < 55 * 55).all() and (inf[:, 0] > 0).all()
    assert (seen["55 x 55, inflated"][2][:, 2] > 100).all()
    # r = 0: the sampled bytes; here the window is the map
    assert (seen["every byte value, r 0"][0][0] == Wn.byte_map()).all() and info("every byte value, r 0") == [[256, 1, 0, 0]]
    # every byte under an inflation: 255 stays unless the table's value passes the test; 253 and 254 stay; the rest is max(s, c)
    plain, unknown = seen["every byte value, inflate_unknown 0"][0][0], seen["every byte value, inflate_unknown 1"][0][0]
    assert plain[15, 14] == 254 and plain[15, 13] == 253 and unknown[15, 15] == 253 == plain[15, 15]          # one cell from the lethal one: inscribed
    assert (plain.ravel()[:255] >= Wn.byte_map().ravel()[:255]).all() and (plain[8:, 8:] > Wn.byte_map()[8:, 8:]).any() and (plain[:6] == Wn.byte_map()[:6]).all()
    # the edges: a window wholly outside is outside_value throughout and counts nothing inside
    for outside in (0, 255):
        cost, origin, inf, _ = seen[f"edges, outside {outside}, inflate_unknown 0"]
        assert (cost[5:] == outside).all() and (inf[5:] == 0).all() and (0 < inf[:5, 0]).all() and (inf[:5, 0] < 400).all()
    assert (seen["edges, outside 255, inflate_unknown 1"][0] != seen["edges, outside 255, inflate_unknown 0"][0]).any()
    # lethal cells in the halo only still inflate the window
    assert info("a lethal cell in the halo only")[0][1] == 0 and info("a lethal cell in the halo only")[0][3] > 0 and info("a lethal cell in the halo only")[0][2] > 0
    assert info("1 x 1, r 5: a window smaller than r")[0][3] > 0
    # on the line the origin steps, 1e-12 m below it does not: a cell apart
    org = seen["a pose on a lattice line and just below it"][1]
    assert np.array_equal(org[:3] - org[3:], np.full((3, 2), 0.25)) and (org[1] < 0).all()
    # not finite, or too far for 32-bit cells: all outside, the anchor, -1
    cost, origin, inf, _ = seen["a pose that is not finite"]
    assert (cost[:4] == 255).all() and (origin[:4] == 0.0).all() and inf[:4].tolist() == [[-1, 0, 0, 0]] * 4 and inf[4, 0] == 63


def test_pass_two_agrees_with_the_euclidean_distance_transform(all_cases, seen):
    """scipy's exact transform of the lattice with its halo, squared and rounded, wherever it gives d2 <= r^2; nothing where it gives more"""
    looked = 0
    for c in all_cases:
        r = c.r
        if r == 0:
            continue
        d2 = seen[c.name][3]
        for b in range(c.B):
            if seen[c.name][2][b, 0] < 0:
                assert (d2[b] == -1).all()
                continue
            lattice = _lattice(c, b, seen[c.name][1][b])
            edt = ndimage.distance_transform_edt(lattice != Wn.LETHAL) if (lattice == Wn.LETHAL).any() else np.full(lattice.shape, np.inf)
            want = np.where(np.isfinite(edt), np.rint(edt * edt), 1e18)[r:r + c.H, r:r + c.W]
            assert np.array_equal(d2[b] >= 0, want <= r * r), c.name
            assert np.array_equal(d2[b][d2[b] >= 0], want[want <= r * r].astype(np.int32)), c.name
            looked += int((d2[b] >= 0).sum())
    assert looked > 5000


def _lattice(c, b, origin):
    """the bytes of rule 2 on the window's lattice with its halo of r cells, from the origin the host build gave"""
    r = c.r
    mx = [Wn._index_axis(origin[0], i, c.res, c.map_origin[0], c.map_res, c.map.shape[1]) for i in range(-r, c.W + r)]
    my = [Wn._index_axis(origin[1], j, c.res, c.map_origin[1], c.map_res, c.map.shape[0]) for j in range(-r, c.H + r)]
    return np.array([[c.map[y, x] if x >= 0 and y >= 0 else c.outside for x in mx] for y in my], np.uint8)


def test_table_values_follow_from_the_rule():
    t = np.zeros(26, np.uint8)
    Wn.harness().cwh_table(0.05, 0.17, 10.0, 5, Wn.b_(t))
    assert t[0] == 254 and t[9] == 253 and t[25] == int(252 * math.exp(-0.8)) == 113          # 3 cells: 0.15 m <= 0.17 m; 5 cells: 0.25 m, 0.08 m beyond it
    assert t[10] == 253 and t[16] == int(252 * math.exp(-10.0 * (4 * 0.05 - 0.17))) == 186 and (np.diff(t.astype(int)) <= 0).all()
    c = Wn.Case("", Wn.byte_map(), (0, 0, 0), (4, 4), 0.05, inflation=0.25)
    assert Wn.table_of(c) == t.tolist()
    # scaling 0: 252 everywhere beyond the inscribed radius; inscribed 0: nothing is 253
    Wn.harness().cwh_table(0.1, 0.0, 0.0, 3, Wn.b_(t))
    assert t[:10].tolist() == [254] + [252] * 9


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, restated, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as the restatement gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("costmap_window_host", ("CWH_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    Wn.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, Wn.read_outputs(dst, all_cases)):
        assert Wn.same(got, restated[c.name]) is None, c.name


def test_window_params_from_the_shipped_costmap_files():
    """the four shipped costmap files and the three map files, recorded as data"""
    shipped = json.load(open(GOLDEN))
    values = lambda p: (tuple(p.map_origin), p.map_resolution, tuple(p.lattice_anchor), p.inflation_radius, p.cost_scaling_factor, p.map_size_x, p.map_size_y, p.outside_value,
                        p.inflate_unknown)
    diff, car = shipped["cfg"]["diff_drive"], shipped["cfg"]["carlike"]
    p, size = P.window_params_from_costmap_yaml(diff["local_costmap"], diff["costmap_common"], shipped["maps"]["corridor"], (400, 1200))
    assert size == (55, 55) and values(p) == ((0.0, 0.0), 0.05, (0.0, 0.0), 0.0, 10.0, 1200, 400, 0, 0) and p.inscribed_radius == 0.17
    p, size = P.window_params_from_costmap_yaml(car["local_costmap"], car["costmap_common"], shipped["maps"]["empty_box"], (120, 160))
    assert size == (55, 55) and values(p) == ((-3.0, -3.0), 0.05, (0.0, 0.0), 0.0, 10.0, 160, 120, 0, 0)
    # the carlike footprint [-0.1, 0.5] x [-0.125, 0.125] padded by costmap_2d's default 0.01: the nearest edge is the rear one, 0.11 m from the origin
    assert math.isclose(p.inscribed_radius, 0.11, rel_tol=1e-12)
    assert math.isclose(P._inscribed_radius(car["costmap_common"]["footprint"], 0.0), 0.1, rel_tol=1e-12)
    assert math.isclose(P._inscribed_radius([(1.0, -1.0), (3.0, -1.0), (3.0, 1.0), (1.0, 1.0)], 0.0), 1.0)          # the origin outside: the nearest edge's interior
    assert math.isclose(P._inscribed_radius([(1.0, 1.0), (3.0, 1.0), (3.0, 3.0), (1.0, 3.0)], 0.0), math.sqrt(2.0))          # a vertex
    # with an inflation layer among the plugins: its block of the common file; the local file's keys win
    local = dict(diff["local_costmap"]["local_costmap"])
    local["plugins"] = local["plugins"] + [{"name": "inflation_layer", "type": "costmap_2d::InflationLayer"}]
    p, size = P.window_params_from_costmap_yaml(local, diff["costmap_common"], shipped["maps"]["maze"], (100, 200))
    assert (p.inflation_radius, p.cost_scaling_factor, p.inflate_unknown, p.outside_value) == (0.5, 10.0, 0, 0)
    local.update(track_unknown_space=True, inflation_layer={"inflation_radius": 0.3, "cost_scaling_factor": 4.0, "inflate_unknown": True}, robot_radius=0.2, width=3.04)
    p, size = P.window_params_from_costmap_yaml(local, diff["costmap_common"], shipped["maps"]["maze"], (100, 200))
    assert (p.inflation_radius, p.cost_scaling_factor, p.inflate_unknown, p.outside_value, p.inscribed_radius, size) == (0.3, 4.0, 1, 255, 0.2, (30, 55))
    local["inflation_layer"]["enabled"] = False
    assert P.window_params_from_costmap_yaml(local, None, shipped["maps"]["maze"], (100, 200))[0].inflation_radius == 0.0
    # the refusals
    base = diff["local_costmap"]["local_costmap"]
    for change in ({"rolling_window": False}, {"width": None}, {"height": "wide"}, {"resolution": 0.0}):
        with pytest.raises(P.ParamNotImplemented):
            P.window_params_from_costmap_yaml({**base, **change}, diff["costmap_common"], shipped["maps"]["maze"], (100, 200))
    with pytest.raises(P.ParamNotImplemented):
        P.window_params_from_costmap_yaml({k: v for k, v in base.items() if k != "rolling_window"}, None, shipped["maps"]["maze"], (100, 200))
    with pytest.raises(P.ParamNotImplemented):
        P.window_params_from_costmap_yaml(base, None, {**shipped["maps"]["maze"], "origin": [0.0, 0.0, 0.5]}, (100, 200))
    with pytest.raises(P.ParamError):
        P.window_params_from_costmap_yaml(base, None, {"origin": [0.0, 0.0, 0.0]}, (100, 200))


def test_static_layer_costs_interprets_occupancy_values():
    occ = np.array([[-1, 0, 1, 50, 99, 100], [65, 64, 19, 20, 101, 127]], np.int8)
    assert P.static_layer_costs(occ).tolist() == [[255, 0, 0, 0, 0, 254], [0, 0, 0, 0, 254, 254]]
    assert P.static_layer_costs(occ, track_unknown_space=False).tolist() == [[0, 0, 0, 0, 0, 254], [0, 0, 0, 0, 254, 254]]
    assert P.static_layer_costs(occ, lethal_threshold=65).tolist() == [[255, 0, 0, 0, 254, 254], [254, 0, 0, 0, 254, 254]]
    scaled = P.static_layer_costs(occ, trinary_costmap=False)
    assert scaled.tolist() == [[255, 0, int(0.01 * 254), 127, int(0.99 * 254), 254], [int(0.65 * 254), int(0.64 * 254), int(0.19 * 254), int(0.2 * 254), 254, 254]]
    assert P.static_layer_costs(occ, unknown_cost_value=50).tolist()[0] == [254, 0, 0, 255, 0, 254]          # -1 read as an unsigned char is 255: lethal
    assert P.static_layer_costs(occ, lethal_threshold=400).tolist()[1] == [0, 0, 0, 0, 254, 254] and scaled.dtype == np.uint8
