"""CPU tests of the per-instance rule of mpc_costmap_to_lines* (mpc_local_planner_amd/csrc/mpc_costmap_lines.hpp), compiled for the host with g++ by a tests-only
harness (tests/host_harness/costmap_lines_host.cpp): on every scripted case (tests/_line_cases.py) and on random maps every byte of the container and every count equals
a Python restatement of include/mpc_costmap_lines.h written independently, in unbounded Python integers; the outputs do what the step is for -- every kept cell is
covered, no line reaches into free space, an L keeps its free corner --; and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs the
scripted cases clean and to the same bytes.  The reader of the converter's parameters is tested here too."""
import math
import subprocess

import numpy as np
import pytest

import _cluster_cases as K
import _harness
import _line_cases as L
from mpc_local_planner_amd import params as P


@pytest.fixture(scope="module")
def all_cases():
    return L.cases()


@pytest.fixture(scope="module")
def seen(all_cases):
    return {c.name: L.host_lines(c) for c in all_cases}


@pytest.fixture(scope="module")
def restated(all_cases):
    """(result, meta) of the Python restatement, computed once"""
    return {c.name: L.python_lines(c) for c in all_cases}


@pytest.fixture(scope="module")
def random_maps():
    """(case, host result, restatement's result, meta) of the 80 random maps"""
    return [(c, L.host_lines(c)) + L.python_lines(c) for c in L.random_cases()]


def test_scripted_cases_equal_the_python_restatement(all_cases, seen, restated):
    for c in all_cases:
        assert L.same(seen[c.name], restated[c.name][0]) is None, (c.name, L.same(seen[c.name], restated[c.name][0]))
    assert len(seen) == len(all_cases) >= 26 and max(max(c.W, c.H) for c in all_cases if "4096" not in c.name) <= 48


def test_random_maps_equal_the_python_restatement(random_maps):
    lines = 0
    for c, mine, ref, _ in random_maps:
        assert L.same(mine, ref) is None, (c.name, L.same(mine, ref))
        lines += int(mine[6][0, 2])
    assert len(random_maps) == 80 and lines > 300          # the generator does make walls


def test_the_cases_do_what_they_are_there_for(all_cases, seen):
    by = {c.name: c for c in all_cases}
    no, dr = (lambda name, k=k: seen[name][k].tolist() for k in (0, 5))
    info = lambda name: seen[name][6].tolist()
    shapes = lambda name, b=0: seen[name][1][b, :seen[name][0][b]].tolist()
    index = lambda name, b=0: [((seen[name][2][b, s, :seen[name][1][b, s]] - by[name].origin[b]) / by[name].res - 0.5).tolist() for s in range(int(seen[name][0][b]))]
    assert (no("1 x 1"), info("1 x 1")) == ([0], [[0, 0, 0, 0]])
    assert (shapes("one cell"), info("one cell")) == ([1], [[1, 1, 0, 0]]) and seen["one cell"][3] is None and seen["one cell"][4] is None
    assert (index("straight wall"), info("straight wall")) == ([[[3, 4], [32, 4]]], [[30, 1, 1, 0]])
    # an L is two lines along its walls, whatever V is
    for name in ("L", "L, V 4"):
        assert (index(name), info(name)) == ([[[5, 5], [5, 29]], [[9, 5], [29, 5]]], [[49, 1, 2, 0]]), name
    # the robot-inside rule is rule 2's: a large U is lines, a small one its cells
    assert (shapes("U around the robot"), info("U around the robot")) == ([2, 2, 2], [[57, 1, 3, 0]])
    assert (shapes("small U around the robot"), info("small U around the robot")) == ([1] * 7, [[7, 1, 0, 0]])
    # the doorway: the wall j = 3 is two lines, and no emitted segment comes near the opening's cells
    door = index("doorway")
    assert [[5, 3], [17, 3]] in door and [[30, 3], [41, 3]] in door and info("doorway") == [[152, 1, 5, 1]]
    opening = np.array([(i, 3) for i in range(19, 29)], float)
    for sh in door:
        assert L._seg_dist(opening, sh[0], sh[-1]).min() >= 1.0, sh
    # a wall three cells thick: one line at an inlier distance of 3 cells, three at 0
    assert info("thick wall, inlier 9")[0][2] == 1 and info("thick wall, inlier 0")[0][2] == 3
    assert info("diagonal wall")[0][2] >= 1 and info("6 x 6 blob")[0][2] >= 1
    # fewer than min_inliers cells: the polygon step's output
    small = by["min_inliers - 1 cells"]
    assert info("min_inliers - 1 cells") == [[9, 1, 0, 0]] and L.same(seen[small.name][:6], K.host_polygons(small.polygons())[:6]) is None
    # both enumeration branches, on either side of r (r - 1) / 2 = n_hypotheses
    assert 12 * 11 // 2 == by["12 cells, 66 hypotheses"].nh == by["12 cells, 65 hypotheses"].nh + 1
    assert len(L.hypotheses(12, 0, 66)) == 66 and len(L.hypotheses(12, 0, 65)) == 65 and L.hypotheses(12, 0, 66)[:2] == [(0, 1), (0, 2)] != L.hypotheses(12, 0, 65)[:2]
    assert info("12 cells, 66 hypotheses") == [[12, 1, 2, 0]]
    # r = remaining_outliers: nothing is extracted; one more cell: a line
    assert (info("r = remaining_outliers"), shapes("r = remaining_outliers")) == ([[6, 1, 0, 6]], [1] * 6)
    assert (info("r = remaining_outliers + 1"), index("r = remaining_outliers + 1")) == ([[7, 1, 1, 0]], [[[3, 3], [9, 3]]])
    # the two bars of the plus score 9 each: the one whose pair comes first wins, the other one is two runs of 4 < min_inliers
    assert index("two hypotheses of equal score")[0] == [[4, 8], [12, 8]] and info("two hypotheses of equal score") == [[17, 1, 1, 8]]
    # (2 len)^2 = link_dist_sq len^2 at link_dist_sq 4 is no break, (3 len)^2 is one
    assert [[3, 4], [17, 4]] in index("gap at the threshold") and info("gap at the threshold")[0][2] == 2
    assert [[3, 4], [9, 4]] in index("gap one cell wider") and [[12, 4], [18, 4]] in index("gap one cell wider") and info("gap one cell wider")[0][2] == 3
    # a score of 16 over runs of 4: extraction stops, the cells come out as points
    assert info("largest run of min_inliers - 1") == [[41, 1, 1, 16]] and shapes("largest run of min_inliers - 1") == [2] + [1] * 16
    assert (no("capacity"), dr("capacity"), shapes("capacity")) == ([3], [3], [2, 2, 2])
    assert info("pose not a number") == [[49, 1, 2, 0]] * 2
    # the int64 bound: 4095 cells in one line of a map as long as the step accepts
    for name in ("4096 x 2", "2 x 4096"):
        assert info(name)[0][:2] == [4095, 1] and info(name)[0][2] >= 1 and dr(name) == [0], name


def test_every_kept_cell_is_covered_and_no_line_overreaches(all_cases, seen, restated, random_maps):
    """Conditions that follow from the rule, not measurements.  Cover: every kept cell lies within 2 sqrt(inlier_dist_sq) cells of an emitted obstacle, or inside or
    on an emitted small-cluster shape (inliers are within the inlier distance of the hypothesis line, and so are the two cells the emitted segment ends in).  No
    overreach: every point at quarter-cell spacing on a rule-3 line lies within sqrt(link_dist_sq / 4 + 4 inlier_dist_sq) cells of a kept cell of that cluster (run gaps
    are at most the link distance).  Inputs on which the restatement alone misses a bound are left out first; then the host build's outputs are held to both."""
    inputs = [(c, seen[c.name]) + restated[c.name] for c in all_cases] + list(random_maps)
    chosen = [(c, mine, meta) for c, mine, ref, meta in inputs if L.bounds_miss(c, ref, meta) is None]
    print(f"{len(chosen)} of {len(inputs)} inputs meet both bounds in the restatement")
    assert len(chosen) >= len(inputs) - 5
    for c, mine, meta in chosen:
        assert L.bounds_miss(c, mine, meta) is None, (c.name, L.bounds_miss(c, mine, meta))
    assert sum(int((mine[5] == 0).sum()) for _, mine, _ in chosen) > 60          # the bounds are looked at where nothing was dropped


def test_the_l_keeps_its_free_corner(all_cases, seen):
    """the cell (12, 12) in the corner of the L is strictly inside the triangle the polygon step emits, and at least 3 cells away from everything the line step emits"""
    c = [c for c in all_cases if c.name == "L"][0]
    corner = np.array([[12.0, 12.0]])
    poly = K.host_polygons(c.polygons())
    assert poly[0].tolist() == [1] and poly[1][0, 0] == 3
    tri = (poly[2][0, 0, :3] - c.origin[0]) / c.res - 0.5
    for k in range(3):
        o, a = tri[k], tri[(k + 1) % 3]
        assert (a[0] - o[0]) * (corner[0, 1] - o[1]) - (a[1] - o[1]) * (corner[0, 0] - o[0]) > 0.0
    mine = seen["L"]
    for s in range(int(mine[0][0])):
        sh = (mine[2][0, s, :mine[1][0, s]] - c.origin[0]) / c.res - 0.5
        assert L._seg_dist(corner, sh[0], sh[-1])[0] >= 3.0


def test_slots_and_vertices_that_are_not_written_keep_their_bytes(all_cases, seen):
    for c in all_cases:
        no, nv, vt, rd, vl, _, _ = seen[c.name]
        for b in range(c.B):
            n = int(no[b])
            assert 0 <= n <= c.O and (nv[b, n:] == L.ISENTINEL).all() and (vt[b, n:] == L.SENTINEL).all(), c.name
            assert ((nv[b, :n] >= 1) & (nv[b, :n] <= c.V)).all(), c.name
            for o in range(n):
                assert (vt[b, o, nv[b, o]:] == L.SENTINEL).all() and np.isfinite(vt[b, o, :nv[b, o]]).all(), c.name
            if rd is not None:
                assert (rd[b, :n] == 0).all() and (rd[b, n:] == L.SENTINEL).all(), c.name
            if vl is not None:
                assert (vl[b, :n] == 0).all() and (vl[b, n:] == L.SENTINEL).all(), c.name


def test_results_do_not_depend_on_the_batch(all_cases, seen):
    many = [c for c in all_cases if c.B > 1]
    assert any(c.name == "three maps" for c in many)
    for c in many:
        for b in range(c.B):
            alone = L.host_lines(c.take(b))
            assert L.same(tuple(None if a is None else np.ascontiguousarray(a[b:b + 1]) for a in seen[c.name]), alone) is None, (c.name, b)
    # the same map alone and as entry 5 of 7
    for name in ("doorway", "L", "small U around the robot"):
        c = [c for c in all_cases if c.name == name][0]
        among = L.host_lines(c.at(5, 7))
        assert L.same(tuple(None if a is None else np.ascontiguousarray(a[5:6]) for a in among), seen[name]) is None, name


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, restated, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as the restatement gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("costmap_lines_host", ("CLH_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    L.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, L.read_outputs(dst, all_cases)):
        assert L.same(got, restated[c.name][0]) is None, c.name


def test_line_params_from_options_reads_the_shipped_converter_block():
    """the values of the shipped costmap_converter_params.yaml, typed in here"""
    block = {"cluster_max_distance": 0.4, "cluster_min_pts": 2, "ransac_inlier_distance": 0.15, "ransac_min_inliers": 10, "ransac_no_iterations": 1500,
             "ransac_remainig_outliers": 3, "ransac_convert_outlier_pts": True, "ransac_filter_remaining_outlier_pts": False, "convex_hull_min_pt_separation": 0.1}
    shipped = {"costmap_converter_plugin": "costmap_converter::CostmapToLinesDBSRANSAC", "costmap_converter_spin_thread": True, "costmap_converter_rate": 5,
               "costmap_converter/CostmapToLinesDBSRANSAC": block}
    values = lambda c: (c.link_dist_sq, c.inlier_dist_sq, c.min_inliers, c.n_hypotheses, c.remaining_outliers, c.behind_robot_dist)
    c, notes = P.line_params_from_options(P.plugin_options_from_params(shipped), shipped, 0.05)
    assert (values(c), notes) == ((64, 9, 10, 1500, 3, 1.5), [])
    # nested the other way, other values, the behind-robot distance of the planner's own block
    other = {"costmap_converter_plugin": "costmap_converter::CostmapToLinesDBSRANSAC", "collision_avoidance": {"costmap_obstacles_behind_robot_dist": 0.8},
             "costmap_converter": {"CostmapToLinesDBSRANSAC": {"cluster_max_distance": 0.25, "ransac_inlier_distance": 0.1, "ransac_min_inliers": 6, "ransac_no_iterations": 300,
                                                               "ransac_remainig_outliers": 0}}}
    c, notes = P.line_params_from_options(P.plugin_options_from_params(other), other, 0.05)
    assert (values(c), notes) == ((25, 4, 6, 300, 0, 0.8), [])
    # the defaults without a block; the clamps of the inlier distance at both ends
    c, notes = P.line_params_from_options(P.plugin_options_from_params({}), None, 0.05)
    assert (values(c), notes) == ((64, 9, 10, 1500, 3, 1.5), [])
    key = "costmap_converter/CostmapToLinesDBSRANSAC"
    assert P.line_params_from_options({}, {key: {"ransac_inlier_distance": 0.01}}, 0.05)[0].inlier_dist_sq == 0
    assert P.line_params_from_options({}, {key: {"ransac_inlier_distance": 1.0}}, 0.05)[0].inlier_dist_sq == 64
    # every note
    for change, word in (({"ransac_convert_outlier_pts": False}, "ransac_convert_outlier_pts"), ({"ransac_filter_remaining_outlier_pts": True}, "ransac_filter_remaining_outlier_pts"),
                         ({"convex_hull_min_pt_separation": 0.3}, "convex_hull_min_pt_separation"), ({"cluster_min_pts": 5}, "cluster_min_pts 5")):
        c, notes = P.line_params_from_options({}, {key: {**block, **change}}, 0.05)
        assert len(notes) == 1 and word in notes[0] and values(c) == (64, 9, 10, 1500, 3, 1.5), change
    for plugin in ("costmap_converter::CostmapToPolygonsDBSMCCH", "costmap_converter::CostmapToLinesDBSMCCH"):
        notes = P.line_params_from_options({"costmap_converter_plugin": plugin}, {}, 0.05)[1]
        assert len(notes) == 1 and plugin in notes[0] and "CostmapToLinesDBSRANSAC" in notes[0]
    # cluster_params_from_options still answers the RANSAC plugin with its note
    assert "clusters and convex hulls are what this library builds" in P.cluster_params_from_options(P.plugin_options_from_params(shipped), shipped, 0.05)[1][0]
    assert math.isclose(c.behind_robot_dist, 1.5)
