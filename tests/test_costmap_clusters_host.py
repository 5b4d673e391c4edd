"""CPU tests of the per-instance rule of mpc_costmap_to_polygons* (mpc_local_planner_amd/csrc/mpc_costmap_clusters.hpp), compiled for the host with g++ by a tests-only
harness (tests/host_harness/costmap_clusters_host.cpp): on every scripted case (tests/_cluster_cases.py) and on random maps every byte of the container and every count
equals a Python restatement of include/mpc_costmap_clusters.h written independently (scipy's cKDTree pairs and connected components, a monotone chain in Python integers
that is itself held to scipy.spatial.ConvexHull); and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs the scripted cases clean and to
the same bytes.  The reader of the converter's parameters is tested here too."""
import subprocess

import numpy as np
import pytest
from scipy.spatial import ConvexHull

import _cluster_cases as K
import _harness
from mpc_local_planner_amd import params as P


@pytest.fixture(scope="module")
def all_cases():
    return K.cases()


@pytest.fixture(scope="module")
def seen(all_cases):
    return {c.name: K.host_polygons(c) for c in all_cases}


def test_scripted_cases_equal_the_python_restatement(all_cases, seen):
    for c in all_cases:
        assert K.same(seen[c.name], K.python_polygons(c)) is None, (c.name, K.same(seen[c.name], K.python_polygons(c)))
    assert len(seen) == len(all_cases) >= 30


def test_random_maps_equal_the_python_restatement():
    clusters = 0
    for c in K.random_cases():
        mine, ref = K.host_polygons(c), K.python_polygons(c)
        assert K.same(mine, ref) is None, (c.name, K.same(mine, ref))
        clusters += int(mine[6][0, 1])
    assert clusters > 400          # the generator does make clusters


def test_large_maps_equal_the_python_restatement():
    """the map the kernel cannot keep a bitmap of, and clusters wider than the span that still gets a hull"""
    far, wide = K.large_cases()
    for c in (far, wide):
        assert K.same(K.host_polygons(c), K.python_polygons(c)) is None, c.name
    assert far.W * far.H > 1 << 18
    r = K.host_polygons(wide)
    assert r[6].tolist() == [[2 * 4141 + 1 + 4140 + 2, 3, 1, 0]] and r[1][0, :3].tolist() == [2, 4, 2]          # the diagonal pair, the two rows with their bump as a box, the single row as a line


def test_the_cases_do_what_they_are_there_for(seen):
    no, nv, dr = (lambda name, k=k: seen[name][k].tolist() for k in (0, 1, 5))
    info = lambda name: seen[name][6].tolist()
    shapes = lambda name, b=0: seen[name][1][b, :seen[name][0][b]].tolist()          # the vertex counts of the written slots
    # nothing is visited on 1 x 1; one cell on 2 x 2
    assert (no("1 x 1"), info("1 x 1")) == ([0], [[0, 0, 0, 0]]) and (no("2 x 2"), shapes("2 x 2"), info("2 x 2")) == ([1], [1], [[1, 1, 0, 0]])
    # the cells of the last column and row are not there: 8 of the 12 of 17 x 9 remain, as one cluster across the rows; 33 x 33 has cells in both 16-column pieces
    assert info("17 x 9") == [[8, 1, 0, 0]] and info("33 x 33")[0][0] > 100 and info("33 x 33")[0][1] >= 4
    assert (no("last row and column"), shapes("last row and column")) == ([1], [1])
    assert shapes("lone cell") == [1] and seen["lone cell"][3] is None and seen["lone cell"][4] is None
    # collinear clusters are lines from the first to the last cell
    res = 0.0625
    for name, first, last in (("horizontal run", (3, 3), (9, 3)), ("vertical run", (3, 2), (3, 10)), ("diagonal run", (2, 2), (11, 11)), ("sloped run with gaps", (2, 2), (16, 9))):
        assert shapes(name) == [2], name
        assert seen[name][2][0, 0, :2].tolist() == [[(first[0] + 0.5) * res, (first[1] + 0.5) * res], [(last[0] + 0.5) * res, (last[1] + 0.5) * res]], name
    # counter-clockwise in (i, j) from the first cell
    assert shapes("2 x 2 block") == [4] and (seen["2 x 2 block"][2][0, 0, :4] / res - 0.5).tolist() == [[3, 3], [4, 3], [4, 4], [3, 4]]
    assert (shapes("everything lethal"), info("everything lethal")) == ([4], [[31 * 31, 1, 0, 0]])
    assert (no("checkerboard, link 1"), info("checkerboard, link 1"), set(shapes("checkerboard, link 1"))) == ([128], [[128, 128, 0, 0]], {1})
    assert (shapes("checkerboard, link 2"), info("checkerboard, link 2")) == ([6], [[128, 1, 0, 0]])          # two corners of the board are free: a hexagon
    assert shapes("spiral") == [4] and info("spiral")[0][1:] == [1, 0, 0] and info("spiral")[0][0] > 450          # one long thin cluster
    assert (info("two blobs, link 8")[0][1], info("two blobs, link 9")[0][1]) == (2, 1)
    # hulls of 8, 12 and 20 vertices: the second and third do not fit V and become their boxes
    assert (shapes("disc 3"), info("disc 3")[0][2]) == ([8], 0) and (shapes("disc 4"), info("disc 4")[0][2]) == ([4], 1) and (shapes("disc 8, V 16"), info("disc 8, V 16")[0][2]) == ([4], 1)
    assert (seen["disc 4"][2][0, 0, :4] / res - 0.5).tolist() == [[3, 3], [11, 3], [11, 11], [3, 11]]
    # a shape that contains the robot is emitted as its cells, in scan order
    assert (no("U around the robot"), info("U around the robot"), set(shapes("U around the robot"))) == ([57], [[57, 1, 0, 1]], {1})
    first = (seen["U around the robot"][2][0, :18, 0] / res - 0.5).tolist()
    assert first == [[4, j] for j in range(4, 21)] + [[5, 4]]
    # capacity reached inside the cluster emitted as cells: the two single cells and the line before it take 2 slots ((1, 1) and (2, 1) are one line), 5 cells follow
    assert (no("U, capacity reached inside it"), dr("U, capacity reached inside it")) == ([7, 7], [2 + 57 - 7] * 2)
    assert shapes("U, capacity reached inside it") == [2, 1, 1, 1, 1, 1, 1]
    # a pose that is not a number contains nothing (and nothing is behind it); a heading is not looked at
    assert [i[3] for i in info("U, pose not a number")] == [0, 0, 1] and [n for n in no("U, pose not a number")] == [1, 1, 57]
    # closed sets: on a vertex, on an edge, on the box's edge is inside; one cell away is not
    assert info("robot on a hull vertex")[0][3] == 1 and info("robot on a hull edge")[0][3] == 1 and no("robot on a hull vertex") == [9]
    assert [i[3] for i in info("robot one cell outside")] == [0] * 4 and no("robot one cell outside") == [1] * 4
    assert [i[2:] for i in info("robot on the box's edge")] == [[1, 1]] * 3 and [i[2:] for i in info("robot outside the box")] == [[1, 0]] * 2
    # the behind-robot cut takes the back of the U away: two arms, two lines
    assert info("U, nothing cut") == [[57, 1, 0, 1]] and info("U, the back cut away")[0][1:] == [2, 0, 0] and shapes("U, the back cut away") == [2, 2]


def test_slots_and_vertices_that_are_not_written_keep_their_bytes(all_cases, seen):
    for c in all_cases:
        no, nv, vt, rd, vl, _, _ = seen[c.name]
        for b in range(c.B):
            n = int(no[b])
            assert 0 <= n <= c.O and (nv[b, n:] == K.ISENTINEL).all() and (vt[b, n:] == K.SENTINEL).all(), c.name
            assert ((nv[b, :n] >= 1) & (nv[b, :n] <= c.V)).all(), c.name
            for o in range(n):
                assert (vt[b, o, nv[b, o]:] == K.SENTINEL).all() and np.isfinite(vt[b, o, :nv[b, o]]).all(), c.name
            if rd is not None:
                assert (rd[b, :n] == 0).all() and (rd[b, n:] == K.SENTINEL).all(), c.name
            if vl is not None:
                assert (vl[b, :n] == 0).all() and (vl[b, n:] == K.SENTINEL).all(), c.name


def test_results_do_not_depend_on_the_batch(all_cases, seen):
    many = [c for c in all_cases if c.B > 1]
    assert any(c.name == "three maps" for c in many)
    for c in many:
        for b in range(c.B):
            alone = K.host_polygons(c.take(b))
            assert K.same(tuple(None if a is None else np.ascontiguousarray(a[b:b + 1]) for a in seen[c.name]), alone) is None, (c.name, b)


def test_the_python_chain_equals_scipys_convex_hull():
    """area and vertex count of the restatement's hull on random integer point sets (scipy leaves collinear points out too)"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        pts = np.unique(rng.integers(0, int(rng.integers(3, 20)), (int(rng.integers(3, 60)), 2)), axis=0)
        h = K.hull_of(sorted(map(tuple, pts)))
        if len(h) < 3:
            continue
        area2 = sum(h[k][0] * h[(k + 1) % len(h)][1] - h[(k + 1) % len(h)][0] * h[k][1] for k in range(len(h)))
        ref = ConvexHull(pts.astype(float))
        assert area2 > 0 and abs(area2 / 2 - ref.volume) < 1e-9 and len(h) == len(ref.vertices)
        assert h[0] == tuple(pts[np.lexsort((pts[:, 1], pts[:, 0]))[0]])


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as the restatement gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("costmap_clusters_host", ("CCH_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    K.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, K.read_outputs(dst, all_cases)):
        assert K.same(got, K.python_polygons(c)) is None, c.name


def test_cluster_params_from_options_reads_the_shipped_converter_block():
    """the values of the shipped costmap_converter_params.yaml, typed in here"""
    shipped = {"costmap_converter_plugin": "costmap_converter::CostmapToLinesDBSRANSAC", "costmap_converter_spin_thread": True, "costmap_converter_rate": 5,
               "costmap_converter/CostmapToLinesDBSRANSAC": {"cluster_max_distance": 0.4, "cluster_min_pts": 2, "ransac_inlier_distance": 0.15, "ransac_min_inliers": 10,
                                                             "ransac_no_iterations": 1500, "ransac_remainig_outliers": 3, "ransac_convert_outlier_pts": True,
                                                             "ransac_filter_remaining_outlier_pts": False, "convex_hull_min_pt_separation": 0.1}}
    opts = P.plugin_options_from_params(shipped)
    c, notes = P.cluster_params_from_options(opts, shipped, 0.05)
    assert (c.link_dist_sq, c.behind_robot_dist) == (64, 1.5)
    assert len(notes) == 1 and "CostmapToLinesDBSRANSAC" in notes[0] and "clusters and convex hulls are what this library builds" in notes[0]
    # the polygon variant the file names first, at its own block, nested the other way; no note
    poly = {"costmap_converter_plugin": "costmap_converter::CostmapToPolygonsDBSMCCH", "costmap_converter": {"CostmapToPolygonsDBSMCCH": {"cluster_max_distance": 0.25, "cluster_min_pts": 2}},
            "collision_avoidance": {"costmap_obstacles_behind_robot_dist": 0.8}}
    c, notes = P.cluster_params_from_options(P.plugin_options_from_params(poly), poly, 0.05)
    assert (c.link_dist_sq, c.behind_robot_dist, notes) == (25, 0.8, [])
    # defaults 0.4 and 2 without a block; the clamp at both ends; cluster_min_pts above 2 is a note
    c, notes = P.cluster_params_from_options(P.plugin_options_from_params({}), None, 0.05)
    assert (c.link_dist_sq, notes) == (64, [])
    assert P.cluster_params_from_options({}, {"costmap_converter/CostmapToPolygonsDBSMCCH": {"cluster_max_distance": 0.4}}, 0.025)[0].link_dist_sq == 64
    assert P.cluster_params_from_options({}, {"costmap_converter/CostmapToPolygonsDBSMCCH": {"cluster_max_distance": 0.01}}, 0.05)[0].link_dist_sq == 1
    assert P.cluster_params_from_options({}, {"costmap_converter/CostmapToPolygonsDBSMCCH": {"cluster_max_distance": 0.1}}, 0.05)[0].link_dist_sq == 4
    c, notes = P.cluster_params_from_options({}, {"costmap_converter/CostmapToPolygonsDBSMCCH": {"cluster_min_pts": 5}}, 0.05)
    assert len(notes) == 1 and "cluster_min_pts 5" in notes[0] and "clusters and convex hulls are what this library builds" in notes[0]
    for other in ("costmap_converter::CostmapToLinesDBSMCCH", "costmap_converter::CostmapToPolygonsDBSConcaveHull"):
        assert len(P.cluster_params_from_options({"costmap_converter_plugin": other}, {}, 0.05)[1]) == 1
