"""CPU tests of the per-instance rule of mpc_scan_cast* (mpc_local_planner_amd/csrc/mpc_scan_cast.hpp), compiled for the host with g++ by a tests-only harness
(tests/host_harness/scan_cast_host.cpp): on every scripted case (tests/_cast_cases.py) and on 40 random scenes every range, hit word and count equals, bit for bit, a
Python restatement written from the text of include/mpc_scan_cast.h; the scripted cases do what they are named for; two properties that do not depend on the rule hold
(the analytic wall distance of a rectangular room, no blocking cell in front of a return); the consumer, the host build of mpc_costmap_scans.hpp, marks only blocking
map cells from the cast ranges; and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs the scripted cases clean and to the same bytes.
The reader of a Stage ranger block is tested here too, on the numbers of ex/stage/robots/carlike_robot.inc."""
import math
import subprocess

import numpy as np
import pytest

import _cast_cases as Cc
import _harness
import _scan_cases as Sc
from mpc_local_planner_amd import params as P


@pytest.fixture(scope="module")
def all_cases():
    return Cc.cases()


@pytest.fixture(scope="module")
def seen(all_cases):
    return {c.name: Cc.host_cast(c) for c in all_cases}


@pytest.fixture(scope="module")
def restated(all_cases):
    """name -> (the restatement's result, its trace per instance)"""
    out = {}
    for c in all_cases:
        trace = []
        out[c.name] = (Cc.python_cast(c, trace), trace)
    return out


def test_scripted_cases_equal_the_python_restatement(all_cases, seen, restated):
    for c in all_cases:
        assert Cc.same(seen[c.name], restated[c.name][0]) is None, (c.name, Cc.same(seen[c.name], restated[c.name][0]))
    assert len(seen) == len(all_cases) >= 35


def test_random_scenes_equal_the_python_restatement():
    cs = Cc.random_cases()
    by_map = by_pool = missed = off_map = 0
    for c in cs:
        trace = []
        mine, ref = Cc.host_cast(c), Cc.python_cast(c, trace)
        assert Cc.same(mine, ref) is None, (c.name, Cc.same(mine, ref))
        by_map, by_pool, missed = by_map + int((mine[1] == Cc.MAP).sum()), by_pool + int((mine[1] >= 0).sum()), missed + int((mine[1] == Cc.MISS).sum())
        off_map += sum(t["valid"] and not t["on_map"] for t in trace)
    # the generator gives the step something to do
    assert len(cs) == 40 and max(c.B for c in cs) <= 8
    assert by_map > 1000 and by_pool > 200 and missed > 200 and off_map >= 3, (by_map, by_pool, missed, off_map)


def test_the_cases_do_what_they_are_there_for(all_cases, seen, restated):
    by = {c.name: c for c in all_cases}
    tr = lambda name: restated[name][1]
    rng, hit, info = (lambda name: seen[name][0]), (lambda name: seen[name][1]), (lambda name: seen[name][2])
    f32 = np.float32
    # along an axis: sine exactly 0, cosine exactly 1; the wall 26.5 cells ahead, then up, behind and below
    beams = tr("a beam along an axis")[0]["beams"]
    assert beams[0]["dir"] == (1.0, 0.0) and beams[0]["ties"] == 0 and rng("a beam along an axis")[0, 0] == f32(26.5 * 0.05)
    assert np.allclose(rng("a beam along an axis")[0], [1.325, 0.925, 0.975, 0.975], atol=1e-6) and (hit("a beam along an axis") == Cc.MAP).all()
    # the corner: one step, with a tie, along x into the blocking cell; a step along y would have found (3, 1) and then (4, 1) free and gone on to a miss
    b = tr("a tie at a cell corner")[0]["beams"][0]
    assert b["ties"] >= 1 and b["steps"] == 1 and b["cell"] == (4, 0) and b["t_in"] == b["t_out"] and hit("a tie at a cell corner")[0, 0] == Cc.MAP
    assert rng("a tie at a cell corner")[0, 0] == f32(b["t_in"] * 0.5) and abs(b["t_in"] - math.sqrt(0.5)) < 1e-15
    assert (rng("the sensor's own cell blocking") == 0.0).all() and (hit("the sensor's own cell blocking") == Cc.MAP).all()
    off = "the sensor off the map"
    assert [t["on_map"] for t in tr(off)] == [False] * 3 and (hit(off) != Cc.MAP).all() and (info(off)[:, 3] == 0).all() and (info(off)[:, 0] == 0).all()
    assert (hit(off)[0] == 0).sum() >= 1 and (hit(off)[1:] == Cc.MISS).all()          # the disc off the map is still seen
    assert (hit("a ray leaving the map") == Cc.MISS).all() and np.isinf(rng("a ray leaving the map")).all() and info("a ray leaving the map").tolist() == [[0, 0, 24, 0]]
    # range_max: strictly below it returns, at it does not; the midpoint decides when it is the reported point
    assert rng("a return just inside range_max")[0, 0] == f32(1.325) and hit("a return just inside range_max")[0, 0] == Cc.MAP
    assert np.isinf(rng("a return just beyond range_max")[0, 0]) and hit("a return just beyond range_max")[0, 0] == Cc.MISS
    mid = tr("the midpoint beyond range_max while the entry is inside")[0]["beams"][0]
    assert mid["t_in"] * 0.05 < 1.335 < mid["r_map"] and hit("the midpoint beyond range_max while the entry is inside")[0, 0] == Cc.MISS
    assert rng("the entry inside range_max, reported at the entry")[0, 0] == f32(1.325)
    # the column of 100 at cell 25 (4.5 cells ahead), of 255 at cell 30 (9.5), the wall at 47 (26.5)
    assert [float(rng(n)[0, 0]) for n in ("unknown cells pass, threshold 254", "unknown cells block", "a threshold below 254")] == [float(f32(v * 0.05)) for v in (26.5, 9.5, 4.5)]
    assert (rng("a disc around the sensor") == 0.0).all() and (hit("a disc around the sensor") == 0).all() and info("a disc around the sensor")[0, :3].tolist() == [0, 16, 0]
    assert hit("a disc behind the sensor")[0, 0] == Cc.MAP
    assert hit("a tangent ray")[0, 0] == 0 and rng("a tangent ray")[0, 0] == 1.0 and hit("a ray just past the tangent")[0, 0] == Cc.MAP
    h = hit("self_index honoured")
    assert (h[0] != 0).all() and (h[0] == 1).any() and (h[1] == 0).all() and (h[2] == 0).all()
    assert hit("a segment parallel to the beam")[0, 0] == Cc.MAP
    assert hit("a polygon's closing edge")[0, 0] == 0 and rng("a polygon's closing edge")[0, 0] == 0.5 and rng("the same vertices as an open pair")[0, 0] > 1.0
    near = "a pool entry nearer than the wall and one behind it"
    assert hit(near)[0].tolist() == [0, Cc.MAP] and abs(rng(near)[0, 0] - 0.675) < 1e-6 and tr(near)[0]["beams"][1]["r_pool"] > tr(near)[0]["beams"][1]["r_map"]
    tie = tr("a map/pool tie")[0]["beams"]
    assert all(b["r_map"] == b["r_pool"] == 0.0 for b in tie) and (hit("a map/pool tie") == Cc.MAP).all()
    nf = "a pose that is not finite"
    assert info(nf)[:5].tolist() == [[-1, 0, 0, 0]] * 5 and np.isinf(rng(nf)[:5]).all() and (hit(nf)[:5] == Cc.MISS).all() and info(nf)[5, 0] > 0 and info(nf)[5, 3] > 100
    assert np.isinf(rng("miss_is_inf 1")).all() and (rng("miss_is_inf 0") == f32(1.5)).all() and (hit("miss_is_inf 0") == Cc.MISS).all()
    assert rng("a blocking cell at bit 63")[0, 1] == f32(1.5 * 0.05) and rng("a blocking cell at bit 64")[0, 1] == f32(2.5 * 0.05)
    assert set(np.unique(hit("pool entries that are skipped"))) <= {Cc.MAP, 5} and (hit("pool entries that are skipped") == 5).any()
    assert seen["no hit, no info"][1] is None and seen["no hit, no info"][2] is None
    # rule 5's count: the whole ring of the room lies within Rc of any sensor in it
    assert info("1 beams")[:, 3].tolist() == [2 * 48 + 2 * 38] * 2


def test_a_rectangular_room_gives_the_analytic_wall_distance_within_one_float_ulp():
    """hit_point 0: the return is where the beam enters the wall's ring, at x = 0.05 or 2.35, y = 0.05 or 1.95; the direction is rule 1's"""
    grid = Cc.room()
    rng = np.random.default_rng(3)
    pose = np.column_stack([rng.uniform(0.1, 2.3, 8), rng.uniform(0.1, 1.9, 8), rng.uniform(-3.1, 3.1, 8)])
    c = Cc.Case("room", grid, pose, 360, hit_point=0, range_max=3.0)
    ranges, hit, _ = Cc.host_cast(c)
    assert (hit == Cc.MAP).all()
    for b in range(8):
        for k in range(360):
            sn, cs = Sc.sincos(Sc.wrap((pose[b, 2] + c.angle_min) + k * c.angle_inc))
            tx = ((2.35 if cs > 0 else 0.05) - pose[b, 0]) / cs if cs else math.inf
            ty = ((1.95 if sn > 0 else 0.05) - pose[b, 1]) / sn if sn else math.inf
            want = np.float32(min(tx, ty))
            assert abs(float(ranges[b, k]) - float(want)) <= float(np.spacing(want)), (b, k, ranges[b, k], want)


def test_no_blocking_cell_lies_in_front_of_a_return():
    """hit_point 0, random rooms: along every beam the map returns, sampled every tenth of a cell up to a hundredth of a cell before the return, every cell is free"""
    checked = 0
    for grid, pose in Cc.random_rooms(count=6):
        c = Cc.Case("rooms", grid, pose, 180, hit_point=0, range_max=2.0)
        ranges, hit, _ = Cc.host_cast(c)
        blocking = c.blocking()
        for b in range(c.B):
            th = pose[b, 2] + c.angle_min + c.angle_inc * np.arange(c.n)
            for k in np.flatnonzero(hit[b] == Cc.MAP):
                t = np.arange(0.0, float(ranges[b, k]) / c.res - 0.01, 0.1)
                i, j = np.floor(pose[b, 0] / c.res + t * math.cos(th[k])).astype(int), np.floor(pose[b, 1] / c.res + t * math.sin(th[k])).astype(int)
                assert not blocking[j, i].any(), (b, k)
                checked += len(t)
    assert checked > 100000


def test_the_consumer_marks_only_blocking_map_cells_from_the_cast_ranges():
    """hit_point 1; a window of the map's resolution anchored at map_origin, large enough for range_max on every side; obstacle_range above range_max.  Every cell the host
    build of mpc_costmap_scans.hpp marks is a blocking map cell.  Beams whose chord through the hit cell is below 1e-4 m are left out, and are at most 1 % of all."""
    beams = left_out = marks = 0
    for grid, pose in Cc.random_rooms():
        c = Cc.Case("rooms", grid, pose, 360, hit_point=1, range_max=2.0)
        ranges, hit, _, chord = Cc.host_cast(c, chord=True)
        short = chord < 1e-4
        beams, left_out = beams + int((hit == Cc.MAP).sum()), left_out + int(short.sum())
        fed = np.where(short, np.float32(np.inf), ranges)
        s = Sc.Case("consumer", pose, fed, (100, 100), c.res, angle_min=c.angle_min, angle_inc=c.angle_inc, range_min=0.0, range_max=c.range_max, obstacle_range=c.range_max + 1.0,
                    raytrace_range=c.range_max, clearing=0, track_unknown=0, no_cost=True)
        layer, cell, _, _ = Sc.host_scans(s)
        blocking = c.blocking()
        for b in range(c.B):
            ys, xs = np.nonzero(layer[b] == Sc.LETHAL)
            mx, my = xs + cell[b, 0], ys + cell[b, 1]
            assert ((mx >= 0) & (mx < grid.shape[1]) & (my >= 0) & (my < grid.shape[0])).all(), b
            assert blocking[my, mx].all(), (b, [(int(x), int(y)) for x, y in zip(mx, my) if not blocking[y, x]][:5])
            marks += len(xs)
    assert beams > 40000 and marks > 3000 and left_out <= 0.01 * beams, (beams, left_out, marks)


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, restated, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as the restatement gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("scan_cast_host", ("SCH_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    Cc.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, Cc.read_outputs(dst, all_cases)):
        assert Cc.same(got, restated[c.name][0]) is None, c.name


def test_the_lds_cap_is_what_the_header_says():
    lib = Cc.harness()
    cap = lib.sch_max_rc()
    assert cap == 351 and lib.sch_lds_bytes(cap) <= 65536 < lib.sch_lds_bytes(cap + 1)
    assert lib.sch_lds_bytes(131) < 20000 and lib.sch_lds_bytes(321) <= 65536          # 6.5 m and 16 m at 0.05 m
    assert lib.sch_lds_bytes(cap) == 703 * 11 * 8 + 4 * lib.sch_list_cap() + 64


def test_cast_params_from_the_carlike_ranger():
    """ex/stage/robots/carlike_robot.inc: range_max 6.5, fov 58.0, samples 640, pose [-0.1 0.0 ...]; the map of the demos at 0.05 m"""
    p = P.cast_params_from_ranger(58.0, 640, 6.5, (-0.1, 0.0, 0.0), 0.05, (400, 600))
    assert (p.angle_min, p.angle_increment) == (-math.radians(58.0) / 2, math.radians(58.0) / 639)
    assert abs(p.angle_min + 639 * p.angle_increment - math.radians(29.0)) < 1e-15
    assert (p.range_max, tuple(p.sensor_pose), p.map_resolution, p.map_size_x, p.map_size_y, tuple(p.map_origin)) == (6.5, (-0.1, 0.0, 0.0), 0.05, 600, 400, (0.0, 0.0))
    assert (p.block_threshold, p.unknown_blocks, p.hit_point, p.miss_is_inf) == (254, 0, 1, 1)
    one = P.cast_params_from_ranger(58.0, 1, 6.5, (0, 0, 0), 0.05, (4, 4))
    assert (one.angle_min, one.angle_increment) == (0.0, 0.0)
    with pytest.raises(ValueError):
        P.cast_params_from_ranger(58.0, 0, 6.5, (0, 0, 0), 0.05, (4, 4))
