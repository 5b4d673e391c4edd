"""CPU tests of the per-instance rule of mpc_plant_step* (mpc_local_planner_amd/csrc/mpc_plant.hpp), compiled for the host with g++ by a tests-only harness
(tests/host_harness/plant_host.cpp): on every scripted case (tests/_plant_cases.py) and on 60 random scenes every pose, velocity, stall count and info word equals,
bit for bit, a Python restatement written from the text of include/mpc_plant.h; the scripted cases do what they are named for; properties that do not come from the
restatement hold (no blocking cell under the outline after a free move, omni = diff without a sideways command, the rear-axle car's Euler steps closing in on the exact
arc as they shrink); and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs the scripted cases clean and to the same bytes.  The reader
of a Stage position block is tested here too, on the numbers of the three shipped robot files (tests/golden/shipped_stage_robots.json)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import _cast_cases as Cc
import _harness
import _plant_cases as Pc
from mpc_local_planner_amd import _abi as A, params as P


@pytest.fixture(scope="module")
def all_cases():
    return Pc.cases()


@pytest.fixture(scope="module")
def seen(all_cases):
    return {c.name: Pc.host_step(c) for c in all_cases}


@pytest.fixture(scope="module")
def restated(all_cases):
    """name -> (the restatement's result, its trace per instance)"""
    out = {}
    for c in all_cases:
        trace = []
        out[c.name] = (Pc.python_step(c, trace), trace)
    return out


def test_scripted_cases_equal_the_python_restatement(all_cases, seen, restated):
    for c in all_cases:
        assert Pc.same(seen[c.name], restated[c.name][0]) is None, (c.name, Pc.same(seen[c.name], restated[c.name][0]))
    assert len(seen) == len(all_cases) >= 40


def test_random_scenes_equal_the_python_restatement():
    cs = Pc.random_cases()
    free = by_map = off_map = by_pool = moved = 0
    kinds = set()
    for c in cs:
        mine, ref = Pc.host_step(c), Pc.python_step(c)
        assert Pc.same(mine, ref) is None, (c.name, Pc.same(mine, ref))
        assert 24 <= c.shape[0] <= 48 and 24 <= c.shape[1] <= 48 or c.grid is None
        assert 1 <= c.n_sub <= 8 and 0 <= c.P <= 12
        kinds |= {min(int(n), 3) for n in c.pnv if n > 0}
        if mine[3] is not None:
            info = mine[3][mine[3][:, 0] >= 0]
            free, moved = free + int((info[:, 1] < 0).sum()), moved + int(info[:, 0].sum())
            by_map, off_map, by_pool = by_map + int((info[:, 2] == Pc.MAP).sum()), off_map + int((info[:, 2] == Pc.OFF_MAP).sum()), by_pool + int((info[:, 2] >= 0).sum())
    # the generator gives the step something to do: robots that run free, into the map, off it and into bodies of all three kinds
    assert len(cs) == 60 and kinds == {1, 2, 3}
    assert free >= 20 and moved >= 100 and by_map >= 5 and off_map >= 5 and by_pool >= 5, (free, moved, by_map, off_map, by_pool)


def test_the_cases_do_what_they_are_there_for(all_cases, seen, restated):
    by = {c.name: c for c in all_cases}
    tr = lambda name: restated[name][1]
    pose, vel, stall, info = (lambda n: seen[n][0]), (lambda n: seen[n][1]), (lambda n: seen[n][2]), (lambda n: seen[n][3])
    near = lambda a, b: np.allclose(a, b, rtol=0, atol=1e-12)
    # the four drives, one sub-step of 0.1 s from (1, 1, 0) under (0.4, 0.2, 0.3): what each makes of the command
    assert near(pose("drive: diff")[0], (1.04, 1.0, 0.03)) and near(pose("drive: omni")[0], (1.04, 1.02, 0.03))
    assert near(pose("drive: car, Stage")[0], (1.0 + 0.04 * math.cos(0.3), 1.0, 0.1 * 0.4 * math.sin(0.3) / 0.4))
    assert near(pose("drive: car, rear axle")[0], (1.04, 1.0, 0.1 * 0.4 * math.tan(0.3) / 0.4))
    assert tr("drive: diff")[0]["target"] == [0.4, 0.0, 0.3] and tr("drive: omni")[0]["target"] == [0.4, 0.2, 0.3]
    for name in ("diff", "omni", "car, Stage", "car, rear axle"):
        assert (info(f"drive: {name}")[:, 0] == 1).all() and (info(f"drive: {name}, three sub-steps, the velocity kept")[:, 0] == 3).all(), name
        assert vel(f"drive: {name}") is None and near(vel(f"drive: {name}, three sub-steps, the velocity kept")[0], tr(f"drive: {name}")[0]["target"])          # no a_max: the target at once
    # a_max 1 over 0.1 s: 0.1 per sub-step from rest; 0.4 is reached in the fourth sub-step and kept
    assert vel("the acceleration clamp binds").tolist() == [[0.1, 0.0, 0.1]]
    v = np.array(tr("the acceleration clamp binds, then no longer")[0]["v"])
    assert near(v[:, 0], [0.1, 0.2, 0.3, 0.4, 0.4, 0.4]) and near(v[:, 2], [0.1, 0.2, 0.3, 0.3, 0.3, 0.3]) and v[5, 0] == 0.4 and v[5, 2] == 0.3
    assert near(vel("the acceleration clamp does not bind"), [[0.4, 0.0, 0.3]])
    assert near(pose("the velocity clamp binds"), [[1.025, 1.0, -0.02]]) and near(pose("the velocity clamp does not bind"), [[1.04, 1.0, -0.03]])
    assert vel("no velocity kept") is None and info("no velocity kept").tolist() == [[2, -1, -1, -1]] and tr("no velocity kept")[0]["v"] == [[0.4, 0.0, 0.3]] * 2
    # the wall: moved + stalled = n_substeps, the reason is the map, and the robot stays where the last free sub-step left it
    w = "straight into a wall"
    assert info(w)[0, 0] + stall(w)[0] == by[w].n_sub == 8 and info(w)[0].tolist()[:3] == [4, 4, Pc.MAP] and near(pose(w), [[1.82, 1.0, 0.0]])
    assert [k is None for k in tr(w)[0]["keys"]] == [True] * 4 + [False] * 4
    off = "a vertex off the map, outside_blocks "
    assert info(off + "1")[0].tolist()[:3] == [1, 1, Pc.OFF_MAP] and stall(off + "1")[0] == 3 and info(off + "0").tolist() == [[4, -1, -1, -1]] and pose(off + "0")[0, 0] > 2.1
    # the boundary: the candidate (1, 1.25, 0) and the far end at x = 2 are exact
    e = "an edge that ends on the boundary of a blocking cell"
    assert pose(e).tolist() == [[1.0, 1.25, 0.0]] and info(e).tolist() == [[1, -1, -1, -1]]
    assert info("the same edge from its other end").tolist() == [[0, 0, Pc.MAP, 0]] and pose("the same edge from its other end").tolist() == [[0.5, 1.25, 0.0]]
    assert info("the same edge in a closed outline").tolist() == [[0, 0, Pc.MAP, 1]]          # the edge that BEGINS at the vertex on the boundary
    assert info("a zero-length edge").tolist() == [[3, -1, -1, -1]] and info("a zero-length edge inside a disc").tolist() == [[0, 0, 0, 0]]
    assert info("no footprint").tolist() == [[8, -1, -1, -1]] and pose("no footprint")[0, 0] > 2.35          # through the disc, the wall and the map's edge
    assert info("a footprint of one segment")[0].tolist() == [4, 4, Pc.MAP, 0] and stall("a footprint of one segment")[0] == 4
    for name in ("a disc blocks", "a segment blocks", "a polygon blocks"):
        assert info(name)[0, 0] == 1 and info(name)[0, 1:3].tolist() == [1, 0] and stall(name)[0] == 3, name
        assert Pc.host_step(by[name].variant(pool=None))[3].tolist() == [[4, -1, -1, -1]], name
    assert info("a tie between two pool entries")[0].tolist()[:3] == [1, 1, 1]          # entries 1 and 2 are the same disc; entry 0 is out of the way
    both = "map and pool both block"
    assert info(both)[0].tolist()[:3] == [4, 4, Pc.MAP] and Pc.host_step(by[both].variant(grid=Cc.room() * 0))[3][0].tolist()[:3] == [4, 4, 0]
    assert info("self_index skipped").tolist() == [[2, -1, -1, -1], [0, 0, 0, 0], [0, 0, 0, 0]] and stall("self_index skipped").tolist() == [0, 2, 2]
    nf = "a pose, a command and a velocity that are not finite"
    assert info(nf)[:6].tolist() == [[-1] * 4] * 6 and info(nf)[6].tolist() == [2, -1, -1, -1] and (stall(nf) == 0).all()
    assert pose(nf)[:6].tobytes() == by[nf].pose[:6].tobytes() and vel(nf)[:6].tobytes() == by[nf].vel[:6].tobytes() and not tr(nf)[0]["valid"]
    h = "a heading that does not wrap"
    assert info(h).tolist() == [[-1] * 4, [2, -1, -1, -1]] and pose(h)[0].tolist() == [1.0, 1.0, 1e18]
    t = "a turn so large that the new heading does not wrap"
    assert info(t).tolist() == [[0, 0, Pc.HEADING, -1], [3, -1, -1, -1]] and stall(t).tolist() == [3, 0] and pose(t)[0].tolist() == [1.0, 1.0, 0.0]
    assert info("a steering angle that does not wrap").tolist() == [[-1] * 4, [2, -1, -1, -1]]
    assert seen["no stall, no info"][2] is None and seen["no stall, no info"][3] is None
    assert info("no map").tolist() == [[2, 2, 0, 1], [8, -1, -1, -1]]          # without a map the pool still blocks, and nothing is off it
    assert info("unknown cells block").tolist() == [[0, 0, Pc.MAP, 0]] and info("unknown cells pass").tolist() == [[1, -1, -1, -1]]
    assert (info("a threshold below 254")[:, 2] == Pc.MAP).all()


def test_after_a_free_move_no_blocking_cell_lies_under_the_outline():
    """random rooms, the car-like footprint, one sub-step: the outline at the new pose of every robot that moved, sampled every millimetre with numpy's sine and
    cosine, touches no blocking cell"""
    checked = moved = stalled = 0
    fp = np.array(Pc.CAR + Pc.CAR[:1])
    for grid, pose in Cc.random_rooms(count=12, seed=29):
        c = Pc.Case("rooms", grid, pose, (1.0, 0.0, 0.5), n_sub=1)
        new, _, stall, info = Pc.host_step(c)
        blocking = c.blocking()
        for b in range(c.B):
            if info[b, 0] != 1:
                stalled += 1
                continue
            moved += 1
            x, y, th = new[b]
            w = np.column_stack([x + math.cos(th) * fp[:, 0] - math.sin(th) * fp[:, 1], y + math.sin(th) * fp[:, 0] + math.cos(th) * fp[:, 1]])
            for a, e in zip(w[:-1], w[1:]):
                n = int(np.hypot(*(e - a)) / 1e-3) + 1
                pts = a + np.linspace(0.0, 1.0, n + 1)[:, None] * (e - a)
                i, j = np.floor(pts[:, 0] / c.res).astype(int), np.floor(pts[:, 1] / c.res).astype(int)
                assert not blocking[j, i].any(), (b, new[b])
                checked += len(pts)
    assert moved >= 20 and stalled >= 20 and checked > 30000, (moved, stalled, checked)


def test_omni_and_diff_agree_without_a_sideways_command():
    rng = np.random.default_rng(7)
    grid, pose = Cc.random_rooms(1, seed=3)[0]
    cmd = np.column_stack([rng.uniform(-1, 1, 8), np.zeros(8), rng.uniform(-1, 1, 8)])
    c = Pc.Case("diff", grid, pose, cmd, vel=np.column_stack([rng.uniform(-0.3, 0.3, 8), np.zeros(8), rng.uniform(-0.3, 0.3, 8)]), a_max=(2.0, 2.0, 3.0), n_sub=5, drive=Pc.DIFF)
    assert Pc.same(Pc.host_step(c), Pc.host_step(c.variant(drive=Pc.OMNI))) is None
    assert (Pc.host_step(c)[3][:, 0] > 0).any()


def test_the_rear_axle_car_closes_in_on_the_exact_arc_as_the_step_shrinks():
    """a constant command (0.5 m/s, 0.3 rad) for 1.6 s in 1, 2, 4 .. 64 sub-steps: the exact motion is a circle of radius wheelbase / tan(0.3); the distance of the
    Euler result to it falls with every halving.  The steps are compared with each other, no tolerance is set."""
    v, phi, L, T = 0.5, 0.3, 0.4, 1.6
    w = v * math.tan(phi) / L
    exact = np.array([v / w * math.sin(w * T), v / w * (1.0 - math.cos(w * T))])
    err = []
    for n in (1, 2, 4, 8, 16, 32, 64):
        c = Pc.Case(f"{n} sub-steps", None, (0.0, 0.0, 0.0), (v, 0.0, phi), interval=T / n, n_sub=n, drive=Pc.CAR_REAR, footprint=[])
        pose, _, stall, info = Pc.host_step(c)
        assert info.tolist() == [[n, -1, -1, -1]] and stall[0] == 0
        err.append(float(np.hypot(*(pose[0, :2] - exact))))
    assert all(a > b for a, b in zip(err, err[1:])), err


def test_plant_params_from_the_shipped_position_blocks():
    """the numbers of the reference's three robot files (values only, tests/golden/shipped_stage_robots.json): the car-like block gives the footprint its line 16 prints"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shipped_stage_robots.json")) as f:
        shipped = json.load(f)
    made = {}
    for name, r in shipped["robots"].items():
        p = made[name] = P.plant_params_from_position(r["drive"], r["wheelbase"], r["size"], r["origin"], shipped["interval_sim_ms"]["value"], 0.05, (400, 600))
        assert (p.interval, p.n_substeps, p.n_footprint, p.map_resolution, p.map_size_x, p.map_size_y, tuple(p.map_origin)) == (0.1, 1, 4, 0.05, 600, 400, (0.0, 0.0))
        assert (p.block_threshold, p.unknown_blocks, p.outside_blocks) == (254, 0, shipped["boundary"]["value"]) and p.wheelbase == 0.4
        assert tuple(p.v_min) == (-math.inf,) * 3 and tuple(p.v_max) == tuple(p.a_max) == (math.inf,) * 3
    car = made["carlike_robot"]
    assert np.allclose([tuple(car.footprint[j]) for j in range(4)], shipped["robots"]["carlike_robot"]["footprint_comment"], rtol=0, atol=1e-15) and car.drive == A.DRIVE_CAR_STAGE
    assert [tuple(made["diff_drive_robot"].footprint[j]) for j in range(4)] == [(-0.125, -0.125), (0.125, -0.125), (0.125, 0.125), (-0.125, 0.125)]
    assert (made["diff_drive_robot"].drive, made["omnidir_robot"].drive) == (A.DRIVE_DIFF, A.DRIVE_OMNI)
    with pytest.raises(P.ParamNotImplemented):
        P.plant_params_from_position("tracked", None, (0.25, 0.25, 0.4), (0, 0, 0, 0), 100, 0.05, (4, 4))
    with pytest.raises(P.ParamNotImplemented):
        P.plant_params_from_position("diff", None, (0.25, 0.25, 0.4), (0, 0, 0, 30.0), 100, 0.05, (4, 4))
    with pytest.raises(ValueError):
        P.plant_params_from_position("diff", None, (0.25, 0.25, 0.4), (0, 0, 0, 0), 0, 0.05, (4, 4))


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, restated, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as the restatement gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("plant_host", ("PLH_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    Pc.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, Pc.read_outputs(dst, all_cases)):
        assert Pc.same(got, restated[c.name][0]) is None, c.name


def test_the_kernels_shape_is_what_the_header_says():
    lib = Pc.harness()
    assert lib.plh_list_cap() == 512 and lib.plh_threads() == 64
