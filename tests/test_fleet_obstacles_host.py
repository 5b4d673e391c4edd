"""CPU tests of the per-instance rules of mpc_obstacles_from_pool* and mpc_fleet_pool* (mpc_local_planner_amd/csrc/mpc_fleet_obstacles.hpp), compiled for the host with g++
by a tests-only harness (tests/host_harness/fleet_obstacles_host.cpp): on every scripted case (tests/_fleet_cases.py) every byte of the container and every count equals a
numpy restatement of include/mpc_fleet.h written independently (np.lexsort on (p, key); products and sums as separate numpy operations); the pool-fill rule equals numpy too;
and the harness, built as a stand-alone program with -fsanitize=address,undefined, runs the scripted cases clean and to the same bytes."""
import subprocess

import numpy as np
import pytest

import _fleet_cases as K
import _harness


@pytest.fixture(scope="module")
def all_cases():
    return K.cases()


def test_scripted_cases_equal_the_numpy_restatement(all_cases):
    seen = {}
    for c in all_cases:
        mine, ref = K.host_select(c), K.numpy_select(c)
        assert K.same(mine, ref) is None, (c.name, K.same(mine, ref))
        seen[c.name] = mine
    no, dr, tk = (lambda name, k=k: seen[name][k].tolist() for k in (0, 5, 6))          # n_obstacles, dropped, n_taken of a case
    # the pool sizes the issue names are all there
    assert all(f"P = {P}" in seen for P in (0, 1, 5, 63, 64, 65, 255, 256, 257, 1000, 2049))
    assert (no("P = 0"), dr("P = 0"), tk("P = 0")) == ([0, 1, 2, 3, 3, 5], [0] * 6, [0] * 6)
    # what the cases are there for does happen
    assert (no("free capacity"), dr("free capacity"), tk("free capacity")) == ([12, 12, 12, 12, 12, 9], [9, 8, 0, 1, 6, 0], [0, 1, 9, 8, 3, 9])      # free 0, 1, exact fit, one and six too many, room to spare
    for P in (255, 256, 257, 1000, 2049):          # the cut among all P keys, with 16, 13, 1 and 0 slots left
        assert (tk(f"P = {P}, all within reach"), dr(f"P = {P}, all within reach")) == ([16, 13, 1, 0], [P - 16, P - 13, P - 1, P])
        assert max(dr(f"P = {P}")) > 0
    assert tk("exactly at reach") == [2] and seen["exactly at reach"][2][0, :2, 0].tolist() == [[3.0, 4.0], [-4.0, 3.0]]      # inclusive; the two just beyond are not taken
    assert tk("reach 0") == [1]
    assert all(a == b + 1 or a == b == 16 for a, b in zip(tk("no self index"), tk("self exclusion"))) and tk("no self index") != tk("self exclusion")
    assert tk("self index -1 and out of range") == tk("no self index")
    t = tk("robot pose not finite")          # a position that is not finite takes nothing; a heading is not looked at
    assert [t[0], t[1], t[2], t[4]] == [0, 0, 0, 0] and t[3] > 0 and no("robot pose not finite")[:3] == [2, 0, 5]
    # ties: all 64 keys equal -> the lowest pool indices, in order
    assert (no("lattice, all keys equal"), dr("lattice, all keys equal"), tk("lattice, all keys equal")) == ([6, 6, 6], [58, 60, 64], [6, 4, 0])
    # robot 7 of the 16 x 16 lattice stands at (0.25, 0) with 3 slots left: (0, 0) and (0.5, 0) tie at 0.0625 and are both taken; (0, +-0.5) and (0.5, +-0.5) tie at
    # 0.3125 and the one with the lowest pool index, (0, -0.5) (x is the outer index), gets the last slot; the three are written in pool order
    lat = seen["lattice 16 x 16"]
    assert tk("lattice 16 x 16")[7] == 3 and lat[2][7, 13:16, 0].tolist() == [[0.0, -0.5], [0.0, 0.0], [0.5, 0.0]]
    assert min(dr("lattice 16 x 16")) > 0 and [c for c in all_cases if c.name == "lattice 46 x 46"][0].P > 2048
    # speeds: at the threshold and above moving, below static; a speed that is not a number is static, an infinite one moves
    v = seen["speeds around min_speed"][4][0, :10]
    assert v[0].tolist() == [0.001, 0.0] and v[1].tolist() == [0.0, 0.0] and v[2, 0] > 0.001 and v[3].tolist() == [0.0, -0.001] and v[5].tolist() == [0.0, 0.0]
    assert v[6].tolist() == [-0.3, 0.4] and v[7].tolist() == [0.0, 0.0] and v[8].tolist() == [0.0, np.inf] and v[9].tolist() == [0.0, 0.0]
    # append keeps what the container held; overwrite starts at slot 0; a full container takes nothing; a count above O counts as O, a negative one as 0
    a, o = seen["append"], seen["overwrite"]
    assert a[2][2, :7, 0].tolist() == [[107.0, 200.0 + k] for k in range(7)] and o[2][2, 0, 0].tolist() != [107.0, 200.0]
    assert tk("append")[4:7] == [0, 0, 16] and no("append")[4:7] == [16, 16, 16] and tk("overwrite") == [16] * 8
    assert len(seen) == len(all_cases) >= 30


def test_slots_outside_the_new_entries_keep_their_bytes(all_cases):
    for c in all_cases:
        before, after = c.container(), K.host_select(c)
        for b in range(c.B):
            base = min(max(int(before[0][b]), 0), c.O) if c.append else 0
            end = int(after[0][b])
            assert base <= end <= c.O and end - base == after[6][b], c.name
            keep = np.r_[0:base, end:c.O]
            for x, y in zip(before[1:], after[1:5]):
                assert (x is None) == (y is None), c.name
                if x is not None:
                    assert x[b, keep].tobytes() == y[b, keep].tobytes(), c.name
            n = after[1][b, base:end]
            assert (n >= 1).all() and (n <= c.V).all(), c.name
            for k, o in enumerate(range(base, end)):          # the vertices behind the valid ones of a written slot
                assert (after[2][b, o, n[k]:] == K.SENTINEL).all(), c.name


def test_results_do_not_depend_on_the_batch(all_cases):
    for c in all_cases:
        if c.B < 4:
            continue
        whole = K.host_select(c)
        rows = np.array([c.B - 1, 0, 2])
        part = K.host_select(c.take(rows))
        assert K.same(tuple(None if a is None else np.ascontiguousarray(a[rows]) for a in whole), part) is None, c.name


def test_pool_fill_equals_numpy():
    h = K.harness()
    pose, x, dt, status, radius = K.pool_fill_inputs()
    B, n = x.shape[:2]
    for V, offset, with_x, with_status, per_robot, with_rv in ((1, 0, True, True, True, True), (4, 13, True, False, False, True), (1, 5, False, True, True, True), (2, 0, True, True, False, False)):
        P = offset + B + 3
        pool = (np.full(P, -5, np.int32), np.full((P, V, 2), K.SENTINEL), np.full(P, K.SENTINEL) if with_rv else None, np.full((P, 2), K.SENTINEL) if with_rv else None)
        mine = tuple(None if a is None else a.copy() for a in pool)
        h.fob_pool(B, K.d_(pose), K.d_(x) if with_x else None, n, K.d_(dt) if with_x else None, K.i_(status) if with_status else None, 0.3, K.d_(radius) if per_robot else None, V, offset,
                   K.i_(mine[0]), K.d_(mine[1]), K.d_(mine[2]), K.d_(mine[3]))
        ref = K.numpy_pool_fill(pose, x if with_x else None, dt, status if with_status else None, radius if per_robot else 0.3, V, offset, pool)
        for a, b in zip(mine, ref):
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), (V, offset)
        if with_x and with_status and with_rv:          # every branch was there: failed statuses, dt = 0, < 0, NaN and inf, states that are not finite -- and the two that do not matter
            vel = mine[3][offset:offset + B]
            still = [b for b in range(B) if not vel[b].any()]
            assert set(still) == set(range(3, B, 9)) | {5, 6, 7, 8, 10, 11, 12, 13} and np.isfinite(vel).all()


def test_harness_runs_the_scripted_cases_clean_under_address_and_undefined_sanitizers(all_cases, tmp_path):
    """the stand-alone program (own main) built with -fsanitize=address,undefined reads the scripted cases from a file and writes its results to another: clean, and the
    same bytes as numpy gives; nothing sanitized is loaded into Python"""
    exe = _harness.sanitized("fleet_obstacles_host", ("FOB_MAIN",))
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    K.write_cases(src, all_cases)
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(all_cases)} cases" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    for c, got in zip(all_cases, K.read_outputs(dst, all_cases)):
        assert K.same(got, K.numpy_select(c)) is None, c.name
