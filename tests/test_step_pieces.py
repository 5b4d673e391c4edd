"""CPU test of the piece list of a host-pointer call (mpc_problem.hpp::step_pieces), compiled for the host with g++ by a tests-only harness
(tests/host_harness/step_pieces_host.cpp).  mpc_create sizes the handle's two staging blocks by evaluating the function at max_batch with every optional array
present; mpc_solve_batch / mpc_step_batch pack with the same function.  For every call: what it packs is at most that capacity, no two pieces of a block overlap,
and every piece starts on a 256-byte boundary."""
import ctypes as C
import itertools

import pytest

from mpc_local_planner_amd import _abi as A
import _harness


MAX_BATCH = 16384
OPTIONAL = ("u_prev", "dt_prev", "init", "radius", "velocity")      # bit i of the flags: the call passes that array (init: x_init, u_init and dt_init)
OBSTACLES = {"O0": dict(), "O1_V1": dict(max_obstacles=1, max_vertices=1), "O3_V4": dict(max_obstacles=3, max_vertices=4)}


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(_harness.shared("step_pieces_host"))
    lib.check_call.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_char_p, C.c_int]
    lib.check_call.restype = C.c_int
    return lib


@pytest.mark.parametrize("dynamic", (False, True), ids=("static", "dynamic_obstacles"))
@pytest.mark.parametrize("obstacles", sorted(OBSTACLES))
@pytest.mark.parametrize("B", (1, MAX_BATCH))
@pytest.mark.parametrize("n", (3, 50))
def test_every_call_fits_the_capacity_without_overlap_on_256_byte_boundaries(h, n, B, obstacles, dynamic):
    cfg = A.config_carlike_min_time(n, enable_dynamic_obstacles=dynamic, **OBSTACLES[obstacles])
    for flags in range(1 << len(OPTIONAL)):          # with and without each optional input
        err = C.create_string_buffer(256)
        rc = h.check_call(C.addressof(cfg), MAX_BATCH, B, flags, err, 256)
        assert rc == 0, ([name for i, name in enumerate(OPTIONAL) if flags >> i & 1], err.value.decode())


def test_the_harness_refuses_a_call_beyond_max_batch(h):
    """the check can fail: a call of more instances than the capacity was computed for does not fit"""
    cfg = A.config_carlike_min_time(50)
    err = C.create_string_buffer(256)
    assert h.check_call(C.addressof(cfg), 64, 65, 0, err, 256) == 1 and err.value.decode().startswith("the call packs more than the capacity")
