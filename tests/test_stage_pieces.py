"""CPU test of the layout of a staged host-pointer call (mpc_problem.hpp::stage_layout), compiled for the host with g++ by a tests-only harness
(tests/host_harness/stage_pieces_host.cpp).  staged_call of mpc_capi.hip places the arrays of mpc_evaluate_batch, mpc_plan_inputs_batch, mpc_commands_batch,
mpc_controller_step_batch, mpc_costmap_to_obstacles and mpc_check_feasibility with it in the handle's shared staging pair.  Piece lists of 1 to 24 pieces, every
direction, given and left out, of 0, 1, 255, 256, 257 and 16384 x 24 bytes; for every list: offsets on 256-byte boundaries, no two pieces overlapping, every IN and
INOUT piece (and no OUT piece) inside the range of the one copy to the device, every INOUT and OUT piece (and no IN piece) inside the range of the one copy back,
NULL for an absent piece, and a total that is the end of the last piece."""
import ctypes as C
import itertools
import random

import pytest

import _harness


IN, INOUT, OUT_ = 0, 1, 2
SIZES = (0, 1, 255, 256, 257, 16384 * 24)
MAX_PIECES = 24
ONE = [(d, g, b) for d in (IN, INOUT, OUT_) for g in (0, 1) for b in SIZES]      # every piece there is: direction, given or not, bytes


@pytest.fixture(scope="module")
def h():
    lib = C.CDLL(_harness.shared("stage_pieces_host"))
    lib.check_list.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_int, C.c_char_p, C.c_int]
    lib.check_list.restype = C.c_int
    return lib


def _check(h, pieces):
    n = len(pieces)
    err = C.create_string_buffer(256)
    rc = h.check_list((C.c_int * n)(*[p[0] for p in pieces]), (C.c_uint64 * n)(*[p[2] for p in pieces]), (C.c_int * n)(*[p[1] for p in pieces]), n, err, 256)
    return rc, err.value.decode()


def test_every_single_piece_and_every_pair(h):
    for pieces in itertools.chain(itertools.product(ONE, repeat=1), itertools.product(ONE, repeat=2)):
        assert _check(h, pieces) == (0, ""), pieces


@pytest.mark.parametrize("count", range(3, MAX_PIECES + 1))
def test_lists_of_every_length_in_every_direction(h, count):
    rng = random.Random(count)
    lists = [[(d, rng.randrange(4) != 0, rng.choice(SIZES)) for _ in range(count)] for d in (IN, INOUT, OUT_)]      # one direction only
    lists += [[(d, 1, b) for d in (OUT_, INOUT, IN) for b in SIZES[1:]][:count]]                                    # all given, listed against the block's order
    lists += [[rng.choice(ONE) for _ in range(count)] for _ in range(200)]
    for pieces in lists:
        assert _check(h, pieces) == (0, ""), pieces


def test_the_harness_refuses_a_list_longer_than_a_layout_holds(h):
    """the check can fail"""
    rc, why = _check(h, [(IN, 1, 1)] * (MAX_PIECES + 1))
    assert rc == 1 and why.startswith("the list is longer than a layout holds")
