"""CPU tests of what is particular to include/mpc_costmap_lines.h: the values of its defaults, and what the library can refuse without a GPU.  Its declarations
against _abi.LINE_PROTOTYPES, the layout of mpc_line_params and the binding are held by tests/test_abi.py, like every header's."""
import ctypes as C

from _abi_check import lib      # noqa: F401 (the fixture)


def test_library_exports_binds_and_refuses_without_a_gpu(lib):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MpcLineParams
    # the defaults need no handle: the shipped block at 0.05 m per cell, the clamps at both ends, the floor in between, quotients that are not numbers
    p = MpcLineParams(-1.0, -1, -1, -1, -1, -1)
    for res, d, inl, want in ((0.05, 0.4, 0.15, (64, 9)), (0.025, 0.4, 0.4, (64, 64)), (0.05, 0.01, 0.01, (1, 0)), (0.05, 0.1, 0.1, (4, 4)), (0.05, 0.12, 0.12, (5, 5)),
                              (0.1, 0.3, 0.15, (9, 2)), (0.05, 0.4, 0.0, (64, 0)), (0.05, 0.4, 0.05, (64, 1)), (0.0, 0.0, 0.0, (1, 0))):
        lib.mpc_line_params_defaults(C.byref(p), res, d, inl)
        assert (p.behind_robot_dist, p.link_dist_sq, p.inlier_dist_sq, p.min_inliers, p.n_hypotheses, p.remaining_outliers) == (1.5,) + want + (10, 1500, 3), (res, d, inl)
    lib.mpc_line_params_defaults(None, 0.05, 0.4, 0.15)
    # without a handle: a refusal instead of a crash
    assert lib.mpc_costmap_to_lines_device(None, 1, None, 8, 8, 0.05, None, None, None, None, None, None, None, None, None, None) == MPC_EINVAL
    assert lib.mpc_costmap_to_lines(None, 1, None, 8, 8, 0.05, None, None, C.byref(p), None, None, None, None, None, None, None) == MPC_EINVAL
    assert b"mpc_costmap_to_lines: null argument" in lib.mpc_last_error()
    assert lib.mpc_version() == 900
