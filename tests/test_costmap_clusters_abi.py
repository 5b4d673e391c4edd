"""CPU tests of what is particular to include/mpc_costmap_clusters.h: the values of its defaults, and what the library can refuse without a GPU.  Its declarations
against _abi.CLUSTER_PROTOTYPES, the layout of mpc_cluster_params and the binding are held by tests/test_abi.py, like every header's."""
import ctypes as C

from _abi_check import lib      # noqa: F401 (the fixture)


def test_library_exports_binds_and_refuses_without_a_gpu(lib):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MpcClusterParams
    # the defaults need no handle: the shipped 0.4 m at 0.05 m per cell, the clamp at both ends, the floor in between, a quotient that is not a number
    p = MpcClusterParams(-1.0, -1)
    for res, d, want in ((0.05, 0.4, 64), (0.025, 0.4, 64), (0.05, 0.01, 1), (0.05, 0.1, 4), (0.05, 0.12, 5), (0.1, 0.3, 9), (0.0, 0.0, 1)):
        lib.mpc_cluster_params_defaults(C.byref(p), res, d)
        assert (p.behind_robot_dist, p.link_dist_sq) == (1.5, want), (res, d)
    lib.mpc_cluster_params_defaults(None, 0.05, 0.4)
    # without a handle: a refusal instead of a crash
    assert lib.mpc_costmap_to_polygons_device(None, 1, None, 8, 8, 0.05, None, None, None, None, None, None, None, None, None, None) == MPC_EINVAL
    assert lib.mpc_costmap_to_polygons(None, 1, None, 8, 8, 0.05, None, None, C.byref(p), None, None, None, None, None, None, None) == MPC_EINVAL
    assert b"mpc_costmap_to_polygons: null argument" in lib.mpc_last_error()
    assert lib.mpc_last_costmap_ms(None, None) == MPC_EINVAL
    assert lib.mpc_version() == 900
