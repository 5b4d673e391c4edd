"""CPU tests of what is particular to include/mpc_fleet.h: the defaults that need no handle, and a refusal instead of a crash without one.  Its declarations against
_abi.FLEET_PROTOTYPES, the layouts of mpc_pool and mpc_pool_params and the binding are held by tests/test_abi.py, like every header's."""
import ctypes as C

from _abi_check import lib      # noqa: F401 (the fixture)


def test_library_exports_and_binds_the_fleet_functions(lib):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MpcPoolParams
    # without a handle: the defaults that do not depend on one, and a refusal instead of a crash
    p = MpcPoolParams(-1.0, -1.0, -1)
    lib.mpc_pool_params_defaults(None, C.byref(p))
    assert (p.reach, p.min_speed, p.append) == (0.0, 0.001, 1)
    assert lib.mpc_obstacles_from_pool_device(None, 1, None, None, None, None, None, None, None, None, None, None, None) == MPC_EINVAL
    assert lib.mpc_fleet_pool(None, 1, None, None, None, None, 0.2, None, 0, None, None, None, None) == MPC_EINVAL
    assert b"mpc_fleet_pool: null argument" in lib.mpc_last_error()
    assert lib.mpc_version() == 900
