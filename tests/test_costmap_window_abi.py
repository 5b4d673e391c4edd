"""CPU tests of what is particular to include/mpc_costmap_window.h: the fleet cycle in its leading comment, the values of its defaults, and what the library can refuse
without a GPU.  Its declarations against _abi.WINDOW_PROTOTYPES, the layout of mpc_window_params and the binding are held by tests/test_abi.py, like every header's."""
import ctypes as C
import math

from _abi_check import header_text, lib      # noqa: F401 (lib: the fixture)


def test_the_chain_comment_is_led_by_the_window_step():
    header = header_text("mpc_costmap_window.h")
    chain = header[:header.index("#ifndef")]
    assert 0 < chain.index("mpc_costmap_window_device") < chain.index("mpc_costmap_to_obstacles_device") < chain.index("mpc_controller_step_batch_device")


def test_library_exports_binds_gives_the_defaults_and_refuses_without_a_gpu(lib):
    from mpc_local_planner_amd._abi import MPC_EINVAL, MpcWindowParams
    # the defaults as the header states them
    p = MpcWindowParams((C.c_double * 2)(7.0, 7.0), -1.0, (C.c_double * 2)(7.0, 7.0), -1.0, -1.0, -1.0, -1, -1, -1, -1)
    lib.mpc_window_params_defaults(C.byref(p), 0.05, 1200, 400)
    assert (tuple(p.map_origin), p.map_resolution, tuple(p.lattice_anchor), p.inscribed_radius, p.inflation_radius, p.cost_scaling_factor, p.map_size_x, p.map_size_y,
            p.outside_value, p.inflate_unknown) == ((0.0, 0.0), 0.05, (0.0, 0.0), 0.0, 0.0, 10.0, 1200, 400, 0, 0)
    lib.mpc_window_params_defaults(None, 0.05, 1, 1)
    # without a handle: a refusal instead of a crash, with its text
    for fn in (lib.mpc_costmap_window, lib.mpc_costmap_window_device):
        assert fn(None, 1, None, C.byref(p), None, 8, 8, 0.05, None, None, None) == MPC_EINVAL
        assert b"mpc_costmap_window: null argument" in lib.mpc_last_error()
        assert fn(None, 1, None, None, None, 8, 8, math.nan, None, None, None) == MPC_EINVAL
    assert lib.mpc_version() == 900
