"""The host builds of the tests: every harness of tests/host_harness/ is compiled here, with g++, into tests/host_harness/_build/, by the build-if-stale rule of
mpc_local_planner_amd/_build.py (dependencies from the compiler's depfile, plus the command).  One name, one output: two test modules that ask for the same harness
share the file.  The sanitised builds are stand-alone programs that the tests execute; nothing sanitised is loaded into Python."""
import os

from mpc_local_planner_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness")
BUILD = os.path.join(SRC, "_build")
LAZY = ["-Wl,--unresolved-symbols=ignore-all"]      # a facade harness needs the ABI's declarations only: link lazily, the tested functions make no library calls

_SO = ["-fPIC", "-shared"]
# harness (tests/host_harness/<name>.cpp) -> (library, the flags of its compile, in the order of the command line)
SHARED = {
    "host_solver": ("libmpc_hostdbg.so", ["-O2", "-std=c++17"] + _SO),
    "stage_pieces_host": ("libmpc_stage_pieces.so", ["-O1", "-std=c++17"] + _SO),
    "step_pieces_host": ("libmpc_step_pieces.so", ["-O1", "-std=c++17"] + _SO),
    "launch_plan_host": ("libmpc_launch_plan.so", ["-O1", "-std=c++17"] + _SO),
    "parameter_sets_host": ("libmpc_parameter_sets.so", ["-O1", "-std=c++17"] + _SO),
    "evaluate_host": ("libmpc_evaluate_host.so", ["-O2", "-std=c++17", "-ffp-contract=off"] + _SO),
    "controller_cycle_host": ("libmpc_controller_cycle.so", ["-O2", "-std=c++17", "-ffp-contract=off"] + _SO),
    "plan_inputs_host": ("libmpc_plan_inputs.so", ["-O2", "-std=c++17", "-ffp-contract=off"] + _SO),
    "controller_host": ("libctl_host.so", ["-O1", "-std=c++17"] + _SO + LAZY),
    "params_host": ("libctl_params.so", ["-O1", "-std=c++17"] + _SO + LAZY),
}


def source(name):
    return os.path.join(SRC, name + ".cpp")


def _built(out, command):
    _build.build(out, [command], HERE)
    return out


def shared(name):
    """path of the harness's shared library, compiled if stale"""
    lib, flags = SHARED[name]
    out = os.path.join(BUILD, lib)
    return _built(out, ["g++"] + flags + [source(name), "-o", out])


def sanitized(name, defines, recover="undefined"):
    """path of the harness built as a stand-alone program (its own main behind `defines`) with -fsanitize=address,undefined, compiled if stale"""
    out = os.path.join(BUILD, name[:-len("_host")] + "_sanitized")
    flags = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=" + recover]
    return _built(out, ["g++"] + flags + ["-D" + d for d in defines] + [source(name), "-o", out])
