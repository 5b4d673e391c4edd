"""CPU tests of the build-if-stale helper (mpc_local_planner_amd/_build.py) on a two-file C++ toy compiled with g++ in a temporary directory: what makes an output
stale and what does not; and, on the real tree, that a harness's dependencies are the compiler's, not a list's."""
import json
import os
import shutil

import pytest

import _harness
from mpc_local_planner_amd import _build


@pytest.fixture
def toy(tmp_path):
    """root/src/main.cpp includes root/inc/toy.hpp; returns (root, output, command, the header)"""
    root = tmp_path / "tree"
    (root / "src").mkdir(parents=True)
    (root / "inc").mkdir()
    (root / "inc" / "toy.hpp").write_text("inline int toy() { return TOY; }\n")
    (root / "src" / "main.cpp").write_text('#include "../inc/toy.hpp"\nint main() { return toy(); }\n')
    return root, *_command(root), root / "inc" / "toy.hpp"


def _command(root, *more):
    out = str(root / "out" / "toy")
    return out, ["g++", "-O0", "-DTOY=0", *more, str(root / "src" / "main.cpp"), "-o", out]


def _build_toy(root, out, cmd):
    return _build.build(out, [cmd], str(root / "src"), root=str(root))


def _identity(path):
    st = os.stat(path)
    return st.st_mtime_ns, st.st_ino


def _age(path, seconds):
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + int(seconds * 1e9)))


def test_a_missing_output_builds_and_a_second_call_does_not_compile(toy):
    root, out, cmd, header = toy
    assert _build_toy(root, out, cmd) and os.path.exists(out)
    stamp = json.load(open(out + ".stamp"))
    assert stamp["deps"] == ["inc/toy.hpp", "src/main.cpp"] and stamp["commands"] == [["-O0", "-DTOY=0", "src/main.cpp", "-o", "out/toy"]]      # relative to the tree
    assert not os.path.exists(out + ".d")
    before = _identity(out)
    assert not _build_toy(root, out, cmd) and _identity(out) == before


def test_an_included_header_newer_than_the_output_rebuilds(toy):
    root, out, cmd, header = toy
    _build_toy(root, out, cmd)
    for f in (root / "src" / "main.cpp", header, out):      # everything 20 s into the past, so that a rebuilt output is newer than anything moved below
        _age(f, -20)
    os.utime(header, ns=(os.stat(out).st_atime_ns, os.stat(out).st_mtime_ns))      # as old as the output: not newer
    assert not _build_toy(root, out, cmd)
    _age(header, +10)
    assert _build_toy(root, out, cmd) and not _build_toy(root, out, cmd)


def test_one_more_flag_rebuilds(toy):
    root, out, cmd, header = toy
    _build_toy(root, out, cmd)
    assert _build_toy(root, *_command(root, "-DMORE")) and not _build_toy(root, *_command(root, "-DMORE"))
    assert _build_toy(root, out, cmd)


def test_a_deleted_stamp_rebuilds(toy):
    root, out, cmd, header = toy
    _build_toy(root, out, cmd)
    os.remove(out + ".stamp")
    assert _build_toy(root, out, cmd) and os.path.exists(out + ".stamp")


def test_a_deleted_header_that_is_no_longer_included_rebuilds_without_raising(toy):
    root, out, cmd, header = toy
    _build_toy(root, out, cmd)
    (root / "src" / "main.cpp").write_text("int main() { return 0; }\n")
    os.remove(header)
    assert _build_toy(root, out, cmd)
    assert json.load(open(out + ".stamp"))["deps"] == ["src/main.cpp"] and not _build_toy(root, out, cmd)


def test_the_tree_copied_elsewhere_with_its_outputs_is_not_stale_there(toy, tmp_path):
    root, out, cmd, header = toy
    _build_toy(root, out, cmd)
    there = tmp_path / "elsewhere"
    shutil.copytree(root, there)      # keeps the mtimes
    out2, cmd2 = _command(there)
    before = _identity(out2)
    assert not _build.stale(out2, [cmd2], root=str(there))
    assert not _build_toy(there, out2, cmd2) and _identity(out2) == before


def test_a_harness_s_dependencies_are_the_compiler_s():
    """controller_cycle_host.cpp reaches include/mpc_hip.h through include/mpc_controller.hpp (mpc_cycle_params, MPC_REINIT_*): no hand-kept list had it"""
    deps = json.load(open(_harness.shared("controller_cycle_host") + ".stamp"))["deps"]
    assert {"include/mpc_hip.h", "include/mpc_controller.hpp", "mpc_local_planner_amd/csrc/mpc_controller_cycle.hpp", "tests/host_harness/controller_cycle_host.cpp"} <= set(deps)


def test_a_needed_build_without_the_compiler_says_so(tmp_path):
    from mpc_local_planner_amd import _lib
    out = str(tmp_path / "lib.so")
    with pytest.raises(RuntimeError, match=r"hipcc not found \(needed to build the gfx950 library\)"):
        _lib._make(out, [["no-such-hipcc", "--offload-arch=gfx950", str(tmp_path / "x.hip"), "-o", out]], False, False)
