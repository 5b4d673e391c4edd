"""Loader / builder for the C-ABI library (include/mpc_hip.h -> csrc/libmpc_hip.so).

The library is built IN-TREE with hipcc for gfx950; there is no CPU fallback: if the
shared object is missing or no HIP device is usable, callers get an exception.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

from . import _build
from ._abi import HEADERS, LATER_HEADERS, OPEN_HEADERS, PROTOTYPES

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(CSRC, "libmpc_hip.so")
UBENCH_PATH = os.path.join(CSRC, "libmpc_ubench.so")     # measurement aid of bench.py (full-occupancy FMA rate), not part of the C ABI
EXPORTS = list(PROTOTYPES)


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return "hipcc"      # none here: an up-to-date library still loads (the stamp does not hold the compiler's path); a build that is needed fails in _make


# the compile flags of every object of the split build.  -disable-lsr: LLVM's loop strength reduction gives every LDS pointer of the (manually software-pipelined) stage
# loops two or three induction variables plus a re-materialised base; without it the loops keep the one pointer per stream the source has (headline kernel -3.8 %,
# profiles/r03_lsr_ab.log)
SPLIT_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DMPC_SPLIT_BUILD", "-mllvm", "-disable-lsr"]


def inst_flags(t: str, model: int) -> list:
    """what makes mpc_solve_inst.hip the object of one (arithmetic type, model) pair"""
    return ["-DMPC_SOLVE_INST", f"-DMPC_INST_T={t}", f"-DMPC_INST_MODEL={model}"]


def _make(out, commands, force, verbose) -> str:
    try:
        _build.build(out, commands, CSRC, force=force, verbose=verbose)
    except FileNotFoundError as e:
        raise RuntimeError("hipcc not found (needed to build the gfx950 library)") from e
    return out


def build(force: bool = False, verbose: bool = False, extra_flags=(), out: str | None = None) -> str:
    """hipcc --offload-arch=gfx950 -> csrc/libmpc_hip.so (cross-compiles without a GPU).

    Split build: the ABI + the small kernels (mpc_capi.hip) and one object per (arithmetic type, model) pair of the solve kernel
    (mpc_solve_inst.hip, three kernel instantiations each) are compiled in parallel, then linked.  Nothing else writes libmpc_hip.so.
    mpc_capi.hip without -DMPC_SPLIT_BUILD still compiles as ONE translation unit: a developer build (-DMPC_DEV_ONE_MODEL=<model> for a quick compile,
    assembly inspection) under another output name, not the same library (no -disable-lsr unless given, everything inlined in one module)."""
    if out is None:      # the measurement-only micro-benchmark rides along with the product library, but never stands in its way
        try:
            build_ubench(force=force, verbose=verbose)
        except (OSError, RuntimeError, subprocess.CalledProcessError) as e:
            print(f"mpc_local_planner_amd: libmpc_ubench.so not built ({e}); bench.py will report the data-sheet peaks only")
    out = out or LIB_PATH                      # another `out` (+ extra_flags): an instrumented copy next to the product library (tests), rebuilt by the same rule
    objdir = os.path.join(CSRC, "_obj") if out == LIB_PATH else out + ".obj"
    base = [_hipcc()] + SPLIT_FLAGS + list(extra_flags)
    jobs = [(base + ["-c", os.path.join(CSRC, "mpc_capi.hip"), "-o", os.path.join(objdir, "mpc_capi.o")])]
    for t in ("double", "float"):
        for model in range(4):
            jobs.append(base + inst_flags(t, model) + ["-c", os.path.join(CSRC, "mpc_solve_inst.hip"), "-o", os.path.join(objdir, f"mpc_solve_{t}_{model}.o")])
    link = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared"] + [j[-1] for j in jobs] + ["-o", out]
    return _make(out, jobs + [link], force, verbose)      # all or nothing: the nine objects and the link, when any dependency of any of them moved


def build_ubench(force: bool = False, verbose: bool = False) -> str:
    """csrc/mpc_ubench.hip -> csrc/libmpc_ubench.so: the FMA-rate micro-benchmark bench.py reports next to the data-sheet peaks."""
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", os.path.join(CSRC, "mpc_ubench.hip"), "-o", UBENCH_PATH]
    return _make(UBENCH_PATH, [cmd], force, verbose)


def measured_fma_peak(device: int = 0, fp64: bool = True, iters: int = 20000):
    """(TFLOP/s, ms) of the full-occupancy v_fma_f64 / v_pk_fma_f32 loop of csrc/mpc_ubench.hip on `device`; None without the library."""
    if not os.path.exists(UBENCH_PATH):
        return None
    lib = C.CDLL(UBENCH_PATH)
    fn = lib.mpc_ubench_fma_f64 if fp64 else lib.mpc_ubench_fma_f32
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    tf, ms = C.c_double(0.0), C.c_double(0.0)
    if fn(device, iters, C.byref(tf), C.byref(ms)) != 0:
        return None
    return tf.value, ms.value


_lib = None


def load() -> C.CDLL:
    """dlopen the C-ABI library and declare the prototypes of every header of _abi.HEADERS, _abi.LATER_HEADERS and _abi.OPEN_HEADERS, once."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MPC_HIP_LIB", LIB_PATH)      # developer override (e.g. an instrumented build); default: the in-tree library
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = C.CDLL(path)
    for table, _ in list(HEADERS.values()) + list(LATER_HEADERS.values()) + list(OPEN_HEADERS.values()):
        for name, (restype, argtypes) in table.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib
