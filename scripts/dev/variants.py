"""developer tool: the instrumented variants of the library (csrc/mpc_wave_debug.hpp has the switches), each built NEXT TO the product library by the product's own rule, and
the profile row's column names.
    python scripts/dev/variants.py                      the table
    python scripts/dev/variants.py prof                 builds csrc/libmpc_hip_prof.so, prints its path
    python scripts/dev/variants.py nancheck:3 CMD ...   ... and runs CMD in a fresh child process with MPC_HIP_LIB pointing at it (nancheck:<block>, default 0)
A process loads ONE library (_lib.load), so a variant is always handed to a child process through MPC_HIP_LIB; libmpc_hip.so is never written by anything but _lib.build()."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from mpc_local_planner_amd import _lib

# name -> extra flags of the split build; a name may carry a parameter ("nancheck:3"), which replaces {} (default 0)
VARIANTS = {
    "poison": ("-DMPC_POISON_LDS",),
    "prof": ("-DMPC_PROFILE=1",),
    "prof_mult": ("-DMPC_PROFILE=1", "-DMPC_PROFILE_MULT"),
    "asm_mark": ("-DMPC_ASM_MARK=1",),
    "pit_check": ("-DMPC_PIT_CHECK=64",),
    "pit_verbose": ("-DMPC_PIT_CHECK=64", "-DMPC_PIT_VERBOSE"),      # (workgroups 0 .. 63 are compared, workgroup 64 prints its tiles and roots)
    # {}: the workgroup that prints.  A trace build, not a timing build: with the traces' printf calls and loop strength reduction off, hipcc 7.2's register allocator
    # crashes on the level-2 kernels, so this variant switches it back on (the later -mllvm flag wins)
    "nancheck": ("-DMPC_NANCHECK={}", "-mllvm", "-disable-lsr=false"),
    "dev_switches": ("-DMPC_DEV_SWITCHES",),
}

# one row of mpc_debug_profile per workgroup: enum ProfCol of csrc/mpc_wave_debug.hpp, same order (tests/test_dev_variants.py holds the count to mpc::kProfCols)
PROF_COLUMNS = ("ticks", "wall100MHz", "iters", "nfac", "ntrial",
                "kkt", "barrier_terms", "backward", "forward", "post", "logs0", "trial", "accept", "trial_setup",
                "glue_kkt_to_barrier", "glue_barrier_to_fac", "glue_ls_setup", "glue_trial_to_accept", "glue_back_edge",
                "bwd_loop", "bwd_setup", "fwd_loop", "pit_pre", "fwd_pre", "fwd_post", "spare")
COL = {k: i for i, k in enumerate(PROF_COLUMNS)}
PHASES = PROF_COLUMNS[COL["kkt"]:COL["glue_kkt_to_barrier"]]
GLUE = PROF_COLUMNS[COL["glue_kkt_to_barrier"]:COL["bwd_loop"]]


def flags(name):
    base, _, par = name.partition(":")
    return tuple(f.format(par or "0") for f in VARIANTS[base])


def lib_path(name):
    return os.path.join(_lib.CSRC, "libmpc_hip_%s.so" % name.replace(":", ""))


def build(name, **kw):
    """csrc/libmpc_hip_<name>.so, compiled when a source, a header or a flag changed; for MPC_HIP_LIB of a fresh child process"""
    return _lib.build(extra_flags=flags(name), out=lib_path(name), **kw)


def read_profile(lib, rows):
    """the (rows, len(PROF_COLUMNS)) array of the last launch's counters; lib: the loaded -DMPC_PROFILE library (_lib.load() under MPC_HIP_LIB)"""
    import numpy as np
    buf = np.zeros((rows, len(PROF_COLUMNS)), dtype=np.int64)
    fn = lib.mpc_debug_profile
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    err = fn(buf.ctypes.data_as(C.c_void_p), C.c_int(rows))
    if err:
        raise RuntimeError("mpc_debug_profile: hipError %d" % err)
    return buf


if __name__ == "__main__":
    if len(sys.argv) < 2:
        for k in VARIANTS:
            print("%-13s %s" % (k, " ".join(flags(k))))
        sys.exit(0)
    so = build(sys.argv[1], verbose=True)
    print(so)
    if len(sys.argv) > 2:
        sys.exit(subprocess.run(sys.argv[2:], env=dict(os.environ, MPC_HIP_LIB=so)).returncode)
