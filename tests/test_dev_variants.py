"""CPU tests that keep the instrumented variants of the library alive (scripts/dev/variants.py, csrc/mpc_wave_debug.hpp): every variant still PARSES with the split build's flags
(hipcc -fsyntax-only: nothing is written), the profile row's names cover the header's columns, and no script builds over the product library."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
import variants      # noqa: E402
from mpc_local_planner_amd import _lib      # noqa: E402

SOLVE_INST = _lib.inst_flags("double", 1) + [os.path.join(_lib.CSRC, "mpc_solve_inst.hip")]
CAPI = [os.path.join(_lib.CSRC, "mpc_capi.hip")]
CHECKS = {f"{name}-{tag}": _lib.SPLIT_FLAGS + list(variants.flags(name)) + unit for name in variants.VARIANTS for tag, unit in (("solve_inst", SOLVE_INST), ("capi", CAPI))}
# the developer build that is still one translation unit
CHECKS["one_model-capi"] = [f for f in _lib.SPLIT_FLAGS if f != "-DMPC_SPLIT_BUILD"] + ["-DMPC_DEV_ONE_MODEL=1"] + CAPI


@pytest.fixture(scope="module")
def parsed():
    """every check's compiler run, at most 16 at a time"""
    def run(args):
        return subprocess.run([_lib._hipcc(), "-fsyntax-only"] + args, cwd=_lib.CSRC, capture_output=True, text=True)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 2)) as pool:
        return dict(zip(CHECKS, pool.map(run, CHECKS.values())))


@pytest.mark.parametrize("check", sorted(CHECKS))
def test_variant_parses(parsed, check):
    r = parsed[check]
    assert r.returncode == 0, " ".join(r.args) + "\n" + r.stderr[-4000:]


def test_variants_cover_the_header_s_switches_and_never_the_product_library():
    assert {"poison", "prof", "prof_mult", "asm_mark", "pit_check", "pit_verbose", "nancheck", "dev_switches"} <= set(variants.VARIANTS)
    header = open(os.path.join(_lib.CSRC, "mpc_wave_debug.hpp")).read()
    for switch in ("MPC_PROFILE", "MPC_PROFILE_MULT", "MPC_NANCHECK", "MPC_PIT_CHECK", "MPC_PIT_VERBOSE", "MPC_POISON_LDS", "MPC_ASM_MARK"):
        assert re.search(r"^#\s*if.*\b%s\b" % switch, header, re.M), switch
        assert any(re.match(r"-D%s(=|$)" % switch, f) for fl in variants.VARIANTS.values() for f in fl), switch
    assert variants.flags("nancheck:3")[0] == "-DMPC_NANCHECK=3" and variants.flags("nancheck")[0] == "-DMPC_NANCHECK=0"
    paths = [variants.lib_path(v) for v in variants.VARIANTS]
    assert _lib.LIB_PATH not in paths and len(set(paths)) == len(paths)
    assert variants.lib_path("poison") == os.path.join(_lib.CSRC, "libmpc_hip_poison.so")


def test_profile_names_cover_the_header_s_columns():
    header = open(os.path.join(_lib.CSRC, "mpc_wave_debug.hpp")).read()
    (cols,) = re.findall(r"constexpr int kProfCols = (\d+);", header)
    assert len(variants.PROF_COLUMNS) == int(cols) and len(set(variants.PROF_COLUMNS)) == int(cols)
    # the enumerators, in order, are the names in capitals
    body = re.search(r"enum ProfCol : int \{(.*?)\};", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)
    assert [e.strip()[len("PROF_"):].lower().replace("wall", "wall100mhz") for e in body.split(",")] == [c.lower() for c in variants.PROF_COLUMNS]


def test_no_script_builds_over_the_product_library():
    hits = []
    for top in ("scripts", "tests"):
        for d, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".sh", ".md", ".txt", ".cpp", ".hip")) or "." not in f:
                    text = open(os.path.join(d, f), errors="replace").read()
                    hits += [f"{os.path.relpath(os.path.join(d, f), ROOT)}: {l.strip()}" for l in text.splitlines() if re.search(r"-o\s+(\S*/)?libmpc_hip\.so(\s|\)|;|\"|'|`|$)", l)]
    assert not hits, hits
