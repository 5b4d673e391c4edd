"""GPU test of the `prof` variant of the library (scripts/dev/variants.py; -DMPC_PROFILE, csrc/mpc_wave_debug.hpp): the instrumented kernel solves what the product
kernel solves, and its counters hang together -- for the serial sweeps (n = 12), the partitioned sweeps with leftover stages (n = 43) and the fixed layout (n = 50).

The counters also show what the ABI cannot: which sweeps a factorisation took.  The warm-started end-game cases of tests/_truncated.py rest on the static rule "partitioned
while mu > pit_floor()"; four of them (n = 43 and n = 50, barrier start below and above the floor, four iterations) run here on the instrumented library, and the partitioned
sweeps' counters are zero in every row below the floor and positive in every row above it."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
GRIDS, B = (12, 43, 50), 4
WARM = ("endgame_serial_carlike_n43_below", "endgame_pit_carlike_n43_above", "endgame_fixed_carlike_n50_below", "endgame_fixed_carlike_n50_above")
WARM_CAP = 4

CHILD = """
import sys, numpy as np
sys.path[:0] = [%r, %r, %r]
import torch
torch.zeros(1, device="cuda")
import mpc_local_planner_amd as m
from mpc_local_planner_amd import _lib
import variants
out = {}
for n in %r:
    s = m.BatchSolver(m.config_carlike_min_time(n), max_batch=%d)
    r = s.solve(*m.workloads.carlike_min_time_inputs(%d))
    out["status%%d" %% n], out["iters%%d" %% n], out["prof%%d" %% n] = r.status, r.iters, variants.read_profile(_lib.load(), %d)
    s.close()
import _truncated as T
for name in %r:
    x0, xf, up, dtp, obstacles, ng = T.inputs(name)
    s = m.BatchSolver(T.abi_config(name, %d), max_batch=T.B)
    r = s.solve(x0, xf, up, dtp, init=T.guess(name))
    out["status_" + name], out["iters_" + name], out["prof_" + name] = r.status, r.iters, variants.read_profile(_lib.load(), T.B)
    s.close()
np.savez(%r, **out)
print("PROF_OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{n or warm case: (product result, the prof library's status, iterations and counter rows)}: the product library in this process, the variant in ONE child process"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as m
    import variants
    import _truncated as T
    so = variants.build("prof")      # csrc/libmpc_hip_prof.so: compiled once per change, like the poison library of test_gpu_parity.py
    res = {}
    for n in GRIDS:
        s = m.BatchSolver(m.config_carlike_min_time(n), max_batch=B)
        res[n] = s.solve(*m.workloads.carlike_min_time_inputs(B))
        s.close()
    for name in WARM:
        x0, xf, up, dtp, obstacles, ng = T.inputs(name)
        s = m.BatchSolver(T.abi_config(name, WARM_CAP), max_batch=T.B)
        res[name] = s.solve(x0, xf, up, dtp, init=T.guess(name))
        s.close()
    npz = str(tmp_path_factory.mktemp("prof") / "prof.npz")
    code = CHILD % (ROOT, os.path.join(ROOT, "scripts", "dev"), os.path.join(ROOT, "tests"), GRIDS, B, B, B, WARM, WARM_CAP, npz)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MPC_HIP_LIB=so), timeout=300)
    assert "PROF_OK" in r.stdout, r.stdout + r.stderr
    g = np.load(npz)
    out = {n: (res[n], g["status%d" % n], g["iters%d" % n], g["prof%d" % n]) for n in GRIDS}
    out.update({name: (res[name], g["status_" + name], g["iters_" + name], g["prof_" + name]) for name in WARM})
    return out


@pytest.mark.parametrize("n", GRIDS)
def test_prof_variant_solves_the_same_and_its_counters_add_up(runs, n):
    import variants
    product, status, iters, prof = runs[n]
    assert prof.shape == (B, len(variants.PROF_COLUMNS))
    for i in range(B):
        row = dict(zip(variants.PROF_COLUMNS, prof[i].tolist()))
        print(n, i, "status", int(status[i]), "iters", int(iters[i]), row)
        assert status[i] == product.status[i] and iters[i] == product.iters[i]
        assert row["iters"] == iters[i]
        assert row["nfac"] >= row["iters"]
        assert all(v >= 0 for v in row.values())
        assert 0 < sum(row[k] for k in variants.PHASES + variants.GLUE) <= row["ticks"]
        pit = [row[k] for k in ("pit_pre", "fwd_pre", "fwd_post")]
        assert all(v == 0 for v in pit) if n == 12 else all(v > 0 for v in pit), pit


@pytest.mark.parametrize("name", WARM)
def test_warm_end_game_cases_take_the_sweeps_their_barrier_start_says(runs, name):
    """the warm cases of tests/_truncated.py, four iterations: no factorisation below pit_floor() enters the partitioned sweeps, every row above it does"""
    import variants
    import _truncated as T
    product, status, iters, prof = runs[name]
    assert prof.shape == (T.B, len(variants.PROF_COLUMNS))
    assert (product.status == 1).all() and (product.iters == WARM_CAP).all()
    for i in range(T.B):
        row = dict(zip(variants.PROF_COLUMNS, prof[i].tolist()))
        pit = [row[k] for k in ("pit_pre", "fwd_pre", "fwd_post")]
        print(name, i, "status", int(status[i]), "iters", int(iters[i]), "nfac", row["nfac"], "pit_pre, fwd_pre, fwd_post", pit)
        assert status[i] == product.status[i] and iters[i] == product.iters[i]
        assert row["iters"] == iters[i] and row["nfac"] >= row["iters"]
        assert all(v == 0 for v in pit) if name.endswith("_below") else all(v > 0 for v in pit), pit
