"""GPU test of the `prof` variant of the library (scripts/dev/variants.py; -DMPC_PROFILE, csrc/mpc_wave_debug.hpp): the instrumented kernel solves what the product
kernel solves, and its counters hang together -- for the serial sweeps (n = 12), the partitioned sweeps with leftover stages (n = 43) and the fixed layout (n = 50)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
GRIDS, B = (12, 43, 50), 4

CHILD = """
import sys, numpy as np
sys.path[:0] = [%r, %r]
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
np.savez(%r, **out)
print("PROF_OK")
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{n: (product result, the prof library's status, iterations and counter rows)}: the product library in this process, the variant in ONE child process"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as m
    import variants
    so = variants.build("prof")      # csrc/libmpc_hip_prof.so: compiled once per change, like the poison library of test_gpu_parity.py
    res = {}
    for n in GRIDS:
        s = m.BatchSolver(m.config_carlike_min_time(n), max_batch=B)
        res[n] = s.solve(*m.workloads.carlike_min_time_inputs(B))
        s.close()
    npz = str(tmp_path_factory.mktemp("prof") / "prof.npz")
    code = CHILD % (ROOT, os.path.join(ROOT, "scripts", "dev"), GRIDS, B, B, B, npz)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MPC_HIP_LIB=so), timeout=300)
    assert "PROF_OK" in r.stdout, r.stdout + r.stderr
    g = np.load(npz)
    return {n: (res[n], g["status%d" % n], g["iters%d" % n], g["prof%d" % n]) for n in GRIDS}


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
