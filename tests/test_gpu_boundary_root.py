"""GPU tests (-m gpu) of the wave-uniform work around the partitioned sweeps' root system in the fixed-layout fp64 kernels (profiles/r25_wave_uniform_sweeps.md): the
boundary products of forward_pit compute one output component per lane (mpc_wave_pit.inc, MPC_DPP_BLOCK_BXT) instead of all five in every lane -- lane i's chain is what the
replicated form computed for component i, operand for operand and in the same order --, and the shape-known kernel takes the root system's entries by row broadcasts
(MPC_DPP_BLOCK_ROOT) and solves it with its exchanges as wave-uniform branches (mpc_core.hpp::riccati_root_uniform, also behind the serial sweeps).  Nothing may change: the
shape-known kernel and the run-time-flags fixed-layout kernel (the same handle behind mpc_debug_use_shape_kernel; it has the new products and riccati_root as before) must
agree BIT FOR BIT in x, u, dt, status and iteration count with the generic-layout kernel (a handle created for n = 51 run at the same grid sizes), which keeps the replicated
products, the v_readlane tableau and riccati_root.

The row broadcasts are right when the four DPP rows hold the same bits in Vp[5], omp and Wp[0..2] behind the last combine.  That follows from the combines' text (every row
reads the same tiles, the per-lane constants depend on the lane's place in its row alone), and it is ASSERTED here: the profile build of the library (scripts/dev/variants.py
prof, the library tests/test_gpu_dev_variants.py builds) compares, at every root of backward_pit, every lane's words of the five registers with those of its column in row 0
and counts the roots at which any lane differs (mpc_wave_debug.hpp::MPC_PROF_ROOT_ROWS, the row's last column).  One child process runs all the cases below through that
library's shape-known kernel; every case asserts its count is 0 over all workgroups and that the partitioned sweeps did run there.  (A row that disagreed would not stay
hidden in row 0's shadow either: dd / nu are per-lane values behind the broadcasts, all four rows store the boundary table to the same words, and the exchanges branch when
ANY lane's compare says so.)

The pattern is tests/test_gpu_literal_diet.py's with the bench's own draw of instances: after 1, 2 and 4 iterations and after the full solve, with one candidate and the
headline's four; dt_prev = 0; a warm start; a ragged launch of grid sizes 41, 42, 43, 44, 50 (0, 1, 2, 3 and 1 leftover stages behind the four segments, segments of 10 and of 12
stages); grid sizes 38 / 39 (serial sweeps, which solve the same root system).  Every case asserts the plan's kernel and its occupancy.  64 instances."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, N = 64, 50
SEED = 20260924
SHAPE = 0x103cf      # mpc_core.hpp::kHeadlineShape
FOUR = dict(candidates=(0, 5, 5, 7), candidate_param=(0.0, 2.0, 3.0, 1.5))
CAPS = (100, 45, 40, 35)
FIELDS = ("dt", "status", "iters")


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")          # torch's HIP runtime before the library's
    import mpc_local_planner_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def inputs(m):
    return m.workloads.carlike_min_time_inputs(B, seed=SEED)


def _kw(four, max_iter):
    kw = {}
    if four: kw.update(FOUR, candidate_max_iter=CAPS if max_iter is None else (max_iter,) * 4)
    if max_iter is not None: kw["max_iter"] = max_iter
    return kw


def _plan(s):
    fn = s._lib.mpc_debug_kernel_shape
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    f, k = C.c_int32(-1), C.c_int32(-1)
    assert fn(s._h, B, C.byref(f), C.byref(k)) == 0
    return f.value, k.value


def _use_shape_kernel(s, on):
    fn = s._lib.mpc_debug_use_shape_kernel
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int32]
    assert fn(s._h, int(on)) == 0


def _pad(a):
    return np.concatenate([a, a[:, -1:]], axis=1)      # a guess of 50 grid points for the handle created with 51 (the last point is never read)


def _check(m, kw, inp, init=None, grid=None):
    """the batch through the shape-known kernel, the run-time-flags fixed-layout kernel (both with one component per lane) and the generic-layout kernel (replicated): all equal"""
    ng = np.full(B, N, dtype=np.int32) if grid is None else grid
    s = m.BatchSolver(m.config_carlike_min_time(N, **kw), max_batch=B)
    if grid is not None: s.set_grid_sizes(ng)
    assert _plan(s) == (SHAPE, SHAPE) and s.occupancy(B) == (4, 40128)
    rk = s.solve(*inp, init=init)
    _use_shape_kernel(s, False)
    assert _plan(s) == (SHAPE, 0) and s.occupancy(B) == (4, 40128)
    rf = s.solve(*inp, init=init)
    s.close()
    g = m.BatchSolver(m.config_carlike_min_time(N + 1, **kw), max_batch=B)
    g.set_grid_sizes(ng)
    assert _plan(g) == (SHAPE, 0)
    rg = g.solve(*inp, init=None if init is None else (_pad(init[0]), _pad(init[1]), init[2]))
    g.close()
    print(f"{kw.get('max_iter')} {'four' if 'candidates' in kw else 'one'}: converged {np.mean(rk.status == 0):.3f}, iterations {rk.iters.min()} .. {rk.iters.max()}")
    for r, name in ((rf, "run-time-flags fixed-layout kernel"), (rg, "generic-layout kernel")):
        assert np.array_equal(rk.x[:, :N], r.x[:, :N], equal_nan=True) and np.array_equal(rk.u[:, :N - 1], r.u[:, :N - 1], equal_nan=True), "x / u against the " + name
        for f in FIELDS:
            assert np.array_equal(getattr(rk, f), getattr(r, f), equal_nan=True), f + " against the " + name
    return rk


KINDS = ("iter1", "iter2", "iter4", "full", "dt0", "warm", "ragged")
CASES = [k + "_" + c for k in KINDS for c in ("one", "four")] + ["serial_one"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(m, inputs, name, cache):
    """(config keywords, inputs, initial guess, grid sizes) of a case"""
    kind, cand = name.split("_")
    four = cand == "four"
    x0, xf, up, dtp = inputs
    kw, inp, init, grid = _kw(four, int(kind[4:]) if kind.startswith("iter") else None), inputs, None, None
    if kind == "dt0": inp = (x0, xf, up, np.zeros_like(dtp))      # dt_prev = 0: the first control's rate rows are off at run time
    if kind == "warm":
        if "warm" not in cache:
            cold = m.BatchSolver(m.config_carlike_min_time(N), max_batch=B)
            prev = cold.solve(x0, xf, up, dtp)
            cold.close()
            ok = prev.status == 0
            assert ok.mean() > 0.9
            cache["warm"] = (np.where(ok[:, None, None], prev.x, np.linspace(x0, xf, N, axis=1)), np.where(ok[:, None, None], prev.u, 0.0), np.where(ok, prev.dt, 0.3))
        init = cache["warm"]
    if kind == "ragged": grid = np.array([41, 42, 43, 44, 50], dtype=np.int32)[np.arange(B) % 5]      # 0, 1, 2, 3, 1 leftover stages behind the four segments
    if kind == "serial": grid = np.array([38, 39], dtype=np.int32)[np.arange(B) % 2]      # below 40 grid points the serial sweeps run (both parities of the stage count)
    return kw, inp, init, grid


def profile_rows(npz):
    """(runs in the child process, with the profile build as the library) every case through the shape-known kernel: per case the sums over all workgroups of the row-check
    count (the row's last column), of the factorisations and of the partitioned backward sweep's own ticks"""
    import torch
    torch.zeros(1, device="cuda")
    import mpc_local_planner_amd as m
    from mpc_local_planner_amd import _lib
    import variants
    inputs, cache, out = m.workloads.carlike_min_time_inputs(B, seed=SEED), {}, {}
    for name in CASES:
        kw, inp, init, grid = _case(m, inputs, name, cache)
        s = m.BatchSolver(m.config_carlike_min_time(N, **kw), max_batch=B)
        if grid is not None: s.set_grid_sizes(grid)
        assert _plan(s) == (SHAPE, SHAPE)
        s.solve(*inp, init=init)
        prof = variants.read_profile(_lib.load(), B * (4 if "candidates" in kw else 1))
        s.close()
        out[name] = np.array([prof[:, variants.COL[k]].sum() for k in ("spare", "nfac", "pit_pre")])
    np.savez(npz, **out)
    print("ROWS_OK")


@pytest.fixture(scope="module")
def root_rows(m, tmp_path_factory):
    """{case: (roots at which the four DPP rows differed, factorisations, ticks of the partitioned backward sweep's set-up)} from ONE child process under the profile build"""
    dev = os.path.join(ROOT, "scripts", "dev")
    sys.path.insert(0, dev)
    import variants
    so = variants.build("prof")      # csrc/libmpc_hip_prof.so: compiled once per change (tests/test_gpu_dev_variants.py uses the same file)
    npz = str(tmp_path_factory.mktemp("rows") / "rows.npz")
    code = "import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_boundary_root as t; t.profile_rows(%r)" % (ROOT, dev, os.path.join(ROOT, "tests"), npz)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, MPC_HIP_LIB=so), timeout=300)
    assert "ROWS_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    g = np.load(npz)
    return {k: tuple(int(v) for v in g[k]) for k in CASES}


@pytest.fixture(scope="module")
def cache():
    return {}


@pytest.mark.parametrize("name", CASES)
def test_boundary_products_and_root_equal_the_generic_layout(m, inputs, cache, root_rows, name):
    kind = name.split("_")[0]
    differ, nfac, pit_ticks = root_rows[name]
    print(f"{name}: roots with rows that differ {differ}, factorisations {nfac}, ticks in backward_pit's set-up {pit_ticks}")
    assert differ == 0, "the four DPP rows do not hold the same tableau registers behind the combines"
    assert nfac >= B and (pit_ticks == 0 if kind == "serial" else pit_ticks > 0)      # (the check sits on backward_pit's path: it ran wherever the partitioned sweeps did)
    kw, inp, init, grid = _case(m, inputs, name, cache)
    rk = _check(m, kw, inp, init=init, grid=grid)
    if kind.startswith("iter"):
        assert np.isfinite(rk.x).all() and not np.array_equal(rk.x[:, 1:-1], np.zeros_like(rk.x[:, 1:-1]))      # an iterate was written
    elif kind == "serial":
        assert np.isfinite(rk.x).all() and rk.iters.min() > 4 and (rk.status == 0).any()      # it ran past the truncated cases' depth, and solves converged
    else:
        assert np.mean(rk.status == 0) > 0.9      # (equal failures must not pass)
