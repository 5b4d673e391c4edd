"""CPU test of the shape-known root system (mpc_core.hpp::riccati_root_shape: dt-free and the mask of fixed goal components as compile-time values, the form the
shape-known wave kernel calls) against riccati_root, which reads the shape from the problem record: compiled for the host with g++ (tests/host_harness/
shape_root_host.cpp, -ffp-contract=off) and held BIT FOR BIT in dd, nu[3] and the return code, for all sixteen shapes, on random symmetric systems -- systems with the
inertia the sweep asks for (return 1), arbitrary ones (mostly -1), a pivot that vanishes and non-finite entries (0), a control pivot of the wrong sign counted by the
sweep (V.neg).  Outputs a function does not write (the early returns) are compared as the caller's fill.  The kernel's shape (dt free, all three components fixed)
is held in every case; a shape with identity rows in every case but the values left behind an answer of 0 (a breakdown: no caller reads them).  Also here: the launch plan's shape decision on the host."""
import ctypes as C
import os

import numpy as np
import pytest

from mpc_local_planner_amd import _abi as A
import _harness

SHAPE = 0x103cf      # mpc_core.hpp::kHeadlineShape


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(_harness.BUILD, "libmpc_shape_root.so")
    l = C.CDLL(_harness._built(out, ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", _harness.source("shape_root_host"), "-o", out]))
    l.shape_root.restype = C.c_int
    l.shape_root.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    l.shape_plan.restype = C.c_int
    return l


def _systems(rng, count):
    """(17 words, V.neg, what it is for) per system: P55, p5, S5[3], W[3][3] (symmetric), om[3]"""
    out = []
    for i in range(count):
        kind = ("right_inertia", "right_inertia", "right_inertia", "arbitrary", "neg_counted", "vanishing_pivot", "vanishing_dt_pivot", "nan", "inf", "badly_scaled")[i % 10]
        m = rng.standard_normal((3, 3))
        w = rng.standard_normal((3, 3)); w = w + w.T
        s5 = rng.standard_normal(3)
        p55 = rng.standard_normal()
        if kind != "arbitrary":      # nu block negative definite, dt-dt entry large and positive: one negative eigenvalue per fixed component, whatever the mask
            w = -(m @ m.T) - 1e-3 * np.eye(3)
            p55 = 5.0 + abs(p55)
        if kind == "badly_scaled": w *= 1e-6; p55 *= 1e11      # (the row-relative pivot test: active clearance rows look like this)
        v = np.concatenate([[p55, rng.standard_normal()], s5, w.ravel(), rng.standard_normal(3)])
        if kind == "vanishing_pivot":
            a = int(rng.integers(3))
            v[5 + 3 * a + a] = 0.0 if i % 20 < 10 else 1e-300      # (the denormal-range pivot: its reciprocal overflows)
        if kind == "vanishing_dt_pivot":      # dt-dt entry = what the elimination of nu_0 leaves of it, when only component 0 is fixed; plainly zero columns otherwise
            v[0] = 0.0; v[2:5] = 0.0
        if kind == "nan": v[int(rng.integers(17))] = np.nan
        if kind == "inf": v[int(rng.integers(17))] = np.inf if i % 20 < 10 else -np.inf
        out.append((np.ascontiguousarray(v), 1 if kind == "neg_counted" else 0, kind))
    return out


@pytest.mark.parametrize("dtf", [0, 1])
@pytest.mark.parametrize("fxm", range(8))
def test_shape_known_root_equals_riccati_root_bit_for_bit(lib, dtf, fxm):
    rng = np.random.default_rng(1000 + 8 * dtf + fxm)
    codes = {}
    for v, neg, kind in _systems(rng, 400):
        a, b = np.full(4, 7.0), np.full(4, 7.0)
        ra = lib.shape_root(dtf, fxm, v.ctypes.data, neg, 0, a.ctypes.data)
        rb = lib.shape_root(dtf, fxm, v.ctypes.data, neg, 1, b.ctypes.data)
        assert ra == rb, (kind, ra, rb, v)
        # the kernel's shape has no identity rows: equal in every case, the breakdowns' non-finite values included.  A shape with identity rows: riccati_root drags a NaN
        # of the system through them (0 x NaN) into every unknown before it answers 0, the shape-known form has no such rows -- equal whenever the answer is not 0
        if (dtf, fxm) == (1, 7) or ra != 0:
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (kind, ra, a, b, v)
        codes.setdefault(ra, set()).add(kind)
        if ra == 1:      # absent unknowns solve to +0; the others were written
            want_zero = [0] * (1 - dtf) + [1 + i for i in range(3) if not (fxm >> i) & 1]
            assert all(a.view(np.uint64)[j] == 0 for j in want_zero) and np.isfinite(a).all()
    print(f"dt free {dtf} fixed mask {fxm}: " + ", ".join(f"{c}: {len(k)} kinds" for c, k in sorted(codes.items())))
    # the three answers all occur (a system without unknowns cannot break down: it is solved or has the wrong inertia)
    assert set(codes) == ({1, -1} if (dtf, fxm) == (0, 0) else {1, -1, 0})
    assert "right_inertia" in codes[1] and "neg_counted" in codes[-1]
    if fxm == 7: assert "vanishing_pivot" in codes[0]
    if (dtf, fxm) != (0, 0): assert {"nan", "inf"} <= codes[0]


PLAN_CASES = {
    # configuration -> (the handle's word, the word compiled into the kernel of an fp64 launch)
    "headline": (lambda: A.config_carlike_min_time(50), SHAPE, SHAPE),
    "headline_four_candidates": (lambda: A.config_carlike_min_time(50, candidates=(0, 5, 5, 7), candidate_max_iter=(100, 45, 40, 35), candidate_param=(0.0, 2.0, 3.0, 1.5)), SHAPE, SHAPE),
    "bicycle_n50": (lambda: A.config_bicycle_min_time(50), SHAPE, SHAPE),
    "n49": (lambda: A.config_carlike_min_time(49), SHAPE, 0),
    "n51": (lambda: A.config_carlike_min_time(51), SHAPE, 0),
    "n20_two_waves": (lambda: A.config_carlike_min_time(20), SHAPE, 0),
    "global_form": (lambda: A.config_carlike_min_time(50, stage_data=A.STAGE_GLOBAL), SHAPE, 0),
    "crank_nicolson": (lambda: A.config_carlike_min_time(50, collocation=A.COLLOC_CRANK_NICOLSON), SHAPE, 0),      # (two more trig words: not the fixed record)
    "obstacles": (lambda: A.config_carlike_min_time(50, max_obstacles=4, max_vertices=4), SHAPE, 0),
    "goal_heading_free": (lambda: A.config_carlike_min_time(50, xf_fixed=(True, True, False)), SHAPE & ~4, 0),
    "quadratic_objective": (lambda: A.config_carlike_min_time(50, objective=A.OBJ_QUADRATIC, Q=(2.0, 2.0, 0.25), R=(0.1, 0.05)), (SHAPE | 16) & ~0x10000, 0),
    "has_Qf": (lambda: A.config_carlike_min_time(50, Qf=(10.0, 10.0, 0.5)), SHAPE | 32, 0),
    "rate_row_off": (lambda: A.config_carlike_min_time(50, du_lb=(-1e30, -0.5)), SHAPE & ~64, 0),
    "unicycle_quadratic_n50": (lambda: A.config_unicycle_quadratic(50), 0x3f0, 0),
}


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_plan_hands_the_shape_kernel_to_the_headline_shape_on_the_fixed_layout_alone(lib, name):
    make, word, kernel = PLAN_CASES[name]
    assert lib.shape_headline() == SHAPE
    cfg = make()
    f, k = C.c_int32(-1), C.c_int32(-1)
    assert lib.shape_plan(C.byref(cfg), 0, 1024, C.byref(f), C.byref(k)) == 0
    assert (f.value, k.value) == (word, kernel)
    assert lib.shape_plan(C.byref(cfg), 1, 1024, C.byref(f), C.byref(k)) == 0 and k.value == 0      # no fp32 kernel has a shape compiled in
