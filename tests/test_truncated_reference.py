"""CPU side of the truncated solves (tests/_truncated.py): the reference that tests/test_gpu_truncated_solves.py holds the device to is decidable on every instance.

For every case and cap of the GPU file:
  (a) every CPU solver ends with status max_iter and iters == cap on every instance;
  (b) e_cpu[i] -- the largest distance of an fp64 CPU solver (unrefined numpy dense solve, C oracle's banded LU, host build of the kernel core's Riccati sweeps) to the
      refined reference -- is below 1e-10 at every cap.  This is a condition on the INPUTS (no instance sits on a line-search tie or on an inertia decision that rounding
      flips): a seed that breaks it is replaced, the number is not raised.  Measured over the table: 8e-14 or better after one iteration, 8e-12 or better after four.
  (c) the inputs exercise what the test is for: in every fp64 case with n >= 40 and a free dt at least a third of the instances were regularised (delta_w > 0) by cap 4,
      and for every model at least one instance backtracks (alpha below its fraction-to-boundary limit) by cap 4.  This describes cold starts: the warm cases
      (Case.warm) are exempt from it and have (f) instead;
  (d) refinement does its job (one case, every factorisation): see test_refinement_lowers_the_error_of_every_factorisation for what that can and cannot mean;
  (e) the fp32 yardstick e_cpu32 (host build of the kernel core in float against the reference) is recorded, not bounded;
  (f) warm cases: all 12 first cycles converged (status 0), the ABI configuration leaves mu_init_warm at 0 ("take mu_init") and dual_warm_start off, and every counted
      iteration ran on the stated side of the kernel's pit_floor() by a factor of at least 2: the mu recorded in the oracle's history -- ipm_dense.py::solve updates mu
      once, before it builds the iteration's KKT matrix, and records that value after the step, so it is the one every factorisation of the iteration used -- is at most
      floor / 2 (below: the kernel runs the serial sweeps) or at least 2 x floor (above: the partitioned sweeps) on every instance up to the largest cap.  A condition on
      the inputs like (b): a seed or a barrier start that breaks it is replaced.
IpmOptions.refine_steps = 0 changes nothing: regenerating a base golden set (tests/golden/unicycle_quadratic_n20.npz, the statements of tests/golden/make_golden.py::make)
reproduces it bit for bit (test_refine_steps_zero_reproduces_a_base_golden_set_bit_for_bit)."""
import os

import numpy as np
import pytest

import _truncated as T
from oracle import ipm_dense as I
from oracle import se2_nlp as R


@pytest.mark.parametrize("name,cap", T.CASE_CAPS)
def test_cpu_solvers_agree_with_the_refined_reference(name, cap):
    cs = T.CASES[name]
    ref, ng = T.reference(name, cap), T.inputs(name)[5]
    assert (ref[3] == 1).all() and (ref[4] == cap).all(), (ref[3], ref[4])
    solvers = T.cpu_solvers(name, cap)
    d = {k: T.dist_batch(v, ref, ng) for k, v in solvers.items()}
    h = T.history(name)
    reg = np.mean([any(e["delta"] > 0 for e in hh[:cap]) for hh in h])
    back = np.mean([any(e["alpha"] < e["a_p"] for e in hh[:cap]) for hh in h])
    line = f"[truncated, CPU] {name} cap {cap}: spread " + ", ".join(f"{k} {v.max():.1e}" for k, v in d.items()) + f"; regularised {reg:.2f}, backtracking {back:.2f}"
    if cs.warm:
        mu, al = np.array([[e["mu"] for e in hh[:cap]] for hh in h]), np.array([[e["alpha"] for e in hh[:cap]] for hh in h])
        line += f"; mu {mu.min():.2e} .. {mu.max():.2e}, step length median {np.median(al):.1e}, max {al.max():.1e}"
    if cs.fp32:
        e32 = T.e_cpu32(name, cap)
        line += f"; fp32 host core against the reference: min {e32.min():.1e}, median {np.median(e32):.1e}, max {e32.max():.1e}"          # (e): recorded, not bounded
    print(line)
    for k, v in solvers.items():                                                       # (a)
        assert (v[3] == 1).all() and (v[4] == cap).all(), (k, v[3], v[4])
    assert (T.e_cpu(name, cap) < T.E_CPU_MAX).all(), (name, cap, T.e_cpu(name, cap))   # (b): no instance excluded


def test_the_inputs_reach_the_regularisation_ladder_and_the_line_search():
    """(c)"""
    back = {}
    for name, cs in T.CASES.items():
        if cs.warm:
            continue
        h = T.history(name)
        top = max(cs.caps)
        if not cs.fp32 and cs.n >= 40 and T.nlp_config(name).dt_free:
            reg = sum(any(e["delta"] > 0 for e in hh[:top]) for hh in h)
            assert 3 * reg >= T.B, (name, reg)
        back[cs.model] = back.get(cs.model, 0) + sum(any(e["alpha"] < e["a_p"] for e in hh[:top]) for hh in h)
    assert set(back) == set(T.MODELS) and all(v >= 1 for v in back.values()), back


WARM = [name for name, cs in T.CASES.items() if cs.warm]


@pytest.mark.parametrize("name", WARM)
def test_every_counted_iteration_of_a_warm_case_ran_on_its_side_of_the_floor(name):
    """(f)"""
    cs = T.CASES[name]
    floor, top = T.pit_floor(name), max(cs.caps)
    assert floor == (1e-4 if T.inputs(name)[4] is not None else 1e-6)
    assert (T.cycle1(name)[4] == 0).all(), T.cycle1(name)[4]          # every first cycle converged
    cfg = T.abi_config(name, top)
    assert cfg.mu_init == cs.mu_init and cfg.mu_init_warm == 0.0 and cfg.dual_warm_start == 0
    x0, _, up, dtp, _, ng = T.inputs(name)
    gx = T.guess(name)[0]
    assert (np.abs(gx[:, 0, :2] - x0[:, :2]).max(1) > 1e-4).all() and (dtp == T.PERIOD).all()          # the plant moved: the guess's first vertex is not the start state
    assert all(np.array_equal(up[i], T.guess(name)[1][i, 0]) for i in range(T.B))
    h = T.history(name)
    assert all(len(hh) >= top for hh in h)
    mu = np.array([[e["mu"] for e in hh[:top]] for hh in h])
    print(f"[truncated, CPU] {name}: floor {floor:g}, mu_init {cs.mu_init:g}, mu over {top} iterations {mu.min():.3e} .. {mu.max():.3e}")
    assert name.endswith(("_below", "_above"))
    if name.endswith("_below"):
        assert cs.mu_init < floor and (mu <= floor / 2).all(), mu.max()
    else:
        assert cs.mu_init > floor and (mu >= 2 * floor).all(), mu.min()


def test_refinement_lowers_the_error_of_every_factorisation(monkeypatch):
    """(d) on pit_carlike_n43, every factorisation of every iteration (the refused ones of the regularisation ladder included).

    Asserted: the refined step is nearer than the plain solve to the solution of the fp64 KKT system -- obtained by six further rounds in np.longdouble, unrounded -- on
    every factorisation (measured: largest error 5.0e-9 before, 2.3e-13 after, never above 0.11 x the plain solve's), and every refined step is within one fp64 spacing of
    the solution's largest component of it (it is that solution rounded once; the bound is the rounding's, not a measurement).
    Not asserted, printed: the residual max |K sol - rhs| EVALUATED IN fp64, the first yardstick one would reach for.  It cannot tell the two apart: LU with partial
    pivoting is backward stable, so the plain solve's residual already sits at the rounding level of its own evaluation (median 2.9e-14 here), and the refined step,
    rounded to fp64 once, lands on the same level (median 2.1e-14) -- below the plain solve's on 61 of 78 factorisations, above it on 17, by up to 11 x.  Evaluated in
    np.longdouble the refined step's residual is the smaller one on 77 of 78 (median 5.5e-15 against 2.7e-14).  What refinement removes is the forward error
    (condition number x rounding), which is what moves an iterate."""
    assert np.finfo(np.longdouble).eps < 2e-19
    L = np.longdouble
    rec = []
    plain = I.refine_solution

    def spy(K, rhs, sol, steps):
        out, lr = plain(K, rhs, sol, steps)
        Kl, rl, acc = K.astype(L), rhs.astype(L), out.astype(L)
        for _ in range(6):
            acc = acc + np.linalg.solve(K, (rl - Kl @ acc).astype(np.float64)).astype(L)
        rec.append((lr[0], lr[1], float(np.abs(Kl @ sol.astype(L) - rl).max()), float(np.abs(Kl @ out.astype(L) - rl).max()), float(np.abs(sol - acc).max()), float(np.abs(out - acc).max()), float(np.abs(acc).max())))
        return out, lr
    monkeypatch.setattr(I, "refine_solution", spy)
    T._numpy_run.__wrapped__("pit_carlike_n43", T.REFINE)          # uncached: the spy has to see the solves
    a = np.array(rec)
    assert len(a) > 4 * T.B          # more factorisations than iterations: the ladder ran
    print(f"[refinement] {len(a)} factorisations; error against the extended-precision solution: before max {a[:, 4].max():.1e}, after max {a[:, 5].max():.1e}, worst after / before "
          f"{(a[:, 5] / a[:, 4]).max():.2f}; residual evaluated in fp64: before median {np.median(a[:, 0]):.1e}, after median {np.median(a[:, 1]):.1e}, raised on {int((a[:, 1] > a[:, 0]).sum())}; "
          f"evaluated in longdouble: before median {np.median(a[:, 2]):.1e}, after median {np.median(a[:, 3]):.1e}, raised on {int((a[:, 3] > a[:, 2]).sum())}")
    assert (a[:, 5] <= a[:, 4]).all(), a[a[:, 5] > a[:, 4]]
    assert (a[:, 5] <= np.finfo(np.float64).eps * np.maximum(a[:, 6], 1.0)).all(), (a[:, 5] / a[:, 6]).max()


def test_refine_steps_zero_reproduces_a_base_golden_set_bit_for_bit():
    g = np.load(os.path.join(T.HERE, "golden", "unicycle_quadratic_n20.npz"))
    cfg = R.config_unicycle_quadratic(20)
    assert I.IpmOptions().refine_steps == 0
    for i in range(g["x0"].shape[0]):
        inp = R.CycleInputs(x0=g["x0"][i], xf=g["xf"][i], u_prev=g["u_prev"][i], dt_prev=float(g["dt_prev"][i]))
        res = I.solve(cfg, inp, R.cold_start(cfg, g["x0"][i], g["xf"][i]), opt=I.IpmOptions(max_iter=100))
        assert res.status == 0 and res.iters == g["iters"][i]
        assert np.array_equal(res.traj.x, g["x"][i]) and np.array_equal(res.traj.u, g["u"][i, :-1]) and res.traj.dt == g["dt"][i]
        assert all(e["lin_res"] == [] for e in res.history)
