"""GPU tests (-m gpu): the fused step pass of the one-grid-point-per-lane launches at the headline's own size.

Launches in the LDS form without clearance rows, n <= 64, take the line search's registers straight out of post_pass (mpc_wave_step.inc, kFusedPasses) and read the
solve loop's constants from scalar registers; the global form (MPC_STAGE_GLOBAL) keeps the separate passes (post_pass, then trial_setup / the generic trials).  The
two forms are bit-identical in fp64 (tests/test_gpu_parity.py, up to n = 64 at 32 instances and at n = 50 with the caps 60 45 40 35), so holding one against the other
at car-like n = 50 with 1024 instances -- the batch bench.py times -- holds the fused path to the separate passes where the other tests do not reach: the headline's caps,
a warm-started cycle, row 0 switched off, ragged grids, the unicycle model, fp32.

Every comparison also asserts that more than 90 % of the instances converged: an all-failed batch must not pass as "equal"."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 1024
FIELDS = ("x", "u", "dt", "status", "iters")
HEADLINE = dict(candidates=(0, 5, 5, 7), candidate_max_iter=(100, 45, 40, 35), candidate_param=(0.0, 2.0, 3.0, 1.5))


@pytest.fixture(scope="module")
def m():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("these tests need the MI355X (no HIP device here)")
    torch.zeros(1, device="cuda")          # torch's HIP runtime before the library's
    import mpc_local_planner_amd as pkg
    return pkg


def _forms(m, mk, run):
    """run(solver) -> a list of results, once per form; returns (fused LDS form, separate global form)"""
    from mpc_local_planner_amd import _abi as A
    out = []
    for mode in (A.STAGE_LDS, A.STAGE_GLOBAL):
        s = m.BatchSolver(mk(stage_data=mode), max_batch=B)
        out.append(run(s))
        s.close()
    return out


def _equal_bit_for_bit(label, fused, separate):
    for k, (a, g) in enumerate(zip(fused, separate)):
        print(f"[{label}] solve {k}: converged {np.mean(a.status == 0):.4f} (fused) {np.mean(g.status == 0):.4f} (separate), iterations {a.iters.mean():.2f} / {g.iters.mean():.2f}, "
              f"largest iteration count {a.iters.max()}")
        assert (a.status == 0).mean() > 0.9 and (g.status == 0).mean() > 0.9
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(g, f), equal_nan=True), (label, k, f)


@pytest.mark.parametrize("cand", ["one_candidate", "headline_candidates"])
def test_cold_start_at_the_headline_size(m, cand):
    """car-like n = 50, 1024 instances, bench.py's inputs: the reference path alone, and the headline's four candidates at its caps 100 45 40 35 (the 100-iteration
    stragglers that set the headline time run all of their iterations here)"""
    kw = HEADLINE if cand == "headline_candidates" else {}
    inp = m.workloads.carlike_min_time_inputs(B)
    fused, separate = _forms(m, lambda **k: m.config_carlike_min_time(50, **kw, **k), lambda s: [s.solve(*inp)])
    _equal_bit_for_bit(cand, fused, separate)
    if cand == "headline_candidates":
        assert fused[0].iters.max() >= 100          # a straggler of the reference path is among them


def test_warm_started_second_cycle_from_kept_multipliers(m):
    """dual_warm_start: the second cycle enters the solve loop from the last cycle's trajectory and multipliers (the kernel's other entry into the loop)"""
    inp = m.workloads.carlike_min_time_inputs(B, seed=77)
    def run(s):
        r1 = s.solve(*inp)
        x1 = inp[0].copy(); x1[:, :2] += 0.02
        r2 = s.solve(x1, inp[1], r1.u[:, 0].copy(), inp[3], init=(r1.x.copy(), r1.u.copy(), r1.dt.copy()))
        return [r1, r2]
    fused, separate = _forms(m, lambda **k: m.config_carlike_min_time(50, mu_init_warm=1e-2, dual_warm_start=True, mu_init_dual=1e-3, **k), run)
    _equal_bit_for_bit("warm start", fused, separate)
    assert fused[1].iters.mean() < fused[0].iters.mean()


def test_first_rate_row_switched_off(m):
    """dt_prev = 0: no previous control, the rate rows of grid point 0 are off (row_on(0, q) false in lane 0 only)"""
    x0, xf, up, dtp = m.workloads.carlike_min_time_inputs(B, seed=31)
    inp = (x0, xf, up, np.zeros_like(dtp))
    fused, separate = _forms(m, lambda **k: m.config_carlike_min_time(50, **k), lambda s: [s.solve(*inp)])
    _equal_bit_for_bit("dt_prev = 0", fused, separate)


def test_ragged_batch_of_8_to_50_grid_points(m):
    """set_grid_sizes: n from 8 to 50 in ONE launch of the handle made for 50 -- lanes beyond n - 1 idle in every pass, grids below 40 points take the serial sweeps"""
    sizes = (8 + np.arange(B) % 43).astype(np.int32)
    assert sizes.min() == 8 and sizes.max() == 50
    inp = m.workloads.carlike_min_time_inputs(B, seed=8, goal_range=(0.5, 2.5))
    def run(s):
        s.set_grid_sizes(sizes)
        return [s.solve(*inp)]
    fused, separate = _forms(m, lambda **k: m.config_carlike_min_time(50, **k), run)
    _equal_bit_for_bit("ragged", fused, separate)


@pytest.mark.parametrize("n", [50, 64])
def test_unicycle_model(m, n):
    """the quadratic-form unicycle (another model, the quadratic objective's terms in every pass) at the headline's grid and at the last grid with one point per lane"""
    inp = m.workloads.unicycle_quadratic_inputs(B, seed=n)
    fused, separate = _forms(m, lambda **k: m.config_unicycle_quadratic(n, **k), lambda s: [s.solve(*inp)])
    _equal_bit_for_bit(f"unicycle n = {n}", fused, separate)


def test_fp32_within_the_tolerance_of_the_other_fp32_form_comparisons(m):
    """precision = MPC_FP32 on the headline's inputs.  The two forms agree to rounding only in fp32 (the compiler contracts the fp32 passes differently around global
    loads: tests/test_gpu_parity.py::test_factorisation_data_in_global_memory_equals_lds_bit_for_bit), so the bounds are that test's: converged fractions within 0.02,
    more than half of the instances converged in both forms with the same iteration count, and over those a median largest state difference below 1e-3."""
    from mpc_local_planner_amd import _abi as A
    inp = m.workloads.carlike_min_time_inputs(B)
    fused, separate = _forms(m, lambda **k: m.config_carlike_min_time(50, precision=A.FP32, tol=1e-4, **k), lambda s: [s.solve(*inp)])
    a, g = fused[0], separate[0]
    both = (a.status == 0) & (g.status == 0) & (a.iters == g.iters)
    med = np.median(np.abs(a.x - g.x).reshape(B, -1).max(1)[both]) if both.any() else np.inf
    print(f"[fp32] converged {np.mean(a.status == 0):.4f} (fused) {np.mean(g.status == 0):.4f} (separate), same iteration count {both.mean():.4f}, median largest |dx| {med:.3e}")
    assert (a.status == 0).mean() > 0.9 and (g.status == 0).mean() > 0.9
    assert abs((a.status == 0).mean() - (g.status == 0).mean()) < 0.02 and both.mean() > 0.5
    assert med < 1e-3
