"""The tolerances of test_gpu_refine.py and what the refinement is for, on the
CPU alone (the restatement is refine_ref.py, the method test_cg_trajectory.py's).

The GPU test runs rsp_refine_solve from a seeded b and a non-zero x0 and
compares history, x and the counts with the same loop restated in numpy with
np.longdouble dots. What separates the two is the order in which a dot is
summed, so a value's tolerance is 100 x the spread of the restatement under
three fp64 summation orders, per run; a spread under one fp64 ulp counts as one
ulp. A count's allowance is the spread of the counts itself. Nothing here comes
from a GPU run.

Measured (s_hist; x was bitwise equal under all four dot kinds in every run,
and so were the counts), then the restatement's steps / inner iterations:

    fixed work: 3 steps of 5 inner iterations
      cg S 0         cg T 1.9e-16       bicgstab S 1.3e-16   bicgstab T 2.2e-16
      gmres S 1.4e-16  gmres T 2.4e-16  cg T, M = I 3.4e-16  gmres L 7.0e-16
    to rtol = 1e-12 at inner_rtol = 1e-4
      cg S 1.2e-16, 4 / 181        cg T 1.9e-16, 3 / 17       cg T, M = I 1.9e-16, 3 / 50
      bicgstab S 2.2e-16, 3 / 42   bicgstab T 3.6e-16, 3 / 10
      gmres S 1.6e-16, 4 / 104     gmres T 4.1e-16, 4 / 23

The all-fp32 solver on the same systems, run 200 iterations to its floor,
leaves true residuals between 8.8e-8 (gmres T) and 3.6e-6 (cg S) of ||b||;
the refined solves end between 2.8e-16 and 8.1e-13.
"""
import numpy as np
import pytest

import refine_ref as rf

RUN_IDS = [rf.run_id(r) for r in rf.RUNS]


def test_cases_are_the_ones_listed():
    assert rf.CASES == [("cg", 0, "S", "fp32"), ("cg", 0, "T", "fp32"), ("bicgstab", 0, "S", "fp32"),
                        ("bicgstab", 0, "T", "fp32"), ("gmres", 10, "S", "fp32"), ("gmres", 10, "T", "fp32"),
                        ("cg", 0, "T", "none"), ("gmres", 10, "L", "fp32")]
    assert set(rf.SPREAD) == set(rf.RUNS)
    assert [c for c in rf.CASES if c not in rf.RTOL_CASES] == [("gmres", 10, "L", "fp32")]
    n = {c: rf.case_grid(c).n for c in rf.CASES}
    assert {c[2]: v for c, v in n.items()} == {"S": 3 * 2048 + 5, "T": 2049, "L": 525312}
    # CG runs on the symmetric grid, the other two on the convection-diffusion grid
    g = rf.case_grid(rf.CASES[0])
    assert np.array_equal(g.matvec(np.ones(g.n)), rf.cr.grid("S").matvec(np.ones(g.n)))
    assert rf.case_grid(rf.CASES[2]) is rf.kr.grid("S")


def test_inner_solvers_are_the_trajectories():
    """With no stop (rtol = 0) the three inner solvers are the trajectory
    restatements they were written out from, bit for bit."""
    K = 6
    for name, g, run, ref in (
            ("cg", rf.cr.grid("S"), lambda g, b, x0, d: rf.cg_solve(g, rf.F32, rf.F32, b, x0, 0.0, K, d),
             lambda g, b, x0, d: rf.cr.cg_trajectory(g, rf.F32, rf.F32, K, b, x0, d)),
            ("bicgstab", rf.kr.grid("S"), lambda g, b, x0, d: rf.bicgstab_solve(g, rf.F32, rf.F32, b, x0, 0.0, K, d),
             lambda g, b, x0, d: rf.kr.bicgstab_trajectory(g, rf.F32, rf.F32, K, b, x0, d)),
            ("gmres", rf.kr.grid("S"), lambda g, b, x0, d: rf.fgmres_solve(g, rf.F32, rf.F32, 4, b, x0, 0.0, K, d),
             lambda g, b, x0, d: rf.kr.fgmres_trajectory(g, rf.F32, rf.F32, 4, K, b, x0, d))):
        b, x0 = g.rhs_and_start(rf.F32)
        x, iters, reason = run(g, b, x0, rf.Dot("forward"))
        x_ref, _ = ref(g, b, x0, rf.Dot("forward"))
        assert (iters, reason) == (K, rf.MAX_ITERS), name
        assert x.dtype == rf.F32 and np.array_equal(x, x_ref), name


def test_scaling_is_exact_and_normalises():
    """r32's norm lies in [0.5, 1) up to fp32 rounding, and the scaling commutes
    with a power of two bit for bit: what the GPU scale-invariance test rests on."""
    rng = np.random.default_rng(5)
    r = rng.uniform(-1.0, 1.0, 4099) * 3.1e-11
    rn = float(np.sqrt(np.sum(r * r)))
    e = rf.scale_exp(rn)
    r32 = np.ldexp(r, -e).astype(rf.F32)
    assert 0.5 * (1 - 1e-6) <= np.linalg.norm(r32.astype(np.float64)) < 1.0 + 1e-6
    r2 = np.ldexp(r, -120)
    e2 = rf.scale_exp(float(np.sqrt(np.sum(r2 * r2))))
    assert e2 == e - 120 and np.array_equal(np.ldexp(r2, -e2).astype(rf.F32), r32)
    assert rf.scale_exp(5e-324) == -1022 and rf.scale_exp(1.7e308) == 1022


@pytest.mark.parametrize("run", rf.RUNS, ids=RUN_IDS)
def test_spread_stays_under_the_constants(run):
    ref = rf.reference(run)
    mode = rf.MODES[run[1]]
    assert np.all(np.isfinite(ref.history)) and len(ref.history) == ref.steps + 1
    assert len(ref.inner_history) == len(ref.history) and sum(ref.inner_history) == ref.inner
    if run[1] == "fixed":
        J, K = mode["max_steps"], mode["inner_max_iters"]
        assert (ref.reason, ref.steps, ref.inner) == (rf.MAX_ITERS, J, J * K)
        assert ref.inner_history == [0] + [K] * J
        assert np.all(np.diff(ref.history) < 0.0)
    else:
        assert ref.reason == rf.CONVERGED and ref.steps <= mode["max_steps"]
        assert ref.relres == ref.history[-1] <= 1e-12 < ref.history[-2]
    s = [0.0, 0.0, 0, 0]
    for kind in rf.FP64_ORDERS:
        s = [max(a, b) for a, b in zip(s, rf.deviation(rf.run_case(run, kind), ref))]
    c = rf.SPREAD[run]
    tol = rf.tolerance(run)
    print(f"{rf.run_id(run)}: steps {ref.steps}, inner {ref.inner}; s_hist {s[0]:.2e} (<= {c[0]:.2e}), "
          f"s_x {s[1]:.2e} (<= {c[1]:.2e}), counts off by {s[2]}, {s[3]} (<= {c[2]}, {c[3]}); "
          f"GPU tolerance {tol[0]:.2e}, {tol[1]:.2e}, {tol[2]}, {tol[3]}")
    assert s[0] <= c[0] and s[1] <= c[1] and s[2] <= c[2] and s[3] <= c[3]
    assert tol == (rf.MARGIN * max(c[0], rf.EPS), rf.MARGIN * max(c[1], rf.EPS), c[2], max(c[3], ref.steps, 1))


@pytest.mark.parametrize("case", rf.RTOL_CASES, ids=[rf.case_id(c) for c in rf.RTOL_CASES])
def test_refinement_reaches_what_fp32_cannot(case):
    """Every case run to tolerance reaches 1e-12 within 10 steps, true residual
    included, and the all-fp32 solver on the same system stays above 1e-8."""
    ref = rf.reference((case, "tol"))
    g = rf.case_grid(case)
    b, x0 = g.rhs_and_start(np.float64)
    assert ref.reason == rf.CONVERGED and ref.steps <= 10
    refined = rf.true_relres(g, b, ref.x)
    x32 = rf.all_fp32_solve(g, case[0], case[1], rf.NP[case[3]], b, x0, 0.0, rf.ALL_FP32_ITERS, rf.Dot())
    low = rf.true_relres(g, b, x32)
    print(f"{rf.case_id(case)}: {ref.steps} steps, {ref.inner} inner iterations, true residual {refined:.2e}; "
          f"all fp32: {low:.2e}")
    assert refined <= 1.01e-12
    assert low > 1e-8


def test_cg_on_the_small_grid_takes_few_steps():
    assert rf.reference((("cg", 0, "S", "fp32"), "tol")).steps <= 4
    assert rf.reference((("cg", 0, "T", "fp32"), "tol")).steps == 3


def test_zero_correction_stagnates_and_a_bad_start_breaks_down():
    """inner_max_iters = 0: the first step's residual equals the one before;
    a NaN in b: BREAKDOWN at step 0 with x untouched."""
    case = ("cg", 0, "T", "fp32")
    g = rf.case_grid(case)
    b, x0 = g.rhs_and_start(np.float64)
    res = rf.refine(g, "cg", 0, rf.F32, b, x0, 1e-12, 10, 1e-4, 0, rf.Dot("forward"))
    assert (res.reason, res.steps, res.inner) == (rf.STAGNATED, 0, 0)
    assert len(res.history) == 2 and res.history[0] == res.history[1] == res.relres
    assert np.array_equal(res.x, x0)
    bad = b.copy()
    bad[-1] = np.nan
    res = rf.refine(g, "cg", 0, rf.F32, bad, x0, 1e-12, 10, 1e-4, 5, rf.Dot("forward"))
    assert (res.reason, res.steps) == (rf.BREAKDOWN, 0) and np.array_equal(res.x, x0)
