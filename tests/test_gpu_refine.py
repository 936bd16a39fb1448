"""rsp_refine_solve on the device against its restatement (refine_ref.py), and
the clauses of its contract that need no restatement.

1. test_fixed_work: rtol = inner_rtol = 0, three steps of five inner
   iterations; history and x within refine_ref.tolerance(run) of the longdouble
   restatement (100 x the CPU-measured spread of three fp64 dot orders).
2. test_to_tolerance: rtol = 1e-12 at inner_rtol = 1e-4; CONVERGED, the counts
   within the CPU-measured spread of the restatement's, the true residual
   recomputed on the host within rtol plus that recomputation's rounding
   bound, and the all-fp32 solver on the same system at least 1e3 times worse.
3. test_scale_invariance: (b, x0) and 2^-120 (b, x0) give the same history and
   counts bit for bit and x' = 2^-120 x bit for bit, FTZ off and on: the
   scaling exists, is exact and is applied on both sides.
4. stagnation, breakdown, the ends, repeatability, check_every, every argument
   check of create and solve, and the test_solve driver's --refine.
Every test prints its own figures next to its tolerances. On an MI355X the
histories are off by at most 3.4e-16 (tolerances >= 2.2e-14), x is bitwise the
restatement's in every run, and steps and inner iterations are its counts.
"""
import ctypes as C
import os
import re
import subprocess
import time

import numpy as np
import pytest
import torch

import krylov_ref as kr
import oracle_bind as ob
import refine_ref as rf
from respasol_amd import _lib
from respasol_amd.sparse import CG, GMRES, BiCGStab, Handle, Ilu0, Refine, SpMat, convert_scaled, upload_csr

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


class Devices:
    """What the module shares on the device, per handle mode and matrix: the
    fp64 matrix, its fp32 twin over the same pattern (values narrowed by
    convert_scaled), one analysed ILU(0) and its fp32 factor."""

    def __init__(self):
        self.h = {False: Handle(), True: Handle(ftz=True)}
        self.sys = {}

    def system(self, g, ilu=True, ftz=False):
        key = (id(g), ilu, ftz)
        if key not in self.sys:
            h = self.h[ftz]
            rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values)
            A = SpMat(h, rp, ci, va, g.n)
            low = convert_scaled(h, va, exp2=0, dtype=torch.float32)
            assert np.array_equal(low.cpu().numpy(), g.vals(np.float32))
            A_low = SpMat(h, rp, ci, low, g.n)
            il = fac = None
            if ilu:
                il = Ilu0(h, rp, ci)
                il.analysis()
                fac = low.clone()
                il.factor(fac)
            self.sys[key] = (A, A_low, il, fac, g)  # (g kept: its id is the key)
        return self.sys[key][:4]

    def refine(self, case, ftz=False):
        method, restart, _, pc = case
        A, A_low, il, fac = self.system(rf.case_grid(case), pc != "none", ftz)
        return Refine(self.h[ftz], A, A_low, il, fac, method=method, restart=max(restart, 1))

    def close(self):
        for A, A_low, il, _, _ in self.sys.values():
            if il is not None:
                il.close()
            A_low.close()
            A.close()
        for h in self.h.values():
            h.close()


@pytest.fixture(scope="module")
def dev():
    t0 = time.perf_counter()
    d = Devices()
    yield d
    torch.cuda.synchronize()
    d.close()
    print(f"\ntest_gpu_refine: {time.perf_counter() - t0:.1f} s wall for the module")


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def solve(dev, case, b, x0, ftz=False, **kw):
    s = dev.refine(case, ftz)
    try:
        return s.solve(on_device(b), x0=None if x0 is None else on_device(x0), **kw)
    finally:
        s.close()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def hist_dev(hist, ref):
    return float(np.max(np.abs(np.asarray(hist) - ref) / np.abs(ref)))


CASE_T = ("cg", 0, "T", "fp32")
CASE_S = ("gmres", 10, "S", "fp32")


# ------------------------------------------------------------ 1. fixed work

@pytest.mark.parametrize("case", rf.CASES, ids=[rf.case_id(c) for c in rf.CASES])
def test_fixed_work(dev, case):
    run = (case, "fixed")
    ref = rf.reference(run)
    tol_hist, tol_x, _, _ = rf.tolerance(run)
    J, K = rf.FIXED["max_steps"], rf.FIXED["inner_max_iters"]
    b, x0 = rf.case_grid(case).rhs_and_start(np.float64)
    res = solve(dev, case, b, x0, **rf.FIXED)
    assert res.reason == Refine.MAX_ITERS and res.steps == J and res.iters == J * K
    assert res.inner_history == [0] + [K] * J and len(res.history) == J + 1
    assert res.relres == res.history[-1]
    dh = hist_dev(res.history, ref.history)
    x = res.x.cpu().numpy()
    dx = float(np.max(np.abs(x - ref.x)) / np.max(np.abs(ref.x)))
    print(f"{rf.run_id(run)}: history off by {dh:.2e} (tolerance {tol_hist:.2e}), x by {dx:.2e} "
          f"(tolerance {tol_x:.2e})")
    assert dh <= tol_hist
    assert dx <= tol_x


# ---------------------------------------------------------- 2. to tolerance

def residual_and_bound(g, b, x):
    """||b - A x|| recomputed in fp64 through the oracle's canonical SpMV, and
    the rounding bound of that recomputation: gamma_{row length + 2} of
    || |A||x| + |b| ||, gamma_k = k u / (1 - k u)."""
    r = b - g.matvec(x, np.float64)
    k = int(np.max(np.diff(g.rowptr))) + 2
    gamma = k * U / (1.0 - k * U)
    mag = ob.spmv(g.rowptr, g.colidx, np.abs(g.values), np.abs(x), order="canon") + np.abs(b)
    return float(np.linalg.norm(r)), gamma * float(np.linalg.norm(mag))


def all_fp32(dev, case, b, x0):
    method, restart, _, pc = case
    _, A_low, il, fac = dev.system(rf.case_grid(case), pc != "none")
    h = dev.h[False]
    s = (CG(h, A_low, il, fac) if method == "cg" else BiCGStab(h, A_low, il, fac) if method == "bicgstab"
         else GMRES(h, A_low, il, fac, restart=restart))
    try:
        res = s.solve(on_device(b.astype(np.float32)), x0=on_device(x0.astype(np.float32)), rtol=0.0,
                      max_iters=rf.ALL_FP32_ITERS)
        return res.x.cpu().numpy().astype(np.float64)
    finally:
        s.close()


@pytest.mark.parametrize("case", rf.RTOL_CASES, ids=[rf.case_id(c) for c in rf.RTOL_CASES])
def test_to_tolerance(dev, case):
    run = (case, "tol")
    ref = rf.reference(run)
    tol_hist, tol_x, d_steps, d_inner = rf.tolerance(run)
    g = rf.case_grid(case)
    b, x0 = g.rhs_and_start(np.float64)
    rtol = rf.TO_TOL["rtol"]
    res = solve(dev, case, b, x0, **rf.TO_TOL)
    x = res.x.cpu().numpy()
    rn, bound = residual_and_bound(g, b, x)
    bn = float(np.linalg.norm(b))
    low, _ = residual_and_bound(g, b, all_fp32(dev, case, b, x0))
    print(f"{rf.run_id(run)}: {res.steps} steps (restatement {ref.steps}, allowance {d_steps}), {res.iters} inner "
          f"iterations ({ref.inner}, allowance {d_inner}), relres {res.relres:.2e}; true residual {rn / bn:.2e} of "
          f"||b|| (bound {rtol:.0e} + {bound / bn:.1e}); all fp32: {low / bn:.2e}")
    assert res.reason == Refine.CONVERGED and res.relres <= rtol and res.relres == res.history[-1]
    assert len(res.history) == res.steps + 1 and sum(res.inner_history) == res.iters
    assert abs(res.steps - ref.steps) <= d_steps
    assert abs(res.iters - ref.inner) <= d_inner
    assert rn <= rtol * bn + bound
    assert low >= 1e3 * rn
    if res.steps == ref.steps:  # the same path: the values are the restatement's too
        dh = hist_dev(res.history, ref.history)
        dx = float(np.max(np.abs(x - ref.x)) / np.max(np.abs(ref.x)))
        print(f"    history off by {dh:.2e} (tolerance {tol_hist:.2e}), x by {dx:.2e} (tolerance {tol_x:.2e})")
        if res.inner_history == ref.inner_history:
            assert dh <= tol_hist and dx <= tol_x


# ------------------------------------------------------- 3. scale invariance

@pytest.mark.parametrize("ftz", [False, True], ids=["ieee", "ftz"])
@pytest.mark.parametrize("case", [("cg", 0, "S", "fp32"), CASE_S, ("bicgstab", 0, "T", "fp32")],
                         ids=lambda c: rf.case_id(c))
def test_scale_invariance(dev, case, ftz):
    b, x0 = rf.case_grid(case).rhs_and_start(np.float64)
    a = solve(dev, case, b, x0, ftz=ftz, **rf.TO_TOL)
    s = solve(dev, case, np.ldexp(b, -120), np.ldexp(x0, -120), ftz=ftz, **rf.TO_TOL)
    print(f"{rf.case_id(case)} ftz={ftz}: {a.steps} steps, {a.iters} inner iterations, relres {a.relres:.2e}")
    assert a.reason == Refine.CONVERGED and a.steps >= 2
    assert (s.reason, s.steps, s.iters, s.inner_history) == (a.reason, a.steps, a.iters, a.inner_history)
    assert same_bits(s.history, a.history) and s.relres == a.relres
    assert same_bits(s.x.cpu().numpy(), np.ldexp(a.x.cpu().numpy(), -120))


# ------------------------------------------------ 4. the rest of the contract

def test_zero_correction_stagnates(dev):
    b, x0 = rf.case_grid(CASE_T).rhs_and_start(np.float64)
    res = solve(dev, CASE_T, b, x0, rtol=1e-12, inner_max_iters=0)
    assert (res.reason, res.steps, res.iters) == (Refine.STAGNATED, 0, 0)
    assert len(res.history) == 2 and res.history[0] == res.history[1] == res.relres
    assert res.inner_history == [0, 0]
    assert same_bits(res.x.cpu().numpy(), x0)


def test_breakdown_on_a_nan_in_b(dev):
    b, x0 = rf.case_grid(CASE_T).rhs_and_start(np.float64)
    b = b.copy()
    b[-1] = np.nan
    res = solve(dev, CASE_T, b, x0)
    assert (res.reason, res.steps, res.iters) == (Refine.BREAKDOWN, 0, 0)
    assert len(res.history) == 1 and np.isnan(res.history[0])
    assert same_bits(res.x.cpu().numpy(), x0)


def test_breakdown_of_the_inner_solve(dev):
    """[[0, 1], [-1, 0]] blocks under CG inside: (p, A p) = 0 bit for bit (b of
    ones and zeros, x0 of eighths: every product and sum is exact, also after
    the power-of-two scaling), so the first inner solve breaks down before an
    iteration completes."""
    n = 3 * 2048 + 6
    g = kr.skew_blocks(n)
    b = np.where(np.arange(n) % 2 == 0, 1.0, 0.0)
    x0 = np.random.default_rng(77).integers(-8, 9, n) / 8.0
    h = dev.h[False]
    rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values)
    A = SpMat(h, rp, ci, va, n)
    A_low = SpMat(h, rp, ci, convert_scaled(h, va, exp2=0, dtype=torch.float32), n)
    s = Refine(h, A, A_low, method="cg")
    try:
        res = s.solve(on_device(b), x0=on_device(x0))
        assert (res.reason, res.steps, res.iters) == (Refine.BREAKDOWN, 0, 0)
        r0 = b - g.matvec(x0)
        assert len(res.history) == 1 and res.relres == res.history[0] == np.sqrt(np.sum(r0 * r0)) / np.sqrt(n // 2)
        assert same_bits(res.x.cpu().numpy(), x0)
    finally:
        s.close()
        A_low.close()
        A.close()


def test_ends(dev):
    g = rf.case_grid(CASE_T)
    b, x0 = g.rhs_and_start(np.float64)
    # b = 0: x = 0
    res = solve(dev, CASE_T, np.zeros(g.n), x0)
    assert (res.reason, res.steps, res.iters, res.relres) == (Refine.CONVERGED, 0, 0, 0.0)
    assert res.history == [] and torch.count_nonzero(res.x).item() == 0
    # a start already inside rtol: untouched
    good = solve(dev, CASE_T, b, x0, rtol=1e-12)
    assert good.reason == Refine.CONVERGED and good.steps >= 2
    xg = good.x.cpu().numpy()
    res = solve(dev, CASE_T, b, xg, rtol=1e-10)
    assert (res.reason, res.steps, res.iters) == (Refine.CONVERGED, 0, 0)
    assert res.history == [good.relres] and same_bits(res.x.cpu().numpy(), xg)
    # max_steps = 0: the residual only
    res = solve(dev, CASE_T, b, x0, max_steps=0)
    assert (res.reason, res.steps, res.iters) == (Refine.MAX_ITERS, 0, 0)
    assert res.history == [good.history[0]] == [res.relres] and same_bits(res.x.cpu().numpy(), x0)
    # x0 = None is a zero start
    z = solve(dev, CASE_T, b, None, rtol=1e-12)
    assert z.reason == Refine.CONVERGED and z.history[0] == 1.0


@pytest.mark.parametrize("case", [CASE_T, CASE_S, ("bicgstab", 0, "S", "fp32")], ids=lambda c: rf.case_id(c))
def test_repeatable_and_check_every_changes_no_bit(dev, case):
    b, x0 = rf.case_grid(case).rhs_and_start(np.float64)
    a = solve(dev, case, b, x0, **rf.TO_TOL)
    c = solve(dev, case, b, x0, **rf.TO_TOL)
    assert (a.reason, a.steps, a.iters, a.inner_history) == (c.reason, c.steps, c.iters, c.inner_history)
    assert same_bits(a.history, c.history) and torch.equal(a.x, c.x)
    f1 = solve(dev, case, b, x0, check_every=1, **rf.FIXED)
    f3 = solve(dev, case, b, x0, check_every=3, **rf.FIXED)
    assert (f1.steps, f1.iters) == (f3.steps, f3.iters) == (3, 15)
    assert torch.equal(f1.x, f3.x) and same_bits(f1.history, f3.history)


def test_argument_checks(dev):
    g = rf.case_grid(CASE_T)
    h = dev.h[False]
    A, A_low, il, fac = dev.system(g)
    INV = _lib.STATUS_INVALID_VALUE
    create = _lib.rsp.rsp_refine_create
    out = C.c_void_p()
    facp = C.c_void_p(fac.data_ptr())
    rp, ci, va = upload_csr(g.rowptr[:101], g.colidx[:g.rowptr[100]], g.values[:g.rowptr[100]])
    small = SpMat(h, rp, ci, va.to(torch.float32), g.n)  # 100 x n: neither square nor A's size
    try:
        bad = [
            (h.ptr, None, A_low._mat, il._info, facp, 1, 30, C.byref(out)),
            (h.ptr, A._mat, None, il._info, facp, 1, 30, C.byref(out)),
            (h.ptr, A._mat, A_low._mat, il._info, None, 1, 30, C.byref(out)),
            (h.ptr, A._mat, A_low._mat, il._info, facp, 1, 30, None),
            (h.ptr, A_low._mat, A_low._mat, il._info, facp, 1, 30, C.byref(out)),  # A not fp64
            (h.ptr, A._mat, A._mat, il._info, facp, 1, 30, C.byref(out)),          # A_low not fp32
            (h.ptr, A._mat, small._mat, il._info, facp, 1, 30, C.byref(out)),      # another size
            (h.ptr, A._mat, A_low._mat, il._info, facp, 3, 30, C.byref(out)),
            (h.ptr, A._mat, A_low._mat, il._info, facp, -1, 30, C.byref(out)),
            (h.ptr, A._mat, A_low._mat, il._info, facp, 2, 0, C.byref(out)),
            (h.ptr, A._mat, A_low._mat, il._info, facp, 2, _lib.GMRES_MAX_RESTART + 1, C.byref(out)),
        ]
        for args in bad:
            assert create(*args) == INV, args[5:7]
            assert not out.value
        assert create(None, A._mat, A_low._mat, il._info, facp, 1, 30, C.byref(out)) == _lib.STATUS_NOT_INITIALIZED
        # CG and BiCGStab ignore restart; M = I needs no factor
        for method, restart, info, f in ((0, 0, il._info, facp), (1, -5, il._info, facp), (1, 0, None, None)):
            assert create(h.ptr, A._mat, A_low._mat, info, f, method, restart, C.byref(out)) == _lib.STATUS_SUCCESS
            assert _lib.rsp.rsp_refine_destroy(out) == _lib.STATUS_SUCCESS
            out = C.c_void_p()
        assert _lib.rsp.rsp_refine_destroy(None) == INV
    finally:
        small.close()

    b, x0 = g.rhs_and_start(np.float64)
    d_b, d_x = on_device(b), on_device(x0)
    s = dev.refine(CASE_T)
    try:
        steps, inner, reason, rel = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        pb, px = C.c_void_p(d_b.data_ptr()), C.c_void_p(d_x.data_ptr())
        good = dict(h=h.ptr, s=s._s, b=pb, x=px, rtol=1e-10, max_steps=5, inner_rtol=1e-4, inner=50, every=1,
                    steps=C.byref(steps), inner_iters=C.byref(inner), rel=C.byref(rel), reason=C.byref(reason))
        order = ("h", "s", "b", "x", "rtol", "max_steps", "inner_rtol", "inner", "every", "steps", "inner_iters", "rel",
                 "reason")
        changes = [("s", None), ("b", None), ("x", None), ("steps", None), ("inner_iters", None), ("rel", None),
                   ("reason", None), ("max_steps", -1), ("inner", -1), ("every", 0), ("rtol", -1e-3),
                   ("rtol", float("nan")), ("inner_rtol", -1e-3), ("inner_rtol", float("nan"))]
        for key, value in changes:
            args = dict(good)
            args[key] = value
            assert _lib.rsp.rsp_refine_solve(*[args[k] for k in order]) == INV, (key, value)
        args = dict(good, h=None)
        assert _lib.rsp.rsp_refine_solve(*[args[k] for k in order]) == _lib.STATUS_NOT_INITIALIZED
        torch.cuda.synchronize()
        assert same_bits(d_x.cpu().numpy(), x0)  # nothing was written
        assert _lib.rsp.rsp_refine_solve(*[good[k] for k in order]) == _lib.STATUS_SUCCESS
        assert reason.value == Refine.CONVERGED
        count = C.c_int()
        hist, its = (C.c_double * 8)(), (C.c_int * 8)()
        hp = _lib.rsp.rsp_refine_history
        assert hp(None, 0, None, None, C.byref(count)) == INV
        assert hp(s._s, 0, None, None, None) == INV
        assert hp(s._s, -1, hist, its, C.byref(count)) == INV
        assert hp(s._s, 8, None, its, C.byref(count)) == INV and hp(s._s, 8, hist, None, C.byref(count)) == INV
        assert hp(s._s, 1, hist, its, C.byref(count)) == _lib.STATUS_SUCCESS  # cap below count: the first entry only
        assert count.value == steps.value + 1 and hist[1] == 0.0 and its[0] == 0
        assert hp(s._s, 8, hist, its, C.byref(count)) == _lib.STATUS_SUCCESS
        assert hist[count.value - 1] == rel.value and sum(its[:count.value]) == inner.value
    finally:
        s.close()


# ------------------------------------------------------------------ driver

def run_driver(spec, *flags):
    r = subprocess.run([os.path.join(_lib.BIN_DIR, "test_solve"), spec, *flags], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    got = {}
    for key in ("Symbolic", "Numeric", "Solve", "Iterations", "Reason", "Relative residual", "Refinement steps",
                "Inner iterations"):
        m = re.search(rf"^\s*{key} = (\S+)\s*$", r.stdout, re.M)
        if m:
            got[key] = float(m.group(1))
    return got, r.stdout


@pytest.mark.parametrize("spec,method", [("surrogate:ecology2@0.02", "cg"), ("surrogate:Baumann@0.1", "gmres")])
def test_solve_driver_refines(spec, method):
    """The existing fp64 iteration under the fp32 preconditioner converges on
    the surrogate; --refine then reaches the driver's default rtol (1e-10) too,
    within the margin the other driver tests allow over it (2e-10), and adds
    its two lines after the six of the report."""
    base, _ = run_driver(spec, f"--method={method}", "--precond=fp32")
    assert base["Reason"] == 0 and base["Relative residual"] <= 2e-10
    assert "Refinement steps" not in base
    got, out = run_driver(spec, f"--method={method}", "--precond=fp32", "--refine")
    print(f"{spec} {method}: fp64 iteration {base['Iterations']:.0f} iterations, {base['Relative residual']:.2e}; "
          f"refined {got['Refinement steps']:.0f} steps, {got['Inner iterations']:.0f} inner iterations, "
          f"{got['Relative residual']:.2e}")
    assert got["Reason"] == 0
    assert got["Relative residual"] <= 2e-10
    assert got["Refinement steps"] >= 1 and got["Inner iterations"] == got["Iterations"] >= got["Refinement steps"]
    assert out.startswith("DOUBLE PRECISION ITERATION IN  MILLISECONDS\n Symbolic = ")
    assert re.search(r"Relative residual = \S+\n Refinement steps = \d+\n Inner iterations = \d+\n$", out)
