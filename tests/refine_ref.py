"""Restatement of mixed-precision iterative refinement (rsp_refine_solve,
include/rsp.h) in NumPy (CPU only; test infrastructure for test_refine_ref.py
and test_gpu_refine.py), by the method of krylov_ref.py and cg_ref.py, whose
pieces it imports and never changes.

refine() is the loop of rsp.h: the residual b - A x and its norm in fp64, the
residual scaled by a power of two (math.frexp / np.ldexp) and rounded once to
fp32, an all-fp32 inner solve of the correction from d = 0, and the fp64 update
x + 2^e * double(d). The inner solvers are krylov_ref.bicgstab_trajectory,
cg_ref.cg_trajectory and krylov_ref.fgmres_trajectory written out again with the
library's stopping tests (rtol at every check, check_every = 1), because the
trajectories run a fixed count: every element-wise line is theirs, the SpMV is
the oracle's in the kernels' canonical order, ILU(0) and the triangular solves
are the oracle's in fp32. What separates the restatement from the device is the
order in which a dot product is summed. The dot is pluggable (krylov_ref.Dot):
np.longdouble is the reference, the three fp64 orders give the spread.
"""
import functools
import math

import numpy as np

import cg_ref as cr
import krylov_ref as kr
from krylov_ref import EPS, FP64_ORDERS, MARGIN, Dot, _f8, cgs2, rotate_column  # noqa: F401

CONVERGED, MAX_ITERS, BREAKDOWN, STAGNATED = 0, 1, 2, 3
F32 = np.float32


# ------------------------------------------- the inner solvers, with their stops

def cg_solve(g, precond, dtype, b, x0, rtol, max_iters, dot):
    """rsp_cg_solve at check_every = 1: (x, iters, reason)."""
    M = g.apply(precond)
    A = lambda y: g.matvec(y, dtype)
    x = x0.astype(dtype)
    r = b - A(x)
    bn = math.sqrt(dot(b, b))
    rr = dot(r, r)
    if math.sqrt(rr) / bn <= rtol:
        return x, 0, CONVERGED
    rho, p = 1.0, None
    for it in range(1, max_iters + 1):
        if precond is None:
            z, rho_new = r, rr
        else:
            z = M(r)
            rho_new = dot(r, z)
        if not (rho_new > 0.0 and math.isfinite(rho_new)):
            return x, it - 1, BREAKDOWN
        p = z.copy() if it == 1 else z + dtype(rho_new / rho) * p
        rho = rho_new
        q = A(p)
        pq = dot(p, q)
        if not (pq > 0.0 and math.isfinite(pq)):
            return x, it - 1, BREAKDOWN
        alpha = rho / pq
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        rr = dot(r, r)
        if math.sqrt(rr) / bn <= rtol:
            return x, it, CONVERGED
    return x, max_iters, MAX_ITERS


def bicgstab_solve(g, precond, dtype, b, x0, rtol, max_iters, dot):
    """rsp_bicgstab_solve at check_every = 1: (x, iters, reason)."""
    M = g.apply(precond)
    A = lambda y: g.matvec(y, dtype)
    x = x0.astype(dtype)
    r = b - A(x)
    rh = r.copy()
    bn = math.sqrt(dot(b, b))
    if math.sqrt(dot(r, r)) / bn <= rtol:
        return x, 0, CONVERGED
    rho = alpha = omega = 1.0
    p = v = None
    bad = lambda d: d == 0.0 or not math.isfinite(d)
    for it in range(1, max_iters + 1):
        rho_new = dot(rh, r)
        if bad(rho_new) or (it > 1 and (bad(rho) or bad(omega))):
            return x, it - 1, BREAKDOWN
        if it == 1:
            p = r.copy()
        else:
            beta = (rho_new / rho) * (alpha / omega)
            p = r + dtype(beta) * (p - dtype(omega) * v)
        rho = rho_new
        ph = M(p)
        v = A(ph)
        rhv = dot(rh, v)
        if bad(rhv):
            return x, it - 1, BREAKDOWN
        alpha = rho / rhv
        s = r - dtype(alpha) * v
        sh = M(s)
        t = A(sh)
        ts = dot(t, s)
        tt = dot(t, t)
        omega = ts / tt if tt != 0.0 else 0.0
        x = (x + dtype(alpha) * ph) + dtype(omega) * sh
        r = s - dtype(omega) * t
        if math.sqrt(dot(r, r)) / bn <= rtol:
            return x, it, CONVERGED
    return x, max_iters, MAX_ITERS


def fgmres_solve(g, precond, dtype, restart, b, x0, rtol, max_iters, dot):
    """rsp_gmres_solve at check_every = 1: (x, iters, reason). A check inside a
    cycle tests the estimate and, met, ends the solve after x += Z y; a cycle's
    end and the last iteration test the recomputed residual."""
    M = g.apply(precond)
    A = lambda y: g.matvec(y, dtype)
    m = restart
    x = x0.astype(dtype)
    w = b - A(x)
    bn = math.sqrt(dot(b, b))
    rr = dot(w, w)
    if math.sqrt(rr) / bn <= rtol:
        return x, 0, CONVERGED
    total = 0
    while total < max_iters:
        beta = math.sqrt(rr)
        V = [(_f8(w) / beta).astype(dtype)]
        Z, R = [], np.zeros((m + 1, m))
        cs, sn, gv = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        gv[0] = beta
        cols, by_est = 0, False
        while cols < m and total + cols < max_iters:
            j = cols
            Z.append(M(V[j]))
            w = A(Z[j])
            h, hn, w = cgs2(V, w, dot, dtype)
            col = np.append(h, hn)
            if not rotate_column(col, j, cs, sn, gv):
                return x, total + cols, BREAKDOWN
            R[:j + 2, j] = col
            cols += 1
            if hn == 0.0 or cols == m or total + cols == max_iters:
                break
            V.append((_f8(w) / hn).astype(dtype))
            if abs(gv[j + 1]) / bn <= rtol:
                by_est = True
                break
        y = np.zeros(cols)
        for i in range(cols - 1, -1, -1):
            v = gv[i]
            for l in range(i + 1, cols):
                v -= R[i, l] * y[l]
            y[i] = v / R[i, i]
        d = _f8(x).copy()
        for i in range(cols):
            d += y[i] * _f8(Z[i])
        x = d.astype(dtype)
        total += cols
        if by_est:
            return x, total, CONVERGED
        w = b - A(x)
        rr = dot(w, w)
        if math.sqrt(rr) / bn <= rtol:
            return x, total, CONVERGED
    return x, total, MAX_ITERS


def inner_solve(g, method, restart, precond, b32, rtol, max_iters, dot):
    x0 = np.zeros(g.n, F32)
    if method == "cg":
        return cg_solve(g, precond, F32, b32, x0, rtol, max_iters, dot)
    if method == "bicgstab":
        return bicgstab_solve(g, precond, F32, b32, x0, rtol, max_iters, dot)
    return fgmres_solve(g, precond, F32, restart, b32, x0, rtol, max_iters, dot)


# --------------------------------------------------------------- the refinement

class Result:
    def __init__(self, x, steps, inner, relres, reason, history, inner_history):
        self.x, self.steps, self.inner, self.relres, self.reason = x, steps, inner, relres, reason
        self.history, self.inner_history = np.array(history), list(inner_history)


def scale_exp(rn):
    """e with rn = m * 2^e, 0.5 <= m < 1, kept within what 2^e and 2^-e are normal fp64 values for."""
    return min(max(math.frexp(rn)[1], -1022), 1022)


def refine(g, method, restart, precond, b, x0, rtol, max_steps, inner_rtol, inner_max_iters, dot):
    """rsp_refine_solve at check_every = 1 (b non-zero): a Result."""
    x = x0.astype(np.float64)
    x_old = x
    bn = math.sqrt(dot(b, b))
    hist, inner_hist, inner_last, total, rn_prev = [], [], 0, 0, 0.0
    k = 0
    while True:
        r = b - g.matvec(x, np.float64)
        rn = math.sqrt(dot(r, r))
        hist.append(rn / bn)
        inner_hist.append(inner_last)
        if not (math.isfinite(rn) and math.isfinite(bn)):
            k_acc = max(k - 1, 0)
            return Result(x_old if k > 0 else x, k_acc, total, hist[k_acc], BREAKDOWN, hist, inner_hist)
        if rn / bn <= rtol:
            return Result(x, k, total, hist[k], CONVERGED, hist, inner_hist)
        if k > 0 and rn >= rn_prev:
            return Result(x_old, k - 1, total, hist[k - 1], STAGNATED, hist, inner_hist)
        if k == max_steps:
            return Result(x, k, total, hist[k], MAX_ITERS, hist, inner_hist)
        rn_prev = rn
        e = scale_exp(rn)
        r32 = np.ldexp(r, -e).astype(F32)
        d, inner_last, reason = inner_solve(g, method, restart, precond, r32, inner_rtol, inner_max_iters, dot)
        total += inner_last
        if reason == BREAKDOWN and inner_last == 0:
            return Result(x, k, total, hist[k], BREAKDOWN, hist, inner_hist)
        x_old = x
        x = x + np.ldexp(d.astype(np.float64), e)
        k += 1


def all_fp32_solve(g, method, restart, precond, b, x0, rtol, max_iters, dot):
    """The T = P = fp32 solver on the same system (b, x0 rounded to fp32): x as fp64."""
    b32, x32 = b.astype(F32), x0.astype(F32)
    if method == "cg":
        x, _, _ = cg_solve(g, precond, F32, b32, x32, rtol, max_iters, dot)
    elif method == "bicgstab":
        x, _, _ = bicgstab_solve(g, precond, F32, b32, x32, rtol, max_iters, dot)
    else:
        x, _, _ = fgmres_solve(g, precond, F32, restart, b32, x32, rtol, max_iters, dot)
    return x.astype(np.float64)


def true_relres(g, b, x):
    """||b - A x|| / ||b|| in fp64 through the oracle's canonical SpMV."""
    r = b - g.matvec(np.asarray(x, np.float64), np.float64)
    return float(np.linalg.norm(r) / np.linalg.norm(b))


# ------------------------------------------------------------------ the cases
#
# (method, restart, size, inner preconditioner). CG runs on cg_ref.SymGrid, the
# other two on krylov_ref.Grid, at krylov_ref.SIZES:
#   S  four workgroups and a 5-element tail (143 x 43 = 3 * 2048 + 5)
#   T  a 1-element tail (683 x 3 = 2049)
#   L  257 workgroups: the combine loop runs twice for thread 0. Fixed work only:
#      what L adds is the reduction's shape, which a fixed count of steps shows,
#      and to tolerance its restatement takes a minute per dot order. GMRES
#      there: five iterations of it reduce the residual at every step, so all
#      three steps are taken (five of CG do not: the second step stagnates)
CASES = [("cg", 0, "S", "fp32"), ("cg", 0, "T", "fp32"),
         ("bicgstab", 0, "S", "fp32"), ("bicgstab", 0, "T", "fp32"),
         ("gmres", 10, "S", "fp32"), ("gmres", 10, "T", "fp32"),
         ("cg", 0, "T", "none"),
         ("gmres", 10, "L", "fp32")]
RTOL_CASES = [c for c in CASES if c[2] != "L"]
# the two modes: a fixed amount of work, and to tolerance
FIXED = dict(rtol=0.0, max_steps=3, inner_rtol=0.0, inner_max_iters=5)
TO_TOL = dict(rtol=1e-12, max_steps=10, inner_rtol=1e-4, inner_max_iters=1000)
MODES = {"fixed": FIXED, "tol": TO_TOL}
RUNS = [(c, "fixed") for c in CASES] + [(c, "tol") for c in RTOL_CASES]
ALL_FP32_ITERS = 200  # of the all-fp32 solve the refined one is compared with (rtol = 0: to its floor)
NP = {"fp32": F32, "none": None}


def case_id(case):
    method, restart, size, pc = case
    return f"{method}{'' if method != 'gmres' else '-m%d' % restart}-{size}-{pc}"


def run_id(run):
    return f"{case_id(run[0])}-{run[1]}"


def case_grid(case):
    return cr.grid(case[2]) if case[0] == "cg" else kr.grid(case[2])


def run_case(run, kind="longdouble"):
    """The restatement of one run: a Result."""
    case, mode = run
    method, restart, _, pc = case
    g = case_grid(case)
    b, x0 = g.rhs_and_start(np.float64)
    return refine(g, method, restart, NP[pc], b, x0, dot=Dot(kind), **MODES[mode])


@functools.lru_cache(maxsize=None)
def reference(run):
    """The longdouble restatement of a run, computed once and left unchanged."""
    res = run_case(run)
    res.x.setflags(write=False)
    res.history.setflags(write=False)
    return res


def deviation(res, ref):
    """(history, x, steps, inner iterations) of a run against the reference:
    the largest relative deviation of a history entry over the steps both have,
    max|x - x_ref| / max|x_ref|, and the differences of the two counts."""
    n = min(len(res.history), len(ref.history))
    dh = float(np.max(np.abs(res.history[:n] - ref.history[:n]) / np.abs(ref.history[:n])))
    dx = float(np.max(np.abs(np.asarray(res.x, np.float64) - ref.x)) / np.max(np.abs(ref.x)))
    return dh, dx, abs(res.steps - ref.steps), abs(res.inner - ref.inner)


# ------------------------------------------------------------- the tolerances
#
# SPREAD[run] = (s_hist, s_x, d_steps, d_inner): the largest deviation of the
# three fp64 dot orders (krylov_ref.FP64_ORDERS) from the longdouble run,
# measured on the CPU, the first two rounded up to two digits;
# test_refine_ref.py recomputes them and holds the table. A spread below one
# fp64 ulp counts as one ulp. Nothing here comes from a GPU run.
SPREAD = {
    (("cg", 0, "S", "fp32"), "fixed"): (EPS, EPS, 0, 0),
    (("cg", 0, "T", "fp32"), "fixed"): (1.9e-16, EPS, 0, 0),
    (("bicgstab", 0, "S", "fp32"), "fixed"): (1.3e-16, EPS, 0, 0),
    (("bicgstab", 0, "T", "fp32"), "fixed"): (2.2e-16, EPS, 0, 0),
    (("gmres", 10, "S", "fp32"), "fixed"): (1.4e-16, EPS, 0, 0),
    (("gmres", 10, "T", "fp32"), "fixed"): (2.4e-16, EPS, 0, 0),
    (("cg", 0, "T", "none"), "fixed"): (3.4e-16, EPS, 0, 0),
    (("gmres", 10, "L", "fp32"), "fixed"): (7.0e-16, EPS, 0, 0),
    (("cg", 0, "S", "fp32"), "tol"): (1.2e-16, EPS, 0, 0),
    (("cg", 0, "T", "fp32"), "tol"): (1.9e-16, EPS, 0, 0),
    (("bicgstab", 0, "S", "fp32"), "tol"): (2.2e-16, EPS, 0, 0),
    (("bicgstab", 0, "T", "fp32"), "tol"): (3.6e-16, EPS, 0, 0),
    (("gmres", 10, "S", "fp32"), "tol"): (1.6e-16, EPS, 0, 0),
    (("gmres", 10, "T", "fp32"), "tol"): (4.1e-16, EPS, 0, 0),
    (("cg", 0, "T", "none"), "tol"): (1.9e-16, EPS, 0, 0),
}


def tolerance(run):
    """(tol_hist, tol_x, steps allowance, inner-iteration allowance) of the GPU
    comparison: MARGIN x the run's spread for the values (cg_ref.tolerance's
    rule); for the counts the CPU-measured spread itself, the inner iterations'
    no less than one per step of the reference."""
    s_hist, s_x, d_steps, d_inner = SPREAD[run]
    ref = reference(run)
    return MARGIN * max(s_hist, EPS), MARGIN * max(s_x, EPS), d_steps, max(d_inner, max(ref.steps, 1))
