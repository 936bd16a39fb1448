"""Trajectory restatement of the preconditioned CG solver (CPU only; test
infrastructure for test_cg_trajectory.py and test_gpu_cg_trajectory.py), by
the method of krylov_ref.py, whose pieces it imports and never changes.

cg_trajectory restates rsp_cg_solve (include/rsp.h) at rtol = 0, max_iters =
K, check_every = 1: exactly K iterations, returning x and the history with the
library's meaning. Every element-wise step is written as krylov.hip's cg_*
kernels write it (the same parenthesisation, scalars rounded to the iteration
type first, no fused multiply-add), the SpMV goes through the oracle in the
kernels' canonical order and ILU(0) and the triangular solves through the
oracle, so what separates the restatement from the device is the order in
which a dot product is summed, and nothing else.

The matrix is the symmetric 5-point grid (SymGrid): diagonal 4 + 2 cx + 2 cy,
west and east -1 - cx, south and north -1 - cy, Dirichlet boundaries, rows
sorted, both triangles stored. It is symmetric, weakly diagonally dominant and
irreducible with strictly dominant boundary rows: positive definite. The
trajectory cases use (cx, cy) = (0, 0) at the sizes of krylov_ref.SIZES.
"""
import functools
import math

import numpy as np

from krylov_ref import (DOTS, EPS, FP64_ORDERS, MARGIN, SEPARATION, SIZES, Csr, Dot, deviation,  # noqa: F401
                        dropped_ranges)

NP = {"fp64": np.float64, "fp32": np.float32, "none": None}


class SymGrid(Csr):
    """The symmetric 5-point grid, built without a Python loop."""

    def __init__(self, nx, ny, cx=0.0, cy=0.0):
        n = nx * ny
        k = np.arange(n, dtype=np.int64)
        i, j = k % nx, k // nx
        cols = np.stack([k - nx, k - 1, k, k + 1, k + nx], axis=1)
        vals = np.broadcast_to(np.array([-1.0 - cy, -1.0 - cx, 4.0 + 2.0 * cx + 2.0 * cy, -1.0 - cx, -1.0 - cy]),
                               (n, 5))
        keep = np.stack([j > 0, i > 0, np.ones(n, bool), i < nx - 1, j < ny - 1], axis=1)
        rowptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
        super().__init__(rowptr, cols[keep], vals[keep])
        self.nx, self.ny = nx, ny

    def dense(self):
        a = np.zeros((self.n, self.n))
        rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))
        a[rows, self.colidx] = self.values
        return a


@functools.lru_cache(maxsize=None)
def grid(label):
    return SymGrid(*SIZES[label])


def cg_trajectory(g, precond, dtype, K, b, x0, dot, watch=None):
    """K iterations of rsp_cg_solve: (x, history), history[i] = ||r|| / ||b||
    of the recurrence residual after iteration i + 1. The dots of an
    iteration, in call order: with M (r,z), (p,q), (r,r); M = I (precond None:
    z is r, and rho' is the (r,r) already there) (p,q), (r,r). Iteration 0 is
    the set-up: (b,b), (r,r). watch(history), called after each entry, ends
    the run early by returning True; x is then None."""
    M = g.apply(precond)
    A = lambda y: g.matvec(y, dtype)
    dot.at(0)
    x = x0.astype(dtype)
    r = b - A(x)
    bn = math.sqrt(dot(b, b))
    rr = dot(r, r)
    rho = 1.0
    p = None
    hist = []
    for it in range(1, K + 1):
        dot.at(it)
        if precond is None:
            z, rho_new = r, rr
        else:
            z = M(r)
            rho_new = dot(r, z)
        assert rho_new > 0.0 and math.isfinite(rho_new)
        if it == 1:
            p = z.copy()
        else:
            beta = rho_new / rho
            p = z + dtype(beta) * p
        rho = rho_new
        q = A(p)
        pq = dot(p, q)
        assert pq > 0.0 and math.isfinite(pq)
        alpha = rho / pq
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        rr = dot(r, r)
        hist.append(math.sqrt(rr) / bn)
        if watch is not None and watch(hist):
            return None, hist
    return x, hist


# ------------------------------------------------------------------ the cases
#
# (size, preconditioner, iteration type, K): the smallest input that exists for
#   S  four workgroups and a 5-element tail (143 x 43 = 3 * 2048 + 5)
#   S fp32 / f32  the all-fp32 iteration
#   T  a 1-element tail (683 x 3 = 2049)
#   L  257 workgroups: the combine loop runs twice for thread 0
#   X  chunk = 4096
CASES = [("S", "fp64", "f64", 6), ("S", "fp32", "f64", 6), ("S", "none", "f64", 6), ("S", "fp32", "f32", 6),
         ("T", "fp64", "f64", 4),
         ("L", "fp64", "f64", 6), ("L", "fp32", "f64", 6), ("L", "none", "f64", 6),
         ("X", "none", "f64", 3)]


def case_id(case):
    size, pc, it, K = case
    return f"cg-K{K}-{size}-{pc}-{it}"


def run_case(case, kind="longdouble", mutate=None, watch=None):
    """(x as fp64, history, the Dot) of one case's restatement."""
    size, pc, it, K = case
    g = grid(size)
    dtype = np.float32 if it == "f32" else np.float64
    b, x0 = g.rhs_and_start(dtype)
    dot = Dot(kind, mutate)
    x, hist = cg_trajectory(g, NP[pc], dtype, K, b, x0, dot, watch)
    return None if x is None else x.astype(np.float64), np.array(hist), dot


@functools.lru_cache(maxsize=None)
def reference(case):
    """The longdouble trajectory of a case: (x, history, dots per iteration)."""
    x, hist, dot = run_case(case)
    x.setflags(write=False)
    hist.setflags(write=False)
    return x, hist, dict(dot.calls)


# ------------------------------------------------------------- the tolerances
#
# SPREAD[case] = (s_hist, s_x): the largest deviation of the three fp64 dot
# orders (krylov_ref.FP64_ORDERS) from the longdouble trajectory of that case,
# measured on the CPU and rounded up to two digits; test_cg_trajectory.py
# recomputes them and holds the table. A spread below one fp64 ulp counts as
# one ulp, the resolution of the comparison. Nothing here comes from a GPU run.
SPREAD = {
    ("S", "fp64", "f64", 6): (7.1e-16, 5.3e-16),
    ("S", "fp32", "f64", 6): (8.5e-16, 7.4e-16),
    ("S", "none", "f64", 6): (4.3e-16, 4.8e-16),
    ("S", "fp32", "f32", 6): (1.3e-16, EPS),
    ("T", "fp64", "f64", 4): (1.6e-15, 3.7e-16),
    ("L", "fp64", "f64", 6): (3.4e-15, 7.1e-16),
    ("L", "fp32", "f64", 6): (1.4e-11, 1.1e-8),
    ("L", "none", "f64", 6): (2.4e-15, 7.6e-16),
    ("X", "none", "f64", 3): (8.1e-16, 7.5e-16),
}


def tolerance(case):
    """(tol_hist, tol_x) of the GPU comparison: MARGIN x the case's spread."""
    s_hist, s_x = SPREAD[case]
    return MARGIN * max(s_hist, EPS), MARGIN * max(s_x, EPS)


def walked_dots(calls):
    """(iteration, k) of every dot of iterations 1-3."""
    return [(it, k) for it in (1, 2, 3) for k in range(calls[it])]
