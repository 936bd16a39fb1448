"""The Chebyshev polynomial preconditioner (rsp_cheby_*, include/rsp.h) restated
in NumPy (CPU only; test infrastructure for test_cheby_ref.py and
test_gpu_cheby.py), by the method of krylov_ref.py, cg_ref.py and refine_ref.py,
whose pieces it imports and never changes.

coefficients() is the host recurrence of rsp.h in fp64, one operation per line
(Python floats: no fused multiply-add). setup() is the set-up kernel: the
diagonal summed in P in storage order, dinv = P(1) / diag, the Gershgorin
quotient with the absolute row sum in fp64 in storage order, their maximum, the
smallest row without a usable diagonal. Poly.apply() is the apply: every product
and sum in arrays of P, the product with A through the oracle's SpMV in the
kernels' canonical order and the epilogue rule of spmv_epilogue_ref.py at
alpha = -1, beta = 1. The device kernels between the SpMVs are element-wise, so
the device's z is this one's bit for bit.

System wraps a matrix and a Poly as the solvers' restatements of refine_ref.py
expect them (matvec, apply), so the same cg_solve / bicgstab_solve /
fgmres_solve / refine run with M^-1 = the polynomial.
"""
import functools

import numpy as np

import cg_ref as cr
import oracle_bind as ob
import refine_ref as rf
import spmv_epilogue_ref as er
from krylov_ref import Csr, Dot

RATIO = 30.0
RTOL = 1e-10
# the grids of test_gpu_cg.py: (nx, ny, cx, cy)
SHAPES = [(40, 40, 0.0, 0.0), (48, 32, 8.0, 0.5), (37, 29, 0.0, 0.0)]
# (shape, polynomial type) -> CG iterations to RTOL at degree 4 and 8, and without a
# preconditioner on 40 x 40: what cg_reference gives (test_cheby_ref.py holds them)
COUNTS = {((40, 40, 0.0, 0.0), "fp64"): (24, 13), ((48, 32, 8.0, 0.5), "fp64"): (34, 19),
          ((37, 29, 0.0, 0.0), "fp64"): (24, 13), ((40, 40, 0.0, 0.0), "fp32"): (29, 17)}
PLAIN_40 = 82


def coefficients(degree, lmin, lmax):
    """(c0, a, b) in fp64: a[j - 1], b[j - 1] belong to term j."""
    theta = (lmax + lmin) / 2.0
    delta = (lmax - lmin) / 2.0
    sigma = theta / delta
    rho = 1.0 / sigma
    c0 = 1.0 / theta
    a, b = [], []
    for _ in range(1, degree):
        rho_j = 1.0 / (2.0 * sigma - rho)
        a.append(rho_j * rho)
        t = 2.0 * rho_j
        b.append(t / delta)
        rho = rho_j
    return c0, np.array(a, np.float64), np.array(b, np.float64)


def setup(rowptr, colidx, values, dtype, jacobi=True):
    """(dinv or None, lmax, bad): the set-up kernel. values are cast to dtype
    first (the matrix the polynomial is built on holds them in P). bad is the
    smallest row whose diagonal is missing, 0 or not finite (-1: none; always
    -1 without scaling); such a row adds nothing to lmax."""
    T = np.dtype(dtype).type
    rp = np.asarray(rowptr, np.int64)
    ci = np.asarray(colidx, np.int64)
    v = np.asarray(values).astype(dtype)
    n = len(rp) - 1
    lens = np.diff(rp)
    diag, has = np.zeros(n, dtype), np.zeros(n, bool)
    absum = np.zeros(n, np.float64)
    av = np.abs(v.astype(np.float64))
    with np.errstate(all="ignore"):
        for p in range(int(lens.max()) if n else 0):  # entry p of every row that has one: storage order
            rows = np.flatnonzero(lens > p)
            k = rp[rows] + p
            absum[rows] = absum[rows] + av[k]
            on = ci[k] == rows
            diag[rows[on]] = diag[rows[on]] + v[k[on]]
            has[rows[on]] = True
        if not jacobi:
            g = absum
            return None, float(np.max(np.where(np.isfinite(g), g, np.inf))) if n else 0.0, -1
        badrow = ~has | (diag == 0) | ~np.isfinite(diag)
        dinv = (T(1) / np.where(badrow, T(1), diag)).astype(dtype)
        g = np.where(badrow, 0.0, absum / np.abs(np.where(badrow, T(1), diag).astype(np.float64)))
        g = np.where(np.isfinite(g), g, np.inf)
    bad = int(np.flatnonzero(badrow)[0]) if badrow.any() else -1
    return dinv, float(np.max(g)), bad


class Poly:
    """rsp_cheby_t on a Csr-like matrix g (rowptr, colidx, values) in type P."""

    def __init__(self, g, dtype, degree, scaling="jacobi", ratio=RATIO, ftz=False):
        self.g, self.dtype, self.degree, self.ftz = g, np.dtype(dtype), int(degree), ftz
        self.vals = np.asarray(g.values).astype(dtype)
        self.dinv, self.lmax, self.bad = setup(g.rowptr, g.colidx, g.values, dtype, scaling == "jacobi")
        self.lmin = self.lmax / ratio

    def set_bounds(self, lmin, lmax):
        self.lmin, self.lmax = float(lmin), float(lmax)

    def rounded(self):
        """The coefficients as the kernels see them: rounded once to P."""
        T = self.dtype.type
        c0, a, b = coefficients(self.degree, self.lmin, self.lmax)
        return T(c0), a.astype(self.dtype), b.astype(self.dtype)

    def apply(self, r):
        T = self.dtype
        r = np.ascontiguousarray(r)
        assert r.dtype == T
        c0, a, b = self.rounded()
        scale = (lambda y: self.dinv * y) if self.dinv is not None else (lambda y: y)
        d = c0 * scale(r)
        z = d.copy()
        w = r.copy()
        for j in range(1, self.degree):
            s = ob.spmv(self.g.rowptr, self.g.colidx, self.vals, d, ftz=self.ftz, order="canon")
            w = er.epilogue(s, w, -1.0, 1.0)
            t = scale(w)
            d = (a[j - 1] * d) + (b[j - 1] * t)
            z = z + d
        assert z.dtype == T
        return z


class System:
    """A matrix and a polynomial on it (of type P, possibly narrower than the
    iteration's) as refine_ref's solvers take their `g`: apply(precond) is the
    polynomial for any precond but None."""

    def __init__(self, g, poly):
        self.g, self.poly, self.n = g, poly, g.n
        self.rowptr, self.colidx, self.values = g.rowptr, g.colidx, g.values

    def matvec(self, x, dtype=np.float64):
        return self.g.matvec(x, dtype)

    def apply(self, precond, ftz=False):
        if precond is None:
            return lambda y: y
        P = self.poly.dtype
        return lambda y: self.poly.apply(y.astype(P)).astype(y.dtype)


@functools.lru_cache(maxsize=None)
def grid(nx, ny, cx=0.0, cy=0.0):
    return cr.SymGrid(nx, ny, cx, cy)


def true_relres(g, b, x):
    return rf.true_relres(g, b, x)


@functools.lru_cache(maxsize=None)
def cg_reference(shape, degree, ptype="fp64", rtol=RTOL, bounds=None, max_iters=1000):
    """CG with the polynomial (degree 0: M = I) on grid(*shape), b = 1, x0 = 0,
    in fp64 with a polynomial of type ptype: (x, iterations, reason). Computed
    once and left unchanged."""
    g = grid(*shape)
    b = np.ones(g.n)
    if degree == 0:
        x, it, reason = rf.cg_solve(g, None, np.float64, b, np.zeros(g.n), rtol, max_iters, Dot("longdouble"))
    else:
        poly = Poly(g, cr.NP[ptype], degree)
        if bounds is not None:
            poly.set_bounds(*bounds)
        x, it, reason = rf.cg_solve(System(g, poly), True, np.float64, b, np.zeros(g.n), rtol, max_iters,
                                    Dot("longdouble"))
    x.setflags(write=False)
    return x, it, reason


@functools.lru_cache(maxsize=None)
def solver_reference(method, degree, rtol=RTOL):
    """BiCGStab / GMRES(30) / refinement (inner CG to 1e-4) with the polynomial
    (degree 0: M = I) on the 40 x 40 grid, b = 1, x0 = 0: (x, iterations)."""
    g = grid(40, 40)
    b, x0 = np.ones(g.n), np.zeros(g.n)
    dot = Dot("longdouble")
    if method == "refine":
        sys_ = System(g, Poly(g, np.float32, degree)) if degree else g
        res = rf.refine(sys_, "cg", 0, np.float32 if degree else None, b, x0, rtol, 20, 1e-4, 1000, dot)
        res.x.setflags(write=False)
        return res.x, res.inner
    sys_ = System(g, Poly(g, np.float64, degree)) if degree else g
    pc = True if degree else None
    if method == "bicgstab":
        x, it, _ = rf.bicgstab_solve(sys_, pc, np.float64, b, x0, rtol, 1000, dot)
    else:
        x, it, _ = rf.fgmres_solve(sys_, pc, np.float64, 30, b, x0, rtol, 1000, dot)
    x.setflags(write=False)
    return x, it


def crafted():
    """A 6 x 6 matrix with duplicate diagonal entries, unsorted rows, an
    off-diagonal duplicate and values whose fp32 sums round: rows of (col, value)."""
    rows = [[(1, -0.3), (0, 1.1), (0, 0.7)],
            [(1, 2.0), (0, -0.3), (2, 0.1), (1, 1e-9)],
            [(5, 0.25), (2, 1.0 / 3.0), (1, 0.1), (2, 2.0 / 3.0), (2, 1.0 / 7.0)],
            [(3, -4.0), (4, 1.5), (4, -1.5)],
            [(3, 1.5), (4, 0.1), (4, 0.2), (4, 0.3)],
            [(5, 5.0), (2, 0.25)]]
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], np.float64)
    return Csr(rp, ci, va)
