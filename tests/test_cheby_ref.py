"""The restatement of the Chebyshev polynomial preconditioner (cheby_ref.py)
checked on the CPU: it is the polynomial include/rsp.h names, its coefficients
are the library's bit for bit, and the solvers' restatements that run on it
give the iteration counts the GPU tests are held to and stay inside the
residual bounds those tests use. No GPU is needed.

Counts (ratio 30, rtol 1e-10, b = 1, x0 = 0, CG): a dense NumPy prototype gave
82 unpreconditioned on 40 x 40 and, at degree 4 / 8, 24 / 13 on 40 x 40,
34 / 19 on 48 x 32 (cx = 8, cy = 0.5), 24 / 13 on 37 x 29 and 29 / 18 on
40 x 40 with an fp32 polynomial under the fp64 iteration. The restatement here
is the authority for the pinned values: it gives every one of them but the
last, 17 where the prototype (dense products, another summation order in the
fp32 polynomial) needed 18; the stop is a threshold crossing, and at 17 the
restatement's true residual is 0.22 rtol.
"""
import math

import numpy as np
import pytest
from numpy.polynomial import chebyshev

import cheby_ref as cb
import refine_ref as rf
from respasol_amd import _lib
from respasol_amd.sparse import cheby_coefficients

EPS = 2.0 ** -53
COUNTS, PLAIN_40 = cb.COUNTS, cb.PLAIN_40


@pytest.mark.parametrize("scaling", ["none", "jacobi"])
@pytest.mark.parametrize("degree", [1, 2, 3, 8, 16])
def test_polynomial_is_the_chebyshev_residual_polynomial(degree, scaling):
    """z = p_k(B) D^-1 r with B = D^-1 A and p_k(x) = (1 - T_k((theta - x) /
    delta) / T_k(sigma)) / x, evaluated through eigh on a small SPD grid with a
    constant diagonal (B is then symmetric). Tolerance: the k recurrence steps
    and the eigen-decomposition each err by a few n eps ||B||, and 1 / x
    amplifies by 1 / lambda_min: 100 k cond_2(B) eps, relative to ||z||."""
    g = cb.cr.SymGrid(7, 5, 0.5, 0.25)
    poly = cb.Poly(g, np.float64, degree, scaling)
    dscale = 1.0 if scaling == "none" else 1.0 / g.dense()[0, 0]
    assert np.all(np.diag(g.dense()) == g.dense()[0, 0])
    B = g.dense() * dscale
    lam, V = np.linalg.eigh(B)
    assert lam[0] > 0.0 and lam[-1] <= poly.lmax
    theta, delta = (poly.lmax + poly.lmin) / 2.0, (poly.lmax - poly.lmin) / 2.0
    ek = np.zeros(degree + 1)
    ek[degree] = 1.0
    p = (1.0 - chebyshev.chebval((theta - lam) / delta, ek) / chebyshev.chebval(theta / delta, ek)) / lam
    rng = np.random.default_rng(3)
    r = rng.uniform(-1.0, 1.0, g.n)
    want = V @ (p * (V.T @ (dscale * r)))
    got = poly.apply(r)
    tol = 100.0 * degree * (lam[-1] / lam[0]) * 2.0 * EPS
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"degree {degree} {scaling}: off by {err:.2e} (tolerance {tol:.2e})")
    assert err <= tol
    assert np.all(p > 0.0)  # positive on the whole spectrum: M is positive definite


@pytest.mark.parametrize("degree", [1, 2, 5, 8, 64])
@pytest.mark.parametrize("bounds", [(0.05, 1.5), (1.0 / 15.0, 2.0), (1e-3, 7.25), (0.5, 1.5)])
def test_library_coefficients_are_the_restatements(degree, bounds):
    c0, a, b = cheby_coefficients(degree, *bounds)
    r0, ra, rb = cb.coefficients(degree, *bounds)
    assert np.float64(c0).tobytes() == np.float64(r0).tobytes()
    assert a.tobytes() == ra.tobytes() and b.tobytes() == rb.tobytes()
    assert len(a) == len(b) == degree - 1


def test_coefficient_argument_checks():
    import ctypes as C
    fn = _lib.rsp.rsp_cheby_coefficients_host
    c0, a, b = C.c_double(), (C.c_double * 64)(), (C.c_double * 64)()
    INVALID = _lib.STATUS_INVALID_VALUE
    assert fn(0, 0.1, 1.0, C.byref(c0), a, b) == INVALID
    assert fn(_lib.CHEBY_MAX_DEGREE + 1, 0.1, 1.0, C.byref(c0), a, b) == INVALID
    for lo, hi in ((0.0, 1.0), (-1.0, 1.0), (1.0, 1.0), (2.0, 1.0), (0.1, math.inf), (math.nan, 1.0)):
        assert fn(2, lo, hi, C.byref(c0), a, b) == INVALID
    assert fn(2, 0.1, 1.0, None, a, b) == INVALID
    assert fn(2, 0.1, 1.0, C.byref(c0), None, b) == INVALID
    assert fn(2, 0.1, 1.0, C.byref(c0), a, None) == INVALID
    assert fn(1, 0.1, 1.0, C.byref(c0), None, None) == _lib.STATUS_SUCCESS and c0.value == 1.0 / 0.55


def test_setup_restatement_on_the_crafted_matrix():
    """Duplicates and unsorted rows: the diagonal is the storage-order sum in P."""
    g = cb.crafted()
    f32 = np.float32
    dinv, lmax, bad = cb.setup(g.rowptr, g.colidx, g.values, np.float64)
    assert bad == -1
    assert dinv[0] == 1.0 / (1.1 + 0.7) and dinv[3] == -0.25
    assert dinv[2] == 1.0 / ((1.0 / 3.0 + 2.0 / 3.0) + 1.0 / 7.0)
    assert lmax == max((0.3 + 1.1 + 0.7) / (1.1 + 0.7), (4.0 + 1.5 + 1.5) / 4.0,
                       (((1.5 + 0.1) + 0.2) + 0.3) / ((0.1 + 0.2) + 0.3))
    d32, l32, _ = cb.setup(g.rowptr, g.colidx, g.values, f32)
    assert d32.dtype == f32 and d32[1] == f32(0.5)  # 2 + 1e-9 rounds to 2 in fp32
    assert d32[4] == f32(1) / ((f32(0.1) + f32(0.2)) + f32(0.3))
    assert l32 != lmax
    none, lnone, bad = cb.setup(g.rowptr, g.colidx, g.values, np.float64, jacobi=False)
    assert none is None and bad == -1 and lnone == 4.0 + 1.5 + 1.5


@pytest.mark.parametrize("key", list(COUNTS), ids=lambda k: f"{k[0][0]}x{k[0][1]}-{k[1]}")
def test_cg_counts_and_bounds(key):
    shape, ptype = key
    g = cb.grid(*shape)
    b = np.ones(g.n)
    got = []
    for degree in (4, 8):
        x, it, reason = cb.cg_reference(shape, degree, ptype)
        true = cb.true_relres(g, b, x)
        print(f"{shape} {ptype} degree {degree}: {it} iterations, true residual {true / cb.RTOL:.2f} rtol")
        assert reason == rf.CONVERGED
        assert true <= cb.RTOL  # the reference alone is inside the GPU tests' 2 rtol
        got.append(it)
    assert tuple(got) == COUNTS[key]


def test_unpreconditioned_count():
    assert cb.cg_reference((40, 40, 0.0, 0.0), 0)[1] == PLAIN_40


def test_wrong_bounds_break_down():
    """lmax far below the spectrum's top: p_k changes sign on it, M is
    indefinite and CG's (r,z) test reports it. The prototype broke at
    iteration 2 (one iteration completed)."""
    x, it, reason = cb.cg_reference((40, 40, 0.0, 0.0), 4, "fp64", bounds=(0.05, 0.5))
    assert reason == rf.BREAKDOWN and it == 1
    assert np.all(np.isfinite(x))


@pytest.mark.parametrize("method", ["bicgstab", "gmres", "refine"])
def test_other_solvers_references(method):
    """BiCGStab, GMRES(30) and refinement on the polynomial (degree 4): inside
    the residual bounds test_gpu_solver.py / test_gpu_gmres.py (2 rtol) and
    test_gpu_refine.py (rtol ||b|| + the recomputation's rounding bound) use,
    in no more iterations than without a preconditioner."""
    g = cb.grid(40, 40)
    b = np.ones(g.n)
    rtol = 1e-12 if method == "refine" else cb.RTOL
    x, it = cb.solver_reference(method, 4, rtol)
    _, plain = cb.solver_reference(method, 0, rtol)
    true = cb.true_relres(g, b, x)
    print(f"{method}: {it} iterations (unpreconditioned {plain}), true residual {true / rtol:.2f} rtol")
    assert it <= plain
    assert true <= rtol
