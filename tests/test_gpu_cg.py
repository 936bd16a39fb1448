"""ILU(0)-preconditioned conjugate gradients (rsp_cg_*, respasol_amd.sparse.CG)
against a numpy restatement of the same algorithm.

Matrices: the symmetric 5-point grid nx x ny (cg_ref.SymGrid: diagonal
4 + 2 cx + 2 cy, west / east -1 - cx, south / north -1 - cy, Dirichlet, both
triangles stored): 40 x 40 (0, 0), 48 x 32 (8, 0.5) and 37 x 29 (0, 0);
b = 1, x0 = 0, rtol = 1e-10 unless a test says otherwise.

Reference (ref_cg): the iteration of include/rsp.h in numpy, M = L U applied
through the oracle's ILU(0) and its lower_n / upper solves (in fp32, FTZ or
not, for the reduced-precision preconditioners), dots by np.dot in fp64. Its
iteration counts with an fp64 / fp32 / no preconditioner, pinned by
test_reference_matches_prototype_counts:

    40 x 40            42 / 45 /  82     cond_2 681
    48 x 32 (8, 0.5)   46 / 50 / 124     cond_2 830
    37 x 29            39 / 43 /  86     cond_2 449

The stopping test is a threshold crossing of the recurrence residual, so the
device's count may differ by one (a condition, not a measurement); everything
else is bounded by rtol itself: the true residual by 2 rtol (the reference
reaches 0.43-0.99 rtol, so the reference alone is inside it), and x by
||x - x*||_2 / ||x*||_2 <= cond_2(A) ||r|| / ||b|| <= cond_2(A) 2 rtol, from
x - x* = A^-1 r with cond_2 computed here from numpy.linalg.eigvalsh of the
dense matrix (the same test asserts A == A^T and lambda_min > 0).

All-fp32 iteration at rtol = 1e-4: the fp32 reference needs 19-20 iterations
and reaches 0.73-0.81 rtol; the device's true residual is held to 2 rtol.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cg_ref as cr
import oracle_bind as ob
from respasol_amd import _lib, csr
from respasol_amd.sparse import CG, Handle, Ilu0, RspError, SpMat, upload_csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
SHAPES = [(40, 40, 0.0, 0.0), (48, 32, 8.0, 0.5), (37, 29, 0.0, 0.0)]
NPT = {"fp64": np.float64, "fp32": np.float32, "none": None}
# ref_cg's iterations to 1e-10: fp64 / fp32 / no preconditioner
COUNTS = {(40, 40, 0.0, 0.0): (42, 45, 82), (48, 32, 8.0, 0.5): (46, 50, 124), (37, 29, 0.0, 0.0): (39, 43, 86)}


class Spd:
    """A grid with what the tests need of it: b = 1, the true residual, the
    dense solve, the spectrum."""

    def __init__(self, nx, ny, cx, cy):
        self.g = cr.SymGrid(nx, ny, cx, cy)
        self.n, self.rowptr, self.colidx, self.values = self.g.n, self.g.rowptr, self.g.colidx, self.g.values
        self.b = np.ones(self.n)

    def matvec(self, x, dtype=np.float64):
        return self.g.matvec(x, dtype)

    def true_relres(self, x):
        r = self.b - self.matvec(np.asarray(x, np.float64))
        return float(np.linalg.norm(r) / np.linalg.norm(self.b))

    @functools.cached_property
    def dense(self):
        return self.g.dense()

    @functools.cached_property
    def x_ref(self):
        return np.linalg.solve(self.dense, self.b)

    @functools.cached_property
    def spectrum(self):
        return np.linalg.eigvalsh(self.dense)


@functools.lru_cache(maxsize=None)
def grid(nx, ny, cx, cy):
    return Spd(nx, ny, cx, cy)


def make_apply(g, precond, ftz=False):
    """z = M^-1 y in the preconditioner's precision (None: M = I)."""
    if precond is None:
        return lambda y: y
    fac, sz, zp = ob.ilu0(g.rowptr, g.colidx, g.values.astype(precond), ftz=ftz)
    assert sz == -1 and zp == -1

    def apply(y):
        z = ob.trsv("lower_n", g.rowptr, g.colidx, fac, y.astype(precond), ftz=ftz)
        return ob.trsv("upper", g.rowptr, g.colidx, fac, z, ftz=ftz).astype(y.dtype)
    return apply


@functools.lru_cache(maxsize=None)
def ref_cg(g, precond, ftz=False, dtype=np.float64, rtol=RTOL, max_iters=1000):
    """The algorithm of the solver in numpy: returns (x, iterations)."""
    M = make_apply(g, precond, ftz)
    A = lambda y: g.matvec(y, dtype)
    d = lambda a, c: float(np.dot(a.astype(np.float64), c.astype(np.float64)))
    b = g.b.astype(dtype)
    x = np.zeros(g.n, dtype)
    r = b - A(x)
    bn = np.sqrt(d(b, b))
    rho, p = 1.0, None
    for it in range(1, max_iters + 1):
        z = M(r)
        rho_new = d(r, z)
        assert rho_new > 0.0
        p = z.copy() if it == 1 else z + dtype(rho_new / rho) * p
        rho = rho_new
        q = A(p)
        pq = d(p, q)
        assert pq > 0.0
        alpha = rho / pq
        x = x + dtype(alpha) * p
        r = r - dtype(alpha) * q
        if np.sqrt(d(r, r)) <= rtol * bn:
            return x, it
    return x, max_iters


class Dev:
    """A matrix on the device: SpMat, analysed + factored ILU(0) (or none), CG."""

    def __init__(self, h, g, precond=np.float64, dtype=torch.float64):
        self.g = g
        rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values, dtype)
        self.A = SpMat(h, rp, ci, va, g.n)
        self.ilu = self.fac = None
        if precond is not None:
            self.ilu = Ilu0(h, rp, ci)
            self.ilu.analysis()
            self.fac = torch.from_numpy(g.values.astype(precond)).cuda()
            self.ilu.factor(self.fac)
        self.solver = CG(h, self.A, self.ilu, self.fac)
        self.b = torch.from_numpy(g.b.astype(np.float64 if dtype == torch.float64 else np.float32)).cuda()

    def close(self):
        self.solver.close()
        if self.ilu is not None:
            self.ilu.close()
        self.A.close()


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


def assert_as_reference(g, res, precond, ftz=False):
    x_r, it_r = ref_cg(g, precond, ftz)
    lam = g.spectrum
    assert np.array_equal(g.dense, g.dense.T) and lam[0] > 0.0
    cond = float(lam[-1] / lam[0])
    x = res.x.cpu().numpy()
    true = g.true_relres(x)
    err = float(np.linalg.norm(x - g.x_ref) / np.linalg.norm(g.x_ref))
    print(f"iters={res.iters} ref={it_r} relres={res.relres:.3e} true={true:.3e} (<= {2 * RTOL:.1e}) "
          f"ref_true={g.true_relres(x_r):.3e} cond={cond:.0f} xerr={err:.3e} (<= {cond * 2 * RTOL:.3e})")
    assert res.reason == CG.CONVERGED
    assert abs(res.iters - it_r) <= 1
    assert res.relres <= RTOL
    assert len(res.history) == res.iters and res.history[-1] == res.relres
    assert true <= 2 * RTOL
    assert err <= cond * 2 * RTOL
    return res.iters


@pytest.mark.parametrize("precond", ["fp64", "fp32", "none"])
@pytest.mark.parametrize("shape", SHAPES)
def test_converges_as_reference(handle, shape, precond):
    g = grid(*shape)
    d = Dev(handle, g, NPT[precond])
    try:
        assert_as_reference(g, d.solver.solve(d.b, rtol=RTOL), NPT[precond])
    finally:
        d.close()


def test_reference_matches_prototype_counts():
    """The numpy restatement gives the iteration counts of the CPU prototype
    the solver was specified from, stays inside the bounds the device is held
    to, and FTZ changes no count (no GPU needed)."""
    for shape in SHAPES:
        g = grid(*shape)
        got = []
        for precond in (np.float64, np.float32, None):
            x, it = ref_cg(g, precond)
            got.append(it)
            true = g.true_relres(x)
            err = float(np.max(np.abs(x - g.x_ref)) / np.max(np.abs(g.x_ref)))
            print(f"{shape} {precond}: {it} iterations, true residual {true / RTOL:.2f} rtol, max-norm x error {err:.1e}")
            assert 0.4 * RTOL <= true <= RTOL
            assert err <= 6.7e-12
        assert tuple(got) == COUNTS[shape]
        assert ref_cg(g, np.float32, True)[1] == COUNTS[shape][1]
    cond = [round(float(grid(*s).spectrum[-1] / grid(*s).spectrum[0])) for s in SHAPES]
    assert cond == [681, 830, 449]


def test_fp32_ftz_preconditioner():
    g = grid(40, 40, 0.0, 0.0)
    h = Handle(ftz=True)
    d = Dev(h, g, np.float32)
    try:
        assert_as_reference(g, d.solver.solve(d.b, rtol=RTOL), np.float32, ftz=True)
    finally:
        d.close()
        h.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_all_fp32_iteration(handle, shape):
    g = grid(*shape)
    rtol = 1e-4
    x_r, it_r = ref_cg(g, np.float32, False, np.float32, rtol)
    ref_true = g.true_relres(x_r)
    assert 19 <= it_r <= 20 and 0.7 * rtol <= ref_true <= 0.85 * rtol  # the fp32 reference itself
    d = Dev(handle, g, np.float32, torch.float32)
    try:
        res = d.solver.solve(d.b, rtol=rtol)
        true = g.true_relres(res.x.cpu().numpy())
        print(f"iters={res.iters} ref={it_r} relres={res.relres:.3e} true={true:.3e} ref_true={ref_true:.3e}")
        assert res.x.dtype == torch.float32
        assert res.reason == CG.CONVERGED
        assert true <= 2 * rtol
    finally:
        d.close()


def small(h, rows, precond):
    """A tiny matrix given as rows of (col, value)."""
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], np.float64)
    g = type("G", (), {"rowptr": rp, "colidx": ci, "values": va, "n": len(rows), "b": np.ones(len(rows))})
    return Dev(h, g, precond)


def test_edge_n1(handle):
    for precond in (None, np.float64, np.float32):
        d = small(handle, [[(0, 2.0)]], precond)
        try:
            res = d.solver.solve(d.b)
            assert res.reason == CG.CONVERGED and res.iters == 1
            assert res.x.cpu().numpy().tolist() == [0.5]
        finally:
            d.close()


def test_edge_identity_from_loader(handle):
    m = csr.load_matrix_market(os.path.join(ROOT, "tests", "golden", "mtx", "one.mtx"))
    assert m.m == m.n == 7
    g = type("G", (), {"rowptr": m.rowptr, "colidx": m.colidx, "values": m.values, "n": m.n})
    b = np.arange(1.0, 8.0) / 3.0
    g.b = b
    for check_every in (1, 4):  # r == 0 exactly: seen at the first check, 1 iteration either way
        d = Dev(handle, g, None)
        try:
            res = d.solver.solve(d.b, rtol=0.0, max_iters=8, check_every=check_every)
            assert res.reason == CG.CONVERGED and res.iters == 1 and res.relres == 0.0
            assert np.array_equal(res.x.cpu().numpy(), b)
        finally:
            d.close()


def test_zero_pivot_from_create(handle):
    """[[1, 1], [1, 1]]: u_22 = 1 - 1 * 1 = 0."""
    rp, ci, va = upload_csr(np.array([0, 2, 4]), np.array([0, 1, 0, 1]), np.ones(4))
    A = SpMat(handle, rp, ci, va, 2)
    ilu = Ilu0(handle, rp, ci)
    try:
        ilu.analysis()
        fac = va.clone()
        ilu.factor(fac)
        with pytest.raises(RspError) as e:
            CG(handle, A, ilu, fac)
        assert e.value.status == _lib.STATUS_ZERO_PIVOT
    finally:
        ilu.close()
        A.close()


def test_argument_checks(handle):
    """One assertion per clause of rsp_cg_create / solve / history / destroy
    in include/rsp.h (the clauses are rsp_bicgstab_*'s)."""
    g, g2 = grid(37, 29, 0.0, 0.0), grid(40, 40, 0.0, 0.0)
    rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values)
    _, _, va32 = upload_csr(g.rowptr, g.colidx, g.values, torch.float32)
    rp2, ci2, _ = upload_csr(g2.rowptr, g2.colidx, g2.values)
    INVALID = _lib.STATUS_INVALID_VALUE
    rsp = _lib.rsp
    vp = lambda t: C.c_void_p(t.data_ptr())

    def status(fn):
        with pytest.raises(RspError) as e:
            fn()
        return e.value.status

    ilu, other = Ilu0(handle, rp, ci), Ilu0(handle, rp2, ci2)
    A = SpMat(handle, rp, ci, va, g.n)
    A32 = SpMat(handle, rp, ci, va32, g.n)
    wide = SpMat(handle, rp, ci, va, g.n + 1)
    try:
        # ---- create
        assert status(lambda: CG(handle, A, ilu, va.clone())) == INVALID  # an info that was never analysed
        ilu.analysis()
        other.analysis()
        fac = va.clone()
        ilu.factor(fac)
        out = C.c_void_p()
        create = lambda h, mat, info, pt, f, o: rsp.rsp_cg_create(h, mat, info, pt, f, o)
        assert create(None, A._mat, ilu._info, _lib.R_64F, vp(fac), C.byref(out)) == _lib.STATUS_NOT_INITIALIZED
        assert create(handle.ptr, A._mat, ilu._info, _lib.R_64F, vp(fac), None) == INVALID  # no place for the solver
        assert create(handle.ptr, None, ilu._info, _lib.R_64F, vp(fac), C.byref(out)) == INVALID  # no matrix
        assert create(handle.ptr, A._mat, ilu._info, _lib.R_64F, None, C.byref(out)) == INVALID  # no factor
        assert create(handle.ptr, A._mat, ilu._info, 99, vp(fac), C.byref(out)) == INVALID  # no such type
        assert not out.value
        assert status(lambda: CG(handle, wide, ilu, fac)) == INVALID  # a non-square A
        assert status(lambda: CG(handle, A, other, fac)) == INVALID  # info's n != rows
        assert status(lambda: CG(handle, A32, ilu, fac)) == INVALID  # fp64 preconditioner, fp32 iteration
        # M = I: precond_type and d_factor are ignored
        assert create(handle.ptr, A._mat, None, 99, None, C.byref(out)) == _lib.STATUS_SUCCESS and out.value
        assert rsp.rsp_cg_destroy(out) == _lib.STATUS_SUCCESS
        # ---- solve
        s = CG(handle, A, ilu, fac)
        b = torch.ones(g.n, dtype=torch.float64, device="cuda")
        x = torch.zeros_like(b)
        assert status(lambda: s.solve(b, check_every=0)) == INVALID
        assert status(lambda: s.solve(b, max_iters=-1)) == INVALID
        assert status(lambda: s.solve(b, rtol=-1e-3)) == INVALID
        assert status(lambda: s.solve(b, rtol=float("nan"))) == INVALID
        it, reason, rel = C.c_int(), C.c_int(), C.c_double()
        good = [handle.ptr, s._s, vp(b), vp(x), 1e-10, 10, 1, C.byref(it), C.byref(rel), C.byref(reason)]
        for k in (1, 2, 3, 7, 8, 9):  # each pointer in turn
            args = list(good)
            args[k] = None
            assert rsp.rsp_cg_solve(*args) == INVALID, k
        args = list(good)
        args[0] = None
        assert rsp.rsp_cg_solve(*args) == _lib.STATUS_NOT_INITIALIZED
        assert torch.count_nonzero(x).item() == 0  # none of them touched x
        assert rsp.rsp_cg_solve(*good) == _lib.STATUS_SUCCESS and it.value == 10 and reason.value == CG.MAX_ITERS
        # ---- history
        count, buf = C.c_int(), (C.c_double * 16)()
        assert rsp.rsp_cg_history(None, 16, buf, C.byref(count)) == INVALID
        assert rsp.rsp_cg_history(s._s, 16, buf, None) == INVALID
        assert rsp.rsp_cg_history(s._s, -1, buf, C.byref(count)) == INVALID
        assert rsp.rsp_cg_history(s._s, 4, None, C.byref(count)) == INVALID
        assert rsp.rsp_cg_history(s._s, 0, None, C.byref(count)) == _lib.STATUS_SUCCESS and count.value == 10
        assert rsp.rsp_cg_history(s._s, 4, buf, C.byref(count)) == _lib.STATUS_SUCCESS and count.value == 10
        assert buf[3] > 0.0 and buf[4] == 0.0 and buf[9] == 0.0  # only the first min(cap, count)
        assert rsp.rsp_cg_history(s._s, 16, buf, C.byref(count)) == _lib.STATUS_SUCCESS and buf[9] == rel.value
        s.close()
        # ---- destroy
        assert rsp.rsp_cg_destroy(None) == INVALID
    finally:
        for o in (ilu, other, A, A32, wide):
            o.close()


@pytest.mark.parametrize("precond", ["fp64", "fp32", "none"])
def test_driver(handle, tmp_path, precond):
    """A symmetric .mtx (lower triangle, symmetric banner): test_solve
    --method=cg loads both triangles and reports CG.solve's iteration count."""
    g = grid(40, 40, 0.0, 0.0)
    d = Dev(handle, g, NPT[precond])
    try:
        want = d.solver.solve(d.b, rtol=RTOL)  # what test_converges_as_reference checks
    finally:
        d.close()
    assert want.reason == CG.CONVERGED
    path = tmp_path / "grid.mtx"
    lower = [(i, g.colidx[k], g.values[k]) for i in range(g.n) for k in range(g.rowptr[i], g.rowptr[i + 1])
             if g.colidx[k] <= i]
    assert 2 * len(lower) - g.n == len(g.colidx)
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real symmetric\n")
        f.write(f"{g.n} {g.n} {len(lower)}\n")
        for i, j, v in lower:
            f.write(f"{i + 1} {j + 1} {float(v)!r}\n")
    r = subprocess.run([os.path.join(_lib.BIN_DIR, "test_solve"), str(path), "--method=cg", f"--precond={precond}"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = {}
    for key in ("Symbolic", "Numeric", "Solve", "Iterations", "Reason", "Relative residual"):
        m = re.search(rf"^\s*{key} = (\S+)\s*$", r.stdout, re.M)
        assert m, (key, r.stdout)
        got[key] = float(m.group(1))
    assert got["Reason"] == 0
    assert got["Relative residual"] <= 2e-10
    assert got["Iterations"] == want.iters
