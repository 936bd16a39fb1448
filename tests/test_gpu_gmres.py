"""Restarted flexible GMRES(m) (rsp_gmres_*, respasol_amd.sparse.GMRES) against
a numpy restatement of the same algorithm.

Matrices: the 5-point convection-diffusion grids of test_gpu_solver.py (nx x
ny, diagonal 4 + cx + cy, west -1 - cx, east -1, south -1 - cy, north -1);
b = 1, x0 = 0, rtol = 1e-10 unless a test says otherwise.

Reference (ref_fgmres): the algorithm of include/rsp.h — classical
Gram-Schmidt twice in fp64 with w rounded to the iteration type after each
pass, Givens rotations, x += Z y — with M = L U applied through the oracle's
ILU(0) and its lower_n / upper solves in the preconditioner's type, dots by
numpy in fp64, and the solver's stopping rule at check_every = 1: est <= rtol
after a column, or the recomputed residual at a cycle's end. The stop is a
threshold crossing, so counts may differ by one between summation orders;
the true residual is bounded by 2 rtol (the reference reaches at most 0.98
rtol on these systems) and x by the existing tests' 1e-8 against a dense
solve.

All-fp32 iteration (test_all_fp32_iteration): the fp32 restatement reaches a
true residual of 3.2e-5 on (48, 32, 8, 0.5) at rtol = 1e-4 (10 iterations),
inside 2 rtol, so rtol stays at the 1e-4 first proposed.
"""
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import oracle_bind as ob
from respasol_amd import _lib, csr
from respasol_amd.sparse import GMRES, Handle, Ilu0, RspError, SpMat, upload_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10
gpu = pytest.mark.gpu


class Grid:
    def __init__(self, nx, ny, cx, cy):
        n = nx * ny
        rp, ci, va = [0], [], []
        for j in range(ny):
            for i in range(nx):
                k = j * nx + i
                if j > 0:
                    ci.append(k - nx), va.append(-1.0 - cy)
                if i > 0:
                    ci.append(k - 1), va.append(-1.0 - cx)
                ci.append(k), va.append(4.0 + cx + cy)
                if i < nx - 1:
                    ci.append(k + 1), va.append(-1.0)
                if j < ny - 1:
                    ci.append(k + nx), va.append(-1.0)
                rp.append(len(ci))
        self.n = n
        self.rowptr = np.array(rp, np.int32)
        self.colidx = np.array(ci, np.int32)
        self.values = np.array(va, np.float64)
        self.b = np.ones(n)

    def matvec(self, x, dtype=np.float64):
        return ob.spmv(self.rowptr, self.colidx, self.values.astype(dtype), x.astype(dtype))

    def true_relres(self, x):
        r = self.b - self.matvec(np.asarray(x, np.float64))
        return float(np.linalg.norm(r) / np.linalg.norm(self.b))

    @functools.cached_property
    def dense(self):
        A = np.zeros((self.n, self.n))
        for i in range(self.n):
            s, e = self.rowptr[i], self.rowptr[i + 1]
            A[i, self.colidx[s:e]] = self.values[s:e]
        return A

    @functools.cached_property
    def x_ref(self):
        return np.linalg.solve(self.dense, self.b)


@functools.lru_cache(maxsize=None)
def grid(nx, ny, cx, cy):
    return Grid(nx, ny, cx, cy)


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


def rotate_column(col, j, cs, sn, gv):
    """rsp::gmres_lsq's column step; False: the rotated diagonal is 0."""
    for i in range(j):
        a, b = col[i], col[i + 1]
        col[i], col[i + 1] = cs[i] * a + sn[i] * b, cs[i] * b - sn[i] * a
    a, b = col[j], col[j + 1]
    s = max(abs(a), abs(b))
    if s == 0.0 or not math.isfinite(s):
        return False
    r = s * math.sqrt((a / s) ** 2 + (b / s) ** 2)
    cs[j], sn[j] = a / r, b / r
    col[j], col[j + 1] = r, 0.0
    gv[j], gv[j + 1] = cs[j] * gv[j], -(sn[j] * gv[j])
    return True


@functools.lru_cache(maxsize=None)
def ref_fgmres(g, precond, restart, ftz=False, dtype=np.float64, rtol=RTOL, max_iters=2000):
    """The algorithm of the solver in numpy: returns (x, iterations)."""
    M = make_apply(g, precond, ftz)
    A = lambda y: g.matvec(y, dtype)
    f8 = lambda a: a.astype(np.float64)
    m = restart
    b = g.b.astype(dtype)
    x = np.zeros(g.n, dtype)
    bn = math.sqrt(float(np.dot(f8(b), f8(b))))
    total = 0
    while True:
        r = b - A(x)
        beta = math.sqrt(float(np.dot(f8(r), f8(r))))
        if beta <= rtol * bn or total >= max_iters:
            return x, total
        V = [(f8(r) / beta).astype(dtype)]
        Z, R = [], np.zeros((m + 1, m))
        cs, sn, gv = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        gv[0] = beta
        k, by_est = 0, False
        for j in range(m):
            if total + j >= max_iters:
                break
            Z.append(M(V[j]))
            w = A(Z[j])
            Vd = f8(np.array(V))
            h = np.zeros(j + 1)
            for _ in range(2):
                hp = Vd @ f8(w)
                w = (f8(w) - hp @ Vd).astype(dtype)
                h += hp
            hn = math.sqrt(float(np.dot(f8(w), f8(w))))
            col = np.append(h, hn)
            if not rotate_column(col, j, cs, sn, gv):
                break
            R[:j + 2, j] = col
            k = j + 1
            if hn == 0.0:
                break
            V.append((f8(w) / hn).astype(dtype))
            if k < m and total + k < max_iters and abs(gv[k]) / bn <= rtol:
                by_est = True
                break
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            y[i] = (gv[i] - R[i, i + 1:k] @ y[i + 1:]) / R[i, i]
        x = (f8(x) + y @ f8(np.array(Z[:k]))).astype(dtype) if k else x
        total += k
        if by_est or k == 0:
            return x, total


class Dev:
    """A grid on the device: SpMat, analysed + factored ILU(0) (or none), GMRES."""

    def __init__(self, h, g, precond=np.float64, dtype=torch.float64, restart=30):
        self.g = g
        rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values, dtype)
        self.A = SpMat(h, rp, ci, va, g.n)
        self.ilu = self.fac = None
        if precond is not None:
            self.ilu = Ilu0(h, rp, ci)
            self.ilu.analysis()
            self.fac = torch.from_numpy(g.values.astype(precond)).cuda()
            self.ilu.factor(self.fac)
        self.solver = GMRES(h, self.A, self.ilu, self.fac, restart=restart)
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


def assert_as_reference(g, res, precond, restart, ftz=False):
    x_r, it_r = ref_fgmres(g, precond, restart, ftz)
    x = res.x.cpu().numpy()
    true = g.true_relres(x)
    err = float(np.max(np.abs(x - g.x_ref)) / np.max(np.abs(g.x_ref)))
    print(f"iters={res.iters} ref={it_r} relres={res.relres:.3e} true={true:.3e} "
          f"ref_true={g.true_relres(x_r):.3e} xerr={err:.3e} checks={len(res.history)}")
    assert res.reason == GMRES.CONVERGED
    assert abs(res.iters - it_r) <= 1
    assert res.relres <= RTOL
    assert res.history[-1] == res.relres
    # one check per iteration; a cycle that ends with the restart is one check
    assert len(res.history) == res.iters
    assert true <= 2 * RTOL
    assert err <= 1e-8


SHAPES = [(40, 40, 2.0, 1.0), (48, 32, 8.0, 0.5), (37, 29, 2.0, 1.0)]
CASES = [(s, p, m) for s in SHAPES for p in (np.float64, np.float32) for m in (30, 5)]
CASES += [((40, 40, 2.0, 1.0), None, 5), ((50, 41, 2.0, 1.0), np.float32, 30)]
# what ref_fgmres gives (the CPU prototype the solver was specified from: 25 /
# 18 / 23 at m = 30 with either preconditioner type, 40 / 29 / 38 at m = 5,
# 120 / 100 / 115 without a preconditioner at m = 5)
PINNED = {(SHAPES[0], "ilu", 30): 25, (SHAPES[1], "ilu", 30): 18, (SHAPES[2], "ilu", 30): 23,
          (SHAPES[0], "ilu", 5): 40, (SHAPES[1], "ilu", 5): 29, (SHAPES[2], "ilu", 5): 38,
          (SHAPES[0], None, 5): 120, (SHAPES[1], None, 5): 100, (SHAPES[2], None, 5): 115}


@gpu
@pytest.mark.parametrize("shape,precond,restart", CASES)
def test_converges_as_reference(handle, shape, precond, restart):
    g = grid(*shape)
    d = Dev(handle, g, precond, restart=restart)
    try:
        assert_as_reference(g, d.solver.solve(d.b, rtol=RTOL), precond, restart)
    finally:
        d.close()


@pytest.mark.parametrize("key", sorted(PINNED, key=str))
def test_reference_counts_are_pinned(key):
    shape, kind, restart = key
    g = grid(*shape)
    for precond in ((np.float64, np.float32) if kind else (None,)):
        x, it = ref_fgmres(g, precond, restart)
        true = g.true_relres(x)
        print(f"{shape} {precond} m={restart}: {it} iterations, true residual {true:.3e}")
        assert it == PINNED[key]
        assert true <= RTOL


@gpu
def test_fp32_ftz_preconditioner():
    g = grid(40, 40, 2.0, 1.0)
    h = Handle(ftz=True)
    d = Dev(h, g, np.float32)
    try:
        assert_as_reference(g, d.solver.solve(d.b, rtol=RTOL), np.float32, 30, ftz=True)
    finally:
        d.close()
        h.close()


def test_fp32_reference_meets_its_bound():
    g = grid(48, 32, 8.0, 0.5)
    x_r, it_r = ref_fgmres(g, np.float32, 30, False, np.float32, 1e-4)
    print(f"fp32 restatement: {it_r} iterations, true residual {g.true_relres(x_r):.3e}")
    assert g.true_relres(x_r) <= 2e-4


@gpu
def test_all_fp32_iteration(handle):
    g = grid(48, 32, 8.0, 0.5)
    rtol = 1e-4
    x_r, it_r = ref_fgmres(g, np.float32, 30, False, np.float32, rtol)
    d = Dev(handle, g, np.float32, torch.float32)
    try:
        res = d.solver.solve(d.b, rtol=rtol)
        true = g.true_relres(res.x.cpu().numpy())
        print(f"iters={res.iters} ref={it_r} relres={res.relres:.3e} true={true:.3e}")
        assert res.x.dtype == torch.float32
        assert res.reason == GMRES.CONVERGED
        assert abs(res.iters - it_r) <= 1
        assert true <= 2 * rtol
    finally:
        d.close()


@gpu
def test_solves_the_bicgstab_breakdown_case(handle):
    """A = [[0, 1], [-1, 0]], b = (1, 0): BiCGStab gives up in iteration 1
    ((rhat, v) = 0); GMRES solves it in two, x = (0, 1) exactly."""
    rp, ci, va = upload_csr(np.array([0, 1, 2]), np.array([1, 0]), np.array([1.0, -1.0]))
    A = SpMat(handle, rp, ci, va, 2)
    s = GMRES(handle, A)
    try:
        b = torch.tensor([1.0, 0.0], dtype=torch.float64, device="cuda")
        res = s.solve(b)
        assert res.reason == GMRES.CONVERGED and res.iters == 2
        assert res.x.cpu().numpy().tolist() == [0.0, 1.0]
        res = s.solve(b, x0=torch.tensor([0.25, -3.0], dtype=torch.float64, device="cuda"))
        x = res.x.cpu().numpy()
        assert res.reason == GMRES.CONVERGED and res.iters == 2
        assert math.hypot(1.0 - x[1], x[0]) <= 1e-14  # b - A x = (1 - x_1, x_0), ||b|| = 1
    finally:
        s.close()
        A.close()


def small(h, rows, precond, b=None, **kw):
    """A tiny matrix given as rows of (col, value)."""
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], np.float64)
    g = type("G", (), {"rowptr": rp, "colidx": ci, "values": va, "n": len(rows),
                       "b": np.ones(len(rows)) if b is None else np.asarray(b, np.float64)})
    return Dev(h, g, precond, **kw)


@gpu
def test_breakdown_reported_not_propagated(handle):
    """A 1 x 1 matrix with a stored 0: the first rotated diagonal is 0."""
    d = small(handle, [[(0, 0.0)]], None)
    try:
        for x0 in (None, torch.tensor([0.75], dtype=torch.float64, device="cuda")):
            res = d.solver.solve(d.b, x0=x0)
            assert res.reason == GMRES.BREAKDOWN and res.iters == 0
            assert torch.isfinite(res.x).all() and math.isfinite(res.relres)
            assert torch.equal(res.x, torch.zeros_like(d.b) if x0 is None else x0)
    finally:
        d.close()


@gpu
def test_breakdown_non_finite_rhs(handle):
    g = grid(37, 29, 2.0, 1.0)
    d = Dev(handle, g, np.float64)
    try:
        b = d.b.clone()
        b[5] = float("inf")
        res = d.solver.solve(b)
        assert res.reason == GMRES.BREAKDOWN and res.iters == 0
        assert torch.count_nonzero(res.x).item() == 0
    finally:
        d.close()


@gpu
def test_edges_zero_rhs_and_exact_start(handle):
    g = grid(37, 29, 2.0, 1.0)
    d = Dev(handle, g, np.float64)
    try:
        x0 = torch.from_numpy(g.x_ref).cuda()
        res = d.solver.solve(torch.zeros_like(d.b), x0=x0)
        assert res.reason == GMRES.CONVERGED and res.iters == 0
        assert torch.count_nonzero(res.x).item() == 0
        res = d.solver.solve(d.b, x0=x0, rtol=RTOL)  # x_ref's residual is ~1e-16 ||b||
        assert res.reason == GMRES.CONVERGED and res.iters == 0
        assert torch.equal(res.x, x0)
    finally:
        d.close()


@gpu
def test_edge_n1(handle):
    for precond in (None, np.float64):
        d = small(handle, [[(0, 2.0)]], precond)
        try:
            res = d.solver.solve(d.b)
            assert res.reason == GMRES.CONVERGED and res.iters == 1
            assert res.x.cpu().numpy().tolist() == [0.5]
        finally:
            d.close()


@gpu
def test_edge_identity_from_loader(handle):
    m = csr.load_matrix_market(os.path.join(ROOT, "tests", "golden", "mtx", "one.mtx"))
    assert m.m == m.n == 7
    b = np.arange(1.0, 8.0) / 3.0
    g = type("G", (), {"rowptr": m.rowptr, "colidx": m.colidx, "values": m.values, "n": m.n, "b": b})
    d = Dev(handle, g, None)
    try:
        res = d.solver.solve(d.b)
        assert res.reason == GMRES.CONVERGED and res.iters == 1
        assert np.array_equal(res.x.cpu().numpy(), b)
    finally:
        d.close()


@gpu
@pytest.mark.parametrize("restart,limit", [(1, 2000), (64, 100)])
def test_edge_restart_lengths(handle, restart, limit):
    g = grid(37, 29, 2.0, 1.0)
    d = Dev(handle, g, np.float64, restart=restart)
    try:
        res = d.solver.solve(d.b, rtol=RTOL, max_iters=limit)
        true = g.true_relres(res.x.cpu().numpy())
        print(f"restart={restart}: iters={res.iters} relres={res.relres:.3e} true={true:.3e}")
        assert res.reason == GMRES.CONVERGED and res.iters <= limit
        assert true <= 2 * RTOL
        if restart == 64:
            assert abs(res.iters - ref_fgmres(g, np.float64, 64)[1]) <= 1
    finally:
        d.close()


@gpu
def test_determinism(handle):
    g = grid(40, 40, 2.0, 1.0)
    d1, d2 = Dev(handle, g, np.float32, restart=5), Dev(handle, g, np.float32, restart=5)
    try:
        a = d1.solver.solve(d1.b, rtol=RTOL)
        b = d1.solver.solve(d1.b, rtol=RTOL)
        c = d2.solver.solve(d2.b, rtol=RTOL)
        for o in (b, c):
            assert torch.equal(a.x, o.x)
            assert a.iters == o.iters and a.history == o.history and a.relres == o.relres
    finally:
        d1.close()
        d2.close()


@gpu
def test_check_every_changes_no_bit(handle):
    g = grid(40, 40, 2.0, 1.0)
    d = Dev(handle, g, np.float64, restart=30)
    d5 = Dev(handle, g, np.float64, restart=5)
    try:
        out = [d.solver.solve(d.b, rtol=0.0, max_iters=8, check_every=k) for k in (1, 4, 8)]
        for o, checks in zip(out, (8, 2, 1)):
            assert o.reason == GMRES.MAX_ITERS and o.iters == 8
            assert len(o.history) == checks
            assert torch.equal(o.x, out[0].x)
            assert o.relres == out[0].relres
        out = [d5.solver.solve(d5.b, rtol=0.0, max_iters=12, check_every=k) for k in (1, 4)]
        assert out[0].iters == out[1].iters == 12
        assert torch.equal(out[0].x, out[1].x) and out[0].relres == out[1].relres
        # restart 5: cycle ends at 5, 10 and the last iteration, plus the checks between
        assert len(out[0].history) == 12 and len(out[1].history) == 5
    finally:
        d.close()
        d5.close()


@gpu
def test_argument_checks(handle):
    g = grid(37, 29, 2.0, 1.0)
    rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values)
    _, _, va32 = upload_csr(g.rowptr, g.colidx, g.values, torch.float32)

    def status(fn):
        with pytest.raises(RspError) as e:
            fn()
        return e.value.status

    ilu = Ilu0(handle, rp, ci)
    A = SpMat(handle, rp, ci, va, g.n)
    A32 = SpMat(handle, rp, ci, va32, g.n)
    try:
        # an info that was never analysed
        assert status(lambda: GMRES(handle, A, ilu, va.clone())) == _lib.STATUS_INVALID_VALUE
        ilu.analysis()
        fac = va.clone()
        ilu.factor(fac)
        for restart in (0, _lib.GMRES_MAX_RESTART + 1):
            assert status(lambda: GMRES(handle, A, ilu, fac, restart=restart)) == _lib.STATUS_INVALID_VALUE
        # an fp64 preconditioner under an fp32 iteration
        assert status(lambda: GMRES(handle, A32, ilu, fac)) == _lib.STATUS_INVALID_VALUE
        s = GMRES(handle, A, ilu, fac)
        b = torch.ones(g.n, dtype=torch.float64, device="cuda")
        assert status(lambda: s.solve(b, check_every=0)) == _lib.STATUS_INVALID_VALUE
        assert status(lambda: s.solve(b, max_iters=-1)) == _lib.STATUS_INVALID_VALUE
        s.close()
    finally:
        for o in (ilu, A, A32):
            o.close()


@gpu
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
            GMRES(handle, A, ilu, fac)
        assert e.value.status == _lib.STATUS_ZERO_PIVOT
    finally:
        ilu.close()
        A.close()


def run_driver(path, *flags):
    r = subprocess.run([os.path.join(_lib.BIN_DIR, "test_solve"), str(path), *flags],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = {}
    for key in ("Symbolic", "Numeric", "Solve", "Iterations", "Reason", "Relative residual"):
        m = re.search(rf"^\s*{key} = (\S+)\s*$", r.stdout, re.M)
        assert m, (key, r.stdout)
        got[key] = float(m.group(1))
    return got


@pytest.fixture(scope="module")
def grid_file(tmp_path_factory):
    g = grid(40, 40, 2.0, 1.0)
    path = tmp_path_factory.mktemp("gmres") / "grid.mtx"
    with open(path, "w") as f:
        f.write("%%MatrixMarket matrix coordinate real general\n")
        f.write(f"{g.n} {g.n} {len(g.colidx)}\n")
        for i in range(g.n):
            for k in range(g.rowptr[i], g.rowptr[i + 1]):
                f.write(f"{i + 1} {g.colidx[k] + 1} {float(g.values[k])!r}\n")
    return path


@gpu
@pytest.mark.parametrize("precond", ["fp64", "fp32", "none"])
def test_driver(handle, grid_file, precond):
    g = grid(40, 40, 2.0, 1.0)
    npdt = {"fp64": np.float64, "fp32": np.float32, "none": None}[precond]
    d = Dev(handle, g, npdt)
    try:
        want = d.solver.solve(d.b, rtol=RTOL).iters
    finally:
        d.close()
    got = run_driver(grid_file, "--method=gmres", f"--precond={precond}")
    assert got["Reason"] == 0
    assert got["Relative residual"] <= 2e-10
    assert abs(got["Iterations"] - want) <= 1


@gpu
def test_driver_default_method_is_bicgstab(grid_file):
    a = run_driver(grid_file, "--precond=fp32")
    b = run_driver(grid_file, "--precond=fp32", "--method=bicgstab")
    for key in ("Iterations", "Reason", "Relative residual"):
        assert a[key] == b[key]
    g = run_driver(grid_file, "--precond=fp32", "--method=gmres", "--restart=5")
    assert g["Reason"] == 0 and g["Iterations"] != a["Iterations"]
