"""BiCGStab and GMRES at sizes where krylov.hip's multi-workgroup machinery
runs, against the longdouble trajectory restatement (krylov_ref.py).

Sizes, cases, the spreads the tolerances come from and the proof that a missed
workgroup partial would leave them are in test_krylov_trajectory.py; the
tolerances are krylov_ref.tolerance(case) = 100 x the CPU-measured spread of
three fp64 summation orders, never anything the device returned.

1. test_trajectory: K iterations at rtol = 0 from a seeded b and a non-zero
   x0; reason, iters, len(history), then every history entry and x.
2. test_alignment_changes_no_bit: b and / or x 8- but not 16-byte aligned (the
   VEC = false kernels) give the bits of the aligned run, and x's neighbours
   are untouched.
3. test_breakdown_*: (rhat, v) = 0 on 3 * 2048 + 6 unknowns, seen by all four
   workgroups; a non-finite b in the last workgroup's range; GMRES solves the
   same system.
4. test_edges_*: b = 0, a start inside rtol, repeatability and check_every, at
   S (four workgroups).
5. test_first_pass_partials: rsp_orthogonalize on V = 2 Q, where the second
   Gram-Schmidt pass cannot repair a first-pass coefficient (the one group of
   dots no solver trajectory can see).

On an MI355X the trajectories are off by at most 8.1e-14 (history) and 2.5e-14
(x) where the tolerances are 4.7e-12 and 1.5e-12 (BiCGStab, S, fp64 ILU(0)); on
T the histories are off by 3.8e-13 of 8.2e-11 (BiCGStab), 8.8e-15 and 2.8e-11
of 7.0e-9 (GMRES, restart 3 and 30); everywhere else by <= 1.5e-15, of
tolerances >= 2.2e-14; x of the all-fp32 iterations is bitwise the
restatement's. Every test prints its own figures.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import krylov_ref as kr
from respasol_amd import _lib
from respasol_amd.sparse import GMRES, BiCGStab, Handle, Ilu0, SpMat, orthogonalize, upload_csr

pytestmark = pytest.mark.gpu
TORCH = {"f64": torch.float64, "f32": torch.float32}
NPT = {"f64": np.float64, "f32": np.float32}


class Devices:
    """What the module shares on the device: one matrix per (size, iteration
    type), one analysed and factored ILU(0) per (size, preconditioner)."""

    def __init__(self):
        self.h = Handle()
        self.mats, self.ilus = {}, {}

    def mat(self, g, it):
        key = (id(g), it)
        if key not in self.mats:
            rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values, TORCH[it])
            self.mats[key] = (SpMat(self.h, rp, ci, va, g.n), rp, ci)
        return self.mats[key]

    def ilu(self, g, it, pc):
        if pc == "none":
            return None, None
        key = (id(g), it, pc)
        if key not in self.ilus:
            _, rp, ci = self.mat(g, it)
            ilu = Ilu0(self.h, rp, ci)
            ilu.analysis()
            fac = torch.from_numpy(g.values.astype(kr.NP[pc])).cuda()
            ilu.factor(fac)
            self.ilus[key] = (ilu, fac)
        return self.ilus[key]

    def solver(self, g, sv, restart, pc="none", it="f64"):
        A = self.mat(g, it)[0]
        ilu, fac = self.ilu(g, it, pc)
        return BiCGStab(self.h, A, ilu, fac) if sv == "bicgstab" else GMRES(self.h, A, ilu, fac, restart=restart)

    def close(self):
        for ilu, _ in self.ilus.values():
            ilu.close()
        for A, _, _ in self.mats.values():
            A.close()
        self.h.close()


@pytest.fixture(scope="module")
def dev():
    t0 = time.perf_counter()
    d = Devices()
    yield d
    torch.cuda.synchronize()
    d.close()
    print(f"\ntest_gpu_krylov_trajectory: {time.perf_counter() - t0:.1f} s wall for the module")


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def max_iters_reason(sv):
    return BiCGStab.MAX_ITERS if sv == "bicgstab" else GMRES.MAX_ITERS


# ------------------------------------------------------------ 1. trajectory

@pytest.mark.parametrize("case", kr.CASES, ids=[kr.case_id(c) for c in kr.CASES])
def test_trajectory(dev, case):
    sv, restart, K, size, pc, it = case
    g = kr.grid(size)
    x_ref, h_ref, _ = kr.reference(case)
    tol_hist, tol_x = kr.tolerance(case)
    b, x0 = g.rhs_and_start(NPT[it])
    s = dev.solver(g, sv, restart, pc, it)
    try:
        res = s.solve(on_device(b), x0=on_device(x0), rtol=0.0, max_iters=K, check_every=1)
    finally:
        s.close()
    assert res.reason == max_iters_reason(sv) and res.iters == K
    # one check per iteration; a GMRES cycle end coincides with its last column's
    assert len(res.history) == K and res.relres == res.history[-1]
    assert res.x.dtype == TORCH[it]
    dh, dx = kr.deviation(res.x.cpu().numpy(), res.history, x_ref, h_ref)
    print(f"{kr.case_id(case)}: history off by {dh:.2e} (tolerance {tol_hist:.2e}), "
          f"x by {dx:.2e} (tolerance {tol_x:.2e})")
    assert dh <= tol_hist
    assert dx <= tol_x


# ------------------------------------------------------------- 2. alignment

def raw_solve(dev, sv, s, b, x, K):
    """rsp_*_solve (rtol = 0) on the pointers as they are: (history, iters, reason)."""
    fn, hist_fn = ((_lib.rsp.rsp_bicgstab_solve, _lib.rsp.rsp_bicgstab_history) if sv == "bicgstab"
                   else (_lib.rsp.rsp_gmres_solve, _lib.rsp.rsp_gmres_history))
    iters, reason, rel, count = C.c_int(), C.c_int(), C.c_double(), C.c_int()
    st = fn(dev.h.ptr, s._s, C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), 0.0, K, 1,
            C.byref(iters), C.byref(rel), C.byref(reason))
    assert st == _lib.STATUS_SUCCESS
    hist = (C.c_double * (K + 1))()
    assert hist_fn(s._s, K + 1, hist, C.byref(count)) == _lib.STATUS_SUCCESS
    return list(hist[:count.value]), iters.value, reason.value


SENTINEL = -7.25


def placed(values, misaligned):
    """values inside a sentinel-filled buffer, 16-byte aligned or 8 bytes past
    that: (buffer, view, elements before the view)."""
    t = on_device(values)
    off = (8 // t.element_size()) if misaligned else (16 // t.element_size())
    buf = torch.full((t.numel() + 2 * off + 4,), SENTINEL, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert view.data_ptr() % 16 == (8 if misaligned else 0)
    return buf, view, off


@pytest.mark.parametrize("sv,restart,K", [("bicgstab", 0, 4), ("gmres", 3, 5)])
@pytest.mark.parametrize("it,pc", [("f64", "fp64"), ("f32", "fp32")])
def test_alignment_changes_no_bit(dev, sv, restart, K, it, pc):
    g = kr.grid("S")
    b, x0 = g.rhs_and_start(NPT[it])
    s = dev.solver(g, sv, restart, pc, it)
    try:
        out = {}
        for mis_b, mis_x in ((False, False), (True, True), (True, False), (False, True)):
            _, bv, _ = placed(b, mis_b)
            xbuf, xv, off = placed(x0, mis_x)
            hist, iters, reason = raw_solve(dev, sv, s, bv, xv, K)
            torch.cuda.synchronize()
            assert iters == K and reason == max_iters_reason(sv) and len(hist) == K
            assert torch.all(xbuf[:off] == SENTINEL) and torch.all(xbuf[off + g.n:] == SENTINEL)
            out[mis_b, mis_x] = (hist, xv.clone())
        hist0, xa = out[False, False]
        assert not torch.equal(xa, on_device(x0))
        for key, (hist, x) in out.items():
            assert hist == hist0, key
            assert torch.equal(x, xa), key
        # b = 0: x = 0 is written through the same ownership rule
        for mis_x in (False, True):
            xbuf, xv, off = placed(x0, mis_x)
            hist, iters, reason = raw_solve(dev, sv, s, torch.zeros_like(on_device(b)), xv, K)
            torch.cuda.synchronize()
            assert (hist, iters, reason) == ([], 0, _lib.SOLVE_CONVERGED)
            assert torch.count_nonzero(xv).item() == 0
            assert torch.all(xbuf[:off] == SENTINEL) and torch.all(xbuf[off + g.n:] == SENTINEL)
    finally:
        s.close()


# ------------------------------------------------------------- 3. breakdown

SKEW_N = 3 * 2048 + 6


@functools.lru_cache(maxsize=None)
def skew_system():
    """[[0, 1], [-1, 0]] blocks, b = (1, 0, 1, 0, ..) and a seeded non-zero x0
    of eighths: r0 = b - A x0 and every product and partial sum of (r0, A r0)
    are exact in fp64, so (rhat, v) = 0 holds bit for bit in any order."""
    g = kr.skew_blocks(SKEW_N)
    b = np.where(np.arange(SKEW_N) % 2 == 0, 1.0, 0.0)
    x0 = np.random.default_rng(77).integers(-8, 9, SKEW_N) / 8.0
    assert np.count_nonzero(x0) > SKEW_N // 2
    return g, b, x0


def test_breakdown_is_seen_by_every_workgroup(dev):
    g, b, x0 = skew_system()
    r0 = b - g.matvec(x0)
    assert np.dot(r0, g.matvec(r0)) == 0.0
    s = dev.solver(g, "bicgstab", 0)
    try:
        d_b, d_x0 = on_device(b), on_device(x0)
        res = s.solve(d_b, x0=d_x0)
        assert res.reason == BiCGStab.BREAKDOWN and res.iters == 0
        assert len(res.history) == 1
        assert torch.equal(res.x, d_x0)  # every element, in every workgroup's range
        # a non-finite b in the last workgroup's range: nothing to iterate on
        for bad in (float("inf"), float("nan")):
            d_bad = d_b.clone()
            d_bad[SKEW_N - 3] = bad
            res = s.solve(d_bad, x0=d_x0)
            assert res.reason == BiCGStab.BREAKDOWN and res.iters == 0 and res.history == []
            assert torch.equal(res.x, d_x0)
    finally:
        s.close()
    s = dev.solver(g, "gmres", 30)
    try:
        d_bad = on_device(b)
        d_bad[SKEW_N - 3] = float("inf")
        res = s.solve(d_bad, x0=on_device(x0))
        assert res.reason == GMRES.BREAKDOWN and res.iters == 0 and res.history == []
        assert torch.equal(res.x, on_device(x0))
    finally:
        s.close()


def test_gmres_solves_the_breakdown_system(dev):
    """A^2 = -I: the Krylov space has two dimensions, GMRES is exact after two
    iterations. The first check (est) and x against the restatement, as in
    test_trajectory with the spread of this system; the second check is the
    recomputed residual of an exact solve, i.e. rounding: bounded absolutely."""
    g, b, x0 = skew_system()
    run = lambda kind: kr.fgmres_trajectory(g, None, np.float64, 30, 2, b, x0, kr.Dot(kind))
    x_ref, h_ref = run("longdouble")
    assert len(h_ref) == 2
    s_hist = s_x = 0.0
    for kind in kr.FP64_ORDERS:
        x, hist = run(kind)
        s_hist = max(s_hist, abs(hist[0] - h_ref[0]) / h_ref[0])
        s_x = max(s_x, float(np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref))))
    tol_hist, tol_x = kr.MARGIN * max(s_hist, kr.EPS), kr.MARGIN * max(s_x, kr.EPS)
    s = dev.solver(g, "gmres", 30)
    try:
        res = s.solve(on_device(b), x0=on_device(x0), rtol=0.0, max_iters=2, check_every=1)
        x = res.x.cpu().numpy()
        dh = abs(res.history[0] - h_ref[0]) / h_ref[0]
        dx = float(np.max(np.abs(x - x_ref)) / np.max(np.abs(x_ref)))
        print(f"est off by {dh:.2e} (tolerance {tol_hist:.2e}), x by {dx:.2e} (tolerance {tol_x:.2e}); "
              f"final residual {res.history[1]:.2e} (restated {h_ref[1]:.2e})")
        assert res.iters == 2 and len(res.history) == 2
        assert dh <= tol_hist and dx <= tol_x
        # ||b - A x|| <= ||b - A x_ref|| + ||A|| ||x - x_ref||_2 with ||A|| = 1, and x is within
        # tol_x max|x_ref| of x_ref in every element
        assert res.history[1] <= h_ref[1] + tol_x * np.max(np.abs(x_ref)) * np.sqrt(SKEW_N) / np.linalg.norm(b)
        # and with a tolerance it converges there
        res = s.solve(on_device(b), x0=on_device(x0), rtol=1e-12)
        assert res.reason == GMRES.CONVERGED and res.iters == 2
        assert np.linalg.norm(b - g.matvec(res.x.cpu().numpy())) <= 1e-12 * np.linalg.norm(b)
    finally:
        s.close()


# ------------------------------------------------- 4. edges, four workgroups

@pytest.fixture(params=["bicgstab", "gmres"])
def s_solver(dev, request):
    s = dev.solver(kr.grid("S"), request.param, 30, "fp64")
    yield s
    s.close()


def test_edges_zero_rhs_and_start_inside_rtol(s_solver):
    g = kr.grid("S")
    b, x0 = (on_device(a) for a in g.rhs_and_start())
    res = s_solver.solve(torch.zeros_like(b), x0=x0)
    assert res.converged and res.iters == 0
    assert torch.count_nonzero(res.x).item() == 0
    solved = s_solver.solve(b, x0=x0, rtol=1e-12)
    assert solved.converged and solved.iters > 0
    true = np.linalg.norm(g.matvec(solved.x.cpu().numpy()) - b.cpu().numpy()) / np.linalg.norm(b.cpu().numpy())
    assert true <= 1e-10  # (what makes it a start inside rtol = 1e-10)
    res = s_solver.solve(b, x0=solved.x, rtol=1e-10)
    assert res.converged and res.iters == 0
    assert torch.equal(res.x, solved.x)


def test_edges_identical_solves_give_identical_bits(s_solver):
    b, x0 = (on_device(a) for a in kr.grid("S").rhs_and_start())
    a = s_solver.solve(b, x0=x0, rtol=1e-10)
    c = s_solver.solve(b, x0=x0, rtol=1e-10)
    assert a.converged and a.iters > 4
    assert torch.equal(a.x, c.x)
    assert a.iters == c.iters and a.history == c.history and a.relres == c.relres


def test_edges_check_every_changes_no_bit(s_solver):
    b, x0 = (on_device(a) for a in kr.grid("S").rhs_and_start())
    out = [s_solver.solve(b, x0=x0, rtol=0.0, max_iters=8, check_every=k) for k in (1, 4, 8)]
    for o, checks in zip(out, (8, 2, 1)):
        assert o.reason == _lib.SOLVE_MAX_ITERS and o.iters == 8
        assert len(o.history) == checks
        assert torch.equal(o.x, out[0].x)
        assert o.relres == out[0].relres


# -------------------------------------------- 5. the first Gram-Schmidt pass

@pytest.mark.parametrize("n,k,dtype", [(6149, 3, np.float64), (6149, 10, np.float64), (6149, 3, np.float32),
                                       (525312, 3, np.float64)])
def test_first_pass_partials(dev, n, k, dtype):
    V, w = kr.ortho_problem(n, k, dtype)
    ref = kr.ortho_run(V, w)
    tol = kr.ortho_tolerance(V, w, ref)
    per16 = 16 // V.itemsize
    ld = -(-n // per16) * per16  # columns 16-byte aligned, as the solver's are
    d_V = torch.zeros((k, ld), dtype=torch.from_numpy(V).dtype, device="cuda")
    d_V[:, :n] = on_device(V)
    d_w = on_device(w)
    h = orthogonalize(dev.h, d_V[:, :n], d_w)
    off = kr.ortho_deviation((h[:k], h[k], d_w.cpu().numpy().astype(np.float64)), ref)
    print(f"n = {n}, k = {k}, {dtype.__name__}: off by {off:.2e} (tolerance {tol:.2e})")
    assert off <= tol
