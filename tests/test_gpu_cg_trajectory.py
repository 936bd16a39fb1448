"""CG at sizes where krylov.hip's multi-workgroup machinery runs, against the
longdouble trajectory restatement (cg_ref.py), modelled on
test_gpu_krylov_trajectory.py.

Sizes, cases, the spreads the tolerances come from and the proof that a missed
workgroup partial would leave them are in test_cg_trajectory.py; the
tolerances are cg_ref.tolerance(case) = 100 x the CPU-measured spread of three
fp64 summation orders, never anything the device returned.

1. test_trajectory: K iterations at rtol = 0 from a seeded b and a non-zero
   x0; reason, iters, len(history), then every history entry and x.
2. test_alignment_changes_no_bit: b and / or x 8- but not 16-byte aligned (the
   VEC = false kernels) give the bits of the aligned run, and x's neighbours
   are untouched (S, fp64 and the mixed form).
3. test_breakdown_*: (p, A p) = 0 on 3 * 2048 + 6 unknowns, seen by all four
   workgroups; the negated S grid (negative definite); a NaN in the last
   workgroup's range of b. Arithmetic conditions handled by a flag.
4. test_edges_*: b = 0, a start inside rtol, repeatability and check_every, at
   S (four workgroups).

On an MI355X the histories are off by at most 1.4e-15 (L under the fp32
preconditioner, where the tolerance is 1.4e-9) and 7.9e-16 elsewhere, of
tolerances >= 2.2e-14; x by at most 7.1e-16, of tolerances >= 2.2e-14; x of
the all-fp32 iteration is bitwise the restatement's. Every test prints its own
figures next to its tolerances.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import cg_ref as cr
import krylov_ref as kr
from respasol_amd import _lib
from respasol_amd.sparse import CG, Handle, Ilu0, SpMat, upload_csr

pytestmark = pytest.mark.gpu
TORCH = {"f64": torch.float64, "f32": torch.float32}
NPT = {"f64": np.float64, "f32": np.float32}


class Devices:
    """What the module shares on the device: one matrix per (matrix, iteration
    type), one analysed and factored ILU(0) per (matrix, preconditioner)."""

    def __init__(self):
        self.h = Handle()
        self.mats, self.ilus = {}, {}

    def mat(self, g, it):
        key = (id(g), it)
        if key not in self.mats:
            rp, ci, va = upload_csr(g.rowptr, g.colidx, g.values, TORCH[it])
            self.mats[key] = (SpMat(self.h, rp, ci, va, g.n), rp, ci, g)  # (g kept: its id is the key)
        return self.mats[key]

    def ilu(self, g, it, pc):
        if pc == "none":
            return None, None
        key = (id(g), it, pc)
        if key not in self.ilus:
            _, rp, ci, _ = self.mat(g, it)
            ilu = Ilu0(self.h, rp, ci)
            ilu.analysis()
            fac = torch.from_numpy(g.values.astype(cr.NP[pc])).cuda()
            ilu.factor(fac)
            self.ilus[key] = (ilu, fac)
        return self.ilus[key]

    def solver(self, g, pc="none", it="f64"):
        A = self.mat(g, it)[0]
        ilu, fac = self.ilu(g, it, pc)
        return CG(self.h, A, ilu, fac)

    def close(self):
        for ilu, _ in self.ilus.values():
            ilu.close()
        for m in self.mats.values():
            m[0].close()
        self.h.close()


@pytest.fixture(scope="module")
def dev():
    t0 = time.perf_counter()
    d = Devices()
    yield d
    torch.cuda.synchronize()
    d.close()
    print(f"\ntest_gpu_cg_trajectory: {time.perf_counter() - t0:.1f} s wall for the module")


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------ 1. trajectory

@pytest.mark.parametrize("case", cr.CASES, ids=[cr.case_id(c) for c in cr.CASES])
def test_trajectory(dev, case):
    size, pc, it, K = case
    g = cr.grid(size)
    x_ref, h_ref, _ = cr.reference(case)
    tol_hist, tol_x = cr.tolerance(case)
    b, x0 = g.rhs_and_start(NPT[it])
    s = dev.solver(g, pc, it)
    try:
        res = s.solve(on_device(b), x0=on_device(x0), rtol=0.0, max_iters=K, check_every=1)
    finally:
        s.close()
    assert res.reason == CG.MAX_ITERS and res.iters == K
    assert len(res.history) == K and res.relres == res.history[-1]
    assert res.x.dtype == TORCH[it]
    dh, dx = cr.deviation(res.x.cpu().numpy(), res.history, x_ref, h_ref)
    print(f"{cr.case_id(case)}: history off by {dh:.2e} (tolerance {tol_hist:.2e}), "
          f"x by {dx:.2e} (tolerance {tol_x:.2e})")
    assert dh <= tol_hist
    assert dx <= tol_x


# ------------------------------------------------------------- 2. alignment

def raw_solve(dev, s, b, x, K):
    """rsp_cg_solve (rtol = 0) on the pointers as they are: (history, iters, reason)."""
    iters, reason, rel, count = C.c_int(), C.c_int(), C.c_double(), C.c_int()
    st = _lib.rsp.rsp_cg_solve(dev.h.ptr, s._s, C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), 0.0, K, 1,
                               C.byref(iters), C.byref(rel), C.byref(reason))
    assert st == _lib.STATUS_SUCCESS
    hist = (C.c_double * (K + 1))()
    assert _lib.rsp.rsp_cg_history(s._s, K + 1, hist, C.byref(count)) == _lib.STATUS_SUCCESS
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


@pytest.mark.parametrize("it,pc", [("f64", "fp64"), ("f64", "fp32"), ("f64", "none"), ("f32", "fp32")])
def test_alignment_changes_no_bit(dev, it, pc):
    K = 6
    g = cr.grid("S")
    b, x0 = g.rhs_and_start(NPT[it])
    s = dev.solver(g, pc, it)
    try:
        out = {}
        for mis_b, mis_x in ((False, False), (True, True), (True, False), (False, True)):
            _, bv, _ = placed(b, mis_b)
            xbuf, xv, off = placed(x0, mis_x)
            hist, iters, reason = raw_solve(dev, s, bv, xv, K)
            torch.cuda.synchronize()
            assert iters == K and reason == CG.MAX_ITERS and len(hist) == K
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
            hist, iters, reason = raw_solve(dev, s, torch.zeros_like(on_device(b)), xv, K)
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
    are exact in fp64, so (p, A p) = 0 holds bit for bit in any order."""
    g = kr.skew_blocks(SKEW_N)
    b = np.where(np.arange(SKEW_N) % 2 == 0, 1.0, 0.0)
    x0 = np.random.default_rng(77).integers(-8, 9, SKEW_N) / 8.0
    assert np.count_nonzero(x0) > SKEW_N // 2
    return g, b, x0


def test_breakdown_is_seen_by_every_workgroup(dev):
    g, b, x0 = skew_system()
    r0 = b - g.matvec(x0)
    assert np.dot(r0, g.matvec(r0)) == 0.0
    s = dev.solver(g)
    try:
        d_b, d_x0 = on_device(b), on_device(x0)
        for check_every in (1, 4):
            res = s.solve(d_b, x0=d_x0, check_every=check_every, max_iters=8)
            assert res.reason == CG.BREAKDOWN and res.iters == 0
            assert len(res.history) == 1
            assert res.relres == np.sqrt(kr.Dot("forward")(r0, r0)) / np.sqrt(SKEW_N // 2)  # r is r0 still (exact sums)
            assert torch.equal(res.x, d_x0)  # every element, in every workgroup's range
        # a non-finite b in the last workgroup's range: nothing to iterate on
        for bad in (float("nan"), float("inf")):
            d_bad = d_b.clone()
            d_bad[SKEW_N - 3] = bad
            res = s.solve(d_bad, x0=d_x0)
            assert res.reason == CG.BREAKDOWN and res.iters == 0 and res.history == []
            assert torch.equal(res.x, d_x0)
        # and a non-finite x0
        d_bad = d_x0.clone()
        d_bad[SKEW_N - 3] = float("nan")
        res = s.solve(d_b, x0=d_bad)
        assert res.reason == CG.BREAKDOWN and res.iters == 0 and res.history == []
    finally:
        s.close()


@functools.lru_cache(maxsize=None)
def negated_s():
    g = cr.grid("S")
    return cr.Csr(g.rowptr, g.colidx, -g.values)


@pytest.mark.parametrize("pc", ["none", "fp64", "fp32"])
def test_breakdown_negative_definite(dev, pc):
    """-A: (p, A p) < 0 without a preconditioner; with one, M = L U of -A is
    negative definite too and (r, z) < 0 comes first. Either way BREAKDOWN at
    iteration 1 and x stays x0."""
    g = negated_s()
    b, x0 = (on_device(a) for a in cr.grid("S").rhs_and_start())
    s = dev.solver(g, pc)
    try:
        res = s.solve(b, x0=x0)
        print(f"-A, {pc}: reason {res.reason}, iters {res.iters}, relres {res.relres:.3e}")
        assert res.reason == CG.BREAKDOWN and res.iters == 0 and len(res.history) == 1
        assert torch.isfinite(res.x).all()
        assert torch.equal(res.x, x0)
    finally:
        s.close()


# ------------------------------------------------- 4. edges, four workgroups

@pytest.fixture(params=["fp64", "fp32", "none"])
def s_solver(dev, request):
    s = dev.solver(cr.grid("S"), request.param)
    yield s
    s.close()


def test_edges_zero_rhs_and_start_inside_rtol(s_solver):
    g = cr.grid("S")
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


def test_edges_identical_solves_give_identical_bits(dev, s_solver):
    b, x0 = (on_device(a) for a in cr.grid("S").rhs_and_start())
    a = s_solver.solve(b, x0=x0, rtol=1e-10)
    c = s_solver.solve(b, x0=x0, rtol=1e-10)
    pc = "none" if s_solver.ilu is None else ("fp32" if s_solver.factor.dtype == torch.float32 else "fp64")
    second = dev.solver(cr.grid("S"), pc)
    try:
        e = second.solve(b, x0=x0, rtol=1e-10)
    finally:
        second.close()
    assert a.converged and a.iters > 4
    for o in (c, e):
        assert torch.equal(a.x, o.x)
        assert a.iters == o.iters and a.history == o.history and a.relres == o.relres


def test_edges_check_every_changes_no_bit(s_solver):
    b, x0 = (on_device(a) for a in cr.grid("S").rhs_and_start())
    out = [s_solver.solve(b, x0=x0, rtol=0.0, max_iters=8, check_every=k) for k in (1, 4, 8)]
    for o, checks in zip(out, (8, 2, 1)):
        assert o.reason == _lib.SOLVE_MAX_ITERS and o.iters == 8
        assert len(o.history) == checks
        assert torch.equal(o.x, out[0].x)
        assert o.relres == out[0].relres
