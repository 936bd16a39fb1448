"""include/rsp.h: "Every call is stream-ordered on the handle's stream".

Every other GPU test runs on the default stream (or synchronises the device
before each call), where the null stream's implicit synchronisation hides a
kernel, memset or copy issued to the wrong stream. Here every call runs on a
non-blocking side stream S behind a DELAYED PRODUCER (run_case below):

  1. all index arrays, plans, analyses and solver objects are built first and
     the device is synchronised; the call's floating-point inputs and outputs
     are filled with NaN;
  2. on S: the test kit's occupant (one workgroup spinning on the wall clock
     for DELAY_US), then the copies of the real data into the inputs, then the
     library call, then the read of its results.

A part of the call that is not ordered on S runs during the delay: it reads
NaN, or its result is overwritten later; both buffers exist, so nothing
faults — the result differs. It must equal, bit for bit, the same call made on
the default stream after a device synchronise (the same helper with no
delay), and the oracle where the other tests have one.

The delay is only a test if S is still busy when the call returns: every case
that is not host-blocking records S.query() there and FAILS if S is already
idle. test_delay_really_reorders is the control: a consumer on another stream
does see the poison.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import krylov_ref as kr
import oracle_bind as ob
from abi_cases import SPMV_MATRICES, occupant_kit, same_bits
from respasol_amd import _lib, csr
from respasol_amd.sparse import (GMRES, BiCGStab, Handle, Ilu0, SpMat, SpmvBatch, dot, gather, orthogonalize, scatter,
                                 upload_csr)

pytestmark = pytest.mark.gpu
NP = {torch.float64: np.float64, torch.float32: np.float32}
# The occupant's time on S. Measured on an MI355X: from the occupant's launch
# to the return of the library call(s), the slowest non-blocking case (the
# ILU(0) factor and its three solves on dc1 0.2, default plan) took 133 us of
# host time (offshore 104, the batched SpMV 70). The issue's floor is 10 x that
# (1.33 ms) and its cap 200 ms; 50 ms leaves a 375 x margin for a busy host and
# costs the file under 2 s. A case whose stream is idle when the call returns
# fails (run_case), so a delay that has become too short cannot pass unseen.
MEASURED_US = 133
DELAY_US = 50_000
HOST_US = {}


# A process's streams share a few hardware queues (4 unless GPU_MAX_HW_QUEUES
# says otherwise), and two streams on one queue run in order: on an MI355X a
# copy on one of about every fourth other stream did wait for the occupant.
HW_QUEUES = 4


def reads_poison(h, S, other):
    """The control's probe: behind the occupant on S the real data is copied
    into `inp`; a plain copy of `inp` on `other`, with no event, finishes
    while S is still held. True if it read the poison (the streams run
    independently), False if it was serialised behind S and read the data."""
    real = dev(np.random.default_rng(9).uniform(-1, 1, 4096))
    inp, _ = late_input(real)
    out = torch.empty_like(real)

    def consumer():
        with torch.cuda.stream(other):
            out.copy_(inp)
        other.synchronize()
    # (blocking: a serialised consumer returns only when S is idle, which is an answer here, not a failure)
    _, (got,) = run_case(h, S, [(inp, real)], consumer, [out], DELAY_US, blocking=True)
    if np.isnan(got).all():
        return True
    assert same_bits(got, real.cpu().numpy())  # (all of one or all of the other)
    return False


@pytest.fixture(scope="module")
def ctx():
    """The handle and its side stream S: a stream that does not share the
    null stream's hardware queue, or an operation that the library issued to
    the null stream (as rsp_ilu0_analysis' memsets once were) would be
    serialised behind S all the same and go unseen."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    S = torch.cuda.Stream()
    h = Handle(stream=S)
    for _ in range(HW_QUEUES):
        if reads_poison(h, S, torch.cuda.default_stream()):
            break
        S = torch.cuda.Stream()
    else:
        pytest.fail("no side stream runs beside the null stream: a delayed producer cannot show anything")
    yield h, S
    torch.cuda.synchronize()
    h.close()
    slow = sorted(HOST_US.items(), key=lambda kv: -kv[1])[:5]
    print("\ntest_gpu_streams: host time from the occupant's launch to the call's return (us), slowest first: "
          + ", ".join(f"{k} {v:.0f}" for k, v in slow) + f"; DELAY_US = {DELAY_US}, chosen from {MEASURED_US} us measured")


def to_host(r):
    if isinstance(r, torch.Tensor):
        return r.cpu().numpy()
    if isinstance(r, (tuple, list)):
        return tuple(to_host(v) for v in r)
    return r


def equal(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and same_bits(a, b)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(equal(u, v) for u, v in zip(a, b))
    return a == b


def run_case(h, stream, feeds, call, outputs, delay_us, blocking=False, label=None):
    """The delayed producer. feeds: (input tensor, tensor holding its real
    data) pairs; outputs: the tensors the call writes. Returns what call()
    returned and the outputs, on the host. delay_us = 0 on the default stream
    is the plain run the delayed one is compared with."""
    torch.cuda.synchronize()
    for t in [dst for dst, _ in feeds] + list(outputs):
        t.fill_(float("nan"))
    torch.cuda.synchronize()
    h.set_stream(stream)
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        if delay_us:
            assert occupant_kit().rsp_testkit_occupy(stream.cuda_stream, 1, delay_us) == 0
        for dst, src in feeds:
            dst.copy_(src)
        ret = call()
        host_us = (time.perf_counter() - t0) * 1e6
        busy = not stream.query()
        ret, got = to_host(ret), to_host(list(outputs))  # (read on the same stream)
    stream.synchronize()
    if delay_us and not blocking:
        if label:
            HOST_US[label] = host_us
        assert busy, (f"{label}: the stream was idle when the call returned ({host_us:.0f} us of host time after the "
                      f"occupant's launch, DELAY_US = {delay_us}): the delay tested nothing")
    return ret, got


def both(ctx, feeds, call, outputs, blocking=False, label=None, stream=None):
    """The plain run on the default stream, then the delayed one on S: equal bits."""
    h, S = ctx
    plain = run_case(h, torch.cuda.default_stream(), feeds, call, outputs, 0)
    late = run_case(h, stream or S, feeds, call, outputs, DELAY_US, blocking, label)
    assert equal(late, plain), f"{label}: behind a delayed producer the call gave other bits"
    for a in late[1] + (late[0] if isinstance(late[0], tuple) else ()):
        if isinstance(a, np.ndarray) and a.dtype.kind == "f":
            assert not np.isnan(a).any(), f"{label}: poison in the result"
    return late


def late_input(real):
    """(the input tensor the call reads, its real data): the first is poisoned
    by run_case and filled from the second on the stream."""
    return torch.empty_like(real), real


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# ------------------------------------------------------------------- SpMV

class Spmv:
    """One of the two matrices (abi_cases.py) on the device: values and x are
    late inputs; the canonical-order oracle's y."""

    def __init__(self, h, name, dtype):
        A = SPMV_MATRICES[name]()
        self.A, self.dtype = A, dtype
        rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dtype)
        self.va, self.va_real = late_input(va)
        self.va.copy_(va)  # (a plan is built from the pattern only; valid values all the same)
        x = np.random.default_rng(3).uniform(-1, 1, A.n).astype(NP[dtype])
        self.x, self.x_real = late_input(dev(x))
        self.M = SpMat(h, rp, ci, self.va, A.n)
        self.y = torch.empty(A.m, dtype=dtype, device="cuda")
        self.canon = ob.spmv(A.rowptr, A.colidx, A.values.astype(NP[dtype]), x, order="canon")

    @property
    def feeds(self):
        return [(self.va, self.va_real), (self.x, self.x_real)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", sorted(SPMV_MATRICES))
def test_spmv(ctx, name, dtype):
    h, S = ctx
    c = Spmv(h, name, dtype)
    _, (y,) = both(ctx, c.feeds, lambda: c.M.spmv(c.x, c.y).numel(), [c.y], label=f"spmv {name}")
    assert same_bits(y, c.canon)
    # beta != 0: y is an input too (2 and 0.5: both scalings exact)
    y0 = np.random.default_rng(4).uniform(-1, 1, c.A.m).astype(NP[dtype])
    y0_real = dev(y0)
    _, (y,) = both(ctx, c.feeds + [(c.y, y0_real)], lambda: c.M.spmv(c.x, c.y, 2.0, 0.5).numel(), [c.y],
                   label=f"spmv beta {name}")
    assert same_bits(y, NP[dtype](2.0) * c.canon + NP[dtype](0.5) * y0)
    c.M.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", sorted(SPMV_MATRICES))
def test_spmv_parts(ctx, name, dtype):
    h, S = ctx
    c = Spmv(h, name, dtype)
    c.M.set_local_cols(c.A.n * 3 // 4)

    def call():
        c.M.spmv_part(c.x, c.y, 1)
        c.M.spmv_part(c.x, c.y, 2)
    _, (y,) = both(ctx, c.feeds, call, [c.y], label=f"spmv_part {name}")
    assert same_bits(y, c.canon)
    c.M.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_spmv_batch(ctx, dtype):
    h, S = ctx
    cs = [Spmv(h, name, dtype) for name in sorted(SPMV_MATRICES)]
    B = SpmvBatch(h, [c.M for c in cs], [c.x for c in cs], [c.y for c in cs])
    _, ys = both(ctx, [f for c in cs for f in c.feeds], lambda: B.run(1.0, 0.0), [c.y for c in cs],
                 label="spmv_batch_run")
    for c, y in zip(cs, ys):
        assert same_bits(y, c.canon)
    B.close()
    for c in cs:
        c.M.close()


def test_set_stream_switch(ctx):
    """One handle, one matrix: a call on S1, then rsp_set_stream(S2) — which
    rsp_get_stream returns — and the delayed producer on S2."""
    h, S = ctx
    c = Spmv(h, "hub", torch.float64)
    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    _, (y,) = both(ctx, c.feeds, lambda: c.M.spmv(c.x, c.y).numel(), [c.y], label="switch S1", stream=S1)
    assert same_bits(y, c.canon)
    S1.synchronize()
    h.set_stream(S2)
    got = C.c_void_p()
    assert _lib.rsp.rsp_get_stream(h.ptr, C.byref(got)) == _lib.STATUS_SUCCESS
    assert (got.value or 0) == S2.cuda_stream and S2.cuda_stream != S1.cuda_stream
    _, (y,) = both(ctx, c.feeds, lambda: c.M.spmv(c.x, c.y).numel(), [c.y], label="switch S2", stream=S2)
    assert same_bits(y, c.canon)
    h.set_stream(S)
    c.M.close()


# ------------------------------------------------------- gather / scatter

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gather_scatter(ctx, dtype):
    h, S = ctx
    n = 100003
    rng = np.random.default_rng(8)
    src_h = rng.uniform(-1, 1, n).astype(NP[dtype])
    perm = rng.permutation(n)
    idx = dev(perm.astype(np.int64))
    src, src_real = late_input(dev(src_h))
    dst = torch.empty(n, dtype=dtype, device="cuda")
    _, (g,) = both(ctx, [(src, src_real)], lambda: gather(h, idx, src, dst), [dst], label="gather")
    assert same_bits(g, src_h[perm])
    _, (s,) = both(ctx, [(src, src_real)], lambda: scatter(h, idx, src, dst), [dst], label="scatter")
    want = np.empty_like(src_h)
    want[perm] = src_h
    assert same_bits(s, want)


# ------------------------------------------------- ILU(0) factor and solves

@pytest.mark.parametrize("name,scale,env,blocks", [("offshore", 0.2, {"RSP_ILU_FAC_ONE": "0"}, False),
                                                   ("dc1", 0.2, {}, True)], ids=["offshore-flow", "dc1-blocks"])
def test_ilu_factor_and_solves(ctx, monkeypatch, name, scale, env, blocks):
    """The factor, then L, L^T and U solves, enqueued without a host wait
    between them; the zero-pivot calls (host-blocking) after the results are
    read. offshore with the factor over L's levels: flow runs, as in
    test_gpu_ilu0.test_flow_launches_beside_an_occupying_kernel; dc1 with the
    default plan: block L / L^T solves and a level-scheduled U solve."""
    h, S = ctx
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    A = csr.surrogate(name, scale)
    rp, ci, va_real = upload_csr(A.rowptr, A.colidx, A.values)
    torch.cuda.synchronize()
    il = Ilu0(h, rp, ci, nnz=A.nnz)
    il.analysis()
    assert il.zero_pivot() == -1
    il.trsv_analysis()
    il.trsv_analysis(transpose=True)
    assert (il.solve_blocks()[0] > 0) == blocks == ob.blocks_wanted(0, A.rowptr, A.colidx)
    xh, _ = csr.dlarnv(2, [0, 0, 0, 1], A.n)
    (va, _), (x, x_real) = late_input(va_real), late_input(dev(xh))
    z, yt, yu = (torch.empty_like(x) for _ in range(3))

    def call():
        il.factor(va)
        il.solve_lower(va, x, y=z)
        il.solve_lower(va, z, y=yt, transpose=True)
        il.solve_upper(va, z, y=yu)
    _, (v, gz, gyt, gyu) = both(ctx, [(va, va_real), (x, x_real)], call, [va, z, yt, yu], label=f"ilu {name}")
    assert il.zero_pivot() == -1
    for which in (il.TRSV_L, il.TRSV_LT, il.TRSV_U):
        assert il.solve_zero_pivot(which) == -1
    rv, sz, zp = ob.ilu0(A.rowptr, A.colidx, A.values)
    assert sz == -1 and zp == -1 and same_bits(v, rv)
    rz = ob.trsv("lower_n", A.rowptr, A.colidx, rv, xh)  # (the block order where the plan has blocks)
    assert same_bits(gz, rz)
    assert same_bits(gyt, ob.trsv("lower_t", A.rowptr, A.colidx, rv, rz))
    assert same_bits(gyu, ob.trsv("upper", A.rowptr, A.colidx, rv, rz))
    il.close()


# ----------------------------------------------------- the Krylov kernels

KRY_N, KRY_K = 6149, 3  # four workgroups (tests/test_gpu_krylov_trajectory.py)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dot_and_orthogonalize(ctx, dtype):
    """Host-blocking calls: they wait for the delayed producer themselves."""
    h, S = ctx
    Vh, wh = kr.ortho_problem(KRY_N, KRY_K, dtype)
    (a, a_real), (b, b_real) = late_input(dev(Vh[0])), late_input(dev(wh))
    d, _ = both(ctx, [(a, a_real), (b, b_real)], lambda: dot(h, a, b), [], blocking=True, label="dot")
    exact = float(np.dot(Vh[0].astype(np.longdouble), wh.astype(np.longdouble)))
    bound = KRY_N * 2.0 ** -52 * float(np.dot(np.abs(Vh[0]).astype(np.float64), np.abs(wh).astype(np.float64)))
    assert abs(d - exact) <= bound  # fp64 products and sums of n terms, in any order
    (V, V_real), (w, w_real) = late_input(dev(Vh)), late_input(dev(wh))
    hcoef, (gw,) = both(ctx, [(V, V_real), (w, w_real)], lambda: orthogonalize(h, V, w), [w], blocking=True,
                        label="orthogonalize")
    assert hcoef.shape == (KRY_K + 1,) and np.all(np.isfinite(hcoef))


@pytest.mark.parametrize("pc", ["fp64", "fp32"])
@pytest.mark.parametrize("sv,restart", [("bicgstab", 0), ("gmres", 3)])
def test_krylov_solve(ctx, sv, restart, pc):
    """Five iterations on the grid of the trajectory tests (four workgroups,
    fp64 iteration, fp64 / fp32 ILU(0)): x, iters, history and reason. b, x0
    and A's values arrive late; the solve is host-blocking (a check per
    iteration)."""
    h, S = ctx
    g = kr.grid("S")
    rp, ci, va_real = upload_csr(g.rowptr, g.colidx, g.values)
    va, _ = late_input(va_real)
    va.copy_(va_real)
    A = SpMat(h, rp, ci, va, g.n)
    ilu = Ilu0(h, rp, ci)
    ilu.analysis()
    fac = dev(g.values.astype(kr.NP[pc]))
    ilu.factor(fac)
    assert ilu.zero_pivot() == -1
    s = BiCGStab(h, A, ilu, fac) if sv == "bicgstab" else GMRES(h, A, ilu, fac, restart=restart)
    bh, x0h = g.rhs_and_start()
    (b, b_real), (x0, x0_real) = late_input(dev(bh)), late_input(dev(x0h))

    def call():
        r = s.solve(b, x0=x0, rtol=0.0, max_iters=5, check_every=1)
        return r.x, r.iters, tuple(r.history), r.reason, r.relres
    (x, iters, hist, reason, _), _ = both(ctx, [(va, va_real), (b, b_real), (x0, x0_real)], call, [], blocking=True,
                                          label=f"{sv} {pc}")
    assert iters == 5 and len(hist) == 5 and reason == _lib.SOLVE_MAX_ITERS
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(x))
    s.close()
    ilu.close()
    A.close()


# ------------------------------------------------------------- the control

def test_delay_really_reorders(ctx):
    """The same helper with a consumer that is NOT ordered behind the
    producer: a plain copy on another stream, no event. It reads the poison —
    so DELAY_US is long enough for a mis-issued operation of the library to be
    caught the same way. Both buffers are valid: a stale read, nothing more.
    On the null stream (where the library's two stray operations went) and on
    a fresh stream: the first of at most HW_QUEUES fresh ones that does not
    share S's hardware queue (see ctx)."""
    h, S = ctx
    assert reads_poison(h, S, torch.cuda.default_stream()), \
        "a copy on the null stream waited for the delayed producer: the delay proves nothing"
    fresh = [torch.cuda.Stream() for _ in range(HW_QUEUES)]
    assert all(o.cuda_stream != S.cuda_stream for o in fresh)
    assert any(reads_poison(h, S, o) for o in fresh), \
        "copies on fresh streams all waited for the delayed producer: the delay proves nothing"
    # and ordered behind it on S, the same copy sees the data
    real = dev(np.random.default_rng(9).uniform(-1, 1, 4096))
    inp, _ = late_input(real)
    out = torch.empty_like(real)
    _, (got,) = run_case(h, S, [(inp, real)], lambda: out.copy_(inp).numel(), [out], DELAY_US, label="control on S")
    assert same_bits(got, real.cpu().numpy())
