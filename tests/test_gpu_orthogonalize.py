"""rsp_orthogonalize (respasol_amd.sparse.orthogonalize): one Gram-Schmidt step
of GMRES, applied twice, by the solver's three kernels, in fp64 and fp32.

Inputs: V = the Q of a numpy QR of seeded normal data, cast to the type (k
columns of n elements); w = seeded uniform(-1, 1) data plus 3 v_0, cast.

Bounds, with u = 2^-53 (the kernels' dots and updates are fp64 whatever the
type), u_T the type's unit roundoff, gamma = n u / (1 - n u), delta =
k max|V^T V - I| of the cast V (measured on the host in fp64: what is left of
orthonormality after the cast) and c = 4 gamma + 4 (k + 2) u_T:
  orthogonality   max_i |fsum(v_i . w_out)|        <= (delta + c) ||w_in||
  reconstruction  ||w_in - w_out - V h[:k]||_2     <= (delta + c) ||w_in|| sqrt(k)
  norm            |h[k]^2 - fsum(w_out^2)|         <= gamma fsum(w_out^2)
  sanity          |h[0] - (3 + (v_0, w_seed))|     <= 1e-6 ||w_in||
The numpy restatement of the two passes is held to the same bounds on the
three smallest sizes without a GPU, which shows that the inputs admit them.
"""
import functools
import math

import numpy as np
import pytest
import torch

from respasol_amd import _lib
from respasol_amd.sparse import Handle, RspError, orthogonalize

C, G = _lib.KRY_CHUNK, _lib.KRY_MAX_GRID
DTYPES = {"fp64": (np.float64, torch.float64, 2.0 ** -53), "fp32": (np.float32, torch.float32, 2.0 ** -24)}
SIZES = [(n, k) for n in (1, 65, C - 1, C, C + 1, 3 * C + 5) for k in (1, 2, 7, 31, 64) if k <= n]
BIG = [((G - 1) * C + 777, 3), (G * C + 12345, 3)]


@functools.lru_cache(maxsize=4)
def inputs(n, k, prec):
    """(V (k, n) of the type, w_in of the type, w_seed fp64, delta)."""
    npdt = DTYPES[prec][0]
    rng = np.random.default_rng(7919 * k + n)
    q, _ = np.linalg.qr(rng.standard_normal((n, k)))
    V = np.ascontiguousarray(q.T).astype(npdt)
    seed = rng.uniform(-1.0, 1.0, n)
    w = (seed + 3.0 * V[0].astype(np.float64)).astype(npdt)
    Vd = V.astype(np.float64)
    delta = k * float(np.max(np.abs(Vd @ Vd.T - np.eye(k))))
    for a in (V, w, seed):
        a.setflags(write=False)
    return V, w, seed, delta


def ref_two_passes(V, w):
    """The kernels' algorithm in numpy: fp64 dots and updates, w rounded to
    the type after each pass."""
    Vd = V.astype(np.float64)
    h = np.zeros(V.shape[0])
    for _ in range(2):
        wd = w.astype(np.float64)
        hp = Vd @ wd
        w = (wd - hp @ Vd).astype(V.dtype)
        h += hp
    return w, np.append(h, math.sqrt(float(np.dot(w.astype(np.float64), w.astype(np.float64)))))


def check_bounds(n, k, prec, w_out, h):
    V, w_in, seed, delta = inputs(n, k, prec)
    u, uT = 2.0 ** -53, DTYPES[prec][2]
    gamma = n * u / (1.0 - n * u)
    c = 4.0 * gamma + 4.0 * (k + 2) * uT
    Vd, wi, wo = V.astype(np.float64), w_in.astype(np.float64), w_out.astype(np.float64)
    nin = math.sqrt(math.fsum(wi * wi))
    orth = max(abs(math.fsum(Vd[i] * wo)) for i in range(k))
    rec = float(np.linalg.norm(wi - wo - h[:k] @ Vd))
    ww = math.fsum(wo * wo)
    want0 = 3.0 + math.fsum(Vd[0] * seed)
    print(f"n={n} k={k} {prec}: orth={orth:.3e} rec={rec:.3e} (bound {(delta + c) * nin:.3e}, delta={delta:.2e}) "
          f"norm err={abs(h[k] ** 2 - ww):.3e} (bound {gamma * ww:.3e}) h0 err={abs(h[0] - want0):.3e}")
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(wo))
    assert orth <= (delta + c) * nin
    assert rec <= (delta + c) * nin * math.sqrt(k)
    assert abs(h[k] ** 2 - ww) <= gamma * ww
    assert abs(h[0] - want0) <= 1e-6 * nin


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


def run(handle, n, k, prec, offset=0):
    """orthogonalize on device copies placed `offset` elements past an
    allocation's base; returns (w_out, h) as numpy."""
    V, w, _, _ = inputs(n, k, prec)
    tdt = DTYPES[prec][1]
    ld = n + (-n) % 4  # (whole 16-byte groups per row: every row at the base's alignment)
    vbuf = torch.zeros(offset + k * ld, dtype=tdt, device="cuda")
    wbuf = torch.zeros(offset + n, dtype=tdt, device="cuda")
    Vt = vbuf[offset:offset + k * ld].view(k, ld)[:, :n]
    wt = wbuf[offset:offset + n]
    Vt.copy_(torch.tensor(V))
    wt.copy_(torch.tensor(w))
    h = orthogonalize(handle, Vt, wt)
    assert np.array_equal(Vt.cpu().numpy(), V)  # V is read only
    return wt.cpu().numpy(), h


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,k", SIZES + BIG)
def test_orthogonalize_bounds(handle, n, k, prec):
    w_out, h = run(handle, n, k, prec)
    check_bounds(n, k, prec, w_out, h)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_unaligned_base_changes_no_bit(handle, prec):
    n, k = 3 * C + 5, 7
    w0, h0 = run(handle, n, k, prec)
    w1, h1 = run(handle, n, k, prec, offset=1)
    assert np.array_equal(w0, w1) and np.array_equal(h0, h1)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_repeatable(handle, prec):
    n, k = 3 * C + 5, 31
    w0, h0 = run(handle, n, k, prec)
    w1, h1 = run(handle, n, k, prec)
    assert np.array_equal(w0, w1) and np.array_equal(h0, h1)


@pytest.mark.gpu
def test_argument_checks_and_empty(handle):
    V = torch.zeros(65, 80, dtype=torch.float64, device="cuda")
    w = torch.zeros(80, dtype=torch.float64, device="cuda")

    def status(k, n, ldv):
        h = np.zeros(70)
        return _lib.rsp.rsp_orthogonalize(handle.ptr, _lib.R_64F, n, k, V.data_ptr(), ldv, w.data_ptr(),
                                          h.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double)))

    assert status(0, 80, 80) == _lib.STATUS_INVALID_VALUE
    assert status(_lib.GMRES_MAX_RESTART + 1, 80, 80) == _lib.STATUS_INVALID_VALUE
    assert status(3, 80, 79) == _lib.STATUS_INVALID_VALUE
    assert status(3, 80, 80) == _lib.STATUS_SUCCESS
    with pytest.raises(RspError):
        orthogonalize(handle, V[:0], w)
    # n = 0: h = 0
    h = np.ones(4)
    assert _lib.rsp.rsp_orthogonalize(handle.ptr, _lib.R_64F, 0, 3, None, 0, None,
                                      h.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))) == _lib.STATUS_SUCCESS
    assert h.tolist() == [0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("n,k", [(1, 1), (65, 7), (65, 64), (C - 1, 31)])
def test_restatement_meets_the_bounds(n, k, prec):
    V, w, _, _ = inputs(n, k, prec)
    w_out, h = ref_two_passes(V, w)
    check_bounds(n, k, prec, w_out, h)
