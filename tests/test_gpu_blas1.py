"""rsp_dot (the BiCGStab solver's reduction on its own) in fp64 and fp32.

Bound: the device forms each product x_i*y_i in fp64 (exact for fp32 inputs,
the correctly rounded fp64 product for fp64 inputs — the same number Python
forms) and adds n of them in some fixed order, so against math.fsum of the
same products the error of ANY summation order is at most
gamma_n * sum |x_i*y_i|, gamma_n = n u / (1 - n u), u = 2^-53.

Sizes: the small ones around a wave and a workgroup, the per-workgroup range
C (_lib.KRY_CHUNK) and its neighbours, G-1 full workgroups plus an odd tail
(G = _lib.KRY_MAX_GRID), and one length past G*C, where the grid saturates
and the per-workgroup range grows instead."""
import math

import numpy as np
import pytest
import torch

import oracle_bind as ob
from respasol_amd import _lib
from respasol_amd.sparse import Handle, dot

pytestmark = pytest.mark.gpu

C_, G_ = _lib.KRY_CHUNK, _lib.KRY_MAX_GRID
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, C_ - 1, C_, C_ + 1, 3 * C_ + 5, (G_ - 1) * C_ + 777,
         G_ * C_ + 12345]
NMAX = max(SIZES) + 1


@pytest.fixture(scope="module")
def handle():
    h = Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def data():
    """dlarnv(1) values minus 0.5, once; fp64 and fp32 views of them."""
    x, seed = ob.dlarnv(1, [0, 0, 0, 1], NMAX)
    y, _ = ob.dlarnv(1, seed, NMAX)
    x -= 0.5
    y -= 0.5
    out = {}
    for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        hx, hy = x.astype(npdt), y.astype(npdt)
        out[dt] = (hx, hy, torch.from_numpy(hx).cuda(), torch.from_numpy(hy).cuda())
    return out


def check(h, hx, hy, dx, dy):
    n = hx.shape[0]
    prod = hx.astype(np.float64) * hy.astype(np.float64)
    ref = math.fsum(prod.tolist())
    u = 2.0 ** -53
    bound = n * u / (1.0 - n * u) * math.fsum(np.abs(prod).tolist())
    got = dot(h, dx, dy)
    print(f"n={n} got={got!r} ref={ref!r} err={abs(got - ref):.3e} bound={bound:.3e}")
    assert abs(got - ref) <= bound
    assert dot(h, dx, dy) == got  # bitwise repeatable
    return got


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", SIZES)
def test_dot(handle, data, dtype, n):
    hx, hy, dx, dy = data[dtype]
    check(handle, hx[:n], hy[:n], dx[:n], dy[:n])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [1, 65, C_ + 1, 3 * C_ + 5])
def test_dot_offset_pointer(handle, data, dtype, n):
    """base + 1 element: not 16-byte aligned, so the element-wise path runs;
    the order of summation is the same, so the result equals the aligned one's
    bit for bit."""
    hx, hy, dx, dy = data[dtype]
    assert dx[1:].data_ptr() % 16 != 0
    got = check(handle, hx[1:n + 1], hy[1:n + 1], dx[1:n + 1], dy[1:n + 1])
    ax, ay = dx[1:n + 1].clone(), dy[1:n + 1].clone()
    assert ax.data_ptr() % 16 == 0 and ay.data_ptr() % 16 == 0
    assert dot(handle, ax, ay) == got
    # mixed alignment: one aligned operand, one not
    assert dot(handle, ax, dy[1:n + 1]) == got


def test_dot_argument_checks(handle, data):
    _, _, dx, _ = data[torch.float64]
    _, _, fx, _ = data[torch.float32]
    with pytest.raises(ValueError):
        dot(handle, dx[:4], fx[:4])
    with pytest.raises(ValueError):
        dot(handle, dx[:4], dx[:5])
    assert dot(handle, dx[:0], dx[:0]) == 0.0
