"""rsp_gather / rsp_scatter (the halo pack and unpack of the row-partitioned
SpMV) against numpy indexing, bit for bit: fp64 and fp32, sizes around one
workgroup (256) and around the grid cap (2048 workgroups x 256 threads =
524288 elements, past which each thread strides on), permutations and
repeated indices, pointers 16-byte aligned or one element past that, and
every element of dst that no index names keeps its bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from abi_cases import bits, same_bits
from respasol_amd import _lib
from respasol_amd.sparse import Handle, gather, scatter

pytestmark = pytest.mark.gpu
CAP = 2048 * 256  # the launch's grid cap in elements (spmv.hip gather / scatter)
SIZES = [0, 1, 255, 256, 257, CAP, CAP + 1, CAP + 257]
DTYPES = [np.float64, np.float32]
SENTINEL = -7.25  # never drawn by payload()


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    h = Handle()
    yield h
    h.close()


def payload(rng, n, dtype):
    """Uniform values with a few bit patterns a value-changing copy would not
    keep: -0.0, a denormal, infinities, a NaN with a payload."""
    a = rng.uniform(-1, 1, n).astype(dtype)
    special = np.array([-0.0, np.finfo(dtype).smallest_subnormal, np.inf, -np.inf], dtype)
    k = min(n, special.size)
    a[:k] = special[:k]
    if n > 4:
        bits(a)[4] = 0x7ff8000000000123 if dtype == np.float64 else 0x7fc00123
    return a


def placed(values, shift, pad=3):
    """values on the device inside a sentinel-filled allocation, `shift`
    elements past a 16-byte boundary: (allocation, view, elements before)."""
    t = torch.from_numpy(np.ascontiguousarray(values))
    per16 = 16 // t.element_size()
    off = per16 + shift
    buf = torch.full((t.numel() + off + pad,), SENTINEL, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t)
    assert t.numel() == 0 or view.data_ptr() % 16 == shift * t.element_size()
    return buf, view, off


def borders_intact(buf, off, n):
    return bool(torch.all(buf[:off] == SENTINEL)) and bool(torch.all(buf[off + n:] == SENTINEL))


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("repeat", [False, True], ids=["permutation", "repeated"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_gather(handle, dtype, n, repeat, shift):
    rng = np.random.default_rng(n + 7 * repeat)
    nsrc = max(n // 3, 1) if repeat else n
    idx = rng.integers(0, nsrc, n) if repeat else rng.permutation(n)
    src = payload(rng, nsrc, dtype)
    _, d_src, _ = placed(src, shift)
    dbuf, d_dst, off = placed(np.full(n, SENTINEL, dtype), shift)
    gather(handle, torch.from_numpy(idx.astype(np.int64)).cuda(), d_src, d_dst)
    assert same_bits(d_dst.cpu().numpy(), src[idx])
    assert borders_intact(dbuf, off, n)


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
def test_scatter_leaves_the_rest_of_dst(handle, dtype, n, shift):
    """A permutation's first n indices into a dst of 2 n sentinels: the n
    positions named hold src, the other n (and the allocation around dst)
    keep the sentinel's bits."""
    rng = np.random.default_rng(1000 + n)
    idx = rng.permutation(2 * n)[:n]
    src = payload(rng, n, dtype)
    _, d_src, _ = placed(src, shift)
    want = np.full(2 * n, SENTINEL, dtype)
    dbuf, d_dst, off = placed(want, shift)
    scatter(handle, torch.from_numpy(idx.astype(np.int64)).cuda(), d_src, d_dst)
    want[idx] = src
    assert same_bits(d_dst.cpu().numpy(), want)
    assert borders_intact(dbuf, off, 2 * n)


@pytest.mark.parametrize("fn", ["rsp_gather", "rsp_scatter"])
def test_arguments(handle, fn):
    """n = 0 with NULL pointers is a no-op that succeeds; n < 0, a NULL pointer
    with n > 0 and a type outside the enum are INVALID_VALUE (nothing runs)."""
    f = getattr(_lib.rsp, fn)
    idx = torch.arange(4, dtype=torch.int64, device="cuda")
    a = torch.zeros(4, dtype=torch.float64, device="cuda")
    b = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for dt in (_lib.R_64F, _lib.R_32F):
        assert f(handle.ptr, dt, 0, None, None, None) == _lib.STATUS_SUCCESS
        assert f(handle.ptr, dt, -1, p(idx), p(a), p(b)) == _lib.STATUS_INVALID_VALUE
        for args in ((None, p(a), p(b)), (p(idx), None, p(b)), (p(idx), p(a), None)):
            assert f(handle.ptr, dt, 4, *args) == _lib.STATUS_INVALID_VALUE
    assert f(handle.ptr, 2, 4, p(idx), p(a), p(b)) == _lib.STATUS_INVALID_VALUE
    torch.cuda.synchronize()
    assert torch.all(b == SENTINEL)
    assert f(handle.ptr, _lib.R_64F, 4, p(idx), p(a), p(b)) == _lib.STATUS_SUCCESS
    torch.cuda.synchronize()
    assert torch.all(b == 0.0)
