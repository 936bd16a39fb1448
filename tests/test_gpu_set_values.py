"""rsp_csr_set_values (SpMat.set_values): re-pointing a descriptor's values,
the call a mixed-precision user makes. include/rsp.h promises that the
analysis is kept, that values are read on every call, and that batches holding
the old pointer become stale; the three state rules behind that — the plan
kept for the same type, a re-plan for another type (a tile's capacity depends
on it), a new plan generation for another pointer — are each held to the
canonical-order oracle here, on a matrix with a chunked long row and one of
staged, packed tiles (abi_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_bind as ob
from abi_cases import SPMV_MATRICES, same_bits
from respasol_amd import _lib
from respasol_amd.sparse import Handle, RspError, SpMat, SpmvBatch, upload_csr

pytestmark = pytest.mark.gpu
NP = {torch.float64: np.float64, torch.float32: np.float32}
OTHER = {torch.float64: torch.float32, torch.float32: torch.float64}
MATRICES = sorted(SPMV_MATRICES)
_REF = {}


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    h = Handle()
    yield h
    h.close()


def values_of(name, which):
    """The matrix's own values (which = 0) or a seeded other set."""
    A = SPMV_MATRICES[name]()
    return A.values if which == 0 else np.random.default_rng(40 + which).uniform(-2, 2, A.values.size)


def x_of(name):
    return np.random.default_rng(5).uniform(-1, 1, SPMV_MATRICES[name]().n)


def oracle(name, which, dtype):
    """Canonical-order A x for value set `which`, computed once."""
    key = (name, which, dtype)
    if key not in _REF:
        A = SPMV_MATRICES[name]()
        y = ob.spmv(A.rowptr, A.colidx, values_of(name, which).astype(NP[dtype]), x_of(name).astype(NP[dtype]),
                    order="canon")
        y.setflags(write=False)
        _REF[key] = y
    return _REF[key]


def on_device(a, dtype, shift=0):
    """a as `dtype` on the device, `shift` elements past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a).astype(NP[dtype])).cuda()
    if shift:
        t = torch.cat([t.new_zeros(shift), t])[shift:]
        assert t.data_ptr() % 16 == shift * t.element_size()
    else:
        assert t.data_ptr() % 16 == 0
    return t


def descriptor(handle, name, dtype, which=0):
    A = SPMV_MATRICES[name]()
    rp, ci, _ = upload_csr(A.rowptr, A.colidx, A.values, dtype)
    return SpMat(handle, rp, ci, on_device(values_of(name, which), dtype), A.n), on_device(x_of(name), dtype)


def product(M, x):
    return M.spmv(x, torch.full((M.m,), float("nan"), dtype=M.dtype, device="cuda")).cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", MATRICES)
def test_same_type_other_pointer_keeps_the_plan(handle, name, dtype):
    M, x = descriptor(handle, name, dtype)
    assert same_bits(product(M, x), oracle(name, 0, dtype))
    info = M.plan_info()
    M.set_values(on_device(values_of(name, 1), dtype))
    assert M.plan_info() == info  # no re-plan: rsp_spmv_plan_info needs no new SpMV first
    assert same_bits(product(M, x), oracle(name, 1, dtype))
    assert M.plan_info() == info
    # one element past the alignment: the scalar path of the same schedule, the same bits
    M.set_values(on_device(values_of(name, 1), dtype, shift=1))
    assert M.plan_info() == info
    assert same_bits(product(M, x), oracle(name, 1, dtype))
    M.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", MATRICES)
def test_values_changed_in_place_are_read(handle, name, dtype):
    """Same pointer, no call: "values may [change]: they are read on every call"."""
    M, x = descriptor(handle, name, dtype)
    assert same_bits(product(M, x), oracle(name, 0, dtype))
    M.values.copy_(on_device(values_of(name, 2), dtype))
    assert same_bits(product(M, x), oracle(name, 2, dtype))
    M.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_batches_go_stale_on_another_pointer_only(handle, dtype):
    mats, xs = zip(*(descriptor(handle, name, dtype) for name in MATRICES))
    ys = [torch.full((M.m,), float("nan"), dtype=dtype, device="cuda") for M in mats]
    B = SpmvBatch(handle, list(mats), list(xs), ys)
    B.run()
    for name, y in zip(MATRICES, ys):
        assert same_bits(y.cpu().numpy(), oracle(name, 0, dtype))
    mats[0].set_values(mats[0].values)  # the identical pointer and type: still the batch's
    for y in ys:
        y.fill_(float("nan"))
    B.run()
    for name, y in zip(MATRICES, ys):
        assert same_bits(y.cpu().numpy(), oracle(name, 0, dtype))
    old = mats[1].values
    mats[1].set_values(on_device(values_of(MATRICES[1], 1), dtype))
    with pytest.raises(RspError) as e:
        B.run()
    assert e.value.status == _lib.STATUS_INVALID_VALUE
    mats[1].set_values(old)  # the old pointer again is still a re-point: the batch stays stale
    with pytest.raises(RspError) as e:
        B.run()
    assert e.value.status == _lib.STATUS_INVALID_VALUE
    B.close()
    B = SpmvBatch(handle, list(mats), list(xs), ys)  # a new batch holds the current pointers
    B.run()
    for name, y in zip(MATRICES, ys):
        assert same_bits(y.cpu().numpy(), oracle(name, 0, dtype))
    B.close()
    for M in mats:
        M.close()


@pytest.mark.parametrize("first", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", MATRICES)
def test_type_change_replans(handle, name, first):
    """T -> the other type -> T: each step has the bits of a fresh descriptor
    of that type and of the oracle; the tile count follows the type and comes
    back; a call with the type the descriptor had before is INVALID_VALUE and
    writes nothing."""
    second = OTHER[first]
    fresh, tiles = {}, {}
    for dt in (first, second):
        F, x = descriptor(handle, name, dt)
        fresh[dt] = product(F, x)
        tiles[dt] = F.plan_info()["tiles"]
        assert same_bits(fresh[dt], oracle(name, 0, dt))
        F.close()
    assert tiles[first] != tiles[second]
    M, _ = descriptor(handle, name, first)
    xs = {dt: on_device(x_of(name), dt) for dt in (first, second)}
    assert same_bits(product(M, xs[first]), fresh[first]) and M.plan_info()["tiles"] == tiles[first]
    for dt, stale in ((second, first), (first, second)):
        M.set_values(on_device(values_of(name, 0), dt))
        with pytest.raises(RspError) as e:  # the other type's schedule is gone, not reported as current
            M.plan_info()
        assert e.value.status == _lib.STATUS_NOT_INITIALIZED
        y = torch.full((M.m,), float("nan"), dtype=stale, device="cuda")
        one, zero = (C.c_double(1.0), C.c_double(0.0)) if stale == torch.float64 else (C.c_float(1.0), C.c_float(0.0))
        st = _lib.rsp.rsp_spmv(handle.ptr, _lib.OP_N, C.byref(one), M._mat, C.c_void_p(xs[stale].data_ptr()),
                               C.byref(zero), C.c_void_p(y.data_ptr()), _lib.R_64F if stale == torch.float64
                               else _lib.R_32F, None)
        assert st == _lib.STATUS_INVALID_VALUE
        assert torch.isnan(y).all()
        assert same_bits(product(M, xs[dt]), fresh[dt])
        assert M.plan_info()["tiles"] == tiles[dt]
    M.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("name", MATRICES)
def test_split_schedule_after_a_repoint(handle, name, dtype):
    """set_local_cols, then other values (and then the other type): part 1 +
    part 2 equals part 0 and the oracle for the values in place."""
    M, x = descriptor(handle, name, dtype)
    M.set_local_cols(M.n * 3 // 4)
    for dt, which in ((dtype, 1), (OTHER[dtype], 2)):
        M.set_values(on_device(values_of(name, which), dt))
        xd = on_device(x_of(name), dt)
        whole = product(M, xd)
        y = torch.full((M.m,), float("nan"), dtype=dt, device="cuda")
        M.spmv_part(xd, y, 1)
        M.spmv_part(xd, y, 2)
        assert same_bits(y.cpu().numpy(), whole) and same_bits(whole, oracle(name, which, dt))
    M.close()


def test_arguments(handle):
    M, x = descriptor(handle, MATRICES[0], torch.float64)
    v = C.c_void_p(M.values.data_ptr())
    assert _lib.rsp.rsp_csr_set_values(None, v, _lib.R_64F) == _lib.STATUS_INVALID_VALUE
    for bad in (-1, 2, 7):
        assert _lib.rsp.rsp_csr_set_values(M._mat, v, bad) == _lib.STATUS_INVALID_VALUE
    info = M.plan_info()
    assert same_bits(product(M, x), oracle(MATRICES[0], 0, torch.float64))  # the rejected calls changed nothing
    assert M.plan_info() == info
    with pytest.raises(TypeError):
        M.set_values(M.values.to(torch.float16))
    M.close()
