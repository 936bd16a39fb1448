"""GPU parity of the packed staged SpMV tiles (12-bit slot fields and 16-bit
row offsets in the plan's own record; csrc/spmv_pack.h, RSP_SPMV_PACK): every
y is compared bit for bit with the oracle's canonical summation order
(oracle_bind.spmv(..., order="canon")), which does not know about tiles,
records or the knob. The patterns are those of tests/test_spmv_plan_packed.py,
whose host checks decode the same records without a device."""
import functools

import numpy as np
import pytest
import torch

import oracle_bind as ob
from respasol_amd import csr
from respasol_amd.sparse import Handle, SpMat, SpmvBatch, upload_csr
from test_spmv_plan_packed import EDGE, OTHERS, R32, R64, STENCILS, band_cycle, edge_matrix, stats

pytestmark = pytest.mark.gpu
NP = {torch.float64: np.float64, torch.float32: np.float32}
RDT = {torch.float64: R64, torch.float32: R32}
# dtype, FTZ
FORMS = [(torch.float64, False), (torch.float32, False), (torch.float32, True)]


@pytest.fixture(autouse=True, params=[1, 2], ids=["pack1", "pack2"])
def pack_mode(request, monkeypatch):
    """Every case runs with the slot fields alone and with the packed row
    offsets too (the default)."""
    monkeypatch.setenv("RSP_SPMV_PACK", str(request.param))
    return request.param


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    h = Handle()
    yield h
    h.set_ftz(False)
    h.close()


def bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def surrogate(spec):
    return csr.surrogate(spec)


_XS, _CANON = {}, {}


def x_of(A):
    if id(A) not in _XS:
        _XS[id(A)] = (A, csr.dlarnv(2, [0, 0, 0, 1], A.n)[0])
    return _XS[id(A)][1]


def canon(A, dtype, ftz=False):
    """The oracle's canonical-order y of A x, computed once per (matrix, form)."""
    key = (id(A), dtype, ftz)
    if key not in _CANON:
        y = ob.spmv(A.rowptr, A.colidx, A.values.astype(NP[dtype]), x_of(A).astype(NP[dtype]), ftz=ftz,
                    order="canon")
        y.setflags(write=False)
        _CANON[key] = (A, y)
    return _CANON[key][1]


def device_matrix(handle, A, dtype, shift=0):
    """A on the device; shift = 1: colidx and values are views one element into
    their buffers, so neither is 16-byte aligned (vector_ok = 0)."""
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dtype)
    if shift:
        ci = torch.cat([ci.new_zeros(shift), ci])[shift:]
        va = torch.cat([va.new_zeros(shift), va])[shift:]
        assert ci.data_ptr() % 16 and va.data_ptr() % 16
    mat = SpMat(handle, rp, ci, va, A.n, nnz=max(A.nnz, A.nnz_stored))
    xd = torch.from_numpy(x_of(A).astype(NP[dtype])).cuda()
    return mat, xd


def gpu_y(handle, A, dtype, ftz=False, shift=0):
    handle.set_ftz(ftz)
    mat, xd = device_matrix(handle, A, dtype, shift)
    y = mat.spmv(xd).cpu().numpy()
    handle.set_ftz(False)
    mat.close()
    return y


def assert_canon(handle, A, dtype, ftz=False, shift=0):
    y = gpu_y(handle, A, dtype, ftz, shift)
    assert np.array_equal(bits(y), bits(canon(A, dtype, ftz))), "canonical-order mismatch"


@pytest.mark.parametrize("dtype,ftz", FORMS)
@pytest.mark.parametrize("spec", STENCILS)
def test_full_staged_tiles(handle, spec, dtype, ftz, pack_mode):
    A = surrogate(spec)
    s = stats(A, RDT[dtype])
    assert s["packed_tiles"] > 0.9 * s["tiles"] and (s["packed_rowoff_bytes"] > 0) == (pack_mode == 2)
    assert_canon(handle, A, dtype, ftz)


@pytest.mark.parametrize("dtype,ftz", FORMS)
def test_batch_mixes_packed_and_unpacked(handle, dtype, ftz):
    """Two stencils (packed tiles), a circuit and a random band (unpacked
    tiles) in launches of three matrices each, then alpha = 2, beta = 0.5."""
    specs = (STENCILS[0], OTHERS[0], STENCILS[1]), (STENCILS[1], OTHERS[1], STENCILS[0])
    assert stats(surrogate(OTHERS[0]), RDT[dtype])["packed_tiles"] < stats(surrogate(OTHERS[0]), RDT[dtype])["tiles"]
    handle.set_ftz(ftz)
    for trio in specs:
        As = [surrogate(s) for s in trio]
        pairs = [device_matrix(handle, A, dtype) for A in As]
        mats, xs = [p[0] for p in pairs], [p[1] for p in pairs]
        ys = [torch.full((A.m,), float("nan"), dtype=dtype, device="cuda") for A in As]
        b = SpmvBatch(handle, mats, xs, ys)
        b.run()
        got = [y.cpu().numpy() for y in ys]
        for A, y in zip(As, got):
            assert np.array_equal(bits(y), bits(canon(A, dtype, ftz))), "batch: canonical-order mismatch"
        if not ftz:  # y = 2 A x + 0.5 y (both scalings exact): on top of the first result
            b.run(2.0, 0.5)
            for A, y, y0 in zip(As, ys, got):
                want = NP[dtype](2.0) * canon(A, dtype) + NP[dtype](0.5) * y0
                assert np.array_equal(bits(y.cpu().numpy()), bits(want)), "batch alpha/beta mismatch"
        b.close()
        for m in mats:
            m.close()
    handle.set_ftz(False)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_alpha_beta_single(handle, dtype):
    A = surrogate(STENCILS[0])
    mat, xd = device_matrix(handle, A, dtype)
    y0 = np.random.default_rng(2).uniform(-1, 1, A.m).astype(NP[dtype])
    got = mat.spmv(xd, torch.from_numpy(y0.copy()).cuda(), 2.0, 0.5).cpu().numpy()
    want = NP[dtype](2.0) * canon(A, dtype) + NP[dtype](0.5) * y0
    assert np.array_equal(bits(got), bits(want))
    mat.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_partial_vectors(handle, dtype):
    """Row lengths 1 .. 9: packed tiles begin and end inside a 16-byte vector."""
    A = band_cycle()
    s = stats(A, RDT[dtype])
    assert s["packed_tiles"] > 0.9 * s["tiles"]
    vw = 16 // np.dtype(NP[dtype]).itemsize
    assert np.count_nonzero(np.asarray(A.rowptr) % vw) > A.m // 4
    assert_canon(handle, A, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_eligibility_edge(handle, dtype):
    for last, packed in zip(EDGE[RDT[dtype]], (False, True)):
        A, _ = edge_matrix(last, RDT[dtype])
        assert stats(A, RDT[dtype])["packed_tiles"] == 1 + packed
        assert_canon(handle, A, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_end_of_arrays_scalar_path(handle, dtype):
    """The last tile is packed in the plan, but the entry count is not a
    multiple of the vector width: it takes the scalar path, which reads the
    int32 colidx and the caller's row offsets."""
    A, _ = edge_matrix(EDGE[RDT[dtype]][1], RDT[dtype], 1)
    assert A.nnz_stored % (16 // np.dtype(NP[dtype]).itemsize) == 1
    assert stats(A, RDT[dtype])["packed_tiles"] == 2
    assert_canon(handle, A, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_unaligned_arrays_ignore_the_record(handle, dtype):
    for A in (surrogate(STENCILS[0]), edge_matrix(EDGE[RDT[dtype]][1], RDT[dtype])[0]):
        assert_canon(handle, A, dtype, shift=1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_split_schedule(handle, dtype):
    """set_local_cols: part 1 then part 2 equals one whole SpMV bit for bit."""
    A = surrogate(STENCILS[0])
    mat, xd = device_matrix(handle, A, dtype)
    whole = mat.spmv(xd).cpu().numpy()
    mat.set_local_cols(A.n * 3 // 4)
    y = torch.full((A.m,), float("nan"), dtype=dtype, device="cuda")
    mat.spmv_part(xd, y, 1)
    mat.spmv_part(xd, y, 2)
    got = y.cpu().numpy()
    assert np.array_equal(bits(got), bits(whole)) and np.array_equal(bits(got), bits(canon(A, dtype)))
    mat.close()


@pytest.mark.parametrize("dtype,ftz", FORMS)
def test_knob_same_bits(handle, dtype, ftz, monkeypatch):
    A = surrogate(STENCILS[1])
    for mode in (0, 1, 2):
        monkeypatch.setenv("RSP_SPMV_PACK", str(mode))
        s = stats(A, RDT[dtype])
        assert (s["packed_tiles"] == 0) == (mode == 0) and (s["packed_rowoff_bytes"] > 0) == (mode == 2)
        assert_canon(handle, A, dtype, ftz)


def test_replan_and_shared_workspace(handle, monkeypatch):
    """A re-plan with another knob value (rsp_spmv_preprocess) and two matrices
    sharing one workspace keep their bits."""
    A, B = surrogate(STENCILS[0]), band_cycle()
    ma, xa = device_matrix(handle, A, torch.float64)
    mb, xb = device_matrix(handle, B, torch.float64)
    mb.buffer = ma.buffer
    for mode in (2, 0, 1, 2):
        monkeypatch.setenv("RSP_SPMV_PACK", str(mode))
        ma.set_local_cols(A.n)  # re-plans (every column local: one part)
        assert np.array_equal(bits(ma.spmv(xa).cpu().numpy()), bits(canon(A, torch.float64)))
        assert np.array_equal(bits(mb.spmv(xb).cpu().numpy()), bits(canon(B, torch.float64)))
    ma.close()
    mb.close()
