"""Randomised GPU parity of the CSR SpMV (seeded, reproducible): matrices
whose row-length mixtures and column patterns are drawn per seed — empty
rows, short rows, 33-256-entry rows among short ones (the reduce's
eight-lanes-per-row pass), rows longer than a tile (chunked, finished by
the last-arriving chunk), uniform, banded and clustered columns — each
checked bit for bit against the oracle's canonical order, fp64 and fp32, as
single calls and all together as one batched launch. The rectangular
matrices (random_rect_matrix: the multi-GPU slices' shape, rows x (local +
halo) columns) go the same way; tests/test_spmv_plan.py holds them to
covering every kind of tile."""
import functools

import numpy as np
import pytest
import torch

import oracle_bind as ob
from respasol_amd import csr
from respasol_amd.sparse import Handle, SpMat, SpmvBatch, upload_csr

pytestmark = pytest.mark.gpu
NP = {torch.float64: np.float64, torch.float32: np.float32}
SEEDS = range(12)


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64 if a.dtype == np.float64 else np.uint32),
                          b.view(np.uint64 if b.dtype == np.float64 else np.uint32))


def random_matrix(seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.choice([1, 7, 300, 5000, 40000]))
    # row lengths: a mixture of classes, weights drawn per seed
    w = rng.dirichlet(np.ones(4)) * np.array([1.0, 4.0, 1.0, 0.05 if n >= 5000 else 0.0])
    w /= w.sum()
    cls = rng.choice(4, n, p=w)
    lens = np.select([cls == 0, cls == 1, cls == 2, cls == 3],
                     [0, rng.integers(1, 9, n), rng.integers(17, 257, n), rng.integers(300, 9000, n)])
    lens = np.minimum(lens, n).astype(np.int64)
    pattern = seed % 3  # 0 uniform, 1 banded, 2 clustered
    row = np.repeat(np.arange(n), lens)
    if pattern == 0:
        col = rng.integers(0, n, row.size)
    elif pattern == 1:
        width = max(8, n // 50)
        col = np.clip(row + rng.integers(-width, width + 1, row.size), 0, n - 1)
    else:
        centers = rng.integers(0, n, max(1, n // 100))
        col = np.clip(centers[rng.integers(0, centers.size, row.size)] + rng.integers(-64, 65, row.size), 0, n - 1)
    key = np.unique(row.astype(np.int64) * n + col)
    row, col = key // n, key % n
    if n >= 5000:  # a few rows longer than a tile (fp64 2047 / fp32 4093 entries): chunked
        hubs = rng.choice(n, int(rng.integers(1, 6)), replace=False)
        keep = ~np.isin(row, hubs)
        row, col = row[keep], col[keep]
        extra_r = [np.full(int(k), h) for h, k in zip(hubs, rng.integers(2100, min(n, 12000), hubs.size))]
        extra_c = [np.sort(rng.choice(n, r.size, replace=False)) for r in extra_r]
        row = np.concatenate([row] + extra_r)
        col = np.concatenate([col] + extra_c)
        order = np.lexsort((col, row))
        row, col = row[order], col[order]
    rp = np.zeros(n + 1, np.int32)
    np.add.at(rp, row + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    vals = rng.uniform(-1, 1, col.size)
    return csr.CsrMatrix(0, n, n, int(col.size), rp, col.astype(np.int32), vals)


@pytest.mark.parametrize("variant", [0, 512, 1056])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_random_matrices_single_and_batched(monkeypatch, dtype, variant):
    """variant: RSP_SPMV_VARIANT of the handle — 0 the shipped schedule, 512
    small plans spread over every resident slot, 1056 = int32 column
    indices only (32) and no staged tiles (1024): the same bits every time."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    monkeypatch.setenv("RSP_SPMV_VARIANT", str(variant))
    handle = Handle()
    mats, xs, refs, ys = [], [], [], []
    for seed in SEEDS:
        A = random_matrix(seed)
        x = np.random.default_rng(seed).uniform(-1, 1, A.n)
        v, xx = A.values.astype(NP[dtype]), x.astype(NP[dtype])
        canon = ob.spmv(A.rowptr, A.colidx, v, xx, order="canon")
        rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dtype)
        M = SpMat(handle, rp, ci, va, A.n)
        xd = torch.from_numpy(xx).cuda()
        y = M.spmv(xd).cpu().numpy()
        assert same_bits(y, canon), (seed, A.n, A.nnz_stored)
        mats.append(M)
        xs.append(xd)
        refs.append(canon)
        ys.append(torch.empty(A.m, dtype=dtype, device="cuda"))
    B = SpmvBatch(handle, mats, xs, ys)
    B.run(1.0, 0.0)
    torch.cuda.synchronize()
    for seed, (r, y) in enumerate(zip(refs, ys)):
        assert same_bits(y.cpu().numpy(), r), seed
    B.close()
    handle.close()


# rows x cols of the rectangular matrices: one row, fewer columns than a row
# has lanes, cols past 2 x 65536, a tall slice, and a multi-GPU slice's shape
# (rows_local x (local + halo))
RECT_SHAPES = [(1, 70000), (300, 7), (5000, 131075), (40000, 300), (6000, 66000)]
RECT_SEEDS = range(len(RECT_SHAPES))
LONG_ROW = 4200  # past a tile of either type (fp64 2047 / fp32 4093 entries)


@functools.lru_cache(maxsize=None)
def random_rect_matrix(seed):
    """RECT_SHAPES[seed] with the square generator's row-length mixture; the
    columns uniform over all of them (seed % 3 == 0: tiles spanning >= 65536
    columns keep int32 indices), in a band around the scaled diagonal (1) or
    clustered (2); where cols allows it, 1-3 rows longer than a tile."""
    m, cols = RECT_SHAPES[seed]
    rng = np.random.default_rng(3000 + seed)
    w = rng.dirichlet(np.ones(4)) * np.array([1.0, 4.0, 1.0, 0.05 if cols >= 5000 else 0.0])
    w /= w.sum()
    cls = rng.choice(4, m, p=w)
    lens = np.select([cls == 0, cls == 1, cls == 2, cls == 3],
                     [0, rng.integers(1, 9, m), rng.integers(17, 257, m), rng.integers(300, 9000, m)])
    lens = np.minimum(lens, cols).astype(np.int64)
    pattern = seed % 3
    row = np.repeat(np.arange(m), lens)
    if pattern == 0:
        col = rng.integers(0, cols, row.size)
    elif pattern == 1:
        width = max(8, cols // 50)
        col = np.clip(row * cols // m + rng.integers(-width, width + 1, row.size), 0, cols - 1)
    else:
        centers = rng.integers(0, cols, max(1, cols // 100))
        col = np.clip(centers[rng.integers(0, centers.size, row.size)] + rng.integers(-64, 65, row.size),
                      0, cols - 1)
    key = np.unique(row.astype(np.int64) * cols + col)
    row, col = key // cols, key % cols
    if cols > LONG_ROW:
        hubs = rng.choice(m, min(m, int(rng.integers(1, 4))), replace=False)
        keep = ~np.isin(row, hubs)
        row, col = row[keep], col[keep]
        extra_r = [np.full(int(k), h) for h, k in zip(hubs, rng.integers(LONG_ROW, min(cols, 12000), hubs.size))]
        extra_c = [np.sort(rng.choice(cols, r.size, replace=False)) for r in extra_r]
        row = np.concatenate([row] + extra_r)
        col = np.concatenate([col] + extra_c)
        order = np.lexsort((col, row))
        row, col = row[order], col[order]
    rp = np.zeros(m + 1, np.int64)
    np.add.at(rp, row + 1, 1)
    rp = np.cumsum(rp).astype(np.int32)
    vals = rng.uniform(-1, 1, col.size)
    return csr.CsrMatrix(0, m, cols, int(col.size), rp, col.astype(np.int32), vals)


@functools.lru_cache(maxsize=None)
def rect_case(seed, dtype):
    """(matrix, x, the canonical-order oracle's y), computed once."""
    A = random_rect_matrix(seed)
    x = np.random.default_rng(seed).uniform(-1, 1, A.n).astype(NP[dtype])
    y = ob.spmv(A.rowptr, A.colidx, A.values.astype(NP[dtype]), x, order="canon")
    y.setflags(write=False)
    return A, x, y


def rect_on_device(handle, seed, dtype):
    A, x, canon = rect_case(seed, dtype)
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dtype)
    return A, SpMat(handle, rp, ci, va, A.n), torch.from_numpy(x).cuda(), canon


@pytest.mark.parametrize("seed", RECT_SEEDS, ids=[f"{m}x{c}" for m, c in RECT_SHAPES])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rectangular_single(dtype, seed):
    """rows != cols: x has cols elements, y rows; a tile's decoded 16-bit
    columns are clamped to cols - 1 (not rows - 1). The slice shape also split
    at its own columns (set_local_cols): parts 1 + 2 give the whole product."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    handle = Handle()
    A, M, xd, canon = rect_on_device(handle, seed, dtype)
    assert (A.m, A.n) == RECT_SHAPES[seed] and xd.numel() == A.n
    y = torch.full((A.m,), float("nan"), dtype=dtype, device="cuda")
    assert same_bits(M.spmv(xd, y, 1.0, 0.0).cpu().numpy(), canon), (A.m, A.n, A.nnz_stored)
    if RECT_SHAPES[seed] == (6000, 66000):
        whole = y.cpu().numpy()
        M.set_local_cols(6000)
        assert same_bits(M.spmv(xd).cpu().numpy(), whole)  # part 0 of the split schedule
        y = torch.full((A.m,), float("nan"), dtype=dtype, device="cuda")
        M.spmv_part(xd, y, 1)
        assert torch.isnan(y).any() and not torch.isnan(y).all()  # both parts hold rows
        M.spmv_part(xd, y, 2)
        assert same_bits(y.cpu().numpy(), whole)
    M.close()
    handle.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rectangular_batched(dtype):
    """All five shapes as one batched launch: the bits of the single calls."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    handle = Handle()
    cases = [rect_on_device(handle, seed, dtype) for seed in RECT_SEEDS]
    ys = [torch.full((A.m,), float("nan"), dtype=dtype, device="cuda") for A, _, _, _ in cases]
    B = SpmvBatch(handle, [c[1] for c in cases], [c[2] for c in cases], ys)
    B.run(1.0, 0.0)
    torch.cuda.synchronize()
    for seed, (case, y) in enumerate(zip(cases, ys)):
        assert same_bits(y.cpu().numpy(), case[3]), RECT_SHAPES[seed]
    B.close()
    for _, M, _, _ in cases:
        M.close()
    handle.close()
