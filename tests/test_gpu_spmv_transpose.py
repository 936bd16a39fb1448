"""rsp_spmv(op = TRANSPOSE), rsp_csr2csc and the lifecycle of a matrix's
transposed side (include/rsp.h), for fp64, fp32 and fp32 + FTZ.

Expected value everywhere: A^T built in numpy as the stable sort of A's stored
entries by column (the order the header defines), its row sums s from the
canonical-order oracle (oracle_bind.spmv(..., order="canon"), ftz as the case),
alpha / beta by spmv_epilogue_ref.epilogue, compared bit for bit, NaN payloads
included. Every reference is computed once and shared (read-only arrays).

The tall case (5000 x 300) makes the schedule of A^T meet every row kind:
column 7 is in every row (an A^T row of 5000 entries: chunked in both types),
column 8 in 300 rows (the whole-row reduce), columns 20-29 are empty, the rest
hold 0-8 entries; some stored rows are unsorted and one entry is duplicated.
Columns 40 and 41 hold one entry each: a denormal value, and a 1.0 that meets a
denormal of x, so the FTZ result differs from the IEEE one (asserted). The
mirror case (300 x 5000) gives many short A^T rows, empty ones included.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_bind as ob
from abi_cases import same_bits
from respasol_amd import _lib
from respasol_amd.sparse import Handle, RspError, SpMat, csr2csc
from spmv_epilogue_ref import epilogue
from test_gpu_streams import both, ctx, late_input  # noqa: F401  (ctx: the side-stream fixture)

pytestmark = pytest.mark.gpu

CONFIGS = {"fp64": (torch.float64, False), "fp32": (torch.float32, False), "fp32_ftz": (torch.float32, True)}
NP = {torch.float64: np.float64, torch.float32: np.float32}
OTHER = {torch.float64: torch.float32, torch.float32: torch.float64}
SCALARS = [(1.0, 0.0), (-0.5, 0.0), (2.0, 1.0), (1.0, -0.0)]
DENORMAL_VALUE, DENORMAL_X = 2.0 ** -130, 2.0 ** -140  # fp32 denormals (normal numbers in fp64)


class Case:
    """A host CSR matrix (rows x cols), its numpy transpose, x (rows) and y0 (cols)."""

    def __init__(self, rows, cols, rp, ci, values, x, y0, tail=0):
        self.rows, self.cols = rows, cols
        self.nnz = int(rp[-1]) if rows > 0 else 0
        # `tail`: entries past rowptr[rows], as a caller's nnz larger than the pattern (never read)
        self.rp = np.ascontiguousarray(rp, np.int32)
        self.ci = np.concatenate([ci, np.full(tail, cols + 3)]).astype(np.int32)
        self.values = np.concatenate([values, np.full(tail, np.nan)])
        self.x, self.y0 = x, y0
        order = np.argsort(self.ci[:self.nnz], kind="stable")
        self.perm = order.astype(np.int32)
        self.t_ci = np.repeat(np.arange(rows), np.diff(self.rp.astype(np.int64)))[order].astype(np.int32)
        self.t_rp = np.zeros(cols + 1, np.int32)
        np.cumsum(np.bincount(self.ci[:self.nnz], minlength=cols), out=self.t_rp[1:])
        for a in (self.rp, self.ci, self.values, self.x, self.y0, self.perm, self.t_ci, self.t_rp):
            a.setflags(write=False)
        self._s = {}

    def s(self, dtype, ftz, values=None, x=None):
        """The canonical row sums of A^T (cached for the case's own data)."""
        key = (dtype, ftz) if values is None and x is None else None
        if key in self._s:
            return self._s[key]
        v = (self.values if values is None else values)[:self.nnz][self.perm].astype(NP[dtype])
        out = ob.spmv(self.t_rp, self.t_ci, v, (self.x if x is None else x).astype(NP[dtype]), ftz=ftz, order="canon")
        out.setflags(write=False)
        if key is not None:
            self._s[key] = out
        return out

    def expect(self, dtype, ftz, alpha=1.0, beta=0.0, y0=None, values=None, x=None):
        y0 = self.y0 if y0 is None else y0
        return epilogue(self.s(dtype, ftz, values, x), y0.astype(NP[dtype]), alpha, beta)


def finish(rows, cols, per_row, rng, singles, dup_col=None):
    """per_row column lists -> a Case: every fifth row of >= 2 entries is
    stored unsorted, one entry is duplicated (of dup_col, or any), the two
    single-entry columns get the denormal value and the denormal of x."""
    for i, c in enumerate(per_row):
        c.sort()
        if i % 5 == 0 and len(c) >= 2:
            per_row[i] = [int(v) for v in rng.permutation(c)]
    dup = next(i for i, c in enumerate(per_row) if len(c) >= 3 and i not in singles.values())
    per_row[dup].append(per_row[dup][1] if dup_col is None else dup_col)
    rp = np.zeros(rows + 1, np.int32)
    np.cumsum([len(c) for c in per_row], out=rp[1:])
    ci = np.array([c for row in per_row for c in row], np.int32)
    assert any(list(c) != sorted(c) for c in per_row)
    values = rng.uniform(-1, 1, len(ci))
    x = rng.uniform(-1, 1, rows)
    (c_val, r_val), (c_x, r_x) = sorted(singles.items())
    assert (ci == c_val).sum() == 1 and (ci == c_x).sum() == 1
    values[np.flatnonzero(ci == c_val)[0]] = DENORMAL_VALUE
    x[r_val] = 0.75
    values[np.flatnonzero(ci == c_x)[0]] = 1.0
    x[r_x] = DENORMAL_X
    return Case(rows, cols, rp, ci, values, x, rng.uniform(-1, 1, cols))


@functools.lru_cache(maxsize=None)
def tall_case():
    rows, cols = 5000, 300
    rng = np.random.default_rng(71)
    singles = {40: rows // 3, 41: rows // 2}
    per_row = [[7] for _ in range(rows)]
    for i in rng.choice(rows, 300, replace=False):
        per_row[i].append(8)
    for c in range(cols):
        if c in (7, 8) or 20 <= c <= 29:
            continue
        for i in ([singles[c]] if c in singles else rng.choice(rows, int(rng.integers(0, 9)), replace=False)):
            per_row[i].append(c)
    case = finish(rows, cols, per_row, rng, singles, dup_col=7)
    lens = np.diff(case.t_rp)
    caps = [ob.TILE_CAP[np.dtype(t)] for t in (np.float64, np.float32)]
    assert lens[7] == rows + 1 > max(caps)            # chunked in both types (the duplicate is column 7's)
    assert 256 < lens[8] == 300 <= min(caps)          # a whole long row
    assert (lens[20:30] == 0).all() and lens[40] == lens[41] == 1
    assert set(np.delete(lens, [7, 8])) >= set(range(9)) and np.delete(lens, [7, 8]).max() <= 8
    return case


@functools.lru_cache(maxsize=None)
def mirror_case():
    rows, cols = 300, 5000
    rng = np.random.default_rng(72)
    singles = {40: 3, 41: 6}
    pool = np.setdiff1d(np.arange(cols), np.concatenate([np.arange(100, 200), [40, 41]]))
    per_row = [list(rng.choice(pool, int(rng.integers(0, 40)), replace=False)) for _ in range(rows)]
    for c, i in singles.items():
        per_row[i].append(c)
    case = finish(rows, cols, per_row, rng, singles)
    lens = np.diff(case.t_rp)
    assert (lens[100:200] == 0).all() and (lens == 0).sum() > 200 and 2 <= lens.max() <= 32
    return case


@functools.lru_cache(maxsize=None)
def small_case(rows, cols, nnz, tail=0):
    """nnz random entries (unsorted rows, duplicates as they fall)."""
    rng = np.random.default_rng(1000 * rows + 10 * cols + nnz)
    r = np.sort(rng.integers(0, max(rows, 1), nnz))
    rp = np.zeros(rows + 1, np.int32)
    np.cumsum(np.bincount(r, minlength=rows)[:rows], out=rp[1:])
    ci = rng.integers(0, max(cols, 1), nnz).astype(np.int32)
    return Case(rows, cols, rp, ci, rng.uniform(-1, 1, nnz), rng.uniform(-1, 1, rows), rng.uniform(-1, 1, cols), tail)


CASES = {"tall": tall_case, "mirror": mirror_case}


@pytest.fixture(scope="module")
def handles():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    hs = {False: Handle(), True: Handle(ftz=True)}
    yield hs
    for h in hs.values():
        h.close()


def dev(a, dtype=None, shift=0):
    t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the cases' arrays are read-only)
    t = t if dtype is None else t.to(dtype)
    if shift:  # a slice starting `shift` elements into an allocation
        t = torch.cat([t.new_zeros(shift), t])[shift:]
        assert t.data_ptr() % 16 == shift * t.element_size()
    return t


def descriptor(h, case, dtype, values=None, shift=0):
    rp, ci = dev(case.rp), dev(case.ci)
    va = dev((case.values if values is None else values).astype(NP[dtype]), shift=shift)
    return SpMat(h, rp, ci, va, case.cols)


def product_t(M, x, alpha=1.0, beta=0.0, y0=None):
    """op = T into a y holding y0, or NaN where the call may not read it."""
    y = torch.full((M.n,), float("nan"), dtype=M.dtype, device="cuda") if y0 is None else dev(y0, M.dtype)
    return M.spmv(x, y, alpha, beta, transpose=True).cpu().numpy()


def product_n(M, x):
    return M.spmv(x, torch.full((M.m,), float("nan"), dtype=M.dtype, device="cuda")).cpu().numpy()


# ------------------------------------------------------------ the products

@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(CASES))
def test_transposed_product_every_scalar(handles, name, cfg):
    dtype, ftz = CONFIGS[cfg]
    case = CASES[name]()
    if ftz:  # the case cannot pass vacuously: flushing changes the expectation
        assert not same_bits(case.expect(dtype, True), case.expect(dtype, False))
        assert case.expect(dtype, True)[40] == 0 and case.expect(dtype, False)[40] != 0
    M = descriptor(handles[ftz], case, dtype)
    x = dev(case.x, dtype)
    for alpha, beta in SCALARS:
        ignored = beta == 0  # of either sign: y is write-only, the NaN in it is ignored
        y = product_t(M, x, alpha, beta, None if ignored else case.y0)
        want = case.expect(dtype, ftz, alpha, beta)
        assert same_bits(y, want), (name, cfg, alpha, beta, int((y != want).sum()))
        assert not np.isnan(y[np.isfinite(case.s(dtype, ftz))]).any()
    M.close()


DEGENERATE = {
    "nnz0": lambda: small_case(5, 4, 0),
    "one": lambda: small_case(1, 1, 1),
    "nnz_4k+1": lambda: small_case(7, 5, 9),
    "nnz_4k+2": lambda: small_case(7, 5, 10),
    "nnz_4k+3": lambda: small_case(7, 5, 11),
    "nnz_3": lambda: small_case(4, 6, 3),          # less than one vector
    "blocks_tail": lambda: small_case(64, 48, 2051),  # more than one workgroup in both types, odd, 4k + 3
    "caller_nnz_larger": lambda: small_case(9, 7, 20, tail=5),
    "no_rows": lambda: small_case(0, 6, 0),
    "no_cols": lambda: small_case(6, 0, 0),
}


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_shapes(handles, name, cfg):
    dtype, ftz = CONFIGS[cfg]
    case = DEGENERATE[name]()
    M = descriptor(handles[ftz], case, dtype)
    assert M.nnz == case.nnz + (5 if name == "caller_nnz_larger" else 0)
    x = dev(case.x, dtype)
    assert same_bits(product_t(M, x), case.expect(dtype, ftz))
    assert same_bits(product_t(M, x, 2.0, 1.0, case.y0), case.expect(dtype, ftz, 2.0, 1.0))
    M.close()


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["nnz_4k+3", "blocks_tail", "tall"])
def test_values_in_a_slice(handles, name, cfg):
    """A values tensor starting one element into its allocation: aligned to its
    element only. The forward product takes its scalar path, the same bits."""
    dtype, ftz = CONFIGS[cfg]
    case = (DEGENERATE.get(name) or CASES[name])()
    M = descriptor(handles[ftz], case, dtype, shift=1)
    assert M.values.data_ptr() % 16 == M.values.element_size()
    assert same_bits(product_t(M, dev(case.x, dtype)), case.expect(dtype, ftz))
    M.close()


# ------------------------------------------- equality with the explicit path

@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["tall", "mirror", "blocks_tail", "caller_nnz_larger", "nnz0"])
def test_csr2csc_and_the_explicit_transpose(handles, name, cfg):
    dtype, ftz = CONFIGS[cfg]
    h = handles[ftz]
    case = (DEGENERATE.get(name) or CASES[name])()
    vals = case.values.astype(NP[dtype]).copy()
    if case.nnz > 2:  # bits that only a bit move keeps in every mode: a NaN payload, a denormal
        view = vals.view(np.uint64 if dtype == torch.float64 else np.uint32)
        view[0] = 0x7FF0DEADBEEF0001 if dtype == torch.float64 else 0x7FA0BEEF
        vals[1] = np.finfo(NP[dtype]).smallest_subnormal * 5
    rp, ci, va = dev(case.rp), dev(case.ci), dev(vals)
    t_rp, t_ci, t_va = csr2csc(h, rp, ci, va, case.cols)
    assert np.array_equal(t_rp.cpu().numpy(), case.t_rp) and np.array_equal(t_ci.cpu().numpy(), case.t_ci)
    assert same_bits(t_va.cpu().numpy(), vals[:case.nnz][case.perm])
    s_rp, s_ci, s_va = csr2csc(h, rp, ci, None, case.cols)  # symbolic only
    assert s_va is None and torch.equal(s_rp, t_rp) and torch.equal(s_ci, t_ci)
    # a slice as the output values: no 16-byte alignment to rely on
    out = torch.zeros(case.nnz + 2, dtype=dtype, device="cuda")
    st = _lib.rsp.rsp_csr2csc(h.ptr, case.rows, case.cols, ci.numel(), C.c_void_p(rp.data_ptr()),
                              C.c_void_p(ci.data_ptr() if ci.numel() else 0), C.c_void_p(va.data_ptr() if va.numel() else 0),
                              _lib.R_64F if dtype == torch.float64 else _lib.R_32F, C.c_void_p(s_rp.data_ptr()),
                              C.c_void_p(s_ci.data_ptr() if s_ci.numel() else 0), C.c_void_p(out.data_ptr() + out.element_size()))
    assert st == _lib.STATUS_SUCCESS
    got = out.cpu().numpy()
    assert same_bits(got[1:-1], vals[:case.nnz][case.perm]) and got[0] == 0 and got[-1] == 0
    # op = N on the explicit transpose == op = T on A (the case's own values)
    e_rp, e_ci, e_va = csr2csc(h, rp, ci, dev(case.values.astype(NP[dtype])), case.cols)
    E = SpMat(h, e_rp, e_ci, e_va, case.rows)
    M = descriptor(h, case, dtype)
    x = dev(case.x, dtype)
    y_t = product_t(M, x)
    assert same_bits(product_n(E, x), y_t) and same_bits(y_t, case.expect(dtype, ftz))
    E.close()
    M.close()


def test_csr2csc_arguments(handles):
    h = handles[False]
    case = DEGENERATE["nnz_4k+1"]()
    rp, ci, va = dev(case.rp), dev(case.ci), dev(case.values)
    o_rp = torch.full((case.cols + 1,), -7, dtype=torch.int32, device="cuda")
    o_ci = torch.full((case.nnz,), -7, dtype=torch.int32, device="cuda")
    o_va = torch.full((case.nnz,), 7.0, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(rows=case.rows, cols=case.cols, nnz=case.nnz, a=p(rp), b=p(ci), c=p(va), t=_lib.R_64F, d=p(o_rp),
             e=p(o_ci), f=p(o_va), handle=h.ptr):
        return _lib.rsp.rsp_csr2csc(handle, rows, cols, nnz, a, b, c, t, d, e, f)
    assert call(handle=None) == _lib.STATUS_NOT_INITIALIZED
    for bad in (dict(rows=-1), dict(cols=-1), dict(nnz=-1), dict(t=2), dict(a=None), dict(b=None), dict(d=None),
                dict(e=None), dict(c=None), dict(f=None), dict(nnz=case.nnz - 1),  # offsets[rows] > nnz
                dict(cols=int(case.ci.max()))):                                    # a column = cols
        assert call(**bad) == _lib.STATUS_INVALID_VALUE, bad
    bad_rp = case.rp.copy()
    bad_rp[2], bad_rp[3] = 5, 4  # decreasing
    assert call(a=p(dev(bad_rp))) == _lib.STATUS_INVALID_VALUE
    torch.cuda.synchronize()
    assert (o_rp == -7).all() and (o_ci == -7).all() and (o_va == 7.0).all()  # nothing was written
    assert call() == _lib.STATUS_SUCCESS and np.array_equal(o_rp.cpu().numpy(), case.t_rp)


# ------------------------------------------------ values are read every call

@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_values_are_read_on_every_call(handles, cfg):
    dtype, ftz = CONFIGS[cfg]
    h = handles[ftz]
    case = tall_case()
    rng = np.random.default_rng(73)
    v1, v2, v3 = (rng.uniform(-2, 2, case.nnz) for _ in range(3))
    M = descriptor(h, case, dtype)
    xs = {dt: dev(case.x, dt) for dt in (dtype, OTHER[dtype])}
    xn = {dt: dev(rng.uniform(-1, 1, case.cols), dt) for dt in (dtype, OTHER[dtype])}
    forward = product_n(M, xn[dtype])  # before op = T was ever used
    info = M.plan_info()
    assert same_bits(product_t(M, xs[dtype]), case.expect(dtype, ftz))
    M.values.copy_(dev(v1, dtype))  # in place: same pointer, no call
    assert same_bits(product_t(M, xs[dtype]), case.expect(dtype, ftz, values=v1))
    M.set_values(dev(v2, dtype))    # another tensor of the same type: nothing is rebuilt
    assert M.plan_info() == info
    assert same_bits(product_t(M, xs[dtype]), case.expect(dtype, ftz, values=v2))
    other = OTHER[dtype]            # the other type: new room for the values, A^T re-planned by the call
    other_ftz = ftz and other == torch.float32
    M.set_values(dev(v3, other))
    st = _lib.rsp.rsp_spmv(h.ptr, _lib.OP_T, C.byref(C.c_double(1.0)), M._mat, C.c_void_p(xs[dtype].data_ptr()),
                           C.byref(C.c_double(0.0)), C.c_void_p(xn[dtype].data_ptr()), CONFIGS_DT[dtype], None)
    assert st == _lib.STATUS_INVALID_VALUE  # the type the descriptor had before
    assert same_bits(product_t(M, xs[other]), case.expect(other, other_ftz, values=v3))
    assert same_bits(product_t(M, xs[other], 2.0, 1.0, case.y0), case.expect(other, other_ftz, 2.0, 1.0, values=v3))
    # and back; the forward product is what it was before op = T was ever used
    M.set_values(dev(case.values, dtype))
    assert same_bits(product_t(M, xs[dtype]), case.expect(dtype, ftz))
    assert same_bits(product_n(M, xn[dtype]), forward)
    assert same_bits(forward, ob.spmv(case.rp, case.ci[:case.nnz], case.values[:case.nnz].astype(NP[dtype]),
                                      xn[dtype].cpu().numpy(), ftz=ftz, order="canon"))
    M.close()


CONFIGS_DT = {torch.float64: _lib.R_64F, torch.float32: _lib.R_32F}


# ---------------------------------------------------------------- lifecycle

def raw_buffer_size(h, M, op, dt=None):
    size = C.c_size_t(99)
    one, zero = C.c_double(1.0), C.c_double(0.0)
    st = _lib.rsp.rsp_spmv_buffer_size(h.ptr, op, C.byref(one), M._mat, C.byref(zero),
                                       CONFIGS_DT[M.dtype] if dt is None else dt, C.byref(size))
    return st, size.value


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_buffer_size_builds_and_spmv_plans_nothing(handles, cfg):
    dtype, ftz = CONFIGS[cfg]
    h = handles[ftz]
    case = tall_case()
    M = descriptor(h, case, dtype)
    info = M.plan_info()
    assert _lib.rsp.rsp_spmv_transpose_permute(h.ptr, M._mat) == _lib.STATUS_NOT_INITIALIZED  # no side yet
    assert raw_buffer_size(h, M, _lib.OP_T) == (_lib.STATUS_SUCCESS, 0)
    assert _lib.rsp.rsp_spmv_transpose_permute(h.ptr, M._mat) == _lib.STATUS_SUCCESS
    assert M.plan_info() == info  # the forward schedule is untouched
    # the side stands: the call itself is not host-blocking (it leaves the delayed stream busy; test_ordered_...)
    assert same_bits(product_t(M, dev(case.x, dtype)), case.expect(dtype, ftz))
    assert M.plan_info() == info
    assert raw_buffer_size(h, M, _lib.OP_T) == (_lib.STATUS_SUCCESS, 0)
    M.close()


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_preprocess_picks_up_a_changed_pattern(handles, cfg):
    dtype, ftz = CONFIGS[cfg]
    h = handles[ftz]
    case = mirror_case()
    M = descriptor(h, case, dtype)
    x = dev(case.x, dtype)
    assert same_bits(product_t(M, x), case.expect(dtype, ftz))
    # the columns mirrored in place (same offsets, same values): another A^T
    flipped = Case(case.rows, case.cols, case.rp, (case.cols - 1 - case.ci[:case.nnz]).astype(np.int32),
                   case.values[:case.nnz], case.x, case.y0)
    M.colidx.copy_(dev(flipped.ci))
    M.preprocess_transpose()
    want = flipped.expect(dtype, ftz)
    assert not same_bits(want, case.expect(dtype, ftz))
    assert same_bits(product_t(M, x), want)
    # a malformed pattern is an INVALID_VALUE of the rebuild; the side that stood stays usable
    M.colidx[0] = case.cols
    with pytest.raises(RspError) as e:
        M.preprocess_transpose()
    assert e.value.status == _lib.STATUS_INVALID_VALUE
    M.colidx.copy_(dev(flipped.ci))
    assert same_bits(product_t(M, x), want)
    M.close()


def test_argument_errors(handles):
    h = handles[False]
    case = DEGENERATE["nnz_4k+2"]()
    M = descriptor(h, case, torch.float64)
    x, y = dev(case.x), torch.full((case.cols,), float("nan"), dtype=torch.float64, device="cuda")
    one, zero = C.c_double(1.0), C.c_double(0.0)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def spmv(op=_lib.OP_T, handle=h.ptr, a=C.byref(one), mat=M._mat, xx=p(x), b=C.byref(zero), yy=p(y), dt=_lib.R_64F):
        return _lib.rsp.rsp_spmv(handle, op, a, mat, xx, b, yy, dt, None)
    assert spmv(handle=None) == _lib.STATUS_NOT_INITIALIZED
    for bad in (dict(a=None), dict(b=None), dict(mat=None), dict(xx=None), dict(yy=None), dict(dt=_lib.R_32F)):
        assert spmv(**bad) == _lib.STATUS_INVALID_VALUE, bad
    assert torch.isnan(y).all()
    # an op outside the enum: NOT_SUPPORTED, as include/rsp.h documents, in all three calls
    assert spmv(op=2) == _lib.STATUS_NOT_SUPPORTED and spmv(op=-1) == _lib.STATUS_NOT_SUPPORTED
    assert raw_buffer_size(h, M, 2)[0] == _lib.STATUS_NOT_SUPPORTED
    assert _lib.rsp.rsp_spmv_preprocess(h.ptr, 2, C.byref(one), M._mat, None, C.byref(zero), None, _lib.R_64F,
                                        None) == _lib.STATUS_NOT_SUPPORTED
    assert raw_buffer_size(h, M, _lib.OP_T, _lib.R_32F)[0] == _lib.STATUS_INVALID_VALUE
    assert _lib.rsp.rsp_spmv_buffer_size(h.ptr, _lib.OP_T, C.byref(one), M._mat, C.byref(zero), _lib.R_64F,
                                         None) == _lib.STATUS_INVALID_VALUE
    assert spmv() == _lib.STATUS_SUCCESS and same_bits(y.cpu().numpy(), case.expect(torch.float64, False))
    # the Python mirror's length checks, with the roles of m and n swapped
    with pytest.raises(ValueError):
        M.spmv(x[:-1], transpose=True)
    with pytest.raises(ValueError):
        M.spmv(x, y[:-1], transpose=True)
    with pytest.raises(ValueError):
        M.spmv(x.to(torch.float32), transpose=True)
    # a pattern with a column outside the matrix: INVALID_VALUE from the first op = T use
    bad = SpMat(h, dev(np.array([0, 1], np.int32)), dev(np.array([0], np.int32)), dev(np.ones(1)), 1)
    bad.colidx[0] = 1
    with pytest.raises(RspError) as e:
        bad.spmv(dev(np.ones(1)), transpose=True)
    assert e.value.status == _lib.STATUS_INVALID_VALUE
    bad.close()
    M.close()


# -------------------------------------------------------------- determinism

@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_repeats_and_rebuilds_give_the_same_bits(handles, cfg):
    dtype, ftz = CONFIGS[cfg]
    h = handles[ftz]
    case = tall_case()
    x = dev(case.x, dtype)
    want = case.expect(dtype, ftz, 2.0, 1.0)
    for _ in range(3):  # builds
        M = descriptor(h, case, dtype)
        for _ in range(4):  # calls (the long row's tickets go round)
            assert same_bits(product_t(M, x, 2.0, 1.0, case.y0), want)
        M.preprocess_transpose()
        assert same_bits(product_t(M, x, 2.0, 1.0, case.y0), want)
        M.close()


@pytest.mark.parametrize("cfg", sorted(CONFIGS))
def test_ordered_on_a_side_stream(ctx, cfg):
    """The delayed producer of test_gpu_streams.py: the values and x arrive on
    the handle's side stream behind a long-running kernel; the permutation and
    the product must wait for them there. The call leaves the stream busy, so
    it neither synchronised nor re-planned (the side was built before)."""
    dtype, ftz = CONFIGS[cfg]
    h, S = ctx
    h.set_ftz(ftz)
    try:
        case = tall_case()
        va, va_real = late_input(dev(case.values.astype(NP[dtype])))
        va.copy_(va_real)
        x, x_real = late_input(dev(case.x, dtype))
        M = SpMat(h, dev(case.rp), dev(case.ci), va, case.cols)
        y = torch.empty(case.cols, dtype=dtype, device="cuda")
        M.spmv(x_real, y, transpose=True)  # builds the transposed side
        torch.cuda.synchronize()
        _, (got,) = both(ctx, [(va, va_real), (x, x_real)], lambda: M.spmv(x, y, transpose=True).numel(), [y],
                         label=f"spmv op=T {cfg}")
        assert same_bits(got, case.expect(dtype, ftz))
        y0_real = dev(case.y0, dtype)
        _, (got,) = both(ctx, [(va, va_real), (x, x_real), (y, y0_real)],
                         lambda: M.spmv(x, y, 2.0, 1.0, transpose=True).numel(), [y], label=f"spmv op=T beta {cfg}")
        assert same_bits(got, case.expect(dtype, ftz, 2.0, 1.0))
        M.close()
    finally:
        h.set_ftz(False)
