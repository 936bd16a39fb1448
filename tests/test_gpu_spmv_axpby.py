"""GPU tests of the SpMV epilogue y = alpha*A*x + beta*y at every place that
applies the two scalars (spmv.hip: the tile rows' sink, a whole long row, a
chunked row finished by its last-arriving chunk, a chunked row finished by the
fixup kernel), in the one-matrix and the batched kernel, for fp64, fp32 and
fp32 with flush-to-zero.

Everything is bit equality (NaN-class equality where the expectation is NaN)
with the oracle's canonical-order sums put through the restatement
tests/spmv_epilogue_ref.py; tests/test_spmv_epilogue_ref.py shows on the CPU
that the restatement's mutants (a fused multiply-add on either side, fp64
evaluation of fp32, alpha applied per chunk) change bits at every site of the
matrices used here. Nothing is compared with the library's own output except
where the contract is sameness: parts against the whole, FTZ on against off
for fp64."""
import ctypes as C

import numpy as np
import pytest
import torch

import spmv_epilogue_ref as er
from respasol_amd import RspError, _lib
from respasol_amd.sparse import Handle, SpMat, SpmvBatch, upload_csr
from test_gpu_spmv_fuzz import rect_case
from test_spmv_plan_packed import STENCILS

pytestmark = pytest.mark.gpu
TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32}
# dtype, FTZ
FORMS = [(np.float64, False), (np.float32, False), (np.float32, True)]
FORM_IDS = ["fp64", "fp32", "fp32ftz"]
MODES = ["single", "batch"]
NAMES = ("long-row matrix", "all-empty matrix", "stencil")


def tensor(a):
    """A host tensor holding a copy of `a` (the cases' arrays are read-only)."""
    return torch.from_numpy(np.array(a))


class Dev:
    """One case on the device: the matrix, and the x, values and y tensors
    that single calls and the batch both use (tests change them in place)."""

    def __init__(self, handle, case):
        A = case.A
        self.case = case
        rp, ci, self.va = upload_csr(A.rowptr, A.colidx, A.values, TORCH[case.dtype])
        assert np.array_equal(er.bits(self.va.cpu().numpy()), er.bits(case.vals))
        self.mat = SpMat(handle, rp, ci, self.va, A.n)
        self.x = tensor(case.x).cuda()
        self.y = torch.empty(A.m, dtype=TORCH[case.dtype], device="cuda")


class World:
    """One handle of one RSP_SPMV_VARIANT and, per type, the three matrices
    with one batch holding them together."""

    def __init__(self, variant):
        mp = pytest.MonkeyPatch()
        mp.setenv("RSP_SPMV_VARIANT", str(variant))  # read by rsp_create
        try:
            self.handle = Handle()
        finally:
            mp.undo()
        self.variant = variant
        self._types = {}

    def get(self, dtype):
        dtype = np.dtype(dtype)
        if dtype not in self._types:
            cases = (er.epilogue_case(dtype.type), er.empty_case(dtype.type), er.stencil_case(dtype.type, STENCILS[0]))
            devs = [Dev(self.handle, c) for c in cases]
            batch = SpmvBatch(self.handle, [d.mat for d in devs], [d.x for d in devs], [d.y for d in devs])
            self._types[dtype] = (devs, batch)
        return self._types[dtype]

    def run(self, dtype, ftz, mode, alpha, beta, y_init="y0"):
        """One call per matrix, or one batched launch; returns every y.
        y_init: "y0" (NaN instead when beta == 0: y is write-only), a list of
        arrays, or None to leave the buffers as the last call left them."""
        devs, batch = self.get(dtype)
        if y_init == "y0":
            y_init = [np.full(d.case.A.m, np.nan, dtype) if beta == 0 else d.case.y0 for d in devs]
        if y_init is not None:
            for d, y in zip(devs, y_init):
                d.y.copy_(tensor(y))
        self.handle.set_ftz(ftz)
        try:
            if mode == "batch":
                batch.run(alpha, beta)
            else:
                for d in devs:
                    d.mat.spmv(d.x, d.y, alpha, beta)
            return [d.y.cpu().numpy() for d in devs]
        finally:
            self.handle.set_ftz(False)

    def close(self):
        for devs, batch in self._types.values():
            batch.close()
            for d in devs:
                d.mat.close()
        self.handle.close()


@pytest.fixture(scope="module", params=[0, 256], ids=["fused", "fixup"])
def world(request):
    """RSP_SPMV_VARIANT 0: chunked rows finished by the last-arriving chunk;
    256: by the fixup kernel. One handle per variant for the whole module."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    w = World(request.param)
    yield w
    w.close()


def assert_sites(case, got, want, what):
    """Bit equality row group by row group (a failure names the site and the
    first differing row); rows whose expectation is NaN must be NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = np.isnan(want)
    same = np.where(nan, np.isnan(got), er.bits(got) == er.bits(want))
    wrong = []
    for grp, rows in case.groups.items():
        bad = rows[~same[rows]]
        if bad.size:
            wrong.append(f"site {grp}: {bad.size} of {rows.size} rows differ, first row {bad[0]} "
                         f"({case.lens[bad[0]]} entries): got {got[bad[0]]!r} ({er.bits(got)[bad[0]]:#x}), "
                         f"want {want[bad[0]]!r} ({er.bits(want)[bad[0]]:#x})")
    assert not wrong, f"{what}: " + "; ".join(wrong)


# ------------------------------------------------ bitwise against the restatement

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("alpha,beta", er.SCALARS, ids=[f"{a:.3g},{b:.3g}" for a, b in er.SCALARS])
@pytest.mark.parametrize("dtype,ftz", FORMS, ids=FORM_IDS)
def test_epilogue_bits(world, dtype, ftz, alpha, beta, mode):
    devs, _ = world.get(dtype)
    got = world.run(dtype, ftz, mode, alpha, beta)
    for d, y, name in zip(devs, got, NAMES):
        want = er.epilogue(d.case.s, d.case.y0, alpha, beta)
        assert_sites(d.case, y, want, f"{name}, {mode}, alpha {alpha!r} beta {beta!r}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,ftz", FORMS, ids=FORM_IDS)
def test_chain_on_one_buffer(world, dtype, ftz, mode):
    """(1/3, -0.7) three times on the same y, each step the restatement of
    the step before; then (1, 0) gives the plain canonical bits: the long
    rows' tickets and partials are clean after beta != 0 calls."""
    devs, _ = world.get(dtype)
    alpha, beta = er.SCALARS[0]
    prev = [d.case.y0 for d in devs]
    for step in range(3):
        got = world.run(dtype, ftz, mode, alpha, beta, y_init=prev if step == 0 else None)
        for d, y, p, name in zip(devs, got, prev, NAMES):
            assert_sites(d.case, y, er.epilogue(d.case.s, p, alpha, beta), f"{name}, {mode}, step {step}")
        prev = got
    got = world.run(dtype, ftz, mode, 1.0, 0.0, y_init=None)
    for d, y, name in zip(devs, got, NAMES):
        assert_sites(d.case, y, d.case.s, f"{name}, {mode}, (1, 0) after the chain")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,ftz", FORMS, ids=FORM_IDS)
def test_rows_of_more_than_64_chunks(world, dtype, ftz, mode):
    """Rows of 65 and 66 chunks: the second trip of the 64-at-a-time partial
    loads of longrow_arrive / fixup_row. Canonical bits, five times over."""
    devs, _ = world.get(dtype)
    case = devs[0].case
    n = sorted(er.nchunks(int(case.lens[r]), case.cap) for r in case.groups["chunk65"])
    assert len(n) >= 3 and n[0] == 65 and n[-1] == 66
    for rep in range(5):
        got = world.run(dtype, ftz, mode, 1.0, 0.0)
        for d, y, name in zip(devs, got, NAMES):
            assert_sites(d.case, y, d.case.s, f"{name}, {mode}, repeat {rep}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,ftz", FORMS, ids=FORM_IDS)
def test_negative_alpha_on_empty_rows(world, dtype, ftz, mode):
    """(-1, 0): an empty row is alpha * (+0) = -0.0, in the all-empty matrix
    and among the other rows."""
    devs, _ = world.get(dtype)
    got = world.run(dtype, ftz, mode, -1.0, 0.0)
    for d, y, name in zip(devs, got, NAMES):
        rows = d.case.groups["empty"]
        assert np.all(y[rows] == 0) and np.all(np.signbit(y[rows])), name
        assert_sites(d.case, y, er.epilogue(d.case.s, None, -1.0, 0.0), f"{name}, {mode}")
    assert len(devs[0].case.groups["empty"]) > 0 and len(devs[1].case.groups["empty"]) == devs[1].case.A.m


# ------------------------------------------------------------------- parts

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_parts_alpha_and_beta_refusal(world, dtype):
    """On a split schedule part 1 then part 2 with alpha = 1/3 give the bits
    of part 0; beta != 0 is refused for parts 1 and 2 (INVALID_VALUE), by
    rsp_spmv_part and by a batch created with part != 0, and a refused call
    leaves y untouched."""
    h = world.handle
    tdt = TORCH[np.dtype(dtype)]
    A, x, canon = rect_case(4, tdt)  # 6000 x 66000, the multi-GPU slice's shape
    assert (A.m, A.n) == (6000, 66000) and x.dtype == np.dtype(dtype)
    M = SpMat(h, *upload_csr(A.rowptr, A.colidx, A.values, tdt), A.n)
    M.set_local_cols(6000)
    xd = tensor(x).cuda()
    alpha = 1.0 / 3.0
    want = er.epilogue(canon, None, alpha, 0.0)
    nan = torch.full((A.m,), float("nan"), dtype=tdt, device="cuda")
    whole = M.spmv(xd, nan.clone(), alpha, 0.0).cpu().numpy()
    assert np.array_equal(er.bits(whole), er.bits(want)), "part 0"
    y = nan.clone()
    M.spmv_part(xd, y, 1, alpha)
    assert torch.isnan(y).any() and not torch.isnan(y).all()  # both parts hold rows
    M.spmv_part(xd, y, 2, alpha)
    assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(whole)), "part 1 then part 2"
    # refusals: y keeps its pattern
    pattern = np.arange(1, A.m + 1).astype(dtype) / dtype(7)
    y = tensor(pattern).cuda()
    sc = C.c_double if dtype == np.float64 else C.c_float
    a, b = sc(alpha), sc(0.3)
    rdt = _lib.R_64F if dtype == np.float64 else _lib.R_32F
    for part in (1, 2):
        st = _lib.rsp.rsp_spmv_part(h.ptr, C.byref(a), M._mat, C.c_void_p(xd.data_ptr()), C.byref(b),
                                    C.c_void_p(y.data_ptr()), rdt, C.c_void_p(M.buffer.data_ptr()), part)
        assert st == 3, (part, st)
        assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(pattern)), f"rsp_spmv_part {part} wrote y"
    batches = [SpmvBatch(h, [M], [xd], [y], part=part) for part in (1, 2)]
    for part, B in zip((1, 2), batches):
        with pytest.raises(RspError) as e:
            B.run(alpha, 0.3)
        assert e.value.status == 3
        assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(pattern)), f"batch part {part} wrote y"
    # the same batches with beta = 0: the two parts give the whole, alpha included
    y.fill_(float("nan"))
    for B in batches:
        B.run(alpha, 0.0)
    assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(whole)), "batch part 1 then part 2"
    # part 0 takes beta
    y.copy_(tensor(pattern))
    st = _lib.rsp.rsp_spmv_part(h.ptr, C.byref(a), M._mat, C.c_void_p(xd.data_ptr()), C.byref(b),
                                C.c_void_p(y.data_ptr()), rdt, C.c_void_p(M.buffer.data_ptr()), 0)
    assert st == 0
    assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(er.epilogue(canon, pattern, alpha, 0.3))), "part 0, beta"
    for B in batches:
        B.close()
    M.close()


# ------------------------------------------------------- non-finite operands

KINDS = ("pos_inf", "pos_and_neg_inf", "zero_times_inf", "nan_in_x", "nan_unreferenced")


def plant(case, kind):
    """(values, x) with `kind` planted into the products of one row per site
    (case.plants: the row's entry whose column no other entry references, in
    a middle chunk of a chunked row), or NaN in every x no row references."""
    vals, x = case.vals.copy(), case.x.copy()
    ci = case.A.colidx
    inf = case.dtype.type(np.inf)
    if kind == "nan_unreferenced":
        x[case.unreferenced] = np.nan
        return vals, x
    for row, k in case.plants.values():
        if kind == "pos_inf":            # a product of +inf
            vals[k] = np.copysign(inf, x[ci[k]])
        elif kind == "pos_and_neg_inf":  # products of +inf and -inf, neighbours in the row
            vals[k] = np.copysign(inf, x[ci[k]])
            vals[k + 1] = -np.copysign(inf, x[ci[k + 1]])
        elif kind == "zero_times_inf":   # a stored 0.0 whose x is inf
            vals[k] = 0.0
            x[ci[k]] = inf
        else:                            # a NaN in x
            x[ci[k]] = np.nan
    return vals, x


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), er.SCALARS[0]], ids=["1,0", "0.333,-0.7"])
@pytest.mark.parametrize("dtype,ftz", FORMS, ids=FORM_IDS)
def test_non_finite_operands(world, dtype, ftz, alpha, beta, kind):
    """An Inf or NaN among one row's products stays in that row, a 0 * inf is
    not skipped, and x entries that no row references are never used: every
    row without a planted entry keeps the clean run's bits."""
    devs, _ = world.get(dtype)
    big = devs[0]
    case = big.case
    vals, x = plant(case, kind)
    s = case.canon(vals, x, ftz=ftz)
    rows = sorted(r for r, _ in case.plants.values())
    touched = np.flatnonzero(er.bits(s) != er.bits(case.s))
    if kind == "nan_unreferenced":
        assert touched.size == 0 and np.isnan(x[-1])
    else:
        assert list(touched) == rows
        assert np.all(s[rows] == np.inf) if kind == "pos_inf" else np.all(np.isnan(s[rows]))
    want = er.epilogue(s, case.y0, alpha, beta)
    try:
        big.va.copy_(tensor(vals))
        big.x.copy_(tensor(x))
        for mode in MODES:
            got = world.run(dtype, ftz, mode, alpha, beta)
            assert_sites(case, got[0], want, f"{kind}, {mode}")
            for d, y, name in zip(devs[1:], got[1:], NAMES[1:]):
                assert_sites(d.case, y, er.epilogue(d.case.s, d.case.y0, alpha, beta), f"{kind}, {mode}, {name}")
    finally:
        big.va.copy_(tensor(case.vals))
        big.x.copy_(tensor(case.x))


# ------------------------------------------------------- flush-to-zero edges

def tiny_matrix(handle, dtype, rows, x):
    """rows: per row a list of (column, value)."""
    lens = [len(r) for r in rows]
    rp = np.zeros(len(rows) + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.array([c for r in rows for c, _ in r], np.int32)
    va = np.array([v for r in rows for _, v in r], dtype)
    tdt = TORCH[np.dtype(dtype)]
    M = SpMat(handle, torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(va).cuda(), len(x))
    return M, torch.from_numpy(np.array(x, dtype)).cuda(), tdt


def tiny_run(handle, M, xd, tdt, y0, alpha, beta, ftz, mode):
    y = torch.from_numpy(np.array(y0, NP_OF[tdt])).cuda()
    handle.set_ftz(ftz)
    try:
        if mode == "batch":
            B = SpmvBatch(handle, [M], [xd], [y])
            B.run(alpha, beta)
            B.close()
        else:
            M.spmv(xd, y, alpha, beta)
        return y.cpu().numpy()
    finally:
        handle.set_ftz(False)


NP_OF = {torch.float64: np.float64, torch.float32: np.float32}


@pytest.mark.parametrize("mode", MODES)
def test_ftz_edges_fp32(world, mode):
    """fp32 + FTZ: a normal s whose alpha*s is subnormal gives a signed zero,
    and a subnormal beta*y0 counts as zero; both survive without FTZ. Three
    rows: s = 2^-120, an empty row, s = -2^-120."""
    h = world.handle
    f = np.float32
    M, xd, tdt = tiny_matrix(h, f, [[(0, 2.0 ** -120)], [], [(2, -2.0 ** -120)]], [1.0, 1.0, 1.0])
    nan3 = [np.nan] * 3
    # alpha * s = +-2^-128: subnormal
    got = tiny_run(h, M, xd, tdt, nan3, 2.0 ** -8, 0.0, False, mode)
    assert np.array_equal(er.bits(got), er.bits(np.array([2.0 ** -128, 0.0, -2.0 ** -128], f)))
    got = tiny_run(h, M, xd, tdt, nan3, 2.0 ** -8, 0.0, True, mode)
    assert np.array_equal(er.bits(got), er.bits(np.array([0.0, 0.0, -0.0], f)))
    # beta * y0 = +-2^-130: subnormal
    y0 = [2.0 ** -100, -2.0 ** -100, 2.0 ** -100]
    got = tiny_run(h, M, xd, tdt, y0, 1.0, 2.0 ** -30, False, mode)
    want = np.array([2.0 ** -120 + 2.0 ** -130, -2.0 ** -130, -2.0 ** -120 + 2.0 ** -130], f)
    assert np.all(want.astype(np.float64) == [2.0 ** -120 + 2.0 ** -130, -2.0 ** -130, -2.0 ** -120 + 2.0 ** -130])
    assert np.array_equal(er.bits(got), er.bits(want))
    got = tiny_run(h, M, xd, tdt, y0, 1.0, 2.0 ** -30, True, mode)
    # (the empty row: +0 + -0 = +0)
    assert np.array_equal(er.bits(got), er.bits(np.array([2.0 ** -120, 0.0, -2.0 ** -120], f)))
    M.close()


@pytest.mark.parametrize("mode", MODES)
def test_ftz_never_flushes_fp64(world, mode):
    """fp64 subnormal values, products and scaled terms under rsp_set_ftz(1):
    the bits of the run with FTZ off, which are the exact small multiples of
    u = 2^-1074 worked out here."""
    h = world.handle
    u = 2.0 ** -1074
    rows = [[(0, 3 * u)],                                   # a subnormal value: s = 3 u
            [(1, 2.0 ** -540)],                             # a subnormal product: s = 2^-540 * 2^-530 = 16 u
            [(0, 2.0 ** -1030), (2, 2.0 ** -1040)]]         # s = (2^44 + 2^34) u
    M, xd, tdt = tiny_matrix(h, np.float64, rows, [1.0, 2.0 ** -530, 1.0])
    y0 = [2.0 ** -1070, 0.0, -2.0 ** -1060]
    # 0.5 * 3 u = 1.5 u rounds to even, 2 u; 0.25 * 2^-1070 = 4 u; 0.25 * -2^-1060 = -2^12 u
    want = np.array([6 * u, 8 * u, (2.0 ** 43 + 2.0 ** 33 - 2.0 ** 12) * u])
    assert np.all(want > 0) and np.all(want < np.finfo(np.float64).tiny)
    off = tiny_run(h, M, xd, tdt, y0, 0.5, 0.25, False, mode)
    on = tiny_run(h, M, xd, tdt, y0, 0.5, 0.25, True, mode)
    assert np.array_equal(er.bits(off), er.bits(want))
    assert np.array_equal(er.bits(on), er.bits(off))
    M.close()
