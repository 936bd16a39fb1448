"""GPU parity of the block-inverse L / L^T solves (trsv_blocks.hip, plan
ilu_blocks.cpp) on the matrices of tests/blk_cases.py, which reach every rule
of the planner at a position chosen by construction (their facts are pinned
in tests/test_blk_cases.py): chunks cut by the long-row cap, long blocks of 0
to 12 rounds with aligned and unaligned far parts, far terms past one stride
of the prologue, several chunks, the full near width, blocks per chunk around
the chunk walk's unroll depth, the planner knobs, and plans refused because
their coefficient build does not fit the LDS.

Every solve equals the oracle's restatement of the block order bit for bit
(the reference's order where the plan is refused), and rsp_ilu0_solve_blocks
equals the oracle's block counts."""
import numpy as np
import pytest
import torch

import blk_cases as bc
import oracle_bind as ob
from respasol_amd.sparse import Ilu0, upload_csr

pytestmark = pytest.mark.gpu
NP = {torch.float64: np.float64, torch.float32: np.float32}
MODES = [(torch.float64, False), (torch.float32, False), (torch.float32, True)]
MODE_IDS = ["f64", "f32", "f32-ftz"]
ALPHAS = (1.0, -0.75)
LDS_NEED = {c.id: need for c, need in bc.LDS_EDGES}


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from respasol_amd.sparse import Handle
    h = Handle()
    yield h
    h.close()


def set_knobs(monkeypatch, case):
    for k in ("RSP_ILU_BLOCKS", "RSP_BLK_CH", "RSP_BLK_NMAX", "RSP_BLK_YMAX", "RSP_BLK_NW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, str(v))


def refused(case, reverse):
    """Per DAG (L, L^T): the plan's coefficient build does not fit the LDS."""
    need = LDS_NEED.get(case.id)
    if need is None:
        return False, False
    need = need[::-1] if reverse else need
    return need[0] > bc.LDS_MAX, need[1] > bc.LDS_MAX


def factored(handle, A, dtype, ftz):
    """Analysis and factor of A; the factor equals the oracle's bit for bit."""
    handle.set_ftz(ftz)
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dtype)
    il = Ilu0(handle, rp, ci, nnz=A.nnz)
    il.analysis()
    il.factor(va)
    assert il.zero_pivot() == -1
    rv, sz, zp = ob.ilu0(A.rowptr, A.colidx, A.values.astype(NP[dtype]), ftz=ftz)
    assert sz == -1 and zp == -1
    assert np.array_equal(va.cpu().numpy(), rv)
    return il, va, rv


def solve_pair(il, va, x, alpha):
    z = il.solve_lower(va, x, alpha=alpha)
    y = il.solve_lower(va, z, transpose=True, alpha=alpha)
    return z.cpu().numpy(), y.cpu().numpy()


def oracle_pair(case, reverse, A, rv, xx, alpha, ftz):
    """(z, y, (blocks of L, blocks of L^T)) of the oracle: the block order
    under the case's knobs, the reference's order for a refused plan."""
    prm = ob.blk_params_env(case.knobs)
    no_l, no_t = refused(case, reverse)
    if no_l:
        rz, bl = ob.trsv("lower_n_ref", A.rowptr, A.colidx, rv, xx, alpha=alpha, ftz=ftz), 0
    else:
        rz, bl = ob.trsv("lower_n_blocks", A.rowptr, A.colidx, rv, xx, alpha=alpha, ftz=ftz, params=prm, count=True)
    if no_t:
        ry, bt = ob.trsv("lower_t_ref", A.rowptr, A.colidx, rv, rz, alpha=alpha, ftz=ftz), 0
    else:
        ry, bt = ob.trsv("lower_t_blocks", A.rowptr, A.colidx, rv, rz, alpha=alpha, ftz=ftz, params=prm, count=True)
    return rz, ry, (bl, bt)


def same(got, ref, what):
    bad = np.nonzero(got != ref)[0] if got.shape == ref.shape else None
    assert got.dtype == ref.dtype and np.array_equal(got, ref), (
        f"{what}: {bad.size} of {got.size} differ, first at {bad[:8].tolist()}")


@pytest.mark.parametrize("dtype,ftz", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("reverse", [False, True], ids=["orig", "rev"])
@pytest.mark.parametrize("case", bc.CASES, ids=[c.id for c in bc.CASES])
def test_case_matches_the_oracle_bitwise(handle, monkeypatch, case, reverse, dtype, ftz):
    """Factor, L solve, L^T solve of that z, alpha 1 and -0.75: z and y equal
    the oracle's bits, the planned block counts the oracle's. A refused plan
    (LDS) reports 0 blocks, succeeds and follows the reference's order."""
    set_knobs(monkeypatch, case)
    A, x = bc.build(case, reverse)
    try:
        il, va, rv = factored(handle, A, dtype, ftz)
        xx = np.ascontiguousarray(x, NP[dtype])
        xd = torch.from_numpy(xx).cuda()
        for alpha in ALPHAS:
            z, y = solve_pair(il, va, xd, alpha)  # (a failed launch raises: the status is SUCCESS)
            assert il.solve_zero_pivot(il.TRSV_L) == -1 and il.solve_zero_pivot(il.TRSV_LT) == -1
            rz, ry, blocks = oracle_pair(case, reverse, A, rv, xx, alpha, ftz)
            assert il.solve_blocks() == blocks
            assert tuple(b == 0 for b in blocks) == refused(case, reverse)
            same(z, rz, f"L solve, alpha {alpha}")
            same(y, ry, f"L^T solve, alpha {alpha}")
    finally:
        handle.set_ftz(False)


@pytest.mark.parametrize("cid", ["hubs", "capcut", "band11-512", "chain-1088"])
def test_one_plan_alternating_types(handle, monkeypatch, cid):
    """One info, one handle: fp64, then fp32 on a converted factor, then fp64
    again. The plan's scratch (coefficients, y by position, records) is sized
    for fp64 and shared: every result equals a fresh info's bits."""
    case = bc.BY_ID[cid]
    set_knobs(monkeypatch, case)
    A, x = bc.build(case)
    il, va, rv = factored(handle, A, torch.float64, False)
    va32 = va.to(torch.float32)
    x64 = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    x32 = x64.to(torch.float32)
    fresh = {}
    for dt, v, xd in ((torch.float64, va, x64), (torch.float32, va32, x32)):
        rp, ci, _ = upload_csr(A.rowptr, A.colidx, A.values, dt)
        other = Ilu0(handle, rp, ci, nnz=A.nnz)
        other.analysis()
        fresh[dt] = solve_pair(other, v, xd, -0.75)
        rz, ry, blocks = oracle_pair(case, False, A, v.cpu().numpy(), xd.cpu().numpy(), -0.75, False)
        assert other.solve_blocks() == blocks
        same(fresh[dt][0], rz, f"fresh {dt} L")
        same(fresh[dt][1], ry, f"fresh {dt} L^T")
    for dt, v, xd in ((torch.float64, va, x64), (torch.float32, va32, x32), (torch.float64, va, x64),
                      (torch.float32, va32, x32)):
        z, y = solve_pair(il, v, xd, -0.75)
        same(z, fresh[dt][0], f"{dt} L after the other type")
        same(y, fresh[dt][1], f"{dt} L^T after the other type")


def test_knobs_out_of_range_plan_as_the_defaults(handle, monkeypatch):
    """RSP_BLK_CH above the LDS window, RSP_BLK_NMAX above a record's slots
    and any RSP_BLK_NW: the default plan and its bits (n > 16384, a row with
    13 near terms)."""
    case = bc.BY_ID["near-edge"]
    A, x = bc.build(case)
    set_knobs(monkeypatch, case)
    monkeypatch.setenv("RSP_BLK_CH", "20000")
    monkeypatch.setenv("RSP_BLK_NMAX", "13")
    monkeypatch.setenv("RSP_BLK_NW", "8")
    il, va, rv = factored(handle, A, torch.float64, False)
    z, y = solve_pair(il, va, torch.from_numpy(np.ascontiguousarray(x)).cuda(), 1.0)
    rz, bl = ob.trsv("lower_n_blocks", A.rowptr, A.colidx, rv, x, count=True)
    ry, bt = ob.trsv("lower_t_blocks", A.rowptr, A.colidx, rv, rz, count=True)
    assert il.solve_blocks() == (bl, bt)
    same(z, rz, "L solve")
    same(y, ry, "L^T solve")
