"""The level-plan cases of tests/lvl_cases.py through the kernels: every case
(as built and reversed) and every entry of the knob sweep, in fp64, fp32 and
fp32 + FTZ. Per case the device analysis' plan digest equals the host
analysis' (the device-built term plans and the three row classes of
ilu_analysis.hip, at the planners' limits), and the factor, the L solve with
alpha -0.75, the L^T solve and the U solve are each bitwise the oracle's
(ob.ilu0 / ob.trsv, the reference's operation order); no zero pivot is
reported and no flow launch gave up. Then once more with RSP_ILU_THIN_SOLVE=0
and RSP_ILU_THIN_FACTOR=0, so that the same rows also go through the fat-level
and flow kernels. No tolerances: bit equality is the contract.
tests/test_lvl_cases.py proves on the CPU what each case reaches."""
import ctypes as C

import numpy as np
import pytest
import torch

import lvl_cases as lc
import oracle_bind as ob
from respasol_amd._lib import rsp
from respasol_amd.sparse import Handle, Ilu0, upload_csr

pytestmark = pytest.mark.gpu
MODES = [("f64", torch.float64, np.float64, False), ("f32", torch.float32, np.float32, False),
         ("f32ftz", torch.float32, np.float32, True)]
ALPHA = -0.75
ENTRIES = ([(c, r, ()) for c in lc.CASES for r in (False, True)] +
           [(lc.BY_ID[cid], False, knobs) for cid, knobs in lc.SWEEP] +
           # the row limits of the slot layout's own kernels: a ratio no level exceeds
           [(lc.BY_ID[cid], False, (("RSP_ILU_SLOT_PAD", 1 << 20),)) for cid in ("pairs-1024", "entries-256", "pad-rule")])
ENTRY_IDS = [f"{c.id}-{'rev' if r else 'orig'}" + "".join(f"-{k[8:]}={v}" for k, v in kn) for c, r, kn in ENTRIES]


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    h = Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def reference():
    """The oracle's factor and solves per (case, reversed, mode): computed
    once, shared by a case's knob entries, not to be written."""
    memo = {}

    def get(case, reverse, mode):
        key = (case.id, reverse, mode[0])
        if key not in memo:
            _, _, npdt, ftz = mode
            A, x = lc.build(case, reverse)
            v, sz, zp = ob.ilu0(A.rowptr, A.colidx, A.values.astype(npdt), ftz=ftz)
            assert sz == -1 and zp == -1
            z = ob.trsv("lower_n", A.rowptr, A.colidx, v, x.astype(npdt), alpha=ALPHA, ftz=ftz)
            y = ob.trsv("lower_t", A.rowptr, A.colidx, v, z, alpha=ALPHA, ftz=ftz)
            u = ob.trsv("upper", A.rowptr, A.colidx, v, z, alpha=ALPHA, ftz=ftz)
            memo[key] = (v, z, y, u)
        return memo[key]
    return get


def host_digest(A):
    d = C.c_uint64()
    r = np.ascontiguousarray(A.rowptr, np.int32)
    c = np.ascontiguousarray(A.colidx, np.int32)
    assert rsp.rsp_ilu0_analysis_host(A.n, r.ctypes.data, c.ctypes.data, None, None, C.byref(d), None) == 0
    return d.value


def run_once(handle, A, x, mode, ref, what):
    _, dtype, npdt, ftz = mode
    rv, rz, ry, ru = ref
    handle.set_ftz(ftz)
    try:
        rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, dtype)
        il = Ilu0(handle, rp, ci, nnz=A.nnz)
        il.analysis()
        assert il.zero_pivot() == -1, what
        dev = C.c_uint64()
        assert rsp.rsp_ilu0_plan_digest(il._info, C.byref(dev)) == 0
        assert dev.value == host_digest(A), f"{what}: the device analysis built another plan than the host's"
        il.factor(va)
        xx = torch.from_numpy(np.ascontiguousarray(x, npdt)).cuda()
        z = il.solve_lower(va, xx, alpha=ALPHA)
        y = il.solve_lower(va, z, transpose=True, alpha=ALPHA)
        u = il.solve_upper(va, z, alpha=ALPHA)
        torch.cuda.synchronize()
        assert il.zero_pivot() == -1, what  # (raises if the factor's flow launch gave up)
        for which in (il.TRSV_L, il.TRSV_LT, il.TRSV_U):  # (each raises if its flow launch gave up)
            assert il.solve_zero_pivot(which) == -1, (what, which)
        got = [t.cpu().numpy() for t in (va, z, y, u)]
        il.close()
    finally:
        handle.set_ftz(False)
    for name, g, r in zip(("factor", "L solve", "L^T solve", "U solve"), got, (rv, rz, ry, ru)):
        bad = np.nonzero(g.view(np.uint8).reshape(g.size, -1) != r.view(np.uint8).reshape(r.size, -1))[0]
        assert bad.size == 0, f"{what}: {name}: {np.unique(bad).size} of {g.size} values differ, first at {np.unique(bad)[:8].tolist()}"


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("case,reverse,knobs", ENTRIES, ids=ENTRY_IDS)
def test_case_bitwise_the_oracle(handle, reference, monkeypatch, case, reverse, knobs, mode):
    A, x = lc.build(case, reverse)
    lc.set_knobs(monkeypatch, case.env)  # (the oracle follows the plan's order: level-scheduled, no split)
    ref = reference(case, reverse, mode)
    for thin_off in (False, True):
        lc.set_knobs(monkeypatch, case.env + tuple(knobs) +
                     ((("RSP_ILU_THIN_SOLVE", 0), ("RSP_ILU_THIN_FACTOR", 0)) if thin_off else ()))
        monkeypatch.setenv("RSP_ILU_DIGEST", "1")
        run_once(handle, A, x, mode, ref, f"{case.id} {'rev' if reverse else 'orig'} {mode[0]} thin_off={thin_off}")
