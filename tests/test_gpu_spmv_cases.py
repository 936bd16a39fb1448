"""The crafted SpMV patterns (tests/spmv_cases.py) on the GPU: every case but
the x-resource pair (its x would be 2 GiB: host only, tests/test_spmv_cases.py),
in fp64, fp32 and fp32 with flush-to-zero. y for (alpha, beta) = (1, 0) and
(1/3, -0.7) is, bit for bit, the restated epilogue of the oracle's canonical
sums (spmv_epilogue_ref.epilogue over oracle_bind.spmv(order="canon"), neither
of which knows about tiles), and a second call gives the same bits. Then the
same bits again under every knob that changes the plan or the path but never
the result: RSP_SPMV_PACK 0 / 1 / 2, RSP_SPMV_STAGE_LIST=0, RSP_SPMV_VARIANT
32 (int32 tiles only), 64 and 128 (aligned row cuts), 256 (fixup kernel), 512
(spread plans) and 1024 (no staged tiles), and arrays shifted by one element
(the scalar path, the packed record ignored). The whole knob sweep runs on
every case. spmv_cases.SUBSET also runs as members of one rsp_spmv_batch and as
parts 1 + 2 of a split schedule. No tolerances anywhere.

The oracle's sums are computed once per (case, type, FTZ) and shared."""
import numpy as np
import pytest
import torch

import oracle_bind as ob
import spmv_cases as sc
import spmv_epilogue_ref as er
from respasol_amd.sparse import Handle, SpMat, SpmvBatch, upload_csr
from spmv_cases import R32, R64

pytestmark = pytest.mark.gpu
TORCH = {R64: torch.float64, R32: torch.float32}
FORMS = [(R64, False), (R32, False), (R32, True)]
FORM_IDS = ["fp64", "fp32", "fp32ftz"]
IDS = [c.id for c in sc.GPU_CASES]
PAIRS = [(1.0, 0.0), er.SCALARS[0]]
assert PAIRS[1] == (1.0 / 3.0, -0.7)
# name: (plan-time environment, RSP_SPMV_VARIANT of the handle, array shift)
KNOBS = {
    "pack0": ((("RSP_SPMV_PACK", 0),), 0, 0), "pack1": ((("RSP_SPMV_PACK", 1),), 0, 0),
    "pack2": ((("RSP_SPMV_PACK", 2),), 0, 0), "nolist": ((("RSP_SPMV_STAGE_LIST", 0),), 0, 0),
    "int32": ((), 32, 0), "align128": ((), 64, 0), "align64": ((), 128, 0), "fixup": ((), 256, 0),
    "spread": ((), 512, 0), "nostage": ((), 1024, 0), "shift": ((), 0, 1),
}
_CANON = {}


@pytest.fixture(scope="module")
def handles():
    """One handle per RSP_SPMV_VARIANT (rsp_create reads it), made on demand."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    made = {}

    def get(variant):
        if variant not in made:
            mp = pytest.MonkeyPatch()
            mp.setenv("RSP_SPMV_VARIANT", str(variant))
            try:
                made[variant] = Handle()
            finally:
                mp.undo()
        return made[variant]
    yield get
    for h in made.values():
        h.close()


def canon(cid, dt, ftz):
    key = (cid, dt, ftz)
    if key not in _CANON:
        A = sc.build(cid, dt)
        s = ob.spmv(A.rowptr, A.colidx, A.values.astype(sc.NP[dt]), sc.vectors(cid, dt)[0], ftz=ftz, order="canon")
        s.setflags(write=False)
        _CANON[key] = s
    return _CANON[key]


def tensor(a):
    return torch.from_numpy(np.array(a))


def device_matrix(h, cid, dt, shift=0):
    A = sc.build(cid, dt)
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values, TORCH[dt])
    if shift:  # views one element into their buffers: not 16-byte aligned, the scalar path
        ci = torch.cat([ci.new_zeros(shift), ci])[shift:]
        va = torch.cat([va.new_zeros(shift), va])[shift:]
        assert A.nnz == 0 or (ci.data_ptr() % 16 and va.data_ptr() % 16)
    return SpMat(h, rp, ci, va, A.n), tensor(sc.vectors(cid, dt)[0]).cuda()


def first_y(cid, dt, beta):
    """y before the call: the case's y0, or NaN where beta == 0 (write-only)."""
    y0 = sc.vectors(cid, dt)[1]
    return y0 if beta != 0 else np.full(len(y0), np.nan, sc.NP[dt])


def check_calls(h, cid, dt, ftz, shift=0, repeat=False, what=""):
    mat, xd = device_matrix(h, cid, dt, shift)
    h.set_ftz(ftz)
    try:
        for alpha, beta in PAIRS:
            want = er.epilogue(canon(cid, dt, ftz), sc.vectors(cid, dt)[1], alpha, beta)
            for rep in range(2 if repeat else 1):
                y = tensor(first_y(cid, dt, beta)).cuda()
                got = mat.spmv(xd, y, alpha, beta).cpu().numpy()
                bad = np.flatnonzero(er.bits(got) != er.bits(want))
                assert bad.size == 0, (f"{cid} {what} alpha {alpha!r} beta {beta!r} call {rep}: {bad.size} rows differ, "
                                       f"first row {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")
    finally:
        h.set_ftz(False)
        mat.close()


@pytest.mark.parametrize("dt,ftz", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("cid", IDS)
def test_case_bits(handles, cid, dt, ftz, monkeypatch):
    sc.set_knobs(monkeypatch, sc.BY_ID[cid])
    check_calls(handles(0), cid, dt, ftz, repeat=True)


@pytest.mark.parametrize("dt,ftz", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("cid", IDS)
def test_case_bits_under_every_knob(handles, cid, dt, ftz, monkeypatch):
    for name, (env, variant, shift) in KNOBS.items():
        sc.set_knobs(monkeypatch, sc.BY_ID[cid], env)
        check_calls(handles(variant), cid, dt, ftz, shift, what=name)


@pytest.mark.parametrize("dt,ftz", FORMS, ids=FORM_IDS)
def test_subset_as_one_batch(handles, dt, ftz, monkeypatch):
    for k in sc.PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    h = handles(0)
    pairs = [device_matrix(h, cid, dt) for cid in sc.SUBSET]
    mats, xs = [p[0] for p in pairs], [p[1] for p in pairs]
    ys = [torch.empty(m.m, dtype=TORCH[dt], device="cuda") for m in mats]
    batch = SpmvBatch(h, mats, xs, ys)
    h.set_ftz(ftz)
    try:
        for alpha, beta in PAIRS:
            for cid, y in zip(sc.SUBSET, ys):
                y.copy_(tensor(first_y(cid, dt, beta)))
            batch.run(alpha, beta)
            for cid, y in zip(sc.SUBSET, ys):
                want = er.epilogue(canon(cid, dt, ftz), sc.vectors(cid, dt)[1], alpha, beta)
                assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(want)), (cid, alpha, beta)
    finally:
        h.set_ftz(False)
        batch.close()
        for m in mats:
            m.close()


@pytest.mark.parametrize("dt,ftz", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("cid", sc.SUBSET)
def test_subset_as_two_parts(handles, cid, dt, ftz, monkeypatch):
    """Half of the columns local: part 1 then part 2 (alpha = 1/3; parts take
    no beta) write every row once."""
    sc.set_knobs(monkeypatch, sc.BY_ID[cid])
    h = handles(0)
    mat, xd = device_matrix(h, cid, dt)
    mat.set_local_cols(mat.n // 2)
    y = torch.full((mat.m,), float("nan"), dtype=TORCH[dt], device="cuda")
    h.set_ftz(ftz)
    try:
        mat.spmv_part(xd, y, 1, PAIRS[1][0])
        mat.spmv_part(xd, y, 2, PAIRS[1][0])
        want = er.epilogue(canon(cid, dt, ftz), None, PAIRS[1][0], 0.0)
        assert np.array_equal(er.bits(y.cpu().numpy()), er.bits(want))
    finally:
        h.set_ftz(False)
        mat.close()
