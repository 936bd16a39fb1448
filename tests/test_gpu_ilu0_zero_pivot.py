"""Zero pivots and non-finite factors on every ILU(0) kernel path.

The factor goes on after a zero pivot, as csrilu02 and the oracle do:
x / 0 = +-inf, then inf - inf and 0 * inf give NaN downstream, and the
position reported is the smallest row with u_jj == 0 whatever the schedule.
tests/ilu_cases.py plants pivots that are exactly zero at rows whose level
order and index order disagree (proved on the oracle by
tests/test_ilu_cases.py); every path of ilu_cases.PATHS — the knob sets of the
path tests of tests/test_gpu_ilu0.py — must report the smallest of them, each
of them alone, and give the oracle's bits (NaN payloads aside) for the factor
and for the L, L^T and U solves of it. fp32 + FTZ divisions whose operand is a
denormal straight from memory must flush it, as the oracle's DAZ does.

RSP_ILU_BLOCKS is left alone here (tests/test_gpu_ilu0.py pins it to 0): the
solves of a deep DAG take the block-inverse plan, as by default."""
import numpy as np
import pytest
import torch

import ilu_cases as ic
import oracle_bind as ob
from respasol_amd import _lib, csr
from respasol_amd.sparse import GMRES, BiCGStab, Handle, Ilu0, RspError, SpMat, upload_csr

pytestmark = pytest.mark.gpu
ALPHA = -0.75
MODE_IDS = ["f64", "f32", "f32-ftz"]
paths = pytest.mark.parametrize("path", ic.PATHS, ids=ic.PATH_IDS)
modes = pytest.mark.parametrize("kind,ftz", ic.MODES, ids=MODE_IDS)


@pytest.fixture(scope="module")
def handle():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    h = Handle()
    yield h
    h.close()


@pytest.fixture
def ftz_mode(handle):
    """Sets the handle's FTZ mode for one test and clears it afterwards."""
    def set_mode(on):
        handle.set_ftz(on)
    yield set_mode
    handle.set_ftz(False)


def setenv(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))


def analysed(handle, A):
    rp, ci, _ = upload_csr(A.rowptr, A.colidx, A.values)
    il = Ilu0(handle, rp, ci, nnz=A.nnz)
    il.analysis()
    assert il.zero_pivot() == -1
    return il


def device(values, kind):
    return torch.from_numpy(np.ascontiguousarray(values).astype(ic.NP[kind])).cuda()


def factor(il, M, kind):
    """Factor M's values on the analysed pattern: (device values, zero pivot)."""
    va = device(M.values, kind)
    il.factor(va)
    return va, il.zero_pivot()


@paths
@modes
def test_smallest_of_several(handle, monkeypatch, ftz_mode, path, kind, ftz):
    """(a) Every planted row at once: the smallest is reported, as by the oracle."""
    _, name, scale, knobs, l0 = path
    setenv(monkeypatch, knobs)
    A, Ap, J, _ = ic.zero_pivot_case(name, scale, kind, l0)
    ftz_mode(ftz)
    _, zp = factor(analysed(handle, A), Ap, kind)
    assert zp == min(J) == ic.oracle_factor(name, scale, kind, ftz, "all")[1]


@paths
@modes
def test_each_planted_row_alone(handle, monkeypatch, ftz_mode, path, kind, ftz):
    """(b) Each planted row alone — the level-0 row, the mid-level one, the
    deepest — is reported as itself: a kernel that lost its check cannot hide
    behind another row's report."""
    _, name, scale, knobs, l0 = path
    setenv(monkeypatch, knobs)
    A, _, J, alone = ic.zero_pivot_case(name, scale, kind, l0)
    ftz_mode(ftz)
    il = analysed(handle, A)
    for j in J:
        assert factor(il, alone[j], kind)[1] == j, f"row {j} (level {ic.matrix(name, scale)[1].lv[j]})"


@paths
@modes
def test_bits_of_factor_and_solves(handle, monkeypatch, ftz_mode, path, kind, ftz):
    """(c) The factor with its inf and NaN, then L z = alpha x, L^T y = alpha z
    and U y = alpha z: the oracle's bits under the NaN rule (the block order
    where blocks are planned); the unit-lower solves report no pivot, the U
    solve the factor's."""
    _, name, scale, knobs, l0 = path
    setenv(monkeypatch, knobs)
    A, Ap, J, _ = ic.zero_pivot_case(name, scale, kind, l0)
    ftz_mode(ftz)
    il = analysed(handle, A)
    va, zp = factor(il, Ap, kind)
    rv, rzp = ic.oracle_factor(name, scale, kind, ftz, "all")
    assert zp == rzp == min(J)
    ic.assert_same_bits_nan(va.cpu().numpy(), rv, "factor")
    x = csr.dlarnv(2, [0, 0, 0, 1], A.n)[0].astype(ic.NP[kind])
    z = il.solve_lower(va, torch.from_numpy(x).cuda(), alpha=ALPHA)
    yt = il.solve_lower(va, z, transpose=True, alpha=ALPHA)
    assert il.solve_zero_pivot(il.TRSV_L) == -1 and il.solve_zero_pivot(il.TRSV_LT) == -1
    yu = il.solve_upper(va, z, alpha=ALPHA)
    assert il.solve_zero_pivot(il.TRSV_U) == min(J)
    rz = ob.trsv("lower_n", A.rowptr, A.colidx, rv, x, alpha=ALPHA, ftz=ftz)
    ic.assert_same_bits_nan(z.cpu().numpy(), rz, "L solve")
    ic.assert_same_bits_nan(yt.cpu().numpy(), ob.trsv("lower_t", A.rowptr, A.colidx, rv, rz, alpha=ALPHA, ftz=ftz),
                            "L^T solve")
    ic.assert_same_bits_nan(yu.cpu().numpy(), ob.trsv("upper", A.rowptr, A.colidx, rv, rz, alpha=ALPHA, ftz=ftz),
                            "U solve")
    assert not np.all(np.isfinite(rz)), "the solves must meet the factor's non-finite values"


@paths
@modes
def test_one_info_reused(handle, monkeypatch, ftz_mode, path, kind, ftz):
    """(d) Planted, clean, planted values through one info: min(J), -1,
    min(J) (the factor resets its zero-pivot word), and the clean factor has
    the oracle's bits."""
    _, name, scale, knobs, l0 = path
    setenv(monkeypatch, knobs)
    A, Ap, J, _ = ic.zero_pivot_case(name, scale, kind, l0)
    ftz_mode(ftz)
    il = analysed(handle, A)
    assert factor(il, Ap, kind)[1] == min(J)
    va, zp = factor(il, A, kind)
    assert zp == -1 and il.solve_zero_pivot(il.TRSV_U) == -1
    rv, _ = ic.oracle_factor(name, scale, kind, ftz, "clean")
    assert np.array_equal(va.cpu().numpy().view(np.uint8), rv.view(np.uint8))
    assert factor(il, Ap, kind)[1] == min(J)


@pytest.mark.parametrize("solver", [BiCGStab, GMRES])
def test_krylov_create_reports_zero_pivot(handle, solver):
    """rsp_bicgstab_create / rsp_gmres_create on a planted matrix of several
    levels: ZERO_PIVOT (U divides by its diagonal)."""
    A, Ap, J, _ = ic.zero_pivot_case("atmosmodd", 0.01, "f64", False)
    rp, ci, va = upload_csr(A.rowptr, A.colidx, A.values)
    M = SpMat(handle, rp, ci, va, A.n)
    il = Ilu0(handle, rp, ci, nnz=A.nnz)
    try:
        il.analysis()
        fac, zp = factor(il, Ap, "f64")
        assert zp == min(J)
        with pytest.raises(RspError) as e:
            solver(handle, M, il, fac)
        assert e.value.status == _lib.STATUS_ZERO_PIVOT
    finally:
        il.close()
        M.close()


# ------------------------------------------ denormal operands of qdiv (FTZ)

@pytest.mark.parametrize("ftz", [True, False], ids=["ftz", "ieee"])
@pytest.mark.parametrize("variant", [0, 1], ids=["numerator", "divisor"])
@pytest.mark.parametrize("path", ic.DENORMAL_PATHS, ids=[f"{p[0]}-{p[1]}" for p in ic.DENORMAL_PATHS])
def test_factor_division_with_denormal_operand(handle, monkeypatch, ftz_mode, path, variant, ftz):
    """l_ik = a_ik / a_kk with both operands straight from memory and one of
    them denormal (fp32). Under FTZ the operand is zero, as under the oracle's
    DAZ: a denormal numerator gives l_ik = 0 (not 2^-122), a denormal divisor
    l_ik = inf and a zero pivot at k (not 2^115 and none). Without FTZ the IEEE
    quotients. Factor and position as the oracle's. (qdiv's FTZ branch widens
    both operands to double before dividing: on the MI355X a denormal fp32
    input is flushed on the way in under the kernel's fp32 flush mode —
    measured by this test, which pins it.)"""
    _, name, scale, knobs = path
    setenv(monkeypatch, knobs)
    A, S = ic.matrix(name, scale)
    M, pairs = ic.denormal_case(name, scale)[variant]
    ftz_mode(ftz)
    va, zp = factor(analysed(handle, A), M, "f32")
    v = va.cpu().numpy()
    lik = v[[p for _, _, p in pairs]]
    print("l_ik:", lik.tolist(), "zero pivot:", zp)
    if ftz and variant == 0:
        assert np.all(lik == 0.0) and zp == -1
    elif ftz:
        assert np.all(np.isposinf(lik)) and zp == min(k for k, _, _ in pairs)
    else:
        assert np.all(lik == np.float32(2.0 ** (-122 if variant == 0 else 115))) and zp == -1
    rv, _, rzp = ob.ilu0(A.rowptr, A.colidx, M.values.astype(np.float32), ftz=ftz)
    assert zp == rzp
    ic.assert_same_bits_nan(v, rv, "factor")


@pytest.mark.parametrize("ftz", [True, False], ids=["ftz", "ieee"])
@pytest.mark.parametrize("knobs", [{}, dict(zip(ic.THIN, (1024, 1 << 30))), ic.ALL_FAT],
                         ids=["default", "all-thin", "all-fat"])
def test_upper_solve_division_with_denormal_pivot(handle, monkeypatch, ftz_mode, knobs, ftz):
    """y_i = alpha x_i / u_ii in rows without upper entries whose u_ii = 2^-135
    comes straight from memory: +-inf under FTZ, the finite IEEE quotient
    (|alpha x_i| < 2^-20) without."""
    setenv(monkeypatch, knobs)
    A, S = ic.matrix("ss1", 0.05)
    U, _, _ = ob.ilu0(A.rowptr, A.colidx, A.values.astype(np.float32))
    v, rows = ic.denormal_pivots(A, U)
    x = csr.dlarnv(2, [0, 0, 0, 1], A.n)[0].astype(np.float32)
    x[rows] *= np.float32(2.0 ** -20)
    assert np.all(x[rows] != 0)
    ftz_mode(ftz)
    il = analysed(handle, A)
    il.factor(device(A.values, "f32"))
    y = il.solve_upper(torch.from_numpy(v).cuda(), torch.from_numpy(x).cuda(), alpha=ALPHA).cpu().numpy()
    assert il.solve_zero_pivot(il.TRSV_U) == -1  # (the report is the factor's, which was clean)
    print("y_i:", y[rows].tolist())
    ax = np.float32(ALPHA) * x[rows]
    if ftz:
        assert np.all(np.isinf(y[rows])) and np.array_equal(np.signbit(y[rows]), np.signbit(ax))
    else:
        assert np.all(np.isfinite(y[rows])) and np.array_equal(y[rows], ax / np.float32(2.0 ** -135))
    ic.assert_same_bits_nan(y, ob.trsv("upper", A.rowptr, A.colidx, v, x, alpha=ALPHA, ftz=ftz), "U solve")
