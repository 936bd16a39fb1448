"""The generators of tests/ilu_cases.py, proved with the CPU oracle alone, so
that tests/test_gpu_ilu0_zero_pivot.py cannot pass vacuously: for every
(matrix, type) the GPU file uses, the planted pivots are exactly zero where
they are meant to be, the oracle reports the smallest, the factor really holds
inf and NaN, and the denormal operands behave as DAZ/FTZ says."""
import numpy as np
import pytest

import ilu_cases as ic
import oracle_bind as ob

ZP = [(n, s, l0, k) for n, s, l0 in ic.ZP_MATRICES for k in ("f64", "f32")]


@pytest.mark.parametrize("name,scale,level0_only,kind", ZP, ids=[f"{n}-{s}-{k}" for n, s, _, k in ZP])
def test_planted_zero_pivots(name, scale, level0_only, kind):
    A, S = ic.matrix(name, scale)
    _, Ap, J, alone = ic.zero_pivot_case(name, scale, kind, level0_only)
    assert level0_only == (not S.nup.any())
    assert len(J) >= 3 and J == sorted(set(J))
    assert np.array_equal(Ap.rowptr, A.rowptr) and np.array_equal(Ap.colidx, A.colidx)
    # the picker's level and index conditions
    lv = S.lv[J]
    assert 0 in lv
    if level0_only:
        assert not lv.any()
    else:
        assert len(set(lv.tolist())) >= 3 and lv.max() > np.median(S.lv)
        assert lv[0] != lv.min(), "the smallest row index must not be in the lowest level"
        assert lv[0] != lv.max(), "nor in the highest (the last store would be the right one)"
    for j in J:
        assert not (S.descendants(j) & set(J)), "planted rows must be mutually unreachable"
    for ftz in ((False, True) if kind == "f32" else (False,)):
        v, zp = ic.oracle_factor(name, scale, kind, ftz, "all")
        assert zp == min(J)
        for j in J:  # bitwise +0.0 or -0.0
            assert v[S.dpos[j]] == 0 and not (v[S.dpos[j]:S.dpos[j] + 1].view(ic.UINT[v.dtype]) << 1).any()
        ninf, nnan = int(np.isinf(v).sum()), int(np.isnan(v).sum())
        assert ninf >= 1 and 2 * (ninf + nnan) < v.size
        # (a stored lower triangle has no update pairs: nothing subtracts an
        # inf from an inf or multiplies one by a zero; its NaN come with the solves)
        assert nnan >= 1 or level0_only
        for j in J:  # each planted row alone is reported as itself
            assert ic.oracle_factor(name, scale, kind, ftz, j)[1] == j
        assert ic.oracle_factor(name, scale, kind, ftz, "clean")[1] == -1


def test_plant_rejects_reachable_rows():
    A, S = ic.matrix("ss1", 0.05)
    j = int(np.nonzero(S.nlow)[0][-1])
    k = int(S.ci[S.dpos[j] - 1])
    with pytest.raises(ValueError):
        ic.plant_zero_pivots(A, np.float64, rows=[k, j])


@pytest.mark.parametrize("name,scale", ic.DENORMAL_MATRICES)
def test_planted_denormal_operands(name, scale):
    A, S = ic.matrix(name, scale)
    (An, pn), (Ad, pd) = ic.denormal_case(name, scale)
    assert len(pn) >= 4 and len(pd) >= 4
    assert not {k for k, _, _ in pn} & {k for k, _, _ in pd}
    for k, i, p in pn + pd:  # level-0 row k, (i, k) the first lower entry of row i
        assert S.nlow[k] == 0 and S.nlow[i] > 0 and p == S.rp[i] and S.ci[p] == k
    num = An.values.astype(np.float32)
    lik = [p for _, _, p in pn]
    v, _, zp = ob.ilu0(A.rowptr, A.colidx, num, ftz=True)
    assert zp == -1 and np.all(v[lik] == 0.0)
    v, _, zp = ob.ilu0(A.rowptr, A.colidx, num, ftz=False)
    assert zp == -1 and np.all(v[lik] == np.float32(2.0 ** -122))
    div = Ad.values.astype(np.float32)
    lik, ks = [p for _, _, p in pd], sorted(k for k, _, _ in pd)
    v, _, zp = ob.ilu0(A.rowptr, A.colidx, div, ftz=True)
    assert np.all(np.isposinf(v[lik])) and zp == ks[0]
    assert np.all(v[S.dpos[ks]] == np.float32(2.0 ** -135))  # denormal, untouched
    v, _, zp = ob.ilu0(A.rowptr, A.colidx, div, ftz=False)
    assert zp == -1 and np.all(v[lik] == np.float32(2.0 ** 115))


def test_assert_same_bits_nan():
    a = np.array([1.0, np.nan, 0.0, np.inf], np.float32)
    b = a.copy()
    b[1:2].view(np.uint32)[:] = 0xFFC00001  # another NaN: sign and payload are not compared
    ic.assert_same_bits_nan(a, b)
    for i, x in ((2, -0.0), (3, -np.inf), (0, np.nan), (1, 1.0)):
        c = a.copy()
        c[i] = x
        with pytest.raises(AssertionError):
            ic.assert_same_bits_nan(c, a)
