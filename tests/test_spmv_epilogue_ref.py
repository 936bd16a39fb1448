"""CPU checks of the SpMV epilogue restatement (tests/spmv_epilogue_ref.py) and
of the matrices that tests/test_gpu_spmv_axpby.py runs on the device: the
restatement against exact arithmetic, the row-length-to-site rule, every
mutant visible at every site under (1/3, -0.7) for the committed seeds and
invisible under the power-of-two scalars (2, 0.5) the older tests used, the
matrix reaching every site with the rows the GPU tests plant into."""
from fractions import Fraction

import numpy as np
import pytest

import oracle_bind as ob
import spmv_epilogue_ref as er

DTYPES = [np.float64, np.float32]
MAXROWS = {np.dtype(np.float64): 512, np.dtype(np.float32): 1024}  # SpmvTile<T>::kMaxRows
# the groups whose rows a mutant can change (an empty row has s = +0: nothing to round)
SHOWING = ("tile", "heavy", "whole", "chunk", "chunk65")


def applicable(mutant, grp, dtype):
    if mutant == "wide":
        return np.dtype(dtype) == np.float32
    if mutant == "alpha_per_chunk":
        return grp in ("chunk", "chunk65")
    return True


def changed_rows(case, alpha, beta, mutant):
    plain = er.epilogue(case.s, case.y0, alpha, beta)
    mut = er.epilogue(case.s, case.y0, alpha, beta, mutate=mutant, partials=case.partials)
    return np.flatnonzero(er.bits(plain) != er.bits(mut))


@pytest.mark.parametrize("dtype", DTYPES)
def test_site_classification(dtype):
    cap = er.cap_of(dtype)
    assert cap == {np.float64: 2047, np.float32: 4093}[dtype]
    for length, want, grp, n in [(0, "tile", "empty", 1), (1, "tile", "tile", 1), (32, "tile", "tile", 1),
                                 (33, "tile", "heavy", 1), (256, "tile", "heavy", 1), (257, "whole", "whole", 1),
                                 (cap, "whole", "whole", 1), (cap + 1, "chunked", "chunk", 2),
                                 (2 * cap, "chunked", "chunk", 2), (2 * cap + 1, "chunked", "chunk", 3),
                                 (64 * cap, "chunked", "chunk", 64), (64 * cap + 1, "chunked", "chunk65", 65),
                                 (65 * cap, "chunked", "chunk65", 65), (65 * cap + 1, "chunked", "chunk65", 66),
                                 (65 * cap + 7, "chunked", "chunk65", 66), (66 * cap, "chunked", "chunk65", 66)]:
        assert er.site(length, cap) == want, length
        assert er.group(length, cap) == grp, length
        assert er.nchunks(length, cap) == n, length


@pytest.mark.parametrize("dtype", DTYPES)
def test_matrix_reaches_every_site(dtype):
    case = er.epilogue_case(dtype)
    cap, lens, g = case.cap, case.lens, case.groups
    assert 200 <= case.A.m <= 600 and case.A.n == 66 * cap + 64
    assert sum(len(v) for v in g.values()) == case.A.m
    for length in (256, 257, cap, cap + 1, 2 * cap, 2 * cap + 1, 64 * cap, 64 * cap + 1, 65 * cap + 7):
        assert np.count_nonzero(lens == length) >= 1, length
    assert len(g["empty"]) >= 1 and np.count_nonzero((lens >= 1) & (lens <= 8)) >= 8
    assert len(g["tile"]) >= 8 and len(g["heavy"]) >= 8 and len(g["whole"]) >= 8
    assert np.count_nonzero([2 <= er.nchunks(int(k), cap) <= 3 for k in lens]) >= 8
    assert len(g["chunk65"]) >= 3
    assert sorted(er.nchunks(int(lens[r]), cap) for r in g["chunk65"])[-1] == 66
    # rows of 33-256 entries that the tile's second pass sums (full-tile schedule)
    heavy = er.heavy_pass_rows(lens, cap, MAXROWS[np.dtype(dtype)])
    assert len(heavy) >= 8 and set(heavy) <= set(g["heavy"])
    assert {33, 256} <= set(int(lens[r]) for r in heavy)
    # sorted, distinct columns in every row
    ci = case.A.colidx.astype(np.int64)
    inner = np.ones(len(ci), bool)
    inner[case.A.rowptr[:-1][lens > 0]] = False
    assert np.all(np.diff(ci)[inner[1:]] > 0)
    # the canonical sums are the in-order sums of the oracle's chunk partials
    T = np.dtype(dtype).type
    for r, part in case.partials.items():
        assert len(part) == er.nchunks(int(lens[r]), cap)
        acc = T(0)
        for p in part:
            acc = T(acc + p)
        assert er.bits(np.array([acc]))[0] == er.bits(case.s[r:r + 1])[0], r


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_rows_and_columns(dtype):
    """Every planted row's own column is referenced by that one entry alone,
    in the middle of the row (a middle chunk of a chunked one, with its
    neighbour); the unreferenced columns are, the last column among them."""
    case = er.epilogue_case(dtype)
    A, cap = case.A, case.cap
    count = np.bincount(A.colidx, minlength=A.n)
    assert set(case.plants) == set(SHOWING)
    for grp, (row, k) in case.plants.items():
        assert er.group(int(case.lens[row]), cap) == grp
        assert A.rowptr[row] < k < A.rowptr[row + 1] - 1
        assert count[A.colidx[k]] == 1
        assert case.x[A.colidx[k]] != 0 and case.x[A.colidx[k + 1]] != 0
        n = er.nchunks(int(case.lens[row]), cap)
        if n > 1:
            c = (k - A.rowptr[row]) // cap
            assert 0 < c < n - 1 and (k + 1 - A.rowptr[row]) // cap == c
    assert len(case.unreferenced) >= 3 and A.n - 1 in case.unreferenced
    assert np.all(count[case.unreferenced] == 0)
    assert set(np.flatnonzero(count == 0)) == set(case.unreferenced)


@pytest.mark.parametrize("dtype", DTYPES)
def test_restatement_against_exact_arithmetic(dtype):
    """epilogue() is two rounded products and one rounded sum: each compared
    with the exact value rounded once (Fraction), on every row of the case."""
    case = er.epilogue_case(dtype)
    T = np.dtype(dtype).type
    for alpha, beta in er.SCALARS:
        got = er.epilogue(case.s, case.y0, alpha, beta)
        assert got.dtype == np.dtype(dtype)
        a, b = T(alpha), T(beta)
        for i in range(case.A.m):
            fa = Fraction(float(a)) * Fraction(float(case.s[i]))
            pa = er._round_fraction(fa, T) if fa != 0 else T(a * case.s[i])
            want = pa
            if b != 0:
                fb = Fraction(float(b)) * Fraction(float(case.y0[i]))
                pb = er._round_fraction(fb, T) if fb != 0 else T(b * case.y0[i])
                fs = Fraction(float(pa)) + Fraction(float(pb))
                want = er._round_fraction(fs, T) if fs != 0 else T(pa + pb)
            assert er.bits(np.array([want], T))[0] == er.bits(got[i:i + 1])[0], (alpha, beta, i)


def test_round_fraction_ties_and_double_rounding():
    """Ties go to even, and a value that rounding through fp64 gets wrong in
    fp32 is rounded once."""
    one = Fraction(1)
    for T, p in ((np.float32, 23), (np.float64, 52)):
        ulp = Fraction(1, 2 ** p)
        assert er._round_fraction(one + ulp / 2, T) == T(1)                      # tie: down to even
        assert er._round_fraction(one + 3 * ulp / 2, T) == T(1) + T(2.0 ** -p) * 2  # tie: up to even
        assert er._round_fraction(one + ulp / 2 + ulp / 2 ** 40, T) == T(1) + T(2.0 ** -p)
    # just above a fp32 tie, by less than fp64 resolves: fp64 first would land on the tie, then on even
    fr = one + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)
    assert np.float32(float(fr)) == np.float32(1)
    assert er._round_fraction(fr, np.float32) == np.float32(1) + np.float32(2.0 ** -23)


@pytest.mark.parametrize("dtype", DTYPES)
def test_beta_zero_does_not_use_y0(dtype):
    case = er.epilogue_case(dtype)
    nan = np.full(case.A.m, np.nan, dtype)
    for beta in (0.0, -0.0):
        out = er.epilogue(case.s, nan, 1.7, beta)
        assert np.array_equal(er.bits(out), er.bits(er.epilogue(case.s, case.y0, 1.7, beta)))
        assert np.all(np.isfinite(out))


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_rows_with_negative_alpha(dtype):
    """(-1, 0) on an empty row gives -0.0 = alpha * (+0); (-1, 1) leaves y0."""
    case = er.epilogue_case(dtype)
    rows = case.groups["empty"]
    assert np.all(er.bits(case.s[rows]) == 0)
    out = er.epilogue(case.s, case.y0, -1.0, 0.0)[rows]
    assert np.all(out == 0) and np.all(np.signbit(out))
    out = er.epilogue(case.s, case.y0, -1.0, 1.0)[rows]
    assert np.array_equal(er.bits(out), er.bits(case.y0[rows]))
    e = er.empty_case(dtype)
    assert len(e.groups["empty"]) == e.A.m
    assert np.all(np.signbit(er.epilogue(e.s, e.y0, -1.0, 0.0)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_mutant_shows_at_every_site(dtype):
    """Under (1/3, -0.7) each applicable mutant changes the bits of at least
    one row of every group: a condition on the committed seed, not a
    tolerance. A group where a mutant changed nothing would let the GPU test
    pass on that mutant."""
    case = er.epilogue_case(dtype)
    alpha, beta = er.SCALARS[0]
    assert (alpha, beta) == (1.0 / 3.0, -0.7)
    for mutant in er.MUTANTS:
        if not applicable(mutant, "chunk", dtype):  # wide on fp64
            continue
        rows = set(changed_rows(case, alpha, beta, mutant))
        for grp in SHOWING:
            if applicable(mutant, grp, dtype):
                assert rows & set(case.groups[grp]), (mutant, grp)
        if mutant == "alpha_per_chunk":  # rows of one chunk are not touched
            assert rows <= set(case.groups["chunk"]) | set(case.groups["chunk65"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_power_of_two_scalars_hide_every_mutant(dtype):
    """Under (2.0, 0.5) both scalings are exact (no product lands in the
    subnormal range on data from [-1, 1]), so no mutant changes any bit: the
    reason the older (2, 0.5) tests could not see them."""
    case = er.epilogue_case(dtype)
    tiny = np.finfo(dtype).tiny
    s2, y2 = np.abs(2.0 * case.s.astype(np.float64)), np.abs(0.5 * case.y0.astype(np.float64))
    assert np.all((s2 == 0) | (s2 >= tiny)) and np.all((y2 == 0) | (y2 >= tiny))
    for mutant in er.MUTANTS:
        if applicable(mutant, "chunk", dtype):
            assert len(changed_rows(case, 2.0, 0.5, mutant)) == 0, mutant


def test_ftz_restatement_applies_to_the_fp32_case():
    """The fp32 data holds no subnormal operand, product, sum or scaled value,
    so the flush-to-zero kernels must give the plain restatement's bits."""
    for case in (er.epilogue_case(np.float32), er.stencil_case(np.float32, "stencil3d:20000:360000:S")):
        tiny = np.finfo(np.float32).tiny
        prod = np.abs(case.vals[:case.A.nnz_stored] * case.x[case.A.colidx])
        for a in (np.abs(case.vals), np.abs(case.x), np.abs(case.y0), prod, np.abs(case.s)):
            assert np.all((a == 0) | (a >= tiny))
        assert np.array_equal(er.bits(case.canon(ftz=True)), er.bits(case.s))
        for alpha, beta in er.SCALARS:
            for a in (np.abs(np.float32(alpha) * case.s), np.abs(np.float32(beta) * case.y0),
                      np.abs(er.epilogue(case.s, case.y0, alpha, beta))):
                assert np.all((a == 0) | (a >= tiny))
