"""Generators for the ILU(0) zero-pivot and non-finite tests (helper module,
no conftest): matrices whose factor has pivots that are EXACTLY zero at known
rows, fp32 matrices whose first division has a denormal operand straight from
memory, and the bitwise comparison that tolerates NaN payloads.

tests/test_ilu_cases.py proves every generator with the CPU oracle alone;
tests/test_gpu_ilu0_zero_pivot.py runs them through the kernels."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import oracle_bind as ob
from respasol_amd import csr

NP = {"f64": np.float64, "f32": np.float32}
UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}


# ------------------------------------------------------------- comparison

def assert_same_bits_nan(got, ref, what="values"):
    """Equal NaN masks and bitwise equal bytes everywhere else, signs of
    zeros and infinities included. NaN payload and sign are not compared (the
    x86 default NaN is negative, the GPU's positive): the rule of same_bits in
    tests/test_gpu_spmv.py."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype}{got.shape}, {ref.dtype}{ref.shape}"
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), (f"{what}: NaN masks differ at {np.nonzero(gn != rn)[0][:8].tolist()} "
                                    f"({int(gn.sum())} NaN got, {int(rn.sum())} expected)")
    u = UINT[got.dtype]
    bad = np.nonzero((got.view(u) != ref.view(u)) & ~rn)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ, first at {bad[:8].tolist()}: "
                           f"got {got[bad[:4]].tolist()}, expected {ref[bad[:4]].tolist()}")


# --------------------------------------------------------------- structure

class Structure:
    """Diagonal positions, L's levels (longest dependency path) and the strict
    lower part by columns (a row's children in L's dependency DAG)."""

    def __init__(self, A):
        rp, ci, n = np.asarray(A.rowptr, np.int64), np.asarray(A.colidx, np.int64), A.n
        self.n, self.rp, self.ci = n, rp, ci
        rows = np.repeat(np.arange(n), np.diff(rp))
        self.dpos = rp[:-1] + np.bincount(rows[ci < rows], minlength=n)  # first position with column >= i
        self.nlow = self.dpos - rp[:-1]
        assert np.all(self.dpos < rp[1:]) and np.all(ci[self.dpos] == np.arange(n)), "a diagonal is missing"
        self.nup = rp[1:] - self.dpos - 1
        lv = np.zeros(n, np.int64)
        for i in np.nonzero(self.nlow)[0]:
            lv[i] = lv[ci[rp[i]:self.dpos[i]]].max() + 1
        self.lv = lv
        low = ci < rows
        order = np.argsort(ci[low], kind="stable")
        self.kid_rows = rows[low][order]
        self.kid_ptr = np.concatenate(([0], np.cumsum(np.bincount(ci[low], minlength=n))))

    def kids(self, j):
        return self.kid_rows[self.kid_ptr[j]:self.kid_ptr[j + 1]]

    def descendants(self, j):
        """Every row that depends on row j in L's DAG (j itself excluded)."""
        seen, todo = set(), [int(j)]
        while todo:
            for c in self.kids(todo.pop()):
                if int(c) not in seen:
                    seen.add(int(c))
                    todo.append(int(c))
        return seen

    def find(self, i, j):
        """Position of (i, j), or -1."""
        a, b = self.rp[i], self.rp[i + 1]
        p = a + np.searchsorted(self.ci[a:b], j)
        return int(p) if p < b and self.ci[p] == j else -1

    def plantable(self, j):
        """A row with lower entries can carry a planted pivot if the pattern
        holds (k, j) for the column k of its last lower entry."""
        if self.nlow[j] == 0:
            return True
        return self.find(self.ci[self.dpos[j] - 1], j) >= 0


@functools.lru_cache(maxsize=None)
def matrix(name, scale):
    A = csr.surrogate(name, scale)
    return A, Structure(A)


# ------------------------------------------------------------ zero pivots

def _plant(A, S, U, rows):
    new = U.dtype.type(1) * A.values.astype(U.dtype)
    for j in rows:
        lo, d = S.rp[j], S.dpos[j]
        if d == lo:
            new[d] = 0.0
            continue
        k = S.ci[d - 1]
        q = S.find(k, j)
        if q < 0:
            raise ValueError(f"row {j}: the pattern has no ({k}, {j})")
        new[lo:d] = 0.0
        new[d - 1] = U[S.dpos[k]]  # l_jk = u_kk / u_kk = 1
        new[d] = U[q]              # u_jj = fma(-1, u_kj, u_kj) = 0
    return dataclasses.replace(A, values=new.astype(np.float64))


def _nonfinite(v):
    return int(np.isinf(v).sum()), int(np.isnan(v).sum())


def _accept(A, S, Ap, rows, npdt):
    """The numeric conditions of a planted set, by the oracle."""
    v, sz, zp = ob.ilu0(A.rowptr, A.colidx, Ap.values.astype(npdt))
    ninf, nnan = _nonfinite(v)
    want_nan = S.nup.any()  # (a stored lower triangle has no update: no inf - inf)
    return (sz == -1 and zp == min(rows) and all(v[S.dpos[j]] == 0 for j in rows) and ninf > 0
            and (nnan > 0 or not want_nan) and 2 * (ninf + nnan) < v.size)


def pick_rows(A, S, U, level0_only=False, scan=400, width=8):
    """At least three plantable, mutually unreachable rows: in three distinct
    levels, one at level 0, one above the median level, the smallest row index
    in neither the lowest nor the highest of their levels (level order and
    index order disagree both ways: a plain store instead of the atomic
    minimum leaves the last level's row, not the smallest), and late enough in
    the elimination that fewer than half the factor's entries become
    non-finite. With level0_only (a stored lower triangle: no
    (k, j) above the diagonal) three level-0 rows.

    An inf needs only a child of a planted row; a NaN needs an inf to meet
    another inf or a zero (a triangle of the pattern), which is rare in the
    circuit surrogates: the last `scan` candidates are factored alone to find
    one that gives a NaN, and the other two roles are filled from the `width`
    latest rows that fit."""
    npdt = U.dtype.type
    haskid = np.diff(S.kid_ptr) > 0
    zs = np.nonzero((S.nlow == 0) & haskid)[0][::-1]
    if level0_only:
        for t in range(min(scan, len(zs) - 2)):
            rows = sorted(int(z) for z in zs[t:t + 3])
            if _accept(A, S, _plant(A, S, U, rows), rows, npdt):
                return rows
        raise ValueError("no three level-0 rows meet the conditions")
    med = np.median(S.lv)
    low = [int(j) for j in np.nonzero((S.nlow > 0) & haskid)[0][::-1]]
    plantable = functools.lru_cache(maxsize=None)(S.plantable)
    desc = functools.lru_cache(maxsize=None)(S.descendants)

    def latest(rows, ok):
        out = []
        for j in rows:
            if ok(j) and plantable(j):
                out.append(int(j))
                if len(out) == width:
                    break
        return out

    def valid(h, z, m):
        # the smallest index in the middle level: neither level order nor its
        # reverse is index order, so neither the first nor the last store is right
        if not (S.lv[h] > med and 0 < S.lv[m] < S.lv[h] and m < min(h, z)):
            return False
        return not (h in desc(m) or m in desc(h) or h in desc(z) or m in desc(z))

    def gives_nan(j):
        v, _, _ = ob.ilu0(A.rowptr, A.colidx, _plant(A, S, U, [j]).values.astype(npdt))
        return bool(np.isnan(v).any())

    # first the rows just below the latest level-0 rows (where level-0 rows
    # are few, the smallest index has to come from there), then the latest rows
    cand = []
    for z in (int(z) for z in zs[:width]):
        cand += [z] + latest((j for j in low if j < z), lambda j: True)
    cand += sorted([j for j in low if plantable(j)][:scan] + [int(z) for z in zs[:scan]], reverse=True)
    for r in dict.fromkeys(cand):
        if not gives_nan(r):
            continue
        for z in ([r] if S.lv[r] == 0 else [int(z) for z in zs[:width]]):
            def near(ok):  # the latest rows below z and below r, then the latest of all
                return list(dict.fromkeys(latest((j for j in low if j < z), ok) + latest((j for j in low if j < r), ok)
                                          + latest(low, ok)))
            for role in ("z",) if S.lv[r] == 0 else ("h", "m"):
                hs = [r] if role == "h" else near(lambda j: S.lv[j] > med)
                for h in hs:
                    ms = [r] if role == "m" else near(lambda j: 0 < S.lv[j] < S.lv[h])
                    for m in ms:
                        rows = sorted((h, z, m))
                        if valid(h, z, m) and _accept(A, S, _plant(A, S, U, rows), rows, npdt):
                            return rows
    raise ValueError("no planted set meets the conditions on this matrix")


def check_unreachable(S, rows):
    for j in rows:
        d = S.descendants(j)
        hit = [r for r in rows if r in d]
        if hit:
            raise ValueError(f"planted row {j} is an ancestor of {hit}: their pivots would be NaN, not 0")


def plant_zero_pivots(A, dtype, rows=None, level0_only=False):
    """(A', J): A' has A's pattern and values for which the ILU(0) factor in
    the arithmetic of dtype (np.float64 / np.float32) has u_jj exactly zero
    for every j of J (sorted). Exact, not approximate: a row j without lower
    entries gets a_jj = 0; any other gets zeros for its lower values except
    the last, at column k, a_jk = u_kk and a_jj = u_kj bitwise from the
    oracle's factor of A, so that l_jk = 1 and u_jj = fma(-1, u_kj, u_kj) = 0
    (the zeros before k are exact no-ops, nothing lies between k and j). The
    rows must be mutually unreachable in L's DAG (a descendant's pivot would
    be NaN); rows=None picks them (pick_rows)."""
    S = Structure(A)
    U, sz, zp = ob.ilu0(A.rowptr, A.colidx, A.values.astype(dtype))
    assert sz == -1 and zp == -1 and np.all(np.isfinite(U)), "the clean factor must be finite"
    if rows is None:
        rows = pick_rows(A, S, U, level0_only)
    rows = sorted(int(j) for j in rows)
    check_unreachable(S, rows)
    return _plant(A, S, U, rows), rows


@functools.lru_cache(maxsize=None)
def zero_pivot_case(name, scale, kind, level0_only=False):
    """(A, A', J, {j: A' with row j alone planted}) for a surrogate and
    "f64" / "f32"; computed once per session."""
    A, _ = matrix(name, scale)
    Ap, J = plant_zero_pivots(A, NP[kind], level0_only=level0_only)
    alone = {j: plant_zero_pivots(A, NP[kind], rows=[j])[0] for j in J}
    return A, Ap, J, alone


# ------------------------------------------------------ denormal operands

NUM = (2.0 ** -8, 2.0 ** -130)   # a_kk, a_ik: l_ik = 2^-122, or 0 with the numerator flushed
DIV = (2.0 ** -135, 2.0 ** -20)  # a_kk, a_ik: l_ik = 2^115, or inf with the divisor flushed


def _den_ok(A, S, vals, pairs, which):
    """The oracle's verdict on one variant (the conditions of test_ilu_cases)."""
    v32 = vals.astype(np.float32)
    lik = [p for _, _, p in pairs]
    vf, _, zf = ob.ilu0(A.rowptr, A.colidx, v32, ftz=True)
    vn, _, zn = ob.ilu0(A.rowptr, A.colidx, v32, ftz=False)
    if which == "num":
        return zf == -1 and zn == -1 and np.all(vf[lik] == 0) and np.all(vn[lik] == np.float32(2.0 ** -122))
    return (zf == min(k for k, _, _ in pairs) and zn == -1 and np.all(np.isposinf(vf[lik]))
            and np.all(vn[lik] == np.float32(2.0 ** 115)))


def plant_denormal_operands(A, pairs=4):
    """Two fp32 variants of A, each ((A', [(k, i, position of l_ik)])): for
    `pairs` level-0 rows k, each with a dependent row i whose FIRST lower
    entry is (i, k), the numerator variant sets a_kk = 2^-8, a_ik = 2^-130 and
    the divisor variant (other pairs) a_kk = 2^-135, a_ik = 2^-20. The first
    lower entry of a row has an empty update list and a level-0 diagonal is
    never updated, so both operands of l_ik = a_ik / a_kk come straight from
    memory. The rows i are spread over L's levels (thin and wide ones)."""
    S = Structure(A)
    first = S.ci[S.rp[:-1]]
    cand = [i for i in np.nonzero(S.nlow > 0)[0] if S.nlow[first[i]] == 0]
    # one i per k (the k with the fewest dependents first: fewer rows beside the pair change)
    cand.sort(key=lambda i: (S.kids(first[i]).size, S.lv[i], i))
    by_k = {}
    for i in cand:
        by_k.setdefault(int(first[i]), int(i))
    spread = sorted(by_k.items(), key=lambda ki: (S.lv[ki[1]], ki[1]))
    out = []
    for which, (akk, aik), start in (("num", NUM, 0), ("div", DIV, 1)):
        pool = spread[start::2]
        step = max(len(pool) // pairs, 1)
        chosen, vals = [], A.values.copy()
        for k, i in pool[::step] + pool:
            if len(chosen) == pairs:
                break
            if any(k == c[0] or i == c[1] for c in chosen):
                continue
            trial = vals.copy()
            trial[S.dpos[k]], trial[S.rp[i]] = akk, aik
            if _den_ok(A, S, trial, chosen + [(k, i, int(S.rp[i]))], which):
                vals = trial
                chosen.append((k, i, int(S.rp[i])))
        if len(chosen) < pairs:
            raise ValueError(f"only {len(chosen)} {which} pairs meet the conditions")
        out.append((dataclasses.replace(A, values=vals), chosen))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def denormal_case(name, scale):
    return plant_denormal_operands(matrix(name, scale)[0])


def denormal_pivots(A, U, rows=6):
    """U (a clean fp32 factor of A) with u_ii = 2^-135 in `rows` rows without
    upper entries (their U solve is y_i = alpha x_i / u_ii and nothing else),
    spread over the matrix: (values, rows)."""
    S = Structure(A)
    last = np.nonzero(S.nup == 0)[0]
    assert last.size >= rows, "too few rows without upper entries"
    pick = last[np.linspace(0, last.size - 1, rows).astype(int)]
    v = np.array(U, np.float32)
    v[S.dpos[pick]] = np.float32(2.0 ** -135)
    return v, pick


# ------------------------------------------------------------ kernel paths
# (id, surrogate, scale, environment knobs, level0_only): the knob sets of the
# path tests of tests/test_gpu_ilu0.py, which route every level through one
# kernel. The stencil3d surrogates those tests use (stomach, xenon2,
# FEM_3D_thermal2) cannot carry a planted set: in the natural order their only
# level-0 row is row 0, the smallest index of any set and at the lowest level,
# so "level order and index order disagree" has no solution. They are replaced
# by surrogates of the same tests with level-0 rows throughout (ss1,
# ASIC_320ks, tmt_unsym) or, for a 3-D stencil, atmosmodd. The picked rows lie
# late in the elimination (few non-finite entries), where a stencil's levels
# are narrow again, so the flow paths force every level fat, as
# test_numerical_zero_pivot and the give-up tests do.

THIN = _THIN = ("RSP_ILU_THIN_SOLVE", "RSP_ILU_THIN_FACTOR")
_FAT = ("RSP_ILU_FAT_SLOT", "RSP_ILU_FAT_LDS", "RSP_ILU_FAT_PAD", "RSP_ILU_WAVE_LDS", "RSP_ILU_FAT_LONG")
_FLOW = ("RSP_ILU_FLOW", "RSP_ILU_FLOW_WPC", "RSP_ILU_FLOW_MODE")
ALL_FAT = dict(zip(_THIN, (0, 0)))
FAT_SETS = ((0, 1, 0, 0, 3), (0, 0, 1, 1, 8), (1, 1, 1, 1, 8), (1, 1, 1, 0, 3), (1, 1, 0, 1, 1))  # test_fat_level_paths


def _fat(knobs):
    return {**dict(zip(_FAT, knobs)), **ALL_FAT}


PATHS = (
    [("default", "atmosmodd", 0.01, {}, False), ("default", "tmt_unsym", 0.02, {}, False)]
    # test_schedule_variants: every level launched / every level in thin runs / mixed
    + [(f"schedule-{s}-{f}", "ss1", 0.05, dict(zip(_THIN, (s, f))), False)
       for s, f in ((0, 0), (1024, 1 << 30), (1, 1))]
    # test_fat_level_paths: global memory, FacRow + LDS, slot layout
    + [("fat-" + "-".join(map(str, k)), name, scale, _fat(k), False)
       for k in FAT_SETS for name, scale in (("crashbasis", 0.1), ("ASIC_320ks", 0.1))]
    # test_flow_segments: a launch per level, flow launches walked statically / by start tickets
    + [("flow-" + "-".join(map(str, k)), "tmt_unsym", 0.02, {**dict(zip(_FLOW, k)), **ALL_FAT}, False)
       for k in ((0, 8, 0), (1, 4, 0), (1, 4, 2))]
    # test_factor_narrow_waves
    + [(f"narrow-{w}", "dc1", 0.3, {"RSP_ILU_FNARROW_WAVES": w}, False) for w in (1, 4, 16)]
    # a stored lower triangle: ilu0_scale_lower, the one-level plan, L's levels
    + [("lower-scale", "G2_circuit", 0.2, {"RSP_ILU_FAC_SCALE": 1}, True),
       ("lower-one-level", "G2_circuit", 0.2, {"RSP_ILU_FAC_SCALE": 0}, True),
       ("lower-levels", "G2_circuit", 0.2, {"RSP_ILU_FAC_ONE": 0}, True)]
    # block-inverse solves: forced, and the default plan of a deep DAG
    + [("blocks-forced", "atmosmodd", 0.01, {"RSP_ILU_BLOCKS": 1}, False),
       ("blocks-default", "dc1", 0.1, {}, False)])
PATH_IDS = [f"{p[0]}-{p[1]}" for p in PATHS]
ZP_MATRICES = sorted({(p[1], p[2], p[4]) for p in PATHS})

# the paths with a factor kernel of their own, for the denormal operands
DENORMAL_PATHS = [
    ("default", "tmt_unsym", 0.02, {}),
    ("fat-global", "crashbasis", 0.1, _fat(FAT_SETS[1])),
    ("fat-lds", "crashbasis", 0.1, _fat(FAT_SETS[0])),
    ("fat-slot", "crashbasis", 0.1, {**_fat(FAT_SETS[2]), "RSP_ILU_FLOW": 0}),
    ("flow", "tmt_unsym", 0.02, {**dict(zip(_FLOW, (1, 4, 2))), **ALL_FAT}),
    ("narrow", "dc1", 0.3, {"RSP_ILU_FNARROW_WAVES": 4}),
    ("lower-scale", "G2_circuit", 0.2, {"RSP_ILU_FAC_SCALE": 1}),
]
DENORMAL_MATRICES = sorted({(p[1], p[2]) for p in DENORMAL_PATHS})
MODES = (("f64", False), ("f32", False), ("f32", True))


@functools.lru_cache(maxsize=None)
def oracle_factor(name, scale, kind, ftz, which):
    """The oracle's (values, zero pivot) for a zero-pivot case: which =
    "clean", "all" or a planted row (that row alone)."""
    A, Ap, J, alone = zero_pivot_case(name, scale, kind, not matrix(name, scale)[1].nup.any())
    M = A if which == "clean" else Ap if which == "all" else alone[which]
    v, sz, zp = ob.ilu0(M.rowptr, M.colidx, M.values.astype(NP[kind]), ftz=ftz)
    assert sz == -1
    v.setflags(write=False)
    return v, zp
