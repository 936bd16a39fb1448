"""The SpMV epilogue y = alpha*A*x + beta*y restated on the CPU (test
infrastructure for test_spmv_epilogue_ref.py and test_gpu_spmv_axpby.py).

rsp_spmv, rsp_spmv_part and rsp_spmv_batch_run apply the two scalars in four
places of spmv.hip; which one a row takes is a function of its length alone
(site(), cap = oracle_bind.TILE_CAP of the type):

  at most 256 entries   the tile's sink (reduce_rows; reduce_heavy_rows for the
                        33-256-entry rows of a tile of short rows)
  257 .. cap            a whole long row (reduce_long)
  more than cap         ceil(len / cap) chunks, finished by the last-arriving
                        chunk (longrow_arrive) or, with RSP_SPMV_VARIANT bit 8,
                        by the fixup kernel (fixup_row)

All four compute the same thing, and epilogue() is its one restatement: with s
the row's sum in the oracle's canonical order and T the compute type,

    y = round(T(alpha) * s)                        if beta == 0 (either sign:
                                                   y0 is not used at all)
    y = round(round(T(alpha) * s) + round(T(beta) * y0))   otherwise

two rounded products and one rounded sum, no fused multiply-add (the library is
built with -ffp-contract=off). All arithmetic is in numpy arrays of T.

Mutation hook: epilogue(..., mutate=...) returns deliberately wrong forms, the
ones a kernel could slip into without any other test noticing:

  fma_beta         fma(beta, y0, round(alpha*s))
  fma_alpha        fma(alpha, s, round(beta*y0))
  wide             fp32 only: the expression evaluated in fp64, rounded once
  alpha_per_chunk  chunked rows only: alpha applied to each chunk partial
                   before the in-order sum (needs partials=)

The fused forms are computed exactly (fractions.Fraction, rounded once to T).

epilogue_case(dtype) is the one seeded matrix per type that reaches every
site, with its x, y0, canonical s and chunk partials; GROUPS names the row
groups the tests assert on one by one.
"""
import functools
from fractions import Fraction

import numpy as np

import oracle_bind as ob
from respasol_amd import csr

# (alpha, beta): inexact scalings, a sign flip, alpha == 0, and both zeros of beta
SCALARS = [(1.0 / 3.0, -0.7), (-1.0, 1.0), (0.0, 0.3), (1.7, 0.0), (1.7, -0.0)]
MUTANTS = ("fma_beta", "fma_alpha", "wide", "alpha_per_chunk")
LONG_ROW = 256  # rsp::kSpmvLongRow
# row groups by length (a site, or the part of one the tests want named)
GROUPS = ("empty", "tile", "heavy", "whole", "chunk", "chunk65")
# seeds of epilogue_case: every applicable mutant shows in every group
# (test_spmv_epilogue_ref.py asserts it)
SEED = {np.dtype(np.float64): 4, np.dtype(np.float32): 1}


def cap_of(dtype):
    return ob.TILE_CAP[np.dtype(dtype)]


def nchunks(length, cap):
    return (length + cap - 1) // cap if length > cap else 1


def site(length, cap):
    """The place of spmv.hip that writes a row of `length` entries."""
    if length <= LONG_ROW:
        return "tile"
    return "whole" if length <= cap else "chunked"


def group(length, cap):
    if length == 0:
        return "empty"
    if length <= 32:
        return "tile"
    if length <= LONG_ROW:
        return "heavy"
    if length <= cap:
        return "whole"
    return "chunk" if nchunks(length, cap) <= 64 else "chunk65"


def groups_of(rowptr, cap):
    """GROUPS name -> the rows of that group."""
    names = np.array([group(int(k), cap) for k in np.diff(np.asarray(rowptr, np.int64))])
    return {g: np.flatnonzero(names == g) for g in GROUPS}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _round_fraction(fr, T):
    """A non-zero exact value rounded once to T (nearest, ties to even)."""
    c = T(float(fr))  # float() rounds a Fraction correctly to fp64: within one ulp of T's answer
    cands = (np.nextafter(c, T(-np.inf)), c, np.nextafter(c, T(np.inf)))
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - fr), int(bits(np.array([v], T))[0]) & 1))


def _fma(a, b, c, T):
    """fma(a, b, c) in T: the exact a*b + c rounded once."""
    assert np.isfinite(a) and np.isfinite(b) and np.isfinite(c)
    fr = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if fr == 0:  # a zero product plus a zero, or exact cancellation: T's own arithmetic is exact here
        return T(T(a) * T(b) + T(c))
    return _round_fraction(fr, T)


def epilogue(s, y0, alpha, beta, mutate=None, partials=None):
    """y of the call (alpha, beta) on rows whose canonical sums are s and whose
    old values are y0. partials (alpha_per_chunk): {row: its chunk partials}."""
    s = np.ascontiguousarray(s)
    T = s.dtype.type
    a, b = T(alpha), T(beta)
    beta_nz = b != 0  # false for -0.0
    if mutate is None:
        out = a * s
        if beta_nz:
            out = out + b * np.ascontiguousarray(y0, s.dtype)
        assert out.dtype == s.dtype
        return out
    assert mutate in MUTANTS
    y0 = np.ascontiguousarray(y0, s.dtype)
    if mutate == "wide":
        assert s.dtype == np.float32, "wide: fp32 only"
        out = np.float64(a) * s.astype(np.float64)
        if beta_nz:
            out = out + np.float64(b) * y0.astype(np.float64)
        return out.astype(np.float32)
    if mutate == "alpha_per_chunk":
        out = epilogue(s, y0, alpha, beta)
        for row, part in partials.items():
            if len(part) < 2:
                continue
            acc = T(0)
            for p in np.asarray(part, s.dtype):
                acc = T(acc + T(a * p))
            out[row] = T(acc + T(b * y0[row])) if beta_nz else acc
        return out
    if not beta_nz:  # nothing to fuse
        return epilogue(s, y0, alpha, beta)
    out = np.empty_like(s)
    for i in range(len(s)):
        if mutate == "fma_beta":
            out[i] = _fma(b, y0[i], T(a * s[i]), T)
        else:
            out[i] = _fma(a, s[i], T(b * y0[i]), T)
    return out


# ---------------------------------------------------------------- the matrix

class Case:
    """One matrix with everything the tests share about it (read-only)."""

    def __init__(self, A, x, y0, plants=None, unreferenced=None):
        self.A, self.x, self.y0 = A, x, y0
        self.dtype = x.dtype
        self.cap = cap_of(x.dtype)
        self.vals = A.values.astype(x.dtype)
        self.lens = np.diff(np.asarray(A.rowptr, np.int64))
        self.groups = groups_of(A.rowptr, self.cap)
        self.s = ob.spmv(A.rowptr, A.colidx, self.vals, x, order="canon")
        self.plants = plants or {}            # group -> (row, entry index of its private column)
        self.unreferenced = unreferenced if unreferenced is not None else np.zeros(0, np.int64)
        for a in (self.x, self.y0, self.vals, self.s):
            a.setflags(write=False)

    @functools.cached_property
    def partials(self):
        """{row: chunk partials} of the chunked rows."""
        rows = np.concatenate([self.groups["chunk"], self.groups["chunk65"]])
        return {int(r): ob.spmv_canon_partials(self.A.rowptr, self.A.colidx, self.vals, self.x, int(r))
                for r in rows}

    def canon(self, vals=None, x=None, ftz=False):
        """The canonical-order sums of (possibly planted) data."""
        return ob.spmv(self.A.rowptr, self.A.colidx, self.vals if vals is None else vals,
                       self.x if x is None else x, ftz=ftz, order="canon")


def row_lengths(cap, rng):
    """The row lengths of epilogue_case: every site, its edges, >= 8 rows at
    each of tile / heavy / whole / 2-3 chunks and 3 rows of more than 64."""
    def shorts(k):
        return [int(v) for v in rng.choice([0, 1, 1, 2, 3, 4, 5, 6, 7, 8], k)]

    lens = []
    # a tile of > 128 rows: one lane per row, its 33-256-entry rows go to reduce_heavy_rows
    for h in (33, 256, 40, 65, 129, 50, 34, 100):
        lens += shorts(18) + [h]
    specials = [257, cap, 258, 300, 512, 513, 1025, cap - 1, (cap + 257) // 2,            # whole rows
                cap + 1, 2 * cap, 2 * cap + 1, cap + 300, 2 * cap - 1, 3 * cap,           # 2-3 chunks
                2 * cap + 257, cap + cap // 2, 3 * cap - 5,
                64 * cap, 64 * cap + 1, 65 * cap, 65 * cap + 7]                           # 64, 65, 65, 66 chunks
    for k in rng.permutation(len(specials)):
        lens += [specials[k]] + shorts(int(rng.integers(0, 4)))
    # heavy rows of every width among short rows, over several tiles
    for h in rng.integers(33, 257, 16):
        lens += shorts(8) + [int(h)]
    lens += [0, 3]  # the last tile ends the arrays
    return np.array(lens, np.int64)


@functools.lru_cache(maxsize=None)
def epilogue_case(dtype, seed=None):
    """The seeded matrix of one type: a few hundred rows by about 66 * cap
    columns. One row per non-empty group (plants) holds, in the middle of the
    row (a middle chunk of a chunked one), the only entry of a column of its
    own; a few columns, the last among them, are referenced by no row."""
    dtype = np.dtype(dtype)
    cap = cap_of(dtype)
    rng = np.random.default_rng(SEED[dtype] if seed is None else seed)
    lens = row_lengths(cap, rng)
    m, cols = len(lens), 66 * cap + 64
    mid = cols // 2
    own = {"tile": mid - 40, "heavy": mid - 20, "whole": mid, "chunk": mid + 20, "chunk65": mid + 40}
    unref = np.array([7, cols // 3, cols - 1], np.int64)
    pool = np.setdiff1d(np.arange(cols), np.concatenate([list(own.values()), unref]))
    # the planted rows: a 4-8-entry row, the 129-entry heavy row, the 1025-entry
    # whole row, the 3-chunk row 3 cap and the 66-chunk row
    want = {"tile": next(i for i, k in enumerate(lens) if 4 <= k <= 8), "heavy": int(np.flatnonzero(lens == 129)[0]),
            "whole": int(np.flatnonzero(lens == 1025)[0]), "chunk": int(np.flatnonzero(lens == 3 * cap)[0]),
            "chunk65": int(np.flatnonzero(lens == 65 * cap + 7)[0])}
    planted = {r: g for g, r in want.items()}
    rows = []
    for i, k in enumerate(lens):
        k = int(k)
        g = planted.get(i)
        draw = k - 1 if g else k
        if k <= LONG_ROW:  # a window of the pool (around the row's own column, if it has one)
            w = max(4 * k, 64)
            c0 = int(np.searchsorted(pool, own[g])) - w // 2 if g else int(rng.integers(0, len(pool) - w))
            c = rng.choice(pool[c0:c0 + w], draw, replace=False)
        else:
            c = rng.choice(pool, draw, replace=False)
        if g:
            c = np.append(c, own[g])
        rows.append(np.sort(c).astype(np.int32))
    rp = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.concatenate(rows)
    A = csr.CsrMatrix(0, m, cols, len(ci), rp, ci, rng.uniform(-1, 1, len(ci)))
    x = rng.uniform(-1, 1, cols).astype(dtype)
    # y0 at the scale of the row's sum (about sqrt(len) / 3), so that neither
    # term of the epilogue swallows the other's rounding on the long rows
    y0 = (rng.uniform(-1, 1, m) * np.maximum(1.0, np.sqrt(lens) / 3.0)).astype(dtype)
    plants ={g: (r, int(rp[r] + np.flatnonzero(rows[r] == own[g])[0])) for g, r in want.items()}
    return Case(A, x, y0, plants, unref)


@functools.lru_cache(maxsize=None)
def empty_case(dtype, m=37):
    """A small square matrix of all-empty rows."""
    rng = np.random.default_rng(37)
    A = csr.CsrMatrix(0, m, m, 0, np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    return Case(A, rng.uniform(-1, 1, m).astype(dtype), rng.uniform(-1, 1, m).astype(dtype))


@functools.lru_cache(maxsize=None)
def stencil_case(dtype, spec):
    """A stencil surrogate (packed staged tiles) with seeded x and y0."""
    A = csr.surrogate(spec)
    rng = np.random.default_rng(5)
    return Case(A, rng.uniform(-1, 1, A.n).astype(dtype), rng.uniform(-1, 1, A.m).astype(dtype))


def tile_lanes(nrows, nnz):
    """Lanes per row of a tile of `nrows` rows and `nnz` entries (spmv.hip
    reduce_tile_rows): doubled from 1 up to 8 while two groups of rows still
    fit the 256 threads and every lane still sums 4 products of an average row."""
    L = 1
    while L < 8 and 2 * L * nrows <= 256 and 8 * L * nrows <= nnz:
        L <<= 1
    return L


def heavy_rows_of_tile(lens, start, end):
    """(L, the rows of [start, end) that tile hands to reduce_heavy_rows):
    with L < 8, the rows of more than 32 L entries."""
    L = tile_lanes(end - start, int(np.sum(lens[start:end])))
    return L, [i for i in range(start, end) if L < 8 and lens[i] > 32 * L]


def heavy_pass_rows(lens, cap, maxrows):
    """The rows that reduce_heavy_rows sums under the full-tile schedule
    (spmv_plan.cpp build_spmv_plan, spmv.hip reduce_tile_rows): consecutive rows
    of <= 256 entries packed greedily into tiles of <= cap entries / maxrows
    rows; a tile takes L = 1, 2, 4 or 8 lanes per row, and with L < 8 its rows
    of more than 32 L entries go to the second pass."""
    out, r, m = [], 0, len(lens)
    while r < m:
        if lens[r] > LONG_ROW:
            r += 1
            continue
        start, nnz = r, 0
        while r < m and r - start < maxrows:
            if lens[r] > LONG_ROW or (r > start and nnz + lens[r] > cap):
                break
            nnz += int(lens[r])
            r += 1
        out += heavy_rows_of_tile(lens, start, r)[1]
    return np.array(out, np.int64)
