"""Generators for the level-plan tests of ILU(0) (helper module, no conftest):
matrices that put a level, a chunk, a row or a term exactly on a limit of the
level planners (ilu_plan_solve.cpp, ilu_plan_factor.cpp; the constants of
rsp_kernels.h) and one past it, at a position known by construction.

Rows are numbered level by level: level l holds rows S[l] .. S[l] + w[l] - 1
(w = Case.widths), and row r of level l > 0 depends on `terms` rows of the
level before, columns S[l-1] + (r + j) mod w[l-1] for j < terms ("same" is
one term: row r on row r). So the L level of every row is its level here.
`over` changes the term count of named rows. `symmetric` stores the transpose
of these entries too: the factor then has update pairs, and U and L^T see
what L sees. `extra` adds entries to named rows as they are given (no
transpose): lower ones (a column of an earlier level) or upper ones (any
later column; they touch neither L's levels nor L's terms); mirror() gives
both. Every case also comes as its reversed transpose, (i, j) ->
(n - 1 - j, n - 1 - i): the L^T DAG of the reversal is the L DAG of the
original, so L^T (and U, for symmetric cases) meet the edge L meets.

tests/test_lvl_cases.py pins what each case reaches with the planner's own
facts (rsp_ilu0_plan_facts_host) on the CPU; tests/test_gpu_lvl_cases.py holds
the kernels to the oracle on every case."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from respasol_amd import csr


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    widths: tuple
    terms: tuple = ()        # per level >= 1 (index l - 1): lower terms per row; () = 1 everywhere
    over: tuple = ()         # ((level, r, terms), ...)
    extra: tuple = ()        # ((row, (columns, ...)), ...)
    symmetric: bool = False
    env: tuple = ()          # ((knob, value), ...) set before the analysis
    seed: int = 0

    @property
    def n(self):
        return sum(self.widths)

    @property
    def starts(self):
        return tuple(int(v) for v in np.concatenate(([0], np.cumsum(self.widths))))

    def row(self, level, r):
        return self.starts[level] + r


KNOBS = ("RSP_ILU_SLOT_CAP_MB", "RSP_ILU_SLOT_PAD", "RSP_ILU_FLOW_GATE", "RSP_ILU_FLOW_PLAN", "RSP_ILU_HUB",
         "RSP_ILU_DEFER", "RSP_ILU_LOADERS", "RSP_ILU_HOST_TERMS", "RSP_ILU_FAC_SCALE", "RSP_ILU_FAC_ONE",
         "RSP_ILU_THIN_SOLVE", "RSP_ILU_THIN_FACTOR", "RSP_ILU_THIN_TERMS", "RSP_ILU_FAT_LONG", "RSP_ILU_FAT_PAD",
         "RSP_ILU_GROUP", "RSP_ILU_SPLIT", "RSP_ILU_THIN_FACTOR_ITEMS", "RSP_ILU_THIN_FACTOR_FLOW",
         "RSP_ILU_PIECE_ITEMS")


def set_knobs(monkeypatch, knobs):
    """The planners' defaults, level-scheduled solves (the block-inverse plans
    of deep DAGs have their own cases), then the given knobs."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RSP_ILU_BLOCKS", "0")
    for k, v in knobs:
        monkeypatch.setenv(k, str(v))


def _entries(case):
    S, w = case.starts, case.widths
    over = {(l, r): k for l, r, k in case.over}
    rows, cols = [], []
    for l in range(1, len(w)):
        k_l = case.terms[l - 1] if case.terms else 1
        for r in range(w[l]):
            k = over.get((l, r), k_l)
            assert 1 <= k <= w[l - 1], (case.id, l, r, k)
            rows += [S[l] + r] * k
            cols += [S[l - 1] + (r + j) % w[l - 1] for j in range(k)]
    if case.symmetric:
        rows, cols = rows + cols, cols + rows
    level_of = np.repeat(np.arange(len(w)), w)
    for row, cs in case.extra:
        for c in cs:
            assert 0 <= c < case.n and c != row, (case.id, row, c)
            assert c > row or level_of[c] < level_of[row], (case.id, row, c)  # a lower entry: an earlier level
        rows += [row] * len(cs)
        cols += list(cs)
    return np.asarray(rows, np.int64), np.asarray(cols, np.int64)


@functools.lru_cache(maxsize=None)
def build(case, reverse=False):
    """(A, x): the case's matrix (its reversed transpose with reverse=True) and
    a right-hand side. Off-diagonals uniform(-1, 1), diagonal 1 + the sum of
    the row's |off-diagonals|, x uniform(-1, 1). Built once and shared
    between tests: not to be written."""
    n = case.n
    rows, cols = _entries(case)
    if reverse:
        rows, cols = n - 1 - cols, n - 1 - rows
    d = np.arange(n, dtype=np.int64)
    rows, cols = np.concatenate((rows, d)), np.concatenate((cols, d))
    key = np.unique(rows * n + cols)  # (sorted; an entry given twice is stored once)
    rows, cols = key // n, key % n
    rowptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int32)
    rng = np.random.default_rng([case.seed, int(reverse), n])
    vals = rng.uniform(-1.0, 1.0, rows.size)
    off = np.where(rows != cols, np.abs(vals), 0.0)
    vals[rows == cols] = 1.0 + np.bincount(rows, off, minlength=n)
    x = rng.uniform(-1.0, 1.0, n)
    return csr.CsrMatrix(0, n, n, int(rows.size), rowptr, cols.astype(np.int32), vals), x


def pattern_file(case, reverse, path):
    """The pattern as an_host_check --pattern reads it: int32 n, row offsets,
    column indices."""
    A, _ = build(case, reverse)
    with open(path, "wb") as f:
        np.asarray([A.n], np.int32).tofile(f)
        np.ascontiguousarray(A.rowptr, np.int32).tofile(f)
        np.ascontiguousarray(A.colidx, np.int32).tofile(f)
    return path


def mirror(extra):
    """The entries of `extra` and their transposes."""
    return tuple(extra) + tuple((c, (row,)) for row, cs in extra for c in cs)


def _after(row, count, skip=()):
    """`count` columns right after `row` (upper entries), none of `skip`."""
    out, c = [], row + 1
    while len(out) < count:
        if c not in skip:
            out.append(c)
        c += 1
    return tuple(out)


# ------------------------------------------------------------ solve: levels
# kThinSolveRows = 512 rows, kChunkRows = 1024 rows
WIDTH = (Case("width-512", (512,) * 3, symmetric=True),
         Case("width-513", (513,) * 3))
# kThinSolveTerms = 2048 padded terms (8 terms = two groups of 4 per row)
TERMS = (Case("terms-2048", (256,) * 3, terms=(8, 8)),
         Case("terms-2052", (256,) * 3, terms=(8, 8), over=((1, 100, 9),)))
# kChunkTerms = 4096
CHUNK_TERMS = (Case("chunk-terms", (128,) * 5, terms=(16,) * 4),)

# ------------------------------------------------------------ solve: window
# kYWin = 4096 slots: 70 levels of 64 are a run of 4480 slots; the last level
# ends at slot 4480, so slot 384 is 4096 slots before that end, slot 383 4097
_W = Case("window", (64,) * 70)
_wextra = ((_W.row(69, 0), (384, 383)), (_W.row(69, 63), (0,)))
WINDOW = (dataclasses.replace(_W, extra=_wextra),
          dataclasses.replace(_W, id="window-sym", extra=mirror(_wextra), symmetric=True))

# ------------------------------------------------------- solve: row classes
# kLongTerms = 64 (thin levels), kFatLongDefault = 3 and kHubTerms = 256 (fat)
THIN_LONG = (Case("thin-long", (80, 8, 8), over=tuple((1, r, 64 + r // 4) for r in range(8))),)
FAT_CLASSES = (Case("fat-classes", (600,) * 3,
                    over=tuple((l, r, k) for l in (1, 2) for r, k in ((10, 3), (20, 4), (30, 256), (40, 257)))),)
# short rows of a fat level: 64 = one full item, 65 = a full one and one of one row
SHORT = tuple(Case(f"short-{m}", (600,) * 3, over=tuple((l, r, 4) for l in (1, 2) for r in range(m, 600)))
              for m in (64, 65))
# gates: RSP_ILU_FLOW_GATE = 3 levels back, inside the flow segment: fat
# segments of 2, 3 and 4 levels and of 5 (an 8-row thin level between them)
GATE = (Case("gate-2-3-4", (513,) * 2 + (8,) + (513,) * 3 + (8,) + (513,) * 4),
        Case("gate-5", (8,) + (513,) * 5 + (8,)))

# -------------------------------------------------------- factor: row limits
# kFacPairs = 1024 update pairs, kFacRow = 256 entries of a row of a fat level


def _hub(widths, lowers, uppers, lone=0, pad_to=0):
    """Row R = the first row of level 1 with `lowers` lower entries (the first
    rows of level 0); each of those rows holds R and `uppers` columns of level
    2, which R holds too: every lower entry brings 1 + uppers update pairs.
    `lone` more rows of level 0 hold only R (one pair each). pad_to: R gets
    upper entries right after it up to that many stored entries."""
    c = Case("", widths)
    R, lev2 = c.row(1, 0), tuple(c.row(2, j) for j in range(uppers))
    extra = [(k, (R,) + lev2) for k in range(lowers)] + [(k, (R,)) for k in range(lowers, lowers + lone)]
    mine = tuple(range(1, lowers + lone)) + lev2  # (its "same" entry is column 0)
    if pad_to:
        mine += _after(R, pad_to - (lowers + lone + 1 + uppers), skip=lev2)
    return tuple(extra + [(R, mine)])


_HW = (600,) * 3
PAIRS = (Case("pairs-1024", _HW, extra=_hub(_HW, 32, 31)),
         Case("pairs-1025", _HW, extra=_hub(_HW, 32, 31, lone=1)))
ENTRIES = (Case("entries-256", _HW, extra=_hub(_HW, 32, 31, pad_to=256)),
           Case("entries-257", _HW, extra=_hub(_HW, 32, 31, pad_to=257)))
_GW = (1025,) * 3
GLOBAL_IN_FAT = (Case("global-in-fat", _GW, extra=_hub(_GW, 32, 31, pad_to=257)),)

# ------------------------------------------------------ factor: slot layout
# the padding rule (cnt * stride > 2 * own): one 200-entry row among 599 of three
_PW = (600,) * 5
PAD_RULE = (Case("pad-rule", _PW, extra=((Case("", _PW).row(2, 0), _after(Case("", _PW).row(2, 0), 197, skip=(Case("", _PW).row(3, 0),))),),
                 symmetric=True),)
# the budget: 600 rows of 218 entries are slots of 448 ints, 268,800 > 2^18
# ints = 1 MiB; the levels after it have small slots
_BW = (600,) * 4
_bextra = tuple((Case("", _BW).row(1, r), _after(Case("", _BW).row(1, r), 215)) for r in range(600))
BUDGET = (Case("budget-1mb", _BW, extra=_bextra, symmetric=True, env=(("RSP_ILU_SLOT_CAP_MB", 1),)),
          Case("budget-0", (600,) * 3, symmetric=True, env=(("RSP_ILU_SLOT_CAP_MB", 0),)))

# ------------------------------------------------- factor: thin-level limits
# kRndFlowItems = 1024 positions of a level that could run in a flow launch
# (level 0 of 512 rows: the diagonal and one upper entry each; 1025: one more)
FLOW_ITEMS = (Case("flow-items-1024", (512,) * 3, symmetric=True),
              Case("flow-items-1025", (512,) * 3, symmetric=True, extra=((0, (1,)),)))


# kRndItemPairs = 1024 update pairs of one position: R's diagonal gets one
# pair from every lower entry whose row holds R
def _fan(m):
    w = (m + 8, 8, 8)
    R = Case("", w).row(1, 0)
    return Case(f"item-pairs-{m}", w, extra=tuple((k, (R,)) for k in range(m)) + ((R, tuple(range(1, m))),))


ITEM_PAIRS = (_fan(1024), _fan(1025))


# one row of that many stored entries (kAnWaveRow = 128, kAnDevRow = 1024 of
# the device analysis): m - 2 lower entries, the diagonal and one upper entry
# (the row of level 2 that depends on it), the transpose stored too
def _an_row(m):
    w = (max(m + 7, 64), 64, 64)
    return Case(f"an-row-{m}", w, extra=mirror(((Case("", w).row(1, 0), tuple(range(1, m - 2))),)), symmetric=True)


AN_ROWS = tuple(_an_row(m) for m in (128, 129, 1024, 1025))

# --------------------------------------------------------- term group rule
# group 2 iff 100 * sum ceil(c / 2) <= 115 * sum ceil(c / 4) over the rows'
# term counts c: a rows of one term and b rows of four give 100 (a + 2 b) <=
# 115 (a + b), b <= 3 a / 17: 170 / 30 is on the limit, 169 / 31 past it
GROUP_RULE = tuple(Case(f"group-{g}", (200, 200), over=tuple((1, r, 4) for r in range(b)))
                   for g, b in ((2, 30), (4, 31)))

# ------------------------------------------------------------- lower only
# no upper entries: no update pairs, the factor is one level (fac_one) and by
# default one scaling launch (fac_scale); RSP_ILU_FAC_SCALE=0 plans the level
LOWER_ONLY = (Case("lower-thin-noscale", THIN_LONG[0].widths, over=THIN_LONG[0].over, env=(("RSP_ILU_FAC_SCALE", 0),)),
              Case("lower-fat-noscale", (513,) * 3, env=(("RSP_ILU_FAC_SCALE", 0),)),
              Case("lower-window-noscale", _W.widths, extra=_wextra, env=(("RSP_ILU_FAC_SCALE", 0),)))

CASES = (WIDTH + TERMS + CHUNK_TERMS + WINDOW + THIN_LONG + FAT_CLASSES + SHORT + GATE + PAIRS + ENTRIES +
         GLOBAL_IN_FAT + PAD_RULE + BUDGET + FLOW_ITEMS + ITEM_PAIRS + AN_ROWS + GROUP_RULE + LOWER_ONLY)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# ------------------------------------------------------------- knob sweep
# (case id, knobs): every knob that switches shipped code, on the cases it
# concerns (the case's own knobs stay set)
SWEEP = (
    [(cid, (("RSP_ILU_FLOW_GATE", g),)) for cid in ("gate-2-3-4", "gate-5", "fat-classes") for g in (0, 1)] +
    [(cid, (("RSP_ILU_FLOW_PLAN", 0),)) for cid in ("gate-5", "fat-classes", "width-513")] +
    [("fat-classes", (("RSP_ILU_HUB", h),)) for h in (3, 255)] +
    [(cid, (("RSP_ILU_SLOT_PAD", p),)) for cid in ("pad-rule", "entries-256") for p in (1, 16)] +
    [(cid, (("RSP_ILU_DEFER", d),)) for cid in ("window-sym", "an-row-1024") for d in (0, 1 << 30)] +
    [(cid, (("RSP_ILU_LOADERS", v),)) for cid in ("window-sym", "chunk-terms") for v in (0, 1)] +
    [(cid, (("RSP_ILU_HOST_TERMS", 1),)) for cid in ("window-sym", "terms-2052", "thin-long")])
