"""Crafted SpMV patterns (helper module, no conftest): matrices of a few tiles
that put one tile exactly on a limit of the column planner (spmv_plan.cpp
classify_tile / encode_columns / build_spmv_plan and its re-packs) or of the
tile reduce (spmv.hip stream_products_staged, reduce_tile_rows), and one past
it, at a position known by construction.

A case builds its rows from the geometry of the compute type (GEO of
test_spmv_plan_packed.py: fp64 tiles hold 2047 entries / 512 rows / 1536
staged columns, fp32 ones 4093 / 1024 / 2048), so "the limit" is the type's
own. Building blocks:

  runs_cols(lens, gap)     sorted columns in contiguous runs, `gap` unused
                           columns between two runs
  cyc_rows(cols, n, rows)  n entries over `rows` rows walking `cols` cyclically:
                           every column is used, entry U and later repeat one
                           (so n - 1 entries drop a DUPLICATE, never a column)
  SEP                      a row of 257 consecutive columns: longer than
                           kSpmvLongRow, so a tile of its own that closes the
                           tile before it and leaves the next one at an odd k0

Each case pins, per type, the tiles it must produce: T(kind, rows, entries, U,
R, packed), None = not pinned (the numpy recount of the rule still checks it).
tests/test_spmv_cases.py holds the planner to these facts on the CPU and shows
that every limit of LIMITS is met at and past its value;
tests/test_gpu_spmv_cases.py holds the kernels to the oracle on every case."""
from __future__ import annotations

import collections
import dataclasses
import functools
import zlib

import numpy as np

from respasol_amd import csr
from spmv_epilogue_ref import tile_lanes
from test_spmv_plan_packed import GEO, R32, R64, STAGE_RUNS, THREADS, ITER

DTS = (R64, R32)
NP = {R64: np.float64, R32: np.float32}
LONG = 256                                      # rsp::kSpmvLongRow
PACK_MIN = {dt: THREADS * ITER * GEO[dt]["vw"] * 12 // 16 for dt in DTS}  # more entries than this: packed (1536 / 3072)
XRSRC = 0x7ffffffc                              # bytes of the staged x loads' buffer resource
XTOP = {R64: XRSRC // 8 - 1, R32: XRSRC // 4 - 1}  # the last column a staged tile may read
PLAN_KNOBS = ("RSP_SPMV_PACK", "RSP_SPMV_STAGE_LIST", "RSP_SPMV_STAGE_PCT", "RSP_SPMV_LIST_CAP")

# One expected tile. rows: a count, "whole" (a whole long row) or "chunk".
T = collections.namedtuple("T", "kind rows entries U R packed", defaults=(None, None, None))


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    rows: object            # dt -> (list of per-row column arrays, columns of the matrix)
    tiles: object           # dt -> the expected tiles, in plan order
    env: tuple = ()         # ((plan-time knob, value), ...)
    opts: tuple = ()        # ((planner option, dt -> value), ...): spread, local_cols, row_align, use_c16, use_stage
    counts: object = None   # dt -> {"nint" / "nlong" / "nslots": value}
    lanes: object = None    # dt -> lanes per row of every row tile, in plan order
    heavy: object = None    # dt -> rows on the heavy list of every row tile, in plan order
    gpu: bool = True        # False: host only (see the x-resource cases)

    def options(self, dt):
        return {k: int(v(dt)) for k, v in self.opts}


def set_knobs(monkeypatch, case, extra=()):
    """The planner's default knobs, then the case's, then `extra`."""
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env + tuple(extra):
        monkeypatch.setenv(k, str(v))


# ------------------------------------------------------------ building blocks

def runs_cols(lens, gap=1, start=0):
    out, c = [], start
    for n in lens:
        out.append(np.arange(c, c + n))
        c += n + gap
    return np.concatenate(out)


def cyc_rows(cols, n, nrows):
    cols = np.asarray(cols)
    assert n >= len(cols) >= -(-n // nrows) and -(-n // nrows) <= LONG
    seq = cols[np.arange(n) % len(cols)]
    cut = np.concatenate(([0], np.cumsum([n // nrows + (i < n % nrows) for i in range(nrows)])))
    return [np.sort(seq[cut[i]:cut[i + 1]]) for i in range(nrows)]


def band_rows(lens, step=3, start=0):
    """Row i: lens[i] consecutive columns from start + step * i."""
    return [start + step * i + np.arange(n) for i, n in enumerate(lens)]


def ncols_of(rows):
    return int(max(int(r[-1]) for r in rows if len(r))) + 1


SEP = np.arange(LONG + 1)


def fixed(*tiles):
    """The same expected tiles for both types."""
    return lambda dt: list(tiles)


def packed(dt, n):
    return int(n > PACK_MIN[dt])


# ------------------------------------------------------------------- the cases

def _span(span):
    """31 rows, 242 entries, every column its own run 7 apart (U = len, so
    never staged); row 0 holds columns 0 and `span`."""
    def make(dt):
        rows = [np.array([0, span])] + [1 + 7 * (8 * j + np.arange(8)) for j in range(30)]
        return rows, span + 1
    return make


def _span_chunk(span):
    """One row of cap + 10 entries: chunk 0 is columns 0 .. cap - 2 and `span`,
    chunk 1 ten columns after it."""
    def make(dt):
        c = GEO[dt]["cap"]
        return [np.concatenate([np.arange(c - 1), [span], span + 1 + np.arange(10)])], span + 11
    return make


def _span_cut(dt):
    """One row of cap + 10 entries: chunk 0 spans cap - 1 columns, chunk 1
    (nine columns after it and one 65536 past its first) 65536."""
    c = GEO[dt]["cap"]
    return [np.concatenate([np.arange(c + 9), [c + 65536]])], c + 65537


def _slots(over, runs=False):
    """U = ucap + over distinct columns, contiguous (R = 1) or in 254 runs
    (fp64: 12 of 7 and 242 of 6; fp32: 16 of 9 and 238 of 8), over
    ceil(1.25 U) entries (+ 2 past the limit, so the share rule is not what
    fails) in rows of 8."""
    def make(dt):
        u = GEO[dt]["ucap"] + over
        if runs:
            q, r = divmod(u, STAGE_RUNS)
            cols = runs_cols([q + 1] * r + [q] * (STAGE_RUNS - r))
        else:
            cols = np.arange(u)
        n = -(-5 * u // 4) + 2 * over
        rows = cyc_rows(cols, n, n // 8)
        return rows, ncols_of(rows)
    return make


def _slots_tiles(over, R):
    def tiles(dt):
        u = GEO[dt]["ucap"] + over
        n = -(-5 * u // 4) + 2 * over
        return [T("runs", n // 8, n, u, R, packed(dt, n))] if over == 0 else [T("gather16", n // 8, n, 0, 0, 0)]
    return tiles


def _one_col(n):
    return lambda dt: ([np.array([5])] * n, 6)


def _runs(nr, run=4, extra=()):
    """nr runs of 4 columns one unused column apart, each held by two rows:
    2 nr rows, 8 nr entries, U = 4 nr, R = nr (+ the rows of `extra`)."""
    def make(dt):
        cols = runs_cols([run] * nr)
        rows = [cols[run * (i // 2):run * (i // 2 + 1)] for i in range(2 * nr)] + [np.asarray(e) for e in extra]
        return rows, ncols_of(rows)
    return make


def _runs_tiles(nr):
    return lambda dt: [T("runs", 2 * nr, 8 * nr, 4 * nr, nr, packed(dt, 8 * nr))]


def _runs255_tiles(dt):
    # 255 runs: one more than a run table holds. fp64: U = 1020 <= 1536, a
    # column list; 2040 entries > 1536: packed. fp32 has no lists.
    return [T("list", 510, 2040, 1020, 255, 1)] if dt == R64 else [T("gather16", 510, 2040, 0, 0, 0)]


def _gap1(dt):
    """Runs of 3, 5 and 2 columns, one unused column between them, each twice."""
    cols = runs_cols([3, 5, 2])
    rows = [cols[:3], cols[:3], cols[3:8], cols[3:8], cols[8:], cols[8:]]
    return rows, ncols_of(rows)


def _list(U, n=None, per_row=5, lead=()):
    """U columns two apart (R = U) over n >= U entries in rows of <= per_row."""
    def make(dt):
        nn = n or U
        rows = [np.asarray(r) for r in lead] + cyc_rows(2 * np.arange(U), nn, -(-nn // per_row))
        return rows, ncols_of(rows)
    return make


def _list_tiles(U, n=None, per_row=5):
    def tiles(dt):
        nn = n or U
        nr = -(-nn // per_row)
        return [T("list", nr, nn, U, U, packed(dt, nn))] if dt == R64 else [T("gather16", nr, nn, 0, 0, 0)]
    return tiles


def _list_past(dt):
    """1537 columns two apart in rows of 5, closed by SEP, then a tile of 2000
    entries over 1000 contiguous columns: the second tile keeps list_repack
    (more than half of the sampled entries) away, so tile 0 stays whole with
    one column more than a list holds."""
    rows = cyc_rows(2 * np.arange(1537), 1537, 308) + [SEP] + cyc_rows(4000 + np.arange(1000), 2000, 250)
    return rows, ncols_of(rows)


def _repack(dt):
    """600 rows of 8 columns, all two apart: every full tile has more columns
    than a list holds in more runs than a run table holds."""
    rows = [2 * (8 * i + np.arange(8)) for i in range(600)]
    return rows, ncols_of(rows)


def _repack_tiles(dt):
    # fp64: re-packed at 1536 entries = 192 rows: three lists at U = ucap, and
    # 24 rows of 192 columns in 192 runs (<= 254: no list; U = len: no runs).
    # fp32 (no lists, no re-pack): 511 rows = 4088 entries, then 89 rows.
    if dt == R64:
        return [T("list", 192, 1536, 1536, 1536, 0)] * 3 + [T("gather16", 24, 192, 0, 0, 0)]
    return [T("gather16", 511, 4088, 0, 0, 0), T("gather16", 89, 712, 0, 0, 0)]


def _repack64_tiles(dt):
    # RSP_SPMV_LIST_CAP 1 (clamped to 64) and 64: 75 tiles of 8 rows; 64 runs
    # are no list and U = len is not staged
    return [T("gather16", 8, 64, 0, 0, 0)] * 75 if dt == R64 else _repack_tiles(dt)


def _share(U, n, per_row=5):
    """U contiguous columns over n entries."""
    def make(dt):
        rows = cyc_rows(np.arange(U), n, -(-n // per_row))
        return rows, U
    return make


def _rows_cap(dt, start=0):
    """kMaxRows rows holding kMaxNnz entries: rows of 4 and one (fp64) or
    three (fp32) of 3, row i from column start + i (step 1)."""
    g = GEO[dt]
    k3 = 4 * g["maxrows"] - g["cap"]
    return band_rows([4] * (g["maxrows"] - k3) + [3] * k3, step=1, start=start)


def _rows_cap_tile(dt):
    g = GEO[dt]  # columns 0 .. maxrows + 1: one run
    return T("runs", g["maxrows"], g["cap"], g["maxrows"] + 2, 1, 1)


def _rows_full(extra):
    def make(dt):
        rows = _rows_cap(dt) + [np.arange(4)] * extra
        return rows, ncols_of(rows)
    return make


def _entries_cap(dt):
    """Rows of 8 (and one shorter) to exactly kMaxNnz entries in fewer than
    kMaxRows rows, then a row of one entry: cap + 1."""
    c = GEO[dt]["cap"]
    return band_rows([8] * (c // 8) + [c % 8, 1], step=1), c // 8 + 9


def _rows_empty(dt):
    rows = _rows_cap(dt) + [np.zeros(0, np.int64)] * GEO[dt]["maxrows"] + _rows_cap(dt, 7)
    return rows, ncols_of(rows)


def _tail_packed(dt):
    """1000 contiguous columns over PACK_MIN + 65 entries (odd, 1 mod 4)."""
    n = PACK_MIN[dt] + 65
    return cyc_rows(np.arange(1000), n, n // 8), 1000


SPECIAL = (32, 33, 64, 65, 128, 129)  # a row on and past 32 L entries for L = 1, 2, 4


def _reduce(nrows, nnz):
    """A tile of nrows rows and nnz entries: the SPECIAL rows first, the rest
    of the entries spread evenly."""
    def make(dt):
        rest, k = nnz - sum(SPECIAL), nrows - len(SPECIAL)
        lens = list(SPECIAL) + [rest // k + (i < rest % k) for i in range(k)]
        assert max(lens) <= LONG and min(lens) >= 0
        rows = band_rows(lens)
        return rows, ncols_of(rows)
    return make


def _reduce_case(name, nrows, nnz, L):
    heavy = sum(n > 32 * L for n in SPECIAL) if L < 8 else 0
    return Case(name, _reduce(nrows, nnz), fixed(T(None, nrows, nnz)), lanes=fixed(L), heavy=fixed(heavy))


def _heavy(width, pad):
    """As many rows of `width` entries as a tile holds, then pad[dt] empty rows."""
    def make(dt):
        rows = band_rows([width] * (GEO[dt]["cap"] // width)) + [np.zeros(0, np.int64)] * pad[dt]
        return rows, ncols_of(rows)
    return make


def _heavy_tiles(width, pad):
    return lambda dt: [T(None, GEO[dt]["cap"] // width + pad[dt], GEO[dt]["cap"] // width * width)]


def _xrsrc(over):
    """Two rows of the same two columns, the upper one XTOP + over (host only:
    x would be 2 GiB)."""
    return lambda dt: ([np.array([XTOP[dt] + over - 1, XTOP[dt] + over])] * 2, XTOP[dt] + over + 1)


def _align34(short):
    """row_align a = 128 B of y: a rows of 3 k - short entries in all, k / 250
    rows of 250, then a row of 100 that no longer fits (k = 500 fp64, 1000
    fp32: 4 k + 100 > cap). The cut after a rows keeps 3 k - short of 4 k - short
    entries: exactly three quarters with short = 0, less with short = 1."""
    def make(dt):
        a, k = 128 // np.dtype(NP[dt]).itemsize, 500 if dt == R64 else 1000
        n = 3 * k - short
        lens = [n // a + (i < n % a) for i in range(a)] + [250] * (k // 250) + [100]
        rows = band_rows(lens)
        return rows, ncols_of(rows)
    return make


def _align34_tiles(short):
    def tiles(dt):
        a, k = 128 // np.dtype(NP[dt]).itemsize, 500 if dt == R64 else 1000
        if short == 0:
            return [T(None, a, 3 * k), T(None, k // 250 + 1, k + 100)]
        return [T(None, a + k // 250, 4 * k - 1), T(None, 1, 100)]
    return tiles


def _fours(m):
    return lambda dt: (band_rows([4] * m, step=1), m + 3)


def _spread_tiles(dt):
    # 2000 rows of 4 = 8000 entries at 64 entries per tile: 125 tiles of 16 rows
    return [T(None, 16, 64)] * 125


def _local_rows(dt):
    return band_rows([4] * (3 * (GEO[dt]["cap"] // 4)), step=1), 3 * (GEO[dt]["cap"] // 4) + 3


def _local_long(dt):
    """Ten short rows, a row of 2 cap + 5 entries, ten short rows; every
    column local."""
    c = GEO[dt]["cap"]
    rows = band_rows([4] * 10) + [np.arange(2 * c + 5)] + band_rows([4] * 10, start=40)
    return rows, 2 * c + 5


def _first_tile_last_col(dt):
    return GEO[dt]["cap"] // 4 - 1 + 3  # row per - 1 of _local_rows holds columns per - 1 .. per + 2


PAD1 = {R64: 70, R32: 10}   # 62 + 70 = 132 rows, 124 + 10 = 134: more than 128, L = 1
PAD2 = {R64: 40, R32: 10}   # 31 + 40 = 71 rows, 62 + 10 = 72: 65 .. 128, L = 2
PAD4 = {R64: 20, R32: 5}    # 15 + 20 = 35 rows, 31 + 5 = 36: 33 .. 64, L = 4

CASES = (
    # ---- span: hi - lo <= 65535 keeps 16-bit offsets, one more is an int32 tile
    Case("span-65535", _span(65535), fixed(T("gather16", 31, 242, 0, 0, 0))),
    Case("span-65536", _span(65536), fixed(T("int32", 31, 242, 0, 0, 0))),
    # a chunked row: nlong 1, two partial slots; chunks never stage (r1 < 0)
    Case("span-chunk-65535", _span_chunk(65535),
         lambda dt: [T("gather16", "chunk", GEO[dt]["cap"], 0, 0, 0), T("gather16", "chunk", 10, 0, 0, 0)],
         counts=fixed(("nlong", 1), ("nslots", 2))),
    Case("span-chunk-65536", _span_chunk(65536),
         lambda dt: [T("int32", "chunk", GEO[dt]["cap"], 0, 0, 0), T("gather16", "chunk", 10, 0, 0, 0)],
         counts=fixed(("nlong", 1), ("nslots", 2))),
    # every column of a chunk once: at 100 % a row tile would stage, a chunk keeps its offsets by rule
    Case("span-chunk-pct100", _span_chunk(65535),
         lambda dt: [T("gather16", "chunk", GEO[dt]["cap"], 0, 0, 0), T("gather16", "chunk", 10, 0, 0, 0)],
         env=(("RSP_SPMV_STAGE_PCT", 100),)),
    Case("span-cut", _span_cut,
         lambda dt: [T("gather16", "chunk", GEO[dt]["cap"], 0, 0, 0), T("int32", "chunk", 10, 0, 0, 0)]),
    # ---- slots: U <= kStageSlots. 100 U == 80 len too (1536 / 1920, 2048 / 2560)
    Case("slots-ucap", _slots(0), _slots_tiles(0, 1)),
    Case("slots-ucap+1", _slots(1), _slots_tiles(1, 1)),
    Case("slots-ucap-runs254", _slots(0, runs=True), _slots_tiles(0, STAGE_RUNS)),
    # 100 * 1 <= 80 * 2, but not <= 80 * 1
    Case("slots-one-len2", _one_col(2), fixed(T("runs", 2, 2, 1, 1, 0))),
    Case("slots-one-len1", _one_col(1), fixed(T("gather16", 1, 1, 0, 0, 0))),
    # ---- runs: the halving search over nr descriptors (skipped for nr == 1)
    *(Case(f"runs-{nr}", _runs(nr), _runs_tiles(nr)) for nr in (1, 2, 3, 4, 5, 127, 128, 129, 253, 254)),
    Case("runs-255", _runs(255), _runs255_tiles),
    Case("runs-255-nolist", _runs(255), fixed(T("gather16", 510, 2040, 0, 0, 0)), env=(("RSP_SPMV_STAGE_LIST", 0),)),
    Case("runs-gap1", _gap1, fixed(T("runs", 6, 20, 10, 3, 0))),
    # ---- lists (fp64; fp32 gathers): slot 255 / 256 on the 256-thread edge, U % 4 = 3, 0, 1, 2
    *(Case(f"list-u{U}", _list(U), _list_tiles(U)) for U in (255, 256, 257, 258)),
    Case("list-ucap", _list(1536), _list_tiles(1536)),                     # 1536 entries: not packed
    Case("list-ucap-packed", _list(1536, 2000), _list_tiles(1536, 2000)),  # 2000 entries: packed
    # tile 0: 1537 columns in 1537 runs, too many for a list; SEP; 1000 columns over 2000 entries
    Case("list-ucap+1", _list_past,
         lambda dt: [T("gather16", 308, 1537, 0, 0, 0), T("gather16", "whole", 257, 0, 0, 0),
                     T("runs", 250, 2000, 1000, 1, packed(dt, 2000))]),
    Case("list-repack", _repack, _repack_tiles),
    Case("list-repack-cap1", _repack, _repack64_tiles, env=(("RSP_SPMV_LIST_CAP", 1),)),
    Case("list-repack-cap64", _repack, _repack64_tiles, env=(("RSP_SPMV_LIST_CAP", 64),)),
    # ---- share: 100 U <= pct len. 40 / 50 at 80 %, 25 / 50 at 50 %; 49 entries drop a duplicate
    Case("share80-at", _share(40, 50), fixed(T("runs", 10, 50, 40, 1, 0))),
    Case("share80-past", _share(40, 49), fixed(T("gather16", 10, 49, 0, 0, 0))),
    Case("share50-at", _share(25, 50), fixed(T("runs", 10, 50, 25, 1, 0)), env=(("RSP_SPMV_STAGE_PCT", 50),)),
    Case("share50-past", _share(25, 49), fixed(T("gather16", 10, 49, 0, 0, 0)), env=(("RSP_SPMV_STAGE_PCT", 50),)),
    Case("share0", _one_col(50), fixed(T("gather16", 50, 50, 0, 0, 0)), env=(("RSP_SPMV_STAGE_PCT", 0),)),
    Case("share100", _share(50, 50), fixed(T("runs", 10, 50, 50, 1, 0)), env=(("RSP_SPMV_STAGE_PCT", 100),)),
    # ---- rows and entries
    Case("rows-cap", _rows_full(0), lambda dt: [_rows_cap_tile(dt)]),
    Case("rows-cap+1", _rows_full(1), lambda dt: [_rows_cap_tile(dt), T("gather16", 1, 4, 0, 0, 0)]),
    Case("entries-cap", _entries_cap, lambda dt: [T("runs", GEO[dt]["cap"] // 8 + 1, GEO[dt]["cap"], None, 1, 1),
                                                  T("gather16", 1, 1, 0, 0, 0)]),
    # the empty tile has no columns: it stays on the (unread) int32 code; tile 2 starts at k0 = cap (odd)
    Case("rows-empty-tile", _rows_empty,
         lambda dt: [_rows_cap_tile(dt), T("int32", GEO[dt]["maxrows"], 0, 0, 0, 0), _rows_cap_tile(dt)]),
    # the arrays end inside a 16-byte vector (41, 301, PACK_MIN + 65 entries: 1 mod 4): the scalar path
    Case("tail-runs", _runs(5, extra=([0],)), fixed(T("runs", 11, 41, 20, 5, 0))),
    Case("tail-list", _list(300, 301), _list_tiles(300, 301)),
    Case("tail-packed", _tail_packed, lambda dt: [T("runs", (PACK_MIN[dt] + 65) // 8, PACK_MIN[dt] + 65, 1000, 1, 1)]),
    # k0 = 257 after SEP: the tile starts inside a vector
    Case("align-runs", lambda dt: (lambda r: ([SEP] + r[0], max(r[1], 257)))(_runs(5)(dt)),
         fixed(T("gather16", "whole", 257, 0, 0, 0), T("runs", 10, 40, 20, 5, 0))),
    Case("align-list", _list(300, lead=(SEP,)),
         lambda dt: [T("gather16", "whole", 257, 0, 0, 0)] + _list_tiles(300)(dt)),
    # ---- reduce: L doubles while 2 L nrows <= 256 and 8 L nrows <= nnz
    _reduce_case("lanes1-rows128", 128, 1100, 2),   # 2 * 128 == 256 -> 2; 4 * 128 > 256
    _reduce_case("lanes1-rows129", 129, 1100, 1),   # 2 * 129 > 256
    _reduce_case("lanes2-rows64", 64, 1100, 4),     # 4 * 64 == 256 and 16 * 64 <= 1100 -> 4; 8 * 64 > 256
    _reduce_case("lanes2-rows65", 65, 1100, 2),     # 4 * 65 > 256
    _reduce_case("lanes4-rows32", 32, 1100, 8),     # 8 * 32 == 256 and 32 * 32 <= 1100 -> 8
    _reduce_case("lanes4-rows33", 33, 1100, 4),     # 8 * 33 > 256
    _reduce_case("lanes1-nnz800", 100, 800, 2),     # 8 * 100 == 800 -> 2; 4 * 100 > 256
    _reduce_case("lanes1-nnz799", 100, 799, 1),
    _reduce_case("lanes2-nnz800", 50, 800, 4),      # 16 * 50 == 800 -> 4; 8 * 50 > 256
    _reduce_case("lanes2-nnz799", 50, 799, 2),
    _reduce_case("lanes4-nnz800", 25, 800, 8),      # 32 * 25 == 800 -> 8
    _reduce_case("lanes4-nnz799", 25, 799, 4),
    # the longest heavy lists: cap // 33 = 62 / 124 rows at L = 1, cap // 65 = 31 / 62 at L = 2, cap // 129 = 15 / 31 at L = 4
    Case("heavy-max", _heavy(33, PAD1), _heavy_tiles(33, PAD1), lanes=fixed(1), heavy=lambda dt: [GEO[dt]["cap"] // 33]),
    Case("heavy-max-l2", _heavy(65, PAD2), _heavy_tiles(65, PAD2), lanes=fixed(2), heavy=lambda dt: [GEO[dt]["cap"] // 65]),
    Case("heavy-max-l4", _heavy(129, PAD4), _heavy_tiles(129, PAD4), lanes=fixed(4), heavy=lambda dt: [GEO[dt]["cap"] // 129]),
    # ---- the x buffer resource: (hi + 1) * sizeof(T) <= 0x7ffffffc. Host only: an x of 2 GiB is
    # no test of a few seconds on a shared machine.
    Case("xrsrc-at", _xrsrc(0), fixed(T("runs", 2, 4, 2, 1, 0)), gpu=False),
    Case("xrsrc-past", _xrsrc(1), fixed(T("gather16", 2, 4, 0, 0, 0)), gpu=False),
    # ---- planner options
    # runs-5's pattern with the 16-bit offsets, then the staged tiles, switched off
    Case("opt-no-c16", _runs(5), fixed(T("int32", 10, 40, 0, 0, 0)), opts=(("use_c16", lambda dt: 0),)),
    Case("opt-no-stage", _runs(5), fixed(T("gather16", 10, 40, 0, 0, 0)), opts=(("use_stage", lambda dt: 0),)),
    Case("align-3of4", _align34(0), _align34_tiles(0), opts=(("row_align", lambda dt: 128 // np.dtype(NP[dt]).itemsize),)),
    Case("align-below-3of4", _align34(1), _align34_tiles(1),
         opts=(("row_align", lambda dt: 128 // np.dtype(NP[dt]).itemsize),)),
    # 8000 entries: ceil(8000 / 1024) = 8 < 64 is raised to the floor of 64; ceil(8000 / 125) == 64
    Case("spread-below64", _fours(2000), _spread_tiles, opts=(("spread", lambda dt: 1024),)),
    Case("spread-at64", _fours(2000), _spread_tiles, opts=(("spread", lambda dt: 125),)),
    # three tiles of rows of 4; column per + 2 is the first tile's last entry alone
    Case("local-last-out", _local_rows, lambda dt: [T(None, GEO[dt]["cap"] // 4, GEO[dt]["cap"] // 4 * 4)] * 3,
         opts=(("local_cols", _first_tile_last_col),), counts=fixed(("nint", 0))),
    Case("local-last-in", _local_rows, lambda dt: [T(None, GEO[dt]["cap"] // 4, GEO[dt]["cap"] // 4 * 4)] * 3,
         opts=(("local_cols", lambda dt: _first_tile_last_col(dt) + 1),), counts=fixed(("nint", 1))),
    # both row tiles are interior and come first; the chunks of the long row are part 2 whatever they read
    Case("local-long", _local_long,
         lambda dt: [T(None, 10, 40), T(None, 10, 40), T(None, "chunk", GEO[dt]["cap"]), T(None, "chunk", GEO[dt]["cap"]),
                     T(None, "chunk", 5)],
         opts=(("local_cols", lambda dt: 2 * GEO[dt]["cap"] + 5),), counts=fixed(("nint", 2), ("nlong", 1), ("nslots", 3))),
)
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
GPU_CASES = tuple(c for c in CASES if c.gpu)
# run together as one rsp_spmv_batch and as parts 1 + 2 of a split schedule (tests/test_gpu_spmv_cases.py)
SUBSET = ("span-65535", "span-65536", "runs-254", "runs-255", "rows-cap", "heavy-max")


@functools.lru_cache(maxsize=None)
def build(case_id, dt):
    """The case's matrix for one type, values uniform in (-1, 1) seeded by the
    case's name. Shared between tests: not to be written."""
    case = BY_ID[case_id]
    rows, ncols = case.rows(dt)
    rp = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    ci = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.int32) if rp[-1] else np.zeros(0, np.int32)
    for r in rows:
        assert len(r) == 0 or (np.all(np.diff(r) > 0) and 0 <= r[0] and r[-1] < ncols), case_id
    rng = np.random.default_rng(zlib.crc32(case_id.encode()))
    A = csr.CsrMatrix(0, len(rows), int(ncols), int(rp[-1]), rp, ci, rng.uniform(-1.0, 1.0, int(rp[-1])))
    for a in (A.rowptr, A.colidx, A.values):
        a.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def vectors(case_id, dt):
    """(x, y0) of a GPU case in the type: x a seeded permutation of n evenly
    spaced points of (-1, 1), pairwise distinct in fp32 as well, so a wrongly
    decoded column changes the sum; y0 uniform in (-1, 1)."""
    A = build(case_id, dt)
    assert BY_ID[case_id].gpu and A.n < 1 << 20
    rng = np.random.default_rng(zlib.crc32(case_id.encode()) + 1)
    x = ((rng.permutation(A.n) + 0.5) * (2.0 / A.n) - 1.0).astype(NP[dt])
    assert len(np.unique(x)) == A.n
    y0 = rng.uniform(-1.0, 1.0, A.m).astype(NP[dt])
    x.setflags(write=False)
    y0.setflags(write=False)
    return x, y0


# ------------------------------------------------------------------ the limits

def measures(A, dt, tiles, pct=80):
    """What the tiles of one plan reach, per limit of LIMITS: {name: set of
    values}, counted from the pattern (numpy), the tile boundaries alone taken
    from the plan."""
    g = GEO[dt]
    rp, ci = np.asarray(A.rowptr, np.int64), np.asarray(A.colidx, np.int64)
    out = collections.defaultdict(set)
    for t in tiles:
        k0, k1, r0, r1 = t["k0"], t["k1"], t["r0"], t["r1"]
        n = k1 - k0
        if n == 0:
            out["empty-tile-rows"].add(r1 - r0)
            continue
        cols = np.unique(ci[k0:k1])
        U, R, span = len(cols), 1 + int(np.count_nonzero(np.diff(cols) != 1)), int(cols[-1] - cols[0])
        out["span-chunk" if r1 < 0 else "span"].add(span)
        if r1 < 0 or span > 65535:
            continue
        out["xrsrc"].add((int(cols[-1]) + 1) * np.dtype(NP[dt]).itemsize)
        out["runs"].add(R)
        if R > STAGE_RUNS:
            out["list-slots"].add(U)
        if R == 1:
            out["slots-one-run"].add(U)
        if R == STAGE_RUNS:
            out["slots-254-runs"].add(U)
        if U <= g["ucap"] and R <= STAGE_RUNS:
            out[f"share{pct}"].add(pct * n - 100 * U)
        if t["kind"] in ("runs", "list"):
            if k1 == rp[-1] and k1 % g["vw"]:
                out["scalar-tail"].add(t["kind"] + ("-packed" if t["packed"] else ""))
            if k0 % g["vw"]:
                out["odd-k0"].add(t["kind"])
        nrows = r1 - r0
        out["rows-and-entries"].add((nrows, n))
        nxt = int(rp[r1 + 1] - rp[r1]) if r1 < len(rp) - 1 else None
        if nxt is not None and nxt <= LONG and nrows == g["maxrows"] and n + nxt <= g["cap"]:
            out["rows"].add(nrows + 1)          # the next row was kept out by the row limit alone
        out["rows"].add(nrows)
        out["entries"].add(n)
        if nxt is not None and nxt <= LONG and nrows < g["maxrows"]:
            out["entries"].add(n + nxt)         # ... by the entry limit
        for L in (1, 2, 4):
            out[f"lanes{L}-rows"].add(2 * L * nrows)
            out[f"lanes{L}-entries"].add(8 * L * nrows - n)
        lens = np.diff(rp[r0:r1 + 1])
        for L, w in ((1, 32), (2, 64), (4, 128)):
            if tile_lanes(nrows, n) == L:
                out[f"heavy-list-l{L}"].add(int(np.count_nonzero(lens > w)))
    return out


def limits(dt):
    """name: (the value on the limit, the value one past it), per type. Every
    one has to appear among the measures of some case
    (test_spmv_cases.test_every_limit_is_met_and_passed)."""
    g, elem = GEO[dt], np.dtype(NP[dt]).itemsize
    assert (XTOP[dt] + 1) * elem <= XRSRC < (XTOP[dt] + 2) * elem
    lim = {
        "span": (65535, 65536),
        "span-chunk": (65535, 65536),
        "slots-one-run": (g["ucap"], g["ucap"] + 1),
        "slots-254-runs": (g["ucap"], None),
        "runs": (STAGE_RUNS, STAGE_RUNS + 1),
        "share80": (0, -80),
        "share50": (0, -50),
        "xrsrc": ((XTOP[dt] + 1) * elem, (XTOP[dt] + 2) * elem),  # the largest multiple of sizeof(T) <= XRSRC
        "rows-and-entries": ((g["maxrows"], g["cap"]), None),
        "rows": (g["maxrows"], g["maxrows"] + 1),
        "entries": (g["cap"], g["cap"] + 1),
        "empty-tile-rows": (g["maxrows"], None),
        "heavy-list-l1": (g["cap"] // 33, None),
        "heavy-list-l2": (g["cap"] // 65, None),
        "heavy-list-l4": (g["cap"] // 129, None),
    }
    for L in (1, 2, 4):
        lim[f"lanes{L}-rows"] = (256, 256 + 2 * L)
        lim[f"lanes{L}-entries"] = (0, 1)
    if dt == R64:
        lim["list-slots"] = (g["ucap"], g["ucap"] + 1)
    return lim
